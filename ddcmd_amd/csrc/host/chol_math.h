/* chol_math.h -- the arithmetic of ANALYSIS cholAnalysis (cholAnalysis.c:137-157), one statement per operation, shared by the device
 * lane (ddcmi_chol.inl) and the host completion of split molecules (chol.c), so that a molecule finished on the host has the bits
 * it would have whole on one device.  The includer defines
 *    CHOL_FN        the functions' qualifiers (static inline; __device__ __forceinline__)
 *    CHOL_RND(x)    x, rounded once and kept from contraction into an FMA (the host file is compiled with -ffp-contract=off and
 *                   passes x through; the device library is built with -ffp-contract=fast and passes it through zd_rounded)
 * Every product below stands inside CHOL_RND; sums, differences, the division and the square root are single IEEE operations. */
#ifndef DDCMI_CHOL_MATH_H
#define DDCMI_CHOL_MATH_H

/* b = nearestImage(rj - ri) in an orthorhombic box of sides L (invL = 1.0 / L, formed by the caller): the rint form of the
 * project's oracle, da = -rint((1/L) d), d += L da; an open axis (its bit of pbc clear) is not wrapped */
CHOL_FN void chol_bond(const double *L, const double *invL, int pbc, const double *ri, const double *rj, double *b)
{
   for (int a = 0; a < 3; a++)
   {
      double d = rj[a] - ri[a];
      if (pbc >> a & 1)
      {
         const double t = CHOL_RND(invL[a] * d), da = -rint(t), s = CHOL_RND(L[a] * da);
         d = d + s;
      }
      b[a] = d;
   }
}
/* (x . a) / sqrt(x . x), x = u x v; sign -1: the dot product is negated in front of the division */
CHOL_FN double chol_plane_offset(const double *u, const double *v, const double *a, int negate)
{
   double x[3];
   x[0] = CHOL_RND(u[1] * v[2]) - CHOL_RND(u[2] * v[1]);
   x[1] = CHOL_RND(u[2] * v[0]) - CHOL_RND(u[0] * v[2]);
   x[2] = CHOL_RND(u[0] * v[1]) - CHOL_RND(u[1] * v[0]);
   const double p0 = CHOL_RND(x[0] * a[0]), p1 = CHOL_RND(x[1] * a[1]), p2 = CHOL_RND(x[2] * a[2]);
   const double q0 = CHOL_RND(x[0] * x[0]), q1 = CHOL_RND(x[1] * x[1]), q2 = CHOL_RND(x[2] * x[2]);
   double dot = (p0 + p1) + p2;
   const double sq = (q0 + q1) + q2;
   if (negate) dot = -dot;
   return dot / sqrt(sq);
}
/* r[7][3]: the beads of roles 0..6.  A = b(0,1), B = b(0,2), C = b(0,3), D = b(4,5), E = b(4,3), F = b(4,6);
 * dR1 = ((B x C) . A) / |B x C|, dR5 = -((E x F) . D) / |E x F| */
CHOL_FN void chol_offsets_of(const double *L, const double *invL, int pbc, const double *r, double *dR1, double *dR5)
{
   double A[3], B[3], C[3], D[3], E[3], F[3];
   chol_bond(L, invL, pbc, r + 0, r + 3, A);
   chol_bond(L, invL, pbc, r + 0, r + 6, B);
   chol_bond(L, invL, pbc, r + 0, r + 9, C);
   chol_bond(L, invL, pbc, r + 12, r + 15, D);
   chol_bond(L, invL, pbc, r + 12, r + 9, E);
   chol_bond(L, invL, pbc, r + 12, r + 18, F);
   *dR1 = chol_plane_offset(B, C, A, 0);
   *dR5 = chol_plane_offset(E, F, D, 1);
}
/* (int)MIN(MAX((d - rmin)/delta, 0), nbins - 1) with the reference's macros: a NaN fails `> 0` and goes to bin 0 */
CHOL_FN int chol_bin(double d, double rmin, double delta, int nbins)
{
   const double q = (d - rmin) / delta, top = (double)(nbins - 1);
   const double lo = q > 0.0 ? q : 0.0;
   return (int)(lo < top ? lo : top);
}
#endif

/* ddcmi_census.inl -- ANALYSIS types vcmWrite and zdensity on the device (vcmWrite.c:95-110, zdensity.c:66-151): one census pass
 * (ddcmi_census_frame.inl) over the owned beads each.  Included from ddcmi.hip behind ddcmi_vaf.inl.
 *
 * Momentum (k_class_sums<4, MomentumBead>): four values per class, {m vx, m vy, m vz, m}.  m is ctx->d_mass[species]: the mass
 * ddcmi_set_species took, whose reciprocal (d_invmass) the integrator's kick multiplies the force with and which its kinetic energy
 * uses -- the reference's ((ATOMTYPE_PARMS *)species->parm)->mass.
 *
 * Z histogram (k_census_zdensity<SMEAR>), derived in DESIGN.md ("zdensity: the shape of the histogram kernel"):
 *   SMEAR = false  one bin per bead, weight 1: the key's lanes are COUNTED (popcount of the ballot) and the count goes into the
 *                  workgroup's one row of 32-bit integers by an integer LDS add; workgroup partials are 32-bit (a workgroup holds
 *                  fewer than 2^32 beads), the second stage adds them in 64 bits and converts once: exact at any bead count.
 *   SMEAR = true   two (bin, weight) pairs per bead, the lower bin's pass first, then the upper bin's (the reference's kk = 0, 1);
 *                  per-wave rows of doubles: CENSUS_WAVES x 8 B of LDS per bin, hence CENSUS_MAX_NZ.
 * The per-bead arithmetic is the reference's, operation by operation, with every product kept from contraction into an FMA
 * (zd_rounded: the library is built with -ffp-contract=fast), so that a float64 restatement on the host lands in the same bin at an edge.  The position is the
 * one ddcmi_download_state hands out: slot position, shifted once by the box side where it left a periodic box since the last
 * rebuild (export_coord); the reference bins its positions as they are, and so does this -- no further wrap.  A coordinate outside
 * the box reaches the reference's clamp: a label read as unsigned that is >= nz goes to nz - 1 (negative t below -1 included;
 * -1 < t < 0 truncates to bin 0).  The conversion to int saturates at +-2^30 (C leaves it undefined there), NaN goes to -2^30. */

struct MomentumBead
{
   const double *vx, *vy, *vz, *massv;
   __device__ __forceinline__ void load(int i, int s, double (&v)[4]) const
   {
      const double m = massv[s];
      v[0] = m * vx[i]; v[1] = m * vy[i]; v[2] = m * vz[i]; v[3] = m;
   }
};

/* zdensity_output's constants (zdensity.c:66-81), formed on the host in the reference's operations */
struct ZdParms
{
   int nz, method, wrap;              /* method: 0 impulse, 1 hat; wrap: the box is periodic along z */
   double L;                          /* bbox.z */
   double deltai, scaled_corner;      /* nz / L, corner.z * deltai */
   double half, inv;                  /* lSmearHalf.z, lSmearInv.z */
};
__device__ __forceinline__ int zd_int(double x)      /* (int)x, saturating at +-2^30; NaN: -2^30 */
{
   const double lim = 1073741824.0;
   return x >= lim ? (int)lim : (x > -lim ? (int)x : -(int)lim);
}
__device__ __forceinline__ unsigned zd_label(int ig, int nz) { const unsigned l = (unsigned)ig; return l >= (unsigned)nz ? (unsigned)(nz - 1) : l; }
/* a product that stays a product: with -ffp-contract=fast the back end fuses a multiplication into the addition that uses it
 * whatever the source says; a value that went through an (empty) asm statement is no multiplication to it any more */
__device__ __forceinline__ double zd_rounded(double x) { asm volatile("" : "+v"(x)); return x; }
/* r.z of zdensity.c:90 from the slot's z */
__device__ __forceinline__ double zd_t(const ZdParms &zp, double z)
{
   const double a = zd_rounded(export_coord(z, zp.L, zp.wrap) * zp.deltai);
   return a - zp.scaled_corner;
}
/* zdensity.c:105-133: the two bins and weights of a smeared bead */
__device__ __forceinline__ void zd_smear(const ZdParms &zp, double t, unsigned label[2], double w[2])
{
   const double fl = floor(t + 0.5);
   double delta = fl - t;
   delta = delta < zp.half ? delta : zp.half;
   delta = delta > -zp.half ? delta : -zp.half;
   const int iw = zd_int(fl);
   int ig0 = iw - 1, ig1 = iw;
   if (ig0 == -1) ig0 = zp.nz - 1;
   if (ig1 == zp.nz) ig1 = 0;
   if (zp.method == 1)
   {
      const double a = (2 * delta) * zp.inv, b = zd_rounded(fabs(delta) * zp.inv), c = 1.0 - b, d = zd_rounded(a * c);
      w[0] = 0.5 + d;
   }
   else
   {
      const double a = zd_rounded(delta * zp.inv);
      w[0] = 0.5 + a;
   }
   w[1] = 1.0 - w[0];
   label[0] = zd_label(ig0, zp.nz); label[1] = zd_label(ig1, zp.nz);
}
template <bool SMEAR>
__global__ __launch_bounds__(CENSUS_THREADS) void k_census_zdensity(int n, int per_wg, ZdParms zp, const double4 *__restrict__ pos, void *__restrict__ part_)
{
   extern __shared__ double census_s[];      /* SMEAR: double [CENSUS_WAVES][nz]; otherwise unsigned [nz] */
   unsigned *cnt_s = (unsigned *)census_s;
   const int nz = zp.nz;
   if (SMEAR) for (int k = threadIdx.x; k < CENSUS_WAVES * nz; k += CENSUS_THREADS) census_s[k] = 0.0;
   else for (int k = threadIdx.x; k < nz; k += CENSUS_THREADS) cnt_s[k] = 0u;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * nz;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int i = base + (int)threadIdx.x;
      const bool have = i < end;
      unsigned label[2] = {0u, 0u};
      double w[2] = {0.0, 0.0};
      if (have)
      {
         const double t = zd_t(zp, pos[i].z);
         if (SMEAR) zd_smear(zp, t, label, w);
         else label[0] = zd_label(zd_int(t), nz);
      }
#pragma unroll
      for (int kk = 0; kk < (SMEAR ? 2 : 1); kk++)
         wave_for_each_key(__ballot(have && (!SMEAR || !(w[kk] < 1e-20))), (int)label[kk], [&](int k, bool lead, bool mine, unsigned long long same) {
            if (SMEAR)
            {
               const double sw = wave_sum_dpp(mine ? w[kk] : 0.0);
               if (lead) row[k] += sw;
            }
            else if (lead) atomicAdd(&cnt_s[k], (unsigned)__popcll(same));      /* (integers: the order of the waves does not matter) */
         });
   }
   __syncthreads();
   if (SMEAR) census_rows_to_part<RowsSum>(census_s, nz, (double *)part_);
   else
   {
      unsigned *out = (unsigned *)part_ + (size_t)blockIdx.x * nz;
      for (int k = threadIdx.x; k < nz; k += CENSUS_THREADS) out[k] = cnt_s[k];
   }
}

/* ---- host side ---------------------------------------------------------- */
static int census_momentum_check(ddcmi_ctx *ctx, const char *fn, int ngroup, int nspecies, const void *mv, const void *m)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, ngroup != ctx->ngroup, "%s: ngroup = %d, the context has %d groups", fn, ngroup, ctx->ngroup);
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, !mv || !m, "%s: NULL output array (mv %p, m %p)", fn, mv, m);
   if (1 + ngroup + nspecies > census_max_class(4)) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d classes, at most %d", fn, 1 + ngroup + nspecies, census_max_class(4));
   return DDCMI_OK;
}
static int census_zdensity_check(ddcmi_ctx *ctx, const char *fn, int nz, int smear_method, const void *density)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, !density, "%s: NULL output array", fn);
   ARGCHK(ctx, nz < 1, "%s: nz = %d", fn, nz);
   ARGCHK(ctx, smear_method != 0 && smear_method != 1, "%s: smear_method = %d (0 impulse, 1 hat)", fn, smear_method);
   if (nz > CENSUS_MAX_NZ) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: nz = %d, at most %d", fn, nz, CENSUS_MAX_NZ);
   return census_box_check(ctx, fn, 4);
}
/* this rank's sums [sync] */
static int census_momentum_one(ddcmi_ctx *ctx, double *mv, double *m)
{
   const MomentumBead bead = {ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->d_mass.p};
   std::vector<double> h;
   int rc = class_sums_one<4>(ctx, CENSUS_MAX_WG, bead, h);
   if (rc) return rc;
   for (size_t c = 0; c < h.size() / 4; c++) { mv[3 * c] = h[4 * c]; mv[3 * c + 1] = h[4 * c + 1]; mv[3 * c + 2] = h[4 * c + 2]; m[c] = h[4 * c + 3]; }
   return DDCMI_OK;
}
static int census_zdensity_one(ddcmi_ctx *ctx, int nz, double smear_radius, int smear_method, double *density)
{
   (void)hipSetDevice(ctx->device);
   const int n = ctx->nloc;
   if (n <= 0) { for (int k = 0; k < nz; k++) density[k] = 0.0; return DDCMI_OK; }      /* (a domain that holds no bead) */
   const bool smear = smear_radius > 0.0;
   ZdParms zp;
   zp.nz = nz; zp.method = smear_method; zp.wrap = (ctx->pbc >> 2) & 1;
   const double L = zp.L = ctx->h[8];
   const double corner = ctx->h[8] * -0.5;      /* box->corner = h0 * reducedcorner (box.c:69), reducedcorner = -0.5 on this path */
   zp.deltai = nz / L;
   zp.scaled_corner = corner * zp.deltai;
   zp.half = zp.inv = 0.0;
   if (smear)
   {
      const double a = 2.0 * smear_radius, b = L / (1.0 * nz), lSmear = a < b ? a : b;
      zp.inv = 1.0 / lSmear; zp.half = 0.5 * lSmear;
   }
   int per_wg, nwg;
   census_split(n, CENSUS_MAX_WG, &per_wg, &nwg);
   CensusScratch cs;      /* (the counts' 32-bit partials take half of the room) */
   const int part = cs.seg(8, (size_t)nwg * nz), out = cs.seg(8, nz);
   int rc = cs.ensure(ctx);
   if (rc) return rc;
   double *d_part = cs.at<double>(part), *d_out = cs.at<double>(out);
   if (smear)
      hipLaunchKernelGGL(k_census_zdensity<true>, dim3(nwg), dim3(CENSUS_THREADS), (size_t)CENSUS_WAVES * nz * sizeof(double), ctx->stream, n, per_wg, zp, ctx->pos.p, (void *)d_part);
   else
      hipLaunchKernelGGL(k_census_zdensity<false>, dim3(nwg), dim3(CENSUS_THREADS), (size_t)nz * sizeof(unsigned), ctx->stream, n, per_wg, zp, ctx->pos.p, (void *)d_part);
   return census_finish<RowsSum, double>(ctx, nwg, smear ? nz : 0, d_part, d_out, density, smear ? 0 : nz, (const unsigned *)d_part, d_out, density);
}

extern "C" int ddcmi_momentum_by_class(ddcmi_ctx *ctx, int ngroup, int nspecies, double *mv, double *m)
{
   return analysis_single(ctx, "momentum_by_class", true, [=](ddcmi_ctx *c, const char *fn) { return census_momentum_check(c, fn, ngroup, nspecies, mv, m); },
                          [=](ddcmi_ctx *c) { return census_momentum_one(c, mv, m); });
}
extern "C" int ddcmi_zdensity(ddcmi_ctx *ctx, int nz, double smear_radius, int smear_method, double *density)
{
   return analysis_single(ctx, "zdensity", true, [=](ddcmi_ctx *c, const char *fn) { return census_zdensity_check(c, fn, nz, smear_method, density); },
                          [=](ddcmi_ctx *c) { return census_zdensity_one(c, nz, smear_radius, smear_method, density); });
}

/* in-process group: per-rank blocks, rank after rank (mv[r * 3 nclass ...], m[r * nclass ...]; density[r * nz ...]) */
extern "C" int ddcmi_group_momentum_by_class(ddcmi_ctx **ctxs, int n, int ngroup, int nspecies, double *mv, double *m)
{
   const size_t nclass = (size_t)1 + ngroup + nspecies;
   return analysis_group(ctxs, n, "momentum_by_class", [=](ddcmi_ctx *c, const char *fn) { return census_momentum_check(c, fn, ngroup, nspecies, mv, m); },
                         [=](ddcmi_ctx *c, size_t r) { return census_momentum_one(c, mv + r * 3 * nclass, m + r * nclass); });
}
extern "C" int ddcmi_group_zdensity(ddcmi_ctx **ctxs, int n, int nz, double smear_radius, int smear_method, double *density)
{
   return analysis_group(ctxs, n, "zdensity", [=](ddcmi_ctx *c, const char *fn) { return census_zdensity_check(c, fn, nz, smear_method, density); },
                         [=](ddcmi_ctx *c, size_t r) { return census_zdensity_one(c, nz, smear_radius, smear_method, density + r * (size_t)nz); });
}

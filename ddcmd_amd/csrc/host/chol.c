/* chol.c -- ANALYSIS cholAnalysis, the host's share: the molecules whose seven beads are owned by more than one rank.  The device
 * pass (ddcmi_chol_offsets) returns their beads as fragments {mol, role, r}; the caller concatenates the ranks' fragments in rank
 * order and hands them here, where every molecule that is whole after the merge gets the device lane's arithmetic (chol_math.h,
 * this file compiled with -ffp-contract=off) and is folded into the merged counts and statistics in ascending molecule order. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chol.h"

#define CHOL_FN static inline
#define CHOL_RND(x) (x)
#include "chol_math.h"

int ddcmi_chol_complete(int64_t nfrag, const ddcmi_chol_fragment *frag, int64_t nmol, const uint64_t *gid, const double L[3], int pbc, double rmin,
                        double delta, int nbins, int64_t *counts, int64_t *ndone, double *stats, char *err, size_t errlen)
{
#define CHOL_FAIL(...) do { if (err && errlen) snprintf(err, errlen, __VA_ARGS__); free(idx); free(mask); free(tab); return -1; } while (0)
   int64_t *idx = NULL;         /* molecule -> its row of tab, -1: no fragment */
   unsigned char *mask = NULL;  /* row -> the roles seen */
   double *tab = NULL;          /* row -> r[7][3] */
   if (nfrag < 0 || nmol < 0 || (nfrag > 0 && !frag) || (nmol > 0 && !gid) || !L || !counts || !ndone || !stats)
      CHOL_FAIL("ddcmi_chol_complete: bad argument (nfrag %lld, nmol %lld)", (long long)nfrag, (long long)nmol);
   if (nbins < 1 || !(delta > 0.0) || !isfinite(delta) || !isfinite(rmin))
      CHOL_FAIL("ddcmi_chol_complete: nbins = %d, delta = %g, rmin = %g", nbins, delta, rmin);
   if (nfrag == 0) return 0;
   idx = malloc((size_t)(nmol > 0 ? nmol : 1) * sizeof(int64_t));
   mask = calloc((size_t)nfrag, 1);
   tab = calloc((size_t)nfrag * 21, sizeof(double));
   if (!idx || !mask || !tab) CHOL_FAIL("ddcmi_chol_complete: out of memory");
   for (int64_t m = 0; m < nmol; m++) idx[m] = -1;
   int64_t nrow = 0;
   for (int64_t k = 0; k < nfrag; k++)
   {
      const int64_t m = frag[k].mol;
      const int role = frag[k].role;
      if (m < 0 || m >= nmol || role < 0 || role > 6) CHOL_FAIL("ddcmi_chol_complete: fragment %lld names molecule %lld, role %d", (long long)k, (long long)m, role);
      if (idx[m] < 0) idx[m] = nrow++;
      const int64_t row = idx[m];
      if (mask[row] >> role & 1)
         CHOL_FAIL("ddcmi_chol_complete: molecule %lld: gid %llu (role %d) came from two ranks", (long long)m, (unsigned long long)gid[7 * m + role], role);
      mask[row] |= (unsigned char)(1 << role);
      memcpy(tab + 21 * row + 3 * role, frag[k].r, 3 * sizeof(double));
   }
   for (int64_t m = 0; m < nmol; m++)      /* every refusal ahead of the first change */
   {
      if (idx[m] < 0 || mask[idx[m]] == 0x7f) continue;
      int role = 0;
      while (mask[idx[m]] >> role & 1) role++;
      CHOL_FAIL("ddcmi_chol_complete: molecule %lld: gid %llu (role %d) is owned by no rank", (long long)m, (unsigned long long)gid[7 * m + role], role);
   }
   double invL[3];
   for (int a = 0; a < 3; a++) invL[a] = 1.0 / L[a];
   for (int64_t m = 0; m < nmol; m++)
   {
      if (idx[m] < 0) continue;
      double d[2];
      chol_offsets_of(L, invL, pbc, tab + 21 * idx[m], &d[0], &d[1]);
      for (int q = 0; q < 2; q++)
      {
         counts[(size_t)q * nbins + chol_bin(d[q], rmin, delta, nbins)]++;
         stats[3 * q] += d[q];
         if (d[q] < stats[3 * q + 1]) stats[3 * q + 1] = d[q];
         if (d[q] > stats[3 * q + 2]) stats[3 * q + 2] = d[q];
      }
      ++*ndone;
   }
   free(idx); free(mask); free(tab);
   return 0;
#undef CHOL_FAIL
}

/* one molecule whole on the host: the lane's dR1, dR5 and bins (tests, and a caller that holds the positions anyway) */
void ddcmi_chol_molecule(const double r[21], const double L[3], int pbc, double rmin, double delta, int nbins, double d[2], int bin[2])
{
   double invL[3];
   for (int a = 0; a < 3; a++) invL[a] = 1.0 / L[a];
   chol_offsets_of(L, invL, pbc, r, &d[0], &d[1]);
   if (bin) { bin[0] = chol_bin(d[0], rmin, delta, nbins); bin[1] = chol_bin(d[1], rmin, delta, nbins); }
}

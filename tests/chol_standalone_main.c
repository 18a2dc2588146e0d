/* A stand-alone program around the host completion of split cholesterol molecules (ddcmd_amd/csrc/host/chol.c), built by
 * tests/test_chol_host.py with -fsanitize=address,undefined and run as its own process.  Three molecules: 0 whole from two "ranks"
 * (4 + 3 fragments), 1 whole from seven, 2 untouched; then the refusals: a missing bead, a bead given twice, a fragment outside the
 * list.  Prints what the test reads; exits 0 when every call behaved. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "chol.h"

int main(void)
{
   const double L[3] = {90.0, 100.0, 110.0};
   const int nbins = 32;
   const double rmin = -4.0, delta = 0.25;
   /* B = (4,0,0), C = (0,2,0), A = (1,0.5,h1); E = (0,0,-4), F = (2,0,0), D = (0.5,h5,1): dR1 = h1, dR5 = h5 exactly */
   const double h1[2] = {0.5, -44.0 + 45.0 - 2.5}, h5[2] = {-0.25, 3.0};
   uint64_t gid[21];
   ddcmi_chol_fragment *frag = malloc(14 * sizeof(*frag));
   int nf = 0;
   for (int m = 0; m < 3; m++) for (int k = 0; k < 7; k++) gid[7 * m + k] = 1000u * (unsigned)(m + 1) + (unsigned)k;
   for (int pass = 0; pass < 2; pass++)      /* "rank" 0 holds roles 0..3 of molecule 0, "rank" 1 the rest */
      for (int m = 0; m < 2; m++)
      {
         const double r0[3] = {m ? 44.0 : -8.0, 4.0, -8.0};      /* molecule 1 reaches across the +x face: its beads at x > 45 are wrapped */
         double r[7][3] = {{0, 0, 0}, {1, 0.5, h1[m]}, {4, 0, 0}, {0, 2, 0}, {0, 2, 4}, {0.5, 2 + h5[m], 5}, {2, 2, 4}};
         for (int k = 0; k < 7; k++)
         {
            if (m == 0 ? (pass == 0) != (k < 4) : pass == 0) continue;
            frag[nf].mol = m; frag[nf].role = k;
            for (int a = 0; a < 3; a++) frag[nf].r[a] = r0[a] + r[k][a];
            if (frag[nf].r[0] > 45.0) frag[nf].r[0] -= 90.0;
            nf++;
         }
      }
   int64_t counts[64], ndone = 5;
   double stats[6] = {1.0, -3.0, 3.5, 2.0, -3.5, 2.5};
   char err[256] = "";
   memset(counts, 0, sizeof counts);
   int rc = ddcmi_chol_complete(nf, frag, 3, gid, L, 7, rmin, delta, nbins, counts, &ndone, stats, err, sizeof err);
   printf("rc %d nfrag %d ndone %lld\n", rc, nf, (long long)ndone);
   for (int k = 0; k < 64; k++) if (counts[k]) printf("count %d %lld\n", k, (long long)counts[k]);
   printf("stats %.17g %.17g %.17g %.17g %.17g %.17g\n", stats[0], stats[1], stats[2], stats[3], stats[4], stats[5]);
   int bad = rc != 0 || ndone != 7;
   /* the refusals change nothing */
   int64_t c2[64], n2 = 0;
   double s2[6] = {0, 1e300, -1e300, 0, 1e300, -1e300};
   memset(c2, 0, sizeof c2);
   rc = ddcmi_chol_complete(nf - 1, frag, 3, gid, L, 7, rmin, delta, nbins, c2, &n2, s2, err, sizeof err);
   printf("missing: rc %d: %s\n", rc, err);
   bad |= rc == 0 || n2 != 0 || s2[0] != 0.0;
   frag[nf - 1] = frag[0];
   rc = ddcmi_chol_complete(nf, frag, 3, gid, L, 7, rmin, delta, nbins, c2, &n2, s2, err, sizeof err);
   printf("twice: rc %d: %s\n", rc, err);
   bad |= rc == 0 || n2 != 0;
   frag[0].mol = 3;
   rc = ddcmi_chol_complete(nf, frag, 3, gid, L, 7, rmin, delta, nbins, c2, &n2, s2, err, sizeof err);
   printf("outside: rc %d: %s\n", rc, err);
   bad |= rc == 0 || n2 != 0;
   rc = ddcmi_chol_complete(0, NULL, 0, NULL, L, 7, rmin, delta, nbins, c2, &n2, s2, err, sizeof err);
   printf("empty: rc %d\n", rc);
   bad |= rc != 0;
   for (int k = 0; k < 64; k++) bad |= c2[k] != 0;
   free(frag);
   return bad;
}

/* ddcmi_kdist.inl -- ANALYSIS type KINETICENERGYDISTN on the device (kineticEnergyDistn.c:157-188, kineticEnergyDistn_eval): the
 * histogram of the beads' kinetic energies, one histogram ("group") per chosen species, all groups in one read-only pass over the
 * owned beads: a census pass (ddcmi_census_frame.inl) over the velocities and the mass ctx->d_mass[species] that the momentum pass
 * reads.  Included from ddcmi.hip behind ddcmi_census.inl.  The caller combines the ranks' results: counts and sums added, minimum
 * of minima, maximum of maxima.
 *
 * Per bead whose species has a group g (species_dist[species] >= 0), the reference's statements in its operations:
 *    v2 = (vx*vx + vy*vy) + vz*vz;  K = (0.5*mass)*v2;                     every product kept from contraction into an FMA (zd_rounded)
 *    sum[g] += K; cntTotal[g]++; max[g], min[g] follow K (they start at 0.0 and 1e300: `K > max`, `K < min`)
 *    K < emin: subCnt[g]++;  K >= emax: supCnt[g]++;  otherwise cnt[g][(int)((K - emin)/delta)]++   a correctly rounded division
 * What the reference leaves to an assert is defined here:
 *    (K - emin)/delta truncates to nbins for a K just below emax (the quotient rounds up to nbins): the bead goes to bin nbins - 1.
 *    K is NaN: the bead is counted in cntTotal and joins the sum (which becomes NaN), as the reference's statements in front of the
 *       assert would have it; it enters no bin, neither outer count and neither extreme (every comparison with it is false).
 *    K is +inf: a supCnt (inf >= emax); it joins the sum and is the maximum.
 * A group that met no bead returns 0 counts, sum 0, and the initial extremes 1e300 and 0.0.
 *
 * Shape (k_census_kdist).  Slots: the bins of all groups one after the other (off[g] + ibin), then three tallies per group
 * (nbt + 3 g + {0 cntTotal, 1 subCnt, 2 supCnt}); one row of 32-bit integers per workgroup in LDS.  A bead has two keys: its
 * group's cntTotal slot, and its bin or outer tally (none for a NaN); both are counted as in k_census_zdensity<false>.
 * With the first key go the doubles: the sum of the K of those lanes (the other lanes at zero), their minimum and maximum
 * (wave_reduce_dpp with a comparison; the other lanes at 1e300 and 0.0), which the lead lane puts into its wave's own LDS row
 * {sum, min, max} of the group.  Rows and workgroups combine by RowsSumMinMax.
 *
 * The cap.  LDS per workgroup: 4 B per slot and CENSUS_WAVES x 3 x 8 B = 96 B per group of per-wave rows, i.e.
 *    DDCMI_KDIST_LDS_BYTES(ndist, nbt) = 4 (nbt + 3 ndist) + 96 ndist <= DDCMI_KDIST_MAX_LDS = 64 KB
 * (the 64 KB every census kernel stays within): 16357 bins for one group, 16114 in all for ten, 8192 and more for up to 303 groups. */

struct KdGroup { double emin, emax, delta; int nbins, off; };

/* part_d: [nwg][ndist][3] doubles {sum, min, max}; part_c: [nwg][nbt + 3 ndist] 32-bit counts */
__global__ __launch_bounds__(CENSUS_THREADS) void k_census_kdist(int n, int per_wg, int nspecies, int ndist, int nbt, const double *__restrict__ vx,
                                                                 const double *__restrict__ vy, const double *__restrict__ vz, const int *__restrict__ species,
                                                                 const double *__restrict__ massv, const KdGroup *__restrict__ grp, const int *__restrict__ species_dist,
                                                                 double *__restrict__ part_d, unsigned *__restrict__ part_c)
{
   extern __shared__ double census_s[];      /* double [CENSUS_WAVES][ndist][3], then unsigned [nbt + 3 ndist] */
   const int nd3 = 3 * ndist, nslot = nbt + nd3;
   unsigned *cnt_s = (unsigned *)(census_s + (size_t)CENSUS_WAVES * nd3);
   for (int k = threadIdx.x; k < CENSUS_WAVES * nd3; k += CENSUS_THREADS) { const int q = k % 3; census_s[k] = q == 1 ? 1e300 : 0.0; }
   for (int k = threadIdx.x; k < nslot; k += CENSUS_THREADS) cnt_s[k] = 0u;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * nd3;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int i = base + (int)threadIdx.x;
      int g = -1, slot = -1;
      double K = 0.0;
      if (i < end)
      {
         const int s = min(max(species[i], 0), nspecies - 1);      /* (checked at the upload: the reads stay in bounds whatever the array holds) */
         g = species_dist[s];
         if (g >= 0)
         {
            const KdGroup G = grp[g];
            const double x = vx[i], y = vy[i], z = vz[i];
            const double xx = zd_rounded(x * x), yy = zd_rounded(y * y), zz = zd_rounded(z * z);
            const double v2 = (xx + yy) + zz;
            K = zd_rounded((0.5 * massv[s]) * v2);
            if (K < G.emin) slot = nbt + 3 * g + 1;
            else if (K >= G.emax) slot = nbt + 3 * g + 2;
            else if (K == K)
            {
               const int ibin = (int)((K - G.emin) / G.delta);      /* 0 <= quotient <= nbins (1 + 2^-52): no overflow */
               slot = G.off + min(max(ibin, 0), G.nbins - 1);
            }
         }
      }
      /* first key: the group -- cntTotal, and the doubles */
      wave_for_each_key(__ballot(g >= 0), g, [&](int k, bool lead, bool mine, unsigned long long same) {
         const bool ext = mine && K == K;      /* a NaN enters neither extreme */
         const double sk = wave_sum_dpp(mine ? K : 0.0), mn = wave_reduce_dpp<WaveMin>(ext ? K : 1e300), mx = wave_reduce_dpp<WaveMax>(ext ? K : 0.0);
         if (lead)
         {
            atomicAdd(&cnt_s[nbt + 3 * k], (unsigned)__popcll(same));      /* (integers: the order of the waves does not matter) */
            double *r = row + 3 * k;
            r[0] += sk;
            if (mn < r[1]) r[1] = mn;
            if (mx > r[2]) r[2] = mx;
         }
      });
      /* second key: the bin, or the outer tally */
      wave_for_each_key(__ballot(slot >= 0), slot, [&](int k, bool lead, bool, unsigned long long same) {
         if (lead) atomicAdd(&cnt_s[k], (unsigned)__popcll(same));
      });
   }
   __syncthreads();
   census_rows_to_part<RowsSumMinMax>(census_s, nd3, part_d);
   unsigned *out_c = part_c + (size_t)blockIdx.x * nslot;
   for (int k = threadIdx.x; k < nslot; k += CENSUS_THREADS) out_c[k] = cnt_s[k];
}

/* ---- host side ---------------------------------------------------------- */
static int census_kdist_check(ddcmi_ctx *ctx, const char *fn, int nspecies, int ndist, const double *emin, const double *emax, const int *nbins,
                              const int *species_dist, const void *counts, const void *tallies, const void *stats)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, ndist < 0, "%s: ndist = %d", fn, ndist);
   ARGCHK(ctx, !species_dist, "%s: NULL species_dist", fn);
   ARGCHK(ctx, ndist > 0 && (!emin || !emax || !nbins), "%s: NULL input array (emin %p, emax %p, nbins %p)", fn, (const void *)emin, (const void *)emax, (const void *)nbins);
   ARGCHK(ctx, ndist > 0 && (!counts || !tallies || !stats), "%s: NULL output array (counts %p, tallies %p, stats %p)", fn, counts, tallies, stats);
   long nbt = 0;
   for (int g = 0; g < ndist; g++)
   {
      ARGCHK(ctx, nbins[g] < 1, "%s: nbins[%d] = %d", fn, g, nbins[g]);
      ARGCHK(ctx, !std::isfinite(emin[g]) || !std::isfinite(emax[g]), "%s: emin[%d] = %g, emax[%d] = %g: not finite", fn, g, emin[g], g, emax[g]);
      ARGCHK(ctx, !(emax[g] > emin[g]), "%s: emax[%d] = %g <= emin[%d] = %g", fn, g, emax[g], g, emin[g]);
      nbt += nbins[g];
   }
   for (int s = 0; s < nspecies; s++)
      ARGCHK(ctx, species_dist[s] < -1 || species_dist[s] >= ndist, "%s: species_dist[%d] = %d, outside [-1, %d)", fn, s, species_dist[s], ndist);
   if (DDCMI_KDIST_LDS_BYTES((long)ndist, nbt) > DDCMI_KDIST_MAX_LDS)
      SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %ld bins in %d groups need %ld bytes of LDS, at most %d (4 per bin, 108 per group)", fn, nbt, ndist,
             DDCMI_KDIST_LDS_BYTES((long)ndist, nbt), DDCMI_KDIST_MAX_LDS);
   return DDCMI_OK;
}
/* this rank's result [sync] */
static int census_kdist_one(ddcmi_ctx *ctx, int ndist, const double *emin, const double *emax, const int *nbins, const int *species_dist,
                            int64_t *counts, int64_t *tallies, double *stats)
{
   if (ndist == 0) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, ns = ctx->nspecies, nd3 = 3 * ndist;
   std::vector<KdGroup> grp((size_t)ndist);
   int nbt = 0;
   for (int g = 0; g < ndist; g++)
   {
      grp[g].emin = emin[g]; grp[g].emax = emax[g]; grp[g].nbins = nbins[g]; grp[g].off = nbt;
      grp[g].delta = (emax[g] - emin[g]) / nbins[g];      /* kineticEnergyDistn.c:67 */
      nbt += nbins[g];
   }
   if (n <= 0)      /* (a domain that holds no bead) */
   {
      for (int k = 0; k < nbt; k++) counts[k] = 0;
      for (int g = 0; g < ndist; g++) { tallies[3 * g] = tallies[3 * g + 1] = tallies[3 * g + 2] = 0; stats[3 * g] = 0.0; stats[3 * g + 1] = 1e300; stats[3 * g + 2] = 0.0; }
      return DDCMI_OK;
   }
   const int nslot = nbt + nd3;
   int per_wg, nwg;
   census_split(n, CENSUS_MAX_WG, &per_wg, &nwg);
   CensusScratch cs;
   const int s_grp = cs.seg(sizeof(KdGroup), ndist), s_map = cs.seg(4, ns), s_pd = cs.seg(8, (size_t)nwg * nd3), s_od = cs.seg(8, nd3), s_oc = cs.seg(8, nslot),
             s_pc = cs.seg(4, (size_t)nwg * nslot);
   int rc = cs.ensure(ctx);
   if (rc) return rc;
   HIPCHK(ctx, hipMemcpyAsync(cs.at<KdGroup>(s_grp), grp.data(), (size_t)ndist * sizeof(KdGroup), hipMemcpyHostToDevice, st));
   HIPCHK(ctx, hipMemcpyAsync(cs.at<int>(s_map), species_dist, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, st));
   const size_t lds = (size_t)DDCMI_KDIST_LDS_BYTES(ndist, nbt);
   hipLaunchKernelGGL(k_census_kdist, dim3(nwg), dim3(CENSUS_THREADS), lds, st, n, per_wg, ns, ndist, nbt, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->species.p,
                      ctx->d_mass.p, cs.at<KdGroup>(s_grp), cs.at<int>(s_map), cs.at<double>(s_pd), cs.at<unsigned>(s_pc));
   std::vector<long long> hc((size_t)nslot);      /* counts | tallies: two arrays of the caller's */
   if ((rc = census_finish<RowsSumMinMax, long long>(ctx, nwg, nd3, cs.at<double>(s_pd), cs.at<double>(s_od), stats, nslot, cs.at<unsigned>(s_pc),
                                                      cs.at<long long>(s_oc), hc.data()))) return rc;
   for (int k = 0; k < nbt; k++) counts[k] = hc[k];
   for (int k = 0; k < nd3; k++) tallies[k] = hc[(size_t)nbt + k];
   return DDCMI_OK;
}

extern "C" int ddcmi_kinetic_energy_distn(ddcmi_ctx *ctx, int nspecies, int ndist, const double *emin, const double *emax, const int *nbins,
                                          const int *species_dist, int64_t *counts, int64_t *tallies, double *stats)
{
   return analysis_single(ctx, "kinetic_energy_distn", true,
                          [=](ddcmi_ctx *c, const char *fn) { return census_kdist_check(c, fn, nspecies, ndist, emin, emax, nbins, species_dist, counts, tallies, stats); },
                          [=](ddcmi_ctx *c) { return census_kdist_one(c, ndist, emin, emax, nbins, species_dist, counts, tallies, stats); });
}
/* in-process group: per-rank blocks, rank after rank (counts[r * nbt ...], tallies[r * 3 ndist ...], stats[r * 3 ndist ...]) */
extern "C" int ddcmi_group_kinetic_energy_distn(ddcmi_ctx **ctxs, int n, int nspecies, int ndist, const double *emin, const double *emax, const int *nbins,
                                                const int *species_dist, int64_t *counts, int64_t *tallies, double *stats)
{
   return analysis_group(ctxs, n, "kinetic_energy_distn",
                         [=](ddcmi_ctx *c, const char *fn) { return census_kdist_check(c, fn, nspecies, ndist, emin, emax, nbins, species_dist, counts, tallies, stats); },
                         [=](ddcmi_ctx *c, size_t r) {
                            size_t nbt = 0;      /* (the checks have seen nbins by now) */
                            for (int k = 0; k < ndist; k++) nbt += (size_t)nbins[k];
                            return census_kdist_one(c, ndist, emin, emax, nbins, species_dist, counts + r * nbt, tallies + r * 3 * (size_t)ndist, stats + r * 3 * (size_t)ndist);
                         });
}

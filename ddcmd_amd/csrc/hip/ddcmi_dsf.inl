/* ddcmi_dsf.inl -- ANALYSIS type DSF / DynamicStructureFactor on the device (dsf.c:127-217, dsf_eval): the charge-density modes
 *    rho[a][m - 1] = sum over the owned, selected beads j of q_j c_{a,j}^m,   c_{a,j} = exp(i 2 pi r_{a,j} / L_a),   m = 1 .. mmax
 * on the three axes of an orthorhombic box, all of them in one launch of a census pass (ddcmi_census_frame.inl) over the positions
 * and the charge ctx->d_charge_sp[species] of ddcmi_set_species.  Included from ddcmi.hip behind ddcmi_kdist.inl.  The caller adds
 * the ranks' sums and counts and divides by the global count (dsf.c:207-212).
 *
 * Per bead.  The position is the one ddcmi_download_state hands out (census_coord), without a further wrap.  The phase needs none: with t = r / L (one correctly
 * rounded division) the turn count t - rint(t) is exact, |t| <= 1/2 from there on, and sincospi takes 2 m t without ever
 * multiplying by a rounded pi.  A bead outside the box therefore costs its own u |t| of the division and nothing more.
 *
 * Shape (k_census_dsf<C>).  6 mmax sums do not fit in registers, so the modes go in chunks of C = DSF_CHUNK: for the chunk that
 * begins at m0 every lane walks the workgroup's range once more, starts a bead at c^m0 (m0 = 1: c itself; otherwise one sincospi of
 * 2 (m0 t) per axis), adds q c^m into its 6 C private sums and steps to c^(m + 1) by a complex multiplication.  After the range the
 * 6 C sums are reduced over the wave (wave_sum_dpp: the same tree every time) and lane 0 stores them in the wave's LDS row; the
 * rows, the workgroups and the 32-bit counts combine as in every census pass (census_rows_to_part<RowsSum>, k_census_final).
 * Selection is a per-lane predicate: a bead whose species is not selected adds nothing, and the count is the popcount of the
 * ballot, taken in the first chunk.
 *
 * The cap.  CENSUS_WAVES rows of 6 mmax doubles: 192 mmax bytes of LDS, 48 KB at DDCMI_DSF_MAX_M = 256 (the 64 KB every census
 * kernel stays within would admit 341). */

#define DSF_CHUNK 8

struct DsfParms { double L[3]; int pbc, mmax; };

/* part_d: [nwg][3][mmax][2] doubles; part_c: [nwg] 32-bit counts */
template <int C>
__global__ __launch_bounds__(CENSUS_THREADS) void k_census_dsf(int n, int per_wg, int nspecies, DsfParms dp, const double4 *__restrict__ pos,
                                                               const int *__restrict__ species, const double *__restrict__ charge,
                                                               const int *__restrict__ select, double *__restrict__ part_d, unsigned *__restrict__ part_c)
{
   extern __shared__ double census_s[];      /* double [CENSUS_WAVES][3][mmax][2], then one unsigned */
   const int mmax = dp.mmax, nval = 6 * mmax;
   unsigned *cnt_s = (unsigned *)(census_s + (size_t)CENSUS_WAVES * nval);
   for (int k = threadIdx.x; k < CENSUS_WAVES * nval; k += CENSUS_THREADS) census_s[k] = 0.0;
   if (threadIdx.x == 0) cnt_s[0] = 0u;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * nval;
   const int lane = threadIdx.x & 63;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int m0 = 1; m0 <= mmax; m0 += C)      /* (uniform: every lane reaches the wave operations) */
   {
      double acc[3][C][2];
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
         for (int k = 0; k < C; k++) acc[a][k][0] = acc[a][k][1] = 0.0;
      for (int base = beg; base < end; base += CENSUS_THREADS)
      {
         const int i = base + (int)threadIdx.x;
         bool sel = false;
         int s = 0;
         if (i < end)
         {
            s = min(max(species[i], 0), nspecies - 1);      /* (checked at the upload: the reads stay in bounds whatever the array holds) */
            sel = select[s] != 0;
         }
         if (m0 == 1)
         {
            const unsigned long long same = __ballot(sel);
            if (lane == 0 && same) atomicAdd(&cnt_s[0], (unsigned)__popcll(same));      /* (integers: the order of the waves does not matter) */
         }
         if (sel)
         {
            const double q = charge[s];
            const double4 p4 = pos[i];
            const double r[3] = {p4.x, p4.y, p4.z};
#pragma unroll
            for (int a = 0; a < 3; a++)
            {
               double t = census_coord(dp, a, r[a]) / dp.L[a];
               t -= rint(t);      /* exact */
               double cs, cc, ps, pc;
               sincospi(2.0 * t, &cs, &cc);
               if (m0 == 1) { ps = cs; pc = cc; }
               else sincospi(2.0 * ((double)m0 * t), &ps, &pc);
#pragma unroll
               for (int k = 0; k < C; k++)
               {
                  acc[a][k][0] += q * pc;
                  acc[a][k][1] += q * ps;
                  if (k + 1 < C)
                  {
                     const double nc = pc * cc - ps * cs, ns = pc * cs + ps * cc;
                     pc = nc; ps = ns;
                  }
               }
            }
         }
      }
#pragma unroll
      for (int a = 0; a < 3; a++)
#pragma unroll
         for (int k = 0; k < C; k++)
         {
            const double re = wave_sum_dpp(acc[a][k][0]), im = wave_sum_dpp(acc[a][k][1]);
            if (lane == 0 && m0 + k <= mmax)
            {
               double *o = row + 2 * ((size_t)a * mmax + (m0 - 1 + k));
               o[0] = re; o[1] = im;
            }
         }
   }
   __syncthreads();
   census_rows_to_part<RowsSum>(census_s, nval, part_d);
   if (threadIdx.x == 0) part_c[blockIdx.x] = cnt_s[0];
}

/* ---- host side ---------------------------------------------------------- */
static int census_dsf_check(ddcmi_ctx *ctx, const char *fn, int nspecies, int mmax, const void *rho, const void *count)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, !rho || !count, "%s: NULL output (rho %p, count %p)", fn, rho, count);
   ARGCHK(ctx, mmax < 1, "%s: mmax = %d", fn, mmax);
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, ctx->nspecies < 1, "%s needs the species (ddcmi_set_species)", fn);
   if (mmax > DDCMI_DSF_MAX_M) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: mmax = %d, at most %d", fn, mmax, DDCMI_DSF_MAX_M);
   return census_box_check(ctx, fn, 7);
}
/* this rank's sums and count [sync] */
static int census_dsf_one(ddcmi_ctx *ctx, const int *select, int mmax, double *rho, int64_t *count)
{
   (void)hipSetDevice(ctx->device);
   const int n = ctx->nloc, ns = ctx->nspecies, nval = 6 * mmax;
   if (n <= 0)      /* (a domain that holds no bead) */
   {
      for (int k = 0; k < nval; k++) rho[k] = 0.0;
      *count = 0;
      return DDCMI_OK;
   }
   DsfParms dp;
   census_set_box(ctx, dp); dp.mmax = mmax;
   int per_wg, nwg;
   census_split(n, CENSUS_MAX_WG, &per_wg, &nwg);
   CensusScratch cs;
   const int s_sel = cs.seg(4, ns), s_pd = cs.seg(8, (size_t)nwg * nval), s_od = cs.seg(8, nval), s_oc = cs.seg(8, 1), s_pc = cs.seg(4, nwg);
   int rc = cs.ensure(ctx);
   if (rc) return rc;
   std::vector<int> sel;
   if ((rc = census_upload_select(ctx, select, sel, cs.at<int>(s_sel)))) return rc;
   const size_t lds = (size_t)CENSUS_WAVES * nval * sizeof(double) + sizeof(double);
   hipLaunchKernelGGL(k_census_dsf<DSF_CHUNK>, dim3(nwg), dim3(CENSUS_THREADS), lds, ctx->stream, n, per_wg, ns, dp, ctx->pos.p, ctx->species.p, ctx->d_charge_sp.p,
                      cs.at<int>(s_sel), cs.at<double>(s_pd), cs.at<unsigned>(s_pc));
   return census_finish<RowsSum, long long>(ctx, nwg, nval, cs.at<double>(s_pd), cs.at<double>(s_od), rho, 1, cs.at<unsigned>(s_pc), cs.at<long long>(s_oc),
                                            (long long *)count);
}

extern "C" int ddcmi_charge_density_modes(ddcmi_ctx *ctx, int nspecies, const int *select, int mmax, double *rho, int64_t *count)
{
   return analysis_single(ctx, "charge_density_modes", true, [=](ddcmi_ctx *c, const char *fn) { return census_dsf_check(c, fn, nspecies, mmax, rho, count); },
                          [=](ddcmi_ctx *c) { return census_dsf_one(c, select, mmax, rho, count); });
}
/* in-process group: per-rank blocks, rank after rank (rho[r * 6 mmax ...], count[r]) */
extern "C" int ddcmi_group_charge_density_modes(ddcmi_ctx **ctxs, int n, int nspecies, const int *select, int mmax, double *rho, int64_t *count)
{
   return analysis_group(ctxs, n, "charge_density_modes", [=](ddcmi_ctx *c, const char *fn) { return census_dsf_check(c, fn, nspecies, mmax, rho, count); },
                         [=](ddcmi_ctx *c, size_t r) { return census_dsf_one(c, select, mmax, rho + r * 6 * (size_t)mmax, count + r); });
}

/* ddcmi_ssf.inl -- the sums of ANALYSIS type SSF (ssf.c:91-120) on the device, for any list of integer wave vectors:
 *    rho[l] = sum over the owned, selected beads j of w_j exp(i 2 pi (n_x x_j / L_x + n_y y_j / L_y + n_z z_j / L_z)),   (n_x, n_y, n_z) = kvec[l]
 * in an orthorhombic box, w = 1 (ssf.c) or the species' charge (DSF's weight), as a census pass (ddcmi_census_frame.inl): read-only,
 * no communication, no floating-point atomics, the same bits when repeated.  Included from ddcmi.hip behind ddcmi_dsf.inl.
 *
 * Per bead, as k_census_dsf: the position ddcmi_download_state hands out, t = r / L (one correctly rounded division), t -= rint(t)
 * (exact, |t| <= 1/2).  Per bead and vector: phi = n_x t_x + n_y t_y + n_z t_z in turns (a product and two fused multiply-adds:
 * three roundings), phi -= rint(phi) (exact), one sincospi(2 phi): no rounded pi anywhere.
 *
 * Shape (k_structure_modes).  N n_k sincospi are the work, so lanes own wave vectors and beads are broadcast:
 *   grid.x walks the bead ranges of census_split(n, SM_MAX_WG) -- a function of n alone; grid.y walks tiles of CENSUS_THREADS vectors;
 *   a lane keeps its (n_x, n_y, n_z) as doubles and its private (re, im) in registers;
 *   the workgroup stages its range in blocks of CENSUS_THREADS slots: every lane takes one slot, forms (t_x, t_y, t_z, w) if its
 *      species is selected, and the selected ones are packed in slot order into LDS (rank inside the wave by ballot and popcount,
 *      the waves' counts through LDS); the block's count goes into the workgroup's 32-bit count;
 *   every lane then reads staged bead after staged bead -- one address for the whole wave, an LDS broadcast -- and adds w cos, w sin
 *      into its sums.  No cross-lane reduction: a vector's sum over the range is one lane's chain of additions in slot order;
 *   partials [nwg][nk][2]; k_census_final adds the workgroups in order (and the counts of the tiles' first row of workgroups).
 * A vector's value is therefore a function of (the state, the selection, the weight, the vector) alone: neither its place in the
 * list, nor its neighbours, nor nk enter (the lane it lands on changes nothing, all lanes run the same chain).
 *
 * Caps.  |component| <= DDCMI_SM_MAX_N keeps |phi| < 2^11 so that phi's roundings stay below 2^-42 turns; nk <= DDCMI_SM_MAX_K and
 * SM_MAX_WG workgroups bound the partials by 1024 x 4096 x 16 B = 64 MB. */

#define SM_MAX_WG 1024      /* bead ranges: they decide the order of the additions */

struct SmParms { double L[3]; int pbc, weight; };

/* part_d: [nwg][nk][2] doubles; part_c: [nwg] 32-bit counts (written by the first tile's workgroups) */
__global__ __launch_bounds__(CENSUS_THREADS) void k_structure_modes(int n, int per_wg, int nspecies, int nk, SmParms sp, const double4 *__restrict__ pos,
                                                                    const int *__restrict__ species, const double *__restrict__ charge,
                                                                    const int *__restrict__ select, const int *__restrict__ kvec,
                                                                    double *__restrict__ part_d, unsigned *__restrict__ part_c)
{
   __shared__ double4 bead_s[CENSUS_THREADS];      /* (t_x, t_y, t_z, w) of the block's selected beads, in slot order */
   __shared__ int wcnt_s[CENSUS_WAVES];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const int k = blockIdx.y * CENSUS_THREADS + (int)threadIdx.x;
   double nx = 0.0, ny = 0.0, nz = 0.0;
   if (k < nk) { nx = (double)kvec[3 * k]; ny = (double)kvec[3 * k + 1]; nz = (double)kvec[3 * k + 2]; }
   double re = 0.0, im = 0.0;
   unsigned count = 0u;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform: every lane reaches the barriers) */
   {
      const int i = base + (int)threadIdx.x;
      bool sel = false;
      int s = 0;
      if (i < end)
      {
         s = min(max(species[i], 0), nspecies - 1);      /* (checked at the upload: the reads stay in bounds whatever the array holds) */
         sel = select[s] != 0;
      }
      const unsigned long long same = __ballot(sel);
      if (lane == 0) wcnt_s[wave] = __popcll(same);
      double4 b = make_double4(0.0, 0.0, 0.0, 0.0);
      if (sel)
      {
         const double4 p4 = pos[i];
         double r[3] = {p4.x, p4.y, p4.z}, t[3];
#pragma unroll
         for (int a = 0; a < 3; a++)
         {
            const double L = sp.L[a];
            r[a] = export_coord(r[a], L, sp.pbc >> a & 1);
            t[a] = r[a] / L;
            t[a] -= rint(t[a]);      /* exact */
         }
         b = make_double4(t[0], t[1], t[2], sp.weight ? charge[s] : 1.0);
      }
      __syncthreads();      /* the waves' counts are in; the previous block's beads have been read */
      int off = 0, nsel = 0;
#pragma unroll
      for (int w = 0; w < CENSUS_WAVES; w++) { const int c = wcnt_s[w]; if (w < wave) off += c; nsel += c; }
      if (sel) bead_s[off + __popcll(same & ((1ull << lane) - 1ull))] = b;
      __syncthreads();
      count += (unsigned)nsel;
      if (k < nk)
         for (int j = 0; j < nsel; j++)
         {
            const double4 q = bead_s[j];      /* one address per wave: a broadcast */
            double phi = fma(nz, q.z, fma(ny, q.y, nx * q.x));
            phi -= rint(phi);      /* exact */
            double sn, cs;
            sincospi(2.0 * phi, &sn, &cs);
            re += q.w * cs;
            im += q.w * sn;
         }
   }
   if (k < nk)
   {
      double *o = part_d + 2 * ((size_t)blockIdx.x * nk + k);
      o[0] = re; o[1] = im;
   }
   if (blockIdx.y == 0 && threadIdx.x == 0) part_c[blockIdx.x] = count;
}

/* ---- host side ---------------------------------------------------------- */
static int structure_modes_check(ddcmi_ctx *ctx, const char *fn, int nspecies, int weight, int nk, const int32_t *kvec, const void *rho, const void *count)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, !kvec || !rho || !count, "%s: NULL argument (kvec %p, rho %p, count %p)", fn, (const void *)kvec, rho, count);
   ARGCHK(ctx, nk < 1, "%s: nk = %d", fn, nk);
   ARGCHK(ctx, weight != 0 && weight != 1, "%s: weight = %d, 0 (unit) or 1 (the species' charge)", fn, weight);
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, ctx->nspecies < 1, "%s needs the species (ddcmi_set_species)", fn);
   if (nk > DDCMI_SM_MAX_K) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: nk = %d, at most %d", fn, nk, DDCMI_SM_MAX_K);
   for (int l = 0; l < 3 * nk; l++)
      if (kvec[l] > DDCMI_SM_MAX_N || kvec[l] < -DDCMI_SM_MAX_N)
         SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: kvec[%d][%d] = %d, at most %d in magnitude", fn, l / 3, l % 3, (int)kvec[l], DDCMI_SM_MAX_N);
   return census_box_check(ctx, fn, 7);
}
/* this rank's sums and count [sync] */
static int structure_modes_one(ddcmi_ctx *ctx, const int *select, int weight, int nk, const int32_t *kvec, double *rho, int64_t *count)
{
   (void)hipSetDevice(ctx->device);
   const int n = ctx->nloc, ns = ctx->nspecies, nval = 2 * nk;
   if (n <= 0)      /* (a domain that holds no bead) */
   {
      for (int k = 0; k < nval; k++) rho[k] = 0.0;
      *count = 0;
      return DDCMI_OK;
   }
   SmParms sp;
   census_set_box(ctx, sp); sp.weight = weight;
   int per_wg, nwg;
   census_split(n, SM_MAX_WG, &per_wg, &nwg);
   CensusScratch cs;
   const int s_sel = cs.seg(4, ns), s_kv = cs.seg(4, 3 * (size_t)nk), s_pd = cs.seg(8, (size_t)nwg * nval), s_od = cs.seg(8, nval), s_oc = cs.seg(8, 1),
             s_pc = cs.seg(4, nwg);
   int rc = cs.ensure(ctx);
   if (rc) return rc;
   std::vector<int> sel;
   if ((rc = census_upload_select(ctx, select, sel, cs.at<int>(s_sel)))) return rc;
   HIPCHK(ctx, hipMemcpyAsync(cs.at<int>(s_kv), kvec, 3 * (size_t)nk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
   hipLaunchKernelGGL(k_structure_modes, dim3(nwg, cdiv(nk, CENSUS_THREADS)), dim3(CENSUS_THREADS), 0, ctx->stream, n, per_wg, ns, nk, sp, ctx->pos.p, ctx->species.p,
                      ctx->d_charge_sp.p, cs.at<int>(s_sel), cs.at<int>(s_kv), cs.at<double>(s_pd), cs.at<unsigned>(s_pc));
   return census_finish<RowsSum, long long>(ctx, nwg, nval, cs.at<double>(s_pd), cs.at<double>(s_od), rho, 1, cs.at<unsigned>(s_pc), cs.at<long long>(s_oc),
                                            (long long *)count);
}

extern "C" int ddcmi_structure_modes(ddcmi_ctx *ctx, int nspecies, const int *select, int weight, int nk, const int32_t *kvec, double *rho, int64_t *count)
{
   if (ctx && ctx->group_) SETERR(ctx, DDCMI_EINVAL, "ddcmi_structure_modes: contexts of an in-process group: use ddcmi_group_structure_modes");
   return analysis_single(ctx, "structure_modes", true,
                          [=](ddcmi_ctx *c, const char *fn) { return structure_modes_check(c, fn, nspecies, weight, nk, kvec, rho, count); },
                          [=](ddcmi_ctx *c) { return structure_modes_one(c, select, weight, nk, kvec, rho, count); });
}
/* in-process group: per-rank blocks, rank after rank (rho[r * 2 nk ...], count[r]) */
extern "C" int ddcmi_group_structure_modes(ddcmi_ctx **ctxs, int n, int nspecies, const int *select, int weight, int nk, const int32_t *kvec, double *rho,
                                           int64_t *count)
{
   return analysis_group(ctxs, n, "structure_modes",
                         [=](ddcmi_ctx *c, const char *fn) { return structure_modes_check(c, fn, nspecies, weight, nk, kvec, rho, count); },
                         [=](ddcmi_ctx *c, size_t r) { return structure_modes_one(c, select, weight, nk, kvec, rho + r * 2 * (size_t)nk, count + r); });
}

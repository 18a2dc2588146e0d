/* ddcmi_vaf.inl -- ANALYSIS type VELOCITYAUTOCORRELATION on the device (velocityAutocorrelation.c:117-229,
 * velocityAutocorrelation_eval): sum v0.v and sum d.d over the owned beads, for the system, every group and every species.
 * Included from ddcmi.hip behind the multi-domain path.
 *
 * The reference record (the reference's REF {r, v}, velocityAutocorrelation.c:30, registered with particleRegisterinfo so that it
 * follows its bead): VafRec {v0[3], o[3]} per owned bead in slot order, ctx->vaf, allocated by the first ddcmi_vaf_origin.
 *   v0  the bead's velocity at the time origin.
 *   o   the ORIGIN of its displacement: d = (current position) - o.  The reference adds dt*v to REF.r in every drift loop
 *       (nglf.c:79-86, nglfconstraint.c:537-545); the device keeps positions continuous between rebuilds, so the sum of the drift
 *       moves IS the difference of positions, and no step kernel carries an accumulation.  o is corrected where the library moves
 *       a bead by something that is no drift, by exactly what that moved the bead:
 *         the wrap into the box at a rebuild    k_gather_state, k_mig_classify   o += p_wrapped - p
 *         the barostat's scaling                k_vaf_rescale in front of it      o  = s p - (p - o)
 *       ddcmi_upload_positions (host-integrator mode) places every bead at the image nearest to where it was: the whole host move
 *       counts, with no correction.
 * The record moves with its bead like the LCG64 streams: through k_gather_state's permutation, in the migration records of a
 * decomposed run (six more doubles while tracking is on: mig_width), through the growth of the owned arrays (mg_ensure_owned).
 * ddcmi_upload_state drops the records.
 *
 * The sample (k_vaf_sample, k_vaf_final) is read-only with respect to the run and repeats bit for bit: a workgroup owns a
 * contiguous range of slots; a wave adds the sums of its 64 beads class by class -- a ballot picks the lanes of the first pending
 * lane's class, wave_sum_dpp over the wave with the other lanes at zero (not lane order: butterflies inside the rows of 16 lanes,
 * then (r0 + r1) + (r2 + r3) -- the same order every time, which is what repeating bit for bit needs; it is a full 64-lane
 * reduction of two values per distinct class and 64 beads: one or two classes per wave in cell-sorted water, a handful in a
 * bilayer), one lane adds into the wave's own LDS row -- the workgroup adds its waves' rows
 * in wave order into its row of vaf_part, and a second launch adds the workgroups' rows in workgroup order.  No floating-point
 * atomics.  Classes: 0 the system, 1 + g group g, 1 + ngroup + s species s (the order of vaf0 / msd0, without the reference's "one
 * group / species: no block" rule, which belongs to the output). */

#define VAF_THREADS 256
#define VAF_WAVES (VAF_THREADS / 64)
#define VAF_MAX_WG 2048
#define VAF_MAX_CLASS 1024      /* 64 B of LDS per class: 64 KB */

__global__ void k_vaf_origin(int n, const double4 *__restrict__ pos, const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ vz,
                             VafRec *__restrict__ vaf)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   const double4 p = pos[i];
   VafRec r;
   r.v0[0] = vx[i]; r.v0[1] = vy[i]; r.v0[2] = vz[i];
   r.o[0] = p.x; r.o[1] = p.y; r.o[2] = p.z;
   vaf[i] = r;
}
/* the lanes whose key is k add their NV values into row[NV k .. NV k + NV - 1] of the wave's LDS row, class after class (pending: lanes with a
 * bead).  NV = 2: this sample's {v0.v, d.d}; NV = 4: ddcmi_census.inl's {m vx, m vy, m vz, m} */
template <int NV>
__device__ __forceinline__ void vaf_add_classes(unsigned long long pending, int key, const double (&v)[NV], double *row)
{
   const int lane = threadIdx.x & 63;
   while (pending)
   {
      const int lead = __ffsll((long long)pending) - 1;
      const int k = __shfl(key, lead, 64);
      const bool mine = (pending >> lane & 1ull) && key == k;
      double s[NV];
#pragma unroll
      for (int q = 0; q < NV; q++) s[q] = wave_sum_dpp(mine ? v[q] : 0.0);
      if (lane == lead)
      {
#pragma unroll
         for (int q = 0; q < NV; q++) row[NV * k + q] += s[q];
      }
      pending &= ~__ballot(mine);
   }
}
__global__ __launch_bounds__(VAF_THREADS) void k_vaf_sample(int n, int per_wg, int ngroup, int nspecies, const double4 *__restrict__ pos,
                                                            const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ vz,
                                                            const int *__restrict__ group, const int *__restrict__ species, const VafRec *__restrict__ vaf,
                                                            double *__restrict__ part)
{
   extern __shared__ double vaf_s[];      /* [VAF_WAVES][nclass][2] */
   const int nclass = 1 + ngroup + nspecies;
   for (int k = threadIdx.x; k < VAF_WAVES * nclass * 2; k += VAF_THREADS) vaf_s[k] = 0.0;
   __syncthreads();
   double *row = vaf_s + (size_t)(threadIdx.x >> 6) * nclass * 2;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   double sys_a = 0.0, sys_b = 0.0;      /* the system's sums: per lane over the range, one reduction at the end */
   for (int base = beg; base < end; base += VAF_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int i = base + (int)threadIdx.x;
      const bool have = i < end;
      double a = 0.0, b = 0.0;
      int g = 0, s = 0;
      if (have)
      {
         const double4 p = pos[i];
         const VafRec r = vaf[i];
         a = r.v0[0] * vx[i] + r.v0[1] * vy[i] + r.v0[2] * vz[i];
         const double dx = p.x - r.o[0], dy = p.y - r.o[1], dz = p.z - r.o[2];
         b = dx * dx + dy * dy + dz * dz;
         g = min(max(group[i], 0), ngroup - 1); s = min(max(species[i], 0), nspecies - 1);      /* (checked at the upload: the LDS rows stay in bounds whatever the arrays hold) */
      }
      sys_a += a; sys_b += b;
      const unsigned long long pending = __ballot(have);
      const double ab[2] = {a, b};
      vaf_add_classes<2>(pending, 1 + g, ab, row);
      vaf_add_classes<2>(pending, 1 + ngroup + s, ab, row);
   }
   sys_a = wave_sum_dpp(sys_a); sys_b = wave_sum_dpp(sys_b);
   if ((threadIdx.x & 63) == 0) { row[0] = sys_a; row[1] = sys_b; }
   __syncthreads();
   double *out = part + (size_t)blockIdx.x * nclass * 2;
   for (int k = threadIdx.x; k < nclass * 2; k += VAF_THREADS)
   {
      double t = vaf_s[k];
#pragma unroll
      for (int w = 1; w < VAF_WAVES; w++) t += vaf_s[(size_t)w * nclass * 2 + k];
      out[k] = t;
   }
}
/* the workgroups' rows in workgroup order: out[k] = sum over w of part[w][k] */
__global__ void k_vaf_final(int nwg, int nval, const double *__restrict__ part, double *__restrict__ out)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k >= nval) return;
   double t = 0.0;
   for (int w = 0; w < nwg; w++) t += part[(size_t)w * nval + k];
   out[k] = t;
}

/* ---- host side ---------------------------------------------------------- */
static int vaf_origin_one(ddcmi_ctx *ctx)
{
   (void)hipSetDevice(ctx->device);
   const int n = ctx->nloc;
   /* room for what the owned arrays hold: a decomposed rank's beads arrive by migration (mg_ensure_owned grows the records with them) */
   const size_t cap = std::max((size_t)n, ctx->vx.cap) + 1;
   ENSURE(ctx, ctx->vaf, cap);
   if (decomposed(ctx)) ENSURE(ctx, ctx->vaf2, cap);
   if (n > 0)
      hipLaunchKernelGGL(k_vaf_origin, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, n, ctx->pos.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->vaf.p);
   HIPCHK(ctx, hipGetLastError());
   ctx->vaf_on = true;
   return DDCMI_OK;
}
static int vaf_origin_check(ddcmi_ctx *ctx, const char *fn)
{
   ARGCHK(ctx, ctx->nloc <= 0 && !decomposed(ctx), "%s needs an uploaded state (ddcmi_upload_state)", fn);
   ARGCHK(ctx, ctx->nloc > 0 && ctx->vx.cap < (size_t)ctx->nloc, "%s needs an uploaded state (ddcmi_upload_state)", fn);
   return DDCMI_OK;
}
static int vaf_sample_check(ddcmi_ctx *ctx, const char *fn, int ngroup, int nspecies, const void *vaf, const void *msd)
{
   ARGCHK(ctx, ctx->nloc <= 0 && !decomposed(ctx), "%s needs an uploaded state (ddcmi_upload_state)", fn);
   ARGCHK(ctx, !ctx->vaf_on, "%s: no time origin is set (ddcmi_vaf_origin)", fn);
   ARGCHK(ctx, ngroup != ctx->ngroup, "%s: ngroup = %d, the context has %d groups", fn, ngroup, ctx->ngroup);
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, !vaf || !msd, "%s: NULL output array (vaf %p, msd %p)", fn, vaf, msd);
   if (1 + ngroup + nspecies > VAF_MAX_CLASS) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d classes, at most %d", fn, 1 + ngroup + nspecies, VAF_MAX_CLASS);
   return DDCMI_OK;
}
/* this rank's sums [sync] */
static int vaf_sample_one(ddcmi_ctx *ctx, double *vaf, double *msd)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, nclass = 1 + ctx->ngroup + ctx->nspecies, nval = 2 * nclass;
   if (n <= 0) { for (int c = 0; c < nclass; c++) vaf[c] = msd[c] = 0.0; return DDCMI_OK; }      /* (a domain that holds no bead) */
   /* slots per workgroup: whole blocks of VAF_THREADS, at most about VAF_MAX_WG workgroups, every one of them with beads */
   const int per_wg = cdiv(cdiv(n, VAF_MAX_WG), VAF_THREADS) * VAF_THREADS;
   const int nwg = cdiv(n, per_wg);
   ENSURE(ctx, ctx->vaf_part, (size_t)(nwg + 1) * nval);
   double *d_out = ctx->vaf_part.p + (size_t)nwg * nval;
   hipLaunchKernelGGL(k_vaf_sample, dim3(nwg), dim3(VAF_THREADS), (size_t)VAF_WAVES * nval * sizeof(double), st, n, per_wg, ctx->ngroup, ctx->nspecies, ctx->pos.p,
                      ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->group.p, ctx->species.p, ctx->vaf.p, ctx->vaf_part.p);
   hipLaunchKernelGGL(k_vaf_final, dim3(cdiv(nval, 64)), dim3(64), 0, st, nwg, nval, ctx->vaf_part.p, d_out);
   HIPCHK(ctx, hipGetLastError());
   std::vector<double> h((size_t)nval);
   HIPCHK(ctx, hipMemcpyAsync(h.data(), d_out, (size_t)nval * sizeof(double), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   for (int c = 0; c < nclass; c++) { vaf[c] = h[2 * c]; msd[c] = h[2 * c + 1]; }
   return DDCMI_OK;
}

extern "C" int ddcmi_vaf_origin(ddcmi_ctx *ctx)
{
   if (!ctx) return DDCMI_EINVAL;
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group: use ddcmi_group_vaf_origin");
   int rc = vaf_origin_check(ctx, "ddcmi_vaf_origin");
   if (rc) return rc;
   return vaf_origin_one(ctx);
}
extern "C" int ddcmi_vaf_sample(ddcmi_ctx *ctx, int ngroup, int nspecies, double *vaf, double *msd)
{
   if (!ctx) return DDCMI_EINVAL;
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group: use ddcmi_group_vaf_sample");
   int rc = vaf_sample_check(ctx, "ddcmi_vaf_sample", ngroup, nspecies, vaf, msd);
   if (rc) return rc;
   (void)hipSetDevice(ctx->device);
   if ((rc = ddcmi_agree_poll(ctx))) return rc;
   return vaf_sample_one(ctx, vaf, msd);
}
static int vaf_clear_one(ddcmi_ctx *ctx)
{
   (void)hipSetDevice(ctx->device);
   if (ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   ctx->vaf_on = false;
   ctx->vaf.release(); ctx->vaf2.release(); ctx->vaf_part.release();
   return DDCMI_OK;
}
extern "C" int ddcmi_vaf_clear(ddcmi_ctx *ctx)
{
   if (!ctx) return DDCMI_EINVAL;
   /* (one domain of a group without its records while the others send theirs: the migration records would differ in width) */
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group: use ddcmi_group_vaf_clear");
   return vaf_clear_one(ctx);
}

/* in-process group: every domain's origin; per-rank sums, rank after rank (vaf[r * nclass ...], msd[r * nclass ...]) */
extern "C" int ddcmi_group_vaf_origin(ddcmi_ctx **ctxs, int n)
{
   if (!ctxs || n < 1 || !ctxs[0] || !ctxs[0]->group_) return DDCMI_EINVAL;
   ddcmi_group *g = ctxs[0]->group_;
   ARGCHK(ctxs[0], n != (int)g->ranks.size(), "ddcmi_group_vaf_origin: n = %d, the group has %d domains", n, (int)g->ranks.size());
   int rc;
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = vaf_origin_check(c, "ddcmi_group_vaf_origin"))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = vaf_origin_one(c))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   return DDCMI_OK;
}
extern "C" int ddcmi_group_vaf_clear(ddcmi_ctx **ctxs, int n)
{
   if (!ctxs || n < 1 || !ctxs[0] || !ctxs[0]->group_) return DDCMI_EINVAL;
   ddcmi_group *g = ctxs[0]->group_;
   ARGCHK(ctxs[0], n != (int)g->ranks.size(), "ddcmi_group_vaf_clear: n = %d, the group has %d domains", n, (int)g->ranks.size());
   int rc;
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = vaf_clear_one(c))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   return DDCMI_OK;
}
extern "C" int ddcmi_group_vaf_sample(ddcmi_ctx **ctxs, int n, int ngroup, int nspecies, double *vaf, double *msd)
{
   if (!ctxs || n < 1 || !ctxs[0] || !ctxs[0]->group_) return DDCMI_EINVAL;
   ddcmi_group *g = ctxs[0]->group_;
   ARGCHK(ctxs[0], n != (int)g->ranks.size(), "ddcmi_group_vaf_sample: n = %d, the group has %d domains", n, (int)g->ranks.size());
   int rc;
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = vaf_sample_check(c, "ddcmi_group_vaf_sample", ngroup, nspecies, vaf, msd))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   const size_t nclass = (size_t)1 + ngroup + nspecies;
   for (size_t r = 0; r < g->ranks.size(); r++)
      if ((rc = vaf_sample_one(g->ranks[r], vaf + r * nclass, msd + r * nclass))) { if (r) ctxs[0]->err = g->ranks[r]->err; return rc; }
   return DDCMI_OK;
}

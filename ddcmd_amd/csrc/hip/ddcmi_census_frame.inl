/* ddcmi_census_frame.inl -- what the read-only analyses share.  Included from ddcmi.hip behind the multi-domain path and ahead of
 * ddcmi_analysis.inl, ddcmi_vaf.inl, ddcmi_census.inl and ddcmi_kdist.inl.
 *
 * A census pass (VAF sample, momentum, zdensity, kinetic-energy histogram) reads the state ddcmi_download_state returns, changes
 * nothing of the run, needs no communication (the caller combines the ranks' results), uses no floating-point atomics and repeats
 * bit for bit, because every addition has a fixed place:
 *   a workgroup owns a contiguous range of slots (census_split) and walks it in blocks of CENSUS_THREADS, every lane in every trip;
 *   a wave adds its 64 beads key by key (wave_for_each_key): a ballot picks the lanes that share the first pending lane's key,
 *      wave_reduce_dpp combines them with the other lanes at the identity (not lane order: butterflies inside the rows of 16
 *      lanes, then (r0 + r1) + (r2 + r3) -- the same order every time), that one lane adds into the wave's own LDS row: one writer
 *      per row at a time, no bank conflict, no atomic.  Counts (weight 1) are the popcount of the ballot, added by an integer LDS
 *      add into one row per workgroup: their order does not matter;
 *   the workgroup adds its waves' rows in wave order into its row of census_part (census_rows_to_part);
 *   a second launch (k_census_final) adds the workgroups' rows in workgroup order, 32-bit counts in 64-bit integers.
 * Classes of the per-class sums (k_class_sums): 0 the system, 1 + g group g, 1 + ngroup + s species s (the order of vaf0 / msd0,
 * without the reference's "one group / species: no block" rule, which belongs to the output).
 *
 * The entry pairs ddcmi_X / ddcmi_group_X of all analyses, PAIRCORRELATION included, are analysis_single and analysis_group with
 * the analysis's check and run. */

#define CENSUS_THREADS 256
#define CENSUS_WAVES (CENSUS_THREADS / 64)
#define CENSUS_MAX_WG 1024       /* workgroups of a census pass ... */
#define VAF_MAX_WG 2048          /* ... and of the VAF sample: they decide which beads share a workgroup, hence the order of the additions */
#define CENSUS_MAX_NZ 2048       /* CENSUS_WAVES rows x 8 B = 32 B of LDS per bin: 64 KB */
/* per-wave rows of NV doubles per class in 64 KB of LDS: 1024 classes for the VAF sample's two values, 512 for the momentum's four */
static constexpr int census_max_class(int nv) { return 65536 / (CENSUS_WAVES * nv * 8); }

/* f(k, lead, mine, same) once per distinct key k of the pending lanes, first pending lane first: lead -- this lane is the one that
 * writes; mine -- this lane is pending and has key k; same -- the ballot of mine.  Every lane of the wave calls f every time, so
 * the wave operations inside it are convergent; the trip count is uniform (pending is). */
template <class F>
__device__ __forceinline__ void wave_for_each_key(unsigned long long pending, int key, F f)
{
   const int lane = threadIdx.x & 63;
   while (pending)
   {
      const int lead = __ffsll((long long)pending) - 1;
      const int k = __shfl(key, lead, 64);
      const bool mine = (pending >> lane & 1ull) && key == k;
      const unsigned long long same = __ballot(mine);
      f(k, lane == lead, mine, same);
      pending &= ~same;
   }
}
/* the lanes whose key is k add their NV values into row[NV k .. NV k + NV - 1] of the wave's LDS row, class after class */
template <int NV>
__device__ __forceinline__ void vaf_add_classes(unsigned long long pending, int key, const double (&v)[NV], double *row)
{
   wave_for_each_key(pending, key, [&](int k, bool lead, bool mine, unsigned long long) {
      double s[NV];
#pragma unroll
      for (int q = 0; q < NV; q++) s[q] = wave_sum_dpp(mine ? v[q] : 0.0);
      if (lead)
      {
#pragma unroll
         for (int q = 0; q < NV; q++) row[NV * k + q] += s[q];
      }
   });
}

/* how two rows combine at value k: everything adds; the kinetic-energy histogram's doubles are {sum, min, max} by k % 3 */
struct RowsSum { static __device__ __forceinline__ double f(int, double t, double o) { return t + o; } };
struct RowsSumMinMax
{
   static __device__ __forceinline__ double f(int k, double t, double o)
   {
      const int q = k % 3;
      return q == 0 ? t + o : (q == 1 ? (o < t ? o : t) : (o > t ? o : t));
   }
};
/* the waves' LDS rows [CENSUS_WAVES][nval] in wave order into the workgroup's row of the partials (after a __syncthreads) */
template <class Op>
__device__ __forceinline__ void census_rows_to_part(const double *rows, int nval, double *__restrict__ part)
{
   double *out = part + (size_t)blockIdx.x * nval;
   for (int k = threadIdx.x; k < nval; k += CENSUS_THREADS)
   {
      double t = rows[k];
#pragma unroll
      for (int w = 1; w < CENSUS_WAVES; w++) t = Op::f(k, t, rows[(size_t)w * nval + k]);
      out[k] = t;
   }
}
/* the second stage, the workgroups' rows in workgroup order: out_d[k] = part_d[0][k] Op part_d[1][k] Op ... (k < nd), and
 * out_c[k] = (C) sum over w of part_c[w][k] in 64-bit integers (k < nc); either part may be empty.  Starting from row 0 and
 * not from 0.0 makes no difference to a sum: no partial is -0.0 (an LDS row starts at +0.0 and is only added to; so does a
 * lane's system sum; and a sum of terms that are not -0.0 is not -0.0) */
template <class Op, class C>
__global__ void k_census_final(int nwg, int nd, const double *__restrict__ part_d, double *__restrict__ out_d, int nc, const unsigned *__restrict__ part_c,
                               C *__restrict__ out_c)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k < nc)
   {
      unsigned long long t = 0ull;
      for (int w = 0; w < nwg; w++) t += part_c[(size_t)w * nc + k];
      out_c[k] = (C)t;
   }
   if (k < nd)
   {
      double t = part_d[k];
      for (int w = 1; w < nwg; w++) t = Op::f(k, t, part_d[(size_t)w * nd + k]);
      out_d[k] = t;
   }
}

/* NV sums per class over the owned beads.  Bead: a struct of device pointers with
 *    __device__ void load(int i, int s, double (&v)[NV]) const      the NV values of bead i, whose (clamped) species is s
 * part: [nwg][nclass][NV] */
template <int NV, class Bead>
__global__ __launch_bounds__(CENSUS_THREADS) void k_class_sums(int n, int per_wg, int ngroup, int nspecies, const int *__restrict__ group,
                                                               const int *__restrict__ species, const Bead bead, double *__restrict__ part)
{
   extern __shared__ double census_s[];      /* [CENSUS_WAVES][nclass][NV] */
   const int nval = NV * (1 + ngroup + nspecies);
   for (int k = threadIdx.x; k < CENSUS_WAVES * nval; k += CENSUS_THREADS) census_s[k] = 0.0;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * nval;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   double sys[NV];      /* the system's sums: per lane over the range, one reduction at the end */
#pragma unroll
   for (int q = 0; q < NV; q++) sys[q] = 0.0;
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int i = base + (int)threadIdx.x;
      const bool have = i < end;
      double v[NV];
#pragma unroll
      for (int q = 0; q < NV; q++) v[q] = 0.0;
      int g = 0, s = 0;
      if (have)
      {
         g = min(max(group[i], 0), ngroup - 1); s = min(max(species[i], 0), nspecies - 1);      /* (checked at the upload: the LDS rows stay in bounds whatever the arrays hold) */
         bead.load(i, s, v);
      }
#pragma unroll
      for (int q = 0; q < NV; q++) sys[q] += v[q];
      const unsigned long long pending = __ballot(have);
      vaf_add_classes<NV>(pending, 1 + g, v, row);
      vaf_add_classes<NV>(pending, 1 + ngroup + s, v, row);
   }
#pragma unroll
   for (int q = 0; q < NV; q++) sys[q] = wave_sum_dpp(sys[q]);
   if ((threadIdx.x & 63) == 0)
   {
#pragma unroll
      for (int q = 0; q < NV; q++) row[q] = sys[q];
   }
   __syncthreads();
   census_rows_to_part<RowsSum>(census_s, nval, part);
}

/* ---- host side ---------------------------------------------------------- */
/* slots per workgroup: whole blocks of CENSUS_THREADS, at most about max_wg workgroups, every one of them with beads */
static void census_split(int n, int max_wg, int *per_wg, int *nwg)
{
   *per_wg = cdiv(cdiv(n, max_wg), CENSUS_THREADS) * CENSUS_THREADS;
   *nwg = cdiv(n, *per_wg);
}
static int census_state_check(ddcmi_ctx *ctx, const char *fn)
{
   ARGCHK(ctx, ctx->nloc <= 0 && !decomposed(ctx), "%s needs an uploaded state (ddcmi_upload_state)", fn);
   ARGCHK(ctx, ctx->nloc > 0 && ctx->vx.cap < (size_t)ctx->nloc, "%s needs an uploaded state (ddcmi_upload_state)", fn);
   return DDCMI_OK;
}
/* this rank's class sums, h[nclass][NV]: zeros for a domain that holds no bead [sync] */
template <int NV, class Bead>
static int class_sums_one(ddcmi_ctx *ctx, int max_wg, const Bead &bead, std::vector<double> &h)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, nval = NV * (1 + ctx->ngroup + ctx->nspecies);
   h.assign((size_t)nval, 0.0);
   if (n <= 0) return DDCMI_OK;
   int per_wg, nwg;
   census_split(n, max_wg, &per_wg, &nwg);
   ENSURE(ctx, ctx->census_part, (size_t)(nwg + 1) * nval);
   double *d_out = ctx->census_part.p + (size_t)nwg * nval;
   hipLaunchKernelGGL((k_class_sums<NV, Bead>), dim3(nwg), dim3(CENSUS_THREADS), (size_t)CENSUS_WAVES * nval * sizeof(double), st, n, per_wg, ctx->ngroup,
                      ctx->nspecies, ctx->group.p, ctx->species.p, bead, ctx->census_part.p);
   hipLaunchKernelGGL((k_census_final<RowsSum, double>), dim3(cdiv(nval, 64)), dim3(64), 0, st, nwg, nval, ctx->census_part.p, d_out, 0, nullptr, nullptr);
   HIPCHK(ctx, hipGetLastError());
   HIPCHK(ctx, hipMemcpyAsync(h.data(), d_out, (size_t)nval * sizeof(double), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}

/* ddcmi_<name>(ctx, ...): check(ctx, "ddcmi_<name>") refuses the call before anything happens; poll -- the entry joins the
 * ranks' agreement (ddcmi_agree_poll) before it runs */
template <class Check, class Run>
static int analysis_single(ddcmi_ctx *ctx, const char *name, bool poll, Check check, Run run)
{
   if (!ctx) return DDCMI_EINVAL;
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group: use ddcmi_group_%s", name);
   int rc = check(ctx, (std::string("ddcmi_") + name).c_str());
   if (rc) return rc;
   (void)hipSetDevice(ctx->device);
   if (poll && (rc = ddcmi_agree_poll(ctx))) return rc;
   return run(ctx);
}
/* ddcmi_group_<name>(ctxs, n, ...): every check on every rank before anything collective (between(g), once) or any launch
 * (run(rank, r), rank after rank: the outputs are per-rank blocks); a failing rank's message goes to ctxs[0] */
template <class Check, class Between, class Run>
static int analysis_group(ddcmi_ctx **ctxs, int n, const char *name, Check check, Between between, Run run)
{
   if (!ctxs || n < 1 || !ctxs[0] || !ctxs[0]->group_) return DDCMI_EINVAL;
   ddcmi_group *g = ctxs[0]->group_;
   ARGCHK(ctxs[0], n != (int)g->ranks.size(), "ddcmi_group_%s: n = %d, the group has %d domains", name, n, (int)g->ranks.size());
   const std::string fn = std::string("ddcmi_group_") + name;
   int rc;
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = check(c, fn.c_str()))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   if ((rc = between(g))) return rc;
   for (size_t r = 0; r < g->ranks.size(); r++)
      if ((rc = run(g->ranks[r], r))) { if (r) ctxs[0]->err = g->ranks[r]->err; return rc; }
   return DDCMI_OK;
}
template <class Check, class Run>
static int analysis_group(ddcmi_ctx **ctxs, int n, const char *name, Check check, Run run)
{
   return analysis_group(ctxs, n, name, check, [](ddcmi_group *) { return DDCMI_OK; }, run);
}

/* ddcmi_census_frame.inl -- what the read-only analyses share.  Included from ddcmi.hip behind the multi-domain path and ahead of
 * every analysis file.  What it offers, and who uses it:
 *   device  census_coord / census_position over a CensusBox or a struct's own L[3] and pbc: the position a download returns (export_coord of ddcmi_internal.h, the
 *              one copy of k_export_pos's wrap)                       census (z alone), dsf, ssf, subset, coarsegrain, chol, track
 *           gid_find, gid_in_range: the search of an ascending gid list and the prefilter in front of it      subset, chol, track
 *           wave_for_each_key, vaf_add_classes, census_rows_to_part, k_census_final, k_class_sums: the census pass proper (below)
 *                                                                               vaf, census, kdist, dsf, ssf (second stage), chol
 *           k_compact_count / k_compact_scan / k_compact_pack over a functor: the stable compaction in slot order
 *                                                                            subset (beads), coarsegrain (segment heads), chol (fragments)
 *   host    census_split, census_state_check, census_box_check, census_set_box          every pass that reads positions asks for its box
 *           CensusScratch: ctx->census_part carved into typed segments                 class sums, zdensity, kdist, dsf, ssf, chol
 *           census_finish: the second stage, the download of doubles and 64-bit counts, the wait                           the same six
 *           census_upload_select: the per-species selection                                                                    dsf, ssf
 *           compact_count, compact_pack: the compaction's launches                                          subset, coarsegrain, chol
 *           analysis_single / analysis_group: every entry pair; analysis_group_records: counts first, then the ranks' records into
 *              one buffer                                                                                   subset, coarsegrain, chol
 * Left alone: k_structure_modes stages its selected beads and k_cg_scatter ranks per digit with the ranking compact_block_rank does
 * for the pack kernel, but around their own barriers and LDS arrays (the first reads the block's total as a loop bound, the second
 * ranks 256 digits at once); they keep their own lines.  So does the pivot search of k_track_accumulate, an upper bound in LDS.
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

/* the box of a pass: the sides of the orthorhombic box (census_box_check) and the periodic axes' bits.  A pass's parameter struct embeds
 * it, or has members of these names itself where it had them before the frame offered this: a kernel's argument layout decides how its
 * scalar loads come out, so the structs keep theirs.  Box below: either kind (census_set_box fills it) */
struct CensusBox { double L[3]; int pbc; };
/* axis a of the position a download returns (export_coord, ddcmi_internal.h: k_export_pos's operations) */
template <class Box>
__device__ __forceinline__ double census_coord(const Box &bx, int a, double x) { return export_coord(x, bx.L[a], bx.pbc >> a & 1); }
template <class Box>
__device__ __forceinline__ void census_position(const Box &bx, const double4 p, double (&r)[3])
{
   r[0] = census_coord(bx, 0, p.x); r[1] = census_coord(bx, 1, p.y); r[2] = census_coord(bx, 2, p.z);
}

/* the first entry >= g of the ascending ids[lo, hi) -- an index type I, a pointer or an LDS array P: *at = its index (hi: there is
 * none); true where that entry is g */
template <class P, class I>
__device__ __forceinline__ bool gid_find(const P &ids, I lo, I hi, unsigned long long g, I *at)
{
   const I end = hi;
   while (lo < hi)
   {
      const I mid = lo + ((hi - lo) >> 1);
      if (ids[mid] < g) lo = mid + 1; else hi = mid;
   }
   *at = lo;
   return lo < end && ids[lo] == g;
}
/* the prefilter in front of it: g lies between the least and the greatest listed gid (kernel arguments: scalar registers) */
__device__ __forceinline__ bool gid_in_range(unsigned long long g, unsigned long long gmin, unsigned long long gmax) { return !(g < gmin || g > gmax); }

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

/* ---- the stable compaction in slot order -------------------------------- */
/* Sel: a struct of device pointers and parameters with
 *    struct Item                                                         what the predicate hands on to the store, per lane
 *    __device__ bool selected(int i, Item &it) const                     slot i is kept
 *    __device__ void store(int i, unsigned place, const Item &it) const  slot i is the place-th kept slot
 * k_compact_count   a workgroup counts the kept slots of its census_split range: ballot and popcount per wave, the waves' counts
 *                   added through LDS.
 * k_compact_scan    one wave: the exclusive scan of the (at most 2048) counts, and their total behind it.
 * k_compact_pack    the predicate again; a lane's place is the workgroup's offset + the kept slots of the blocks before this one
 *                   + those of the waves before its own (LDS) + the popcount of the ballot below its lane (compact_block_rank). */
template <class Sel>
__global__ __launch_bounds__(CENSUS_THREADS) void k_compact_count(int n, int per_wg, const Sel sel, unsigned *__restrict__ wg_count)
{
   __shared__ unsigned wave_s[CENSUS_WAVES];
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   unsigned mine = 0u;      /* the wave's count: the same in all its lanes */
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the ballot) */
   {
      const int i = base + (int)threadIdx.x;
      typename Sel::Item it;
      mine += (unsigned)__popcll(__ballot(i < end && sel.selected(i, it)));
   }
   if ((threadIdx.x & 63) == 0) wave_s[threadIdx.x >> 6] = mine;
   __syncthreads();
   if (threadIdx.x == 0)
   {
      unsigned t = 0u;
#pragma unroll
      for (int w = 0; w < CENSUS_WAVES; w++) t += wave_s[w];
      wg_count[blockIdx.x] = t;
   }
}
/* one wave: wg_off[k] = wg_count[0] + ... + wg_count[k - 1] for k <= nwg (wg_off[nwg]: the total); lane l takes the entries
 * [l chunk, (l + 1) chunk) */
__global__ __launch_bounds__(64) void k_compact_scan(int nwg, const unsigned *__restrict__ wg_count, unsigned *__restrict__ wg_off)
{
   const int lane = threadIdx.x, chunk = (nwg + 63) / 64;
   const int beg = min(lane * chunk, nwg), end = min(beg + chunk, nwg);
   unsigned t = 0u;
   for (int k = beg; k < end; k++) t += wg_count[k];
   unsigned incl = t;
#pragma unroll
   for (int d = 1; d < 64; d <<= 1)
   {
      const unsigned o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
   }
   unsigned run = incl - t;
   for (int k = beg; k < end; k++) { wg_off[k] = run; run += wg_count[k]; }
   if (lane == 63) wg_off[nwg] = incl;
}
/* the kept slots of this block of CENSUS_THREADS slots in front of this lane's, and all of them: the waves' counts through wave_s
 * (one barrier; the caller alternates between two rows, so that the next block's counts do not overtake this one's readers) */
__device__ __forceinline__ unsigned compact_block_rank(bool sel, unsigned *wave_s, unsigned &all)
{
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const unsigned long long same = __ballot(sel);
   if (lane == 0) wave_s[wave] = (unsigned)__popcll(same);
   __syncthreads();
   unsigned before = 0u;
   all = 0u;
#pragma unroll
   for (int w = 0; w < CENSUS_WAVES; w++) { const unsigned c = wave_s[w]; all += c; if (w < wave) before += c; }
   return before + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
}
template <class Sel>
__global__ __launch_bounds__(CENSUS_THREADS) void k_compact_pack(int n, int per_wg, const Sel sel, const unsigned *__restrict__ wg_off, unsigned nrec)
{
   __shared__ unsigned wave_s[2][CENSUS_WAVES];
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   unsigned run = wg_off[blockIdx.x];
   int par = 0;
   for (int base = beg; base < end; base += CENSUS_THREADS, par ^= 1)      /* (uniform trip count) */
   {
      const int i = base + (int)threadIdx.x;
      typename Sel::Item it;
      const bool kept = i < end && sel.selected(i, it);
      unsigned all;
      const unsigned place = run + compact_block_rank(kept, wave_s[par], all);
      if (kept && place < nrec) sel.store(i, place, it);      /* (place < nrec whenever the state is the one k_compact_count saw) */
      run += all;
   }
}

/* ---- host side ---------------------------------------------------------- */
/* the count and the scan of a compaction over n slots in nwg ranges: wg_count[nwg], wg_off[nwg + 1], wg_off[nwg] the total */
template <class Sel>
static void compact_count(hipStream_t st, int n, int per_wg, int nwg, const Sel &sel, unsigned *wg_count, unsigned *wg_off)
{
   hipLaunchKernelGGL(k_compact_count<Sel>, dim3(nwg), dim3(CENSUS_THREADS), 0, st, n, per_wg, sel, wg_count);
   hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(64), 0, st, nwg, wg_count, wg_off);
}
template <class Sel>
static void compact_pack(hipStream_t st, int n, int per_wg, int nwg, const Sel &sel, const unsigned *wg_off, unsigned nrec)
{
   hipLaunchKernelGGL(k_compact_pack<Sel>, dim3(nwg), dim3(CENSUS_THREADS), 0, st, n, per_wg, sel, wg_off, nrec);
}
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
/* the refusals of a pass that wraps or bins positions: an orthorhombic box with a side on each of `axes` (bits x 1, y 2, z 4).
 * box_first: the missing box is refused ahead of the off-diagonals (COARSEGRAIN's order; the others have it behind them) */
static int census_box_check(ddcmi_ctx *ctx, const char *fn, int axes, bool box_first = false)
{
   bool nobox = false;
   for (int a = 0; a < 3; a++) nobox = nobox || ((axes >> a & 1) && !(ctx->h[4 * a] > 0.0));
   if (box_first && nobox) SETERR(ctx, DDCMI_EINVAL, "%s needs a box (ddcmi_set_box)", fn);
   const int off[6] = {1, 2, 3, 5, 6, 7};
   for (int k = 0; k < 6; k++)
      if (fabs(ctx->h[off[k]]) > 1e-10) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: only orthorhombic boxes are supported (h[%d]=%g)", fn, off[k], ctx->h[off[k]]);
   if (nobox) SETERR(ctx, DDCMI_EINVAL, "%s needs a box (ddcmi_set_box)", fn);
   return DDCMI_OK;
}
template <class Box>
static void census_set_box(const ddcmi_ctx *ctx, Box &bx)
{
   bx.L[0] = ctx->h[0]; bx.L[1] = ctx->h[4]; bx.L[2] = ctx->h[8]; bx.pbc = ctx->pbc;
}
/* ctx->census_part carved into segments, one behind the other in the order of the seg() calls, each of count elements of elem
 * bytes and each starting on an 8-byte boundary; ensure() makes the room, at<T>(k) is segment k */
struct CensusScratch
{
   size_t off[8], total = 0;      /* in doubles */
   int n = 0;
   double *base = nullptr;
   int seg(size_t elem, size_t count)      /* (a ninth segment is counted, not stored: ensure() refuses) */
   {
      if (n < 8) { off[n] = total; total += (elem * count + 7) / 8; }
      return n++;
   }
   int ensure(ddcmi_ctx *ctx)
   {
      if (n > 8) SETERR(ctx, DDCMI_EINVAL, "CensusScratch: %d segments, room for 8", n);
      ENSURE(ctx, ctx->census_part, total);
      base = ctx->census_part.p;
      return DDCMI_OK;
   }
   template <class T> T *at(int k) const { return (T *)(base + off[k]); }
};
/* the second stage and the download: k_census_final<Op, C> over nwg rows of nd doubles and nc counts (either may be empty), its
 * results copied into the caller's h_d[nd] and h_c[nc]; more(): further copies that share the one wait [sync] */
template <class Op, class C, class More>
static int census_finish(ddcmi_ctx *ctx, int nwg, int nd, const double *part_d, double *out_d, double *h_d, int nc, const unsigned *part_c, C *out_c, C *h_c, More more)
{
   hipStream_t st = ctx->stream;
   hipLaunchKernelGGL((k_census_final<Op, C>), dim3(cdiv(std::max(nd, nc), 64)), dim3(64), 0, st, nwg, nd, part_d, out_d, nc, part_c, out_c);
   HIPCHK(ctx, hipGetLastError());
   if (nd > 0) HIPCHK(ctx, hipMemcpyAsync(h_d, out_d, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost, st));
   if (nc > 0) HIPCHK(ctx, hipMemcpyAsync(h_c, out_c, (size_t)nc * sizeof(C), hipMemcpyDeviceToHost, st));
   int rc = more();
   if (rc) return rc;
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}
template <class Op, class C>
static int census_finish(ddcmi_ctx *ctx, int nwg, int nd, const double *part_d, double *out_d, double *h_d, int nc, const unsigned *part_c, C *out_c, C *h_c)
{
   return census_finish<Op, C>(ctx, nwg, nd, part_d, out_d, h_d, nc, part_c, out_c, h_c, [] { return (int)DDCMI_OK; });
}
/* the per-species selection of DSF and the structure modes as 0 / 1 words (select == NULL: every species), uploaded to d_sel on the
 * stream; sel is the caller's, so that it outlives the copy */
static int census_upload_select(ddcmi_ctx *ctx, const int *select, std::vector<int> &sel, int *d_sel)
{
   sel.assign((size_t)ctx->nspecies, 1);
   if (select) for (int s = 0; s < ctx->nspecies; s++) sel[s] = select[s] != 0;
   HIPCHK(ctx, hipMemcpyAsync(d_sel, sel.data(), sel.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
   return DDCMI_OK;
}
/* this rank's class sums, h[nclass][NV]: zeros for a domain that holds no bead [sync] */
template <int NV, class Bead>
static int class_sums_one(ddcmi_ctx *ctx, int max_wg, const Bead &bead, std::vector<double> &h)
{
   (void)hipSetDevice(ctx->device);
   const int n = ctx->nloc, nval = NV * (1 + ctx->ngroup + ctx->nspecies);
   h.assign((size_t)nval, 0.0);
   if (n <= 0) return DDCMI_OK;
   int per_wg, nwg;
   census_split(n, max_wg, &per_wg, &nwg);
   CensusScratch cs;
   const int part = cs.seg(8, (size_t)nwg * nval), out = cs.seg(8, nval);
   int rc = cs.ensure(ctx);
   if (rc) return rc;
   hipLaunchKernelGGL((k_class_sums<NV, Bead>), dim3(nwg), dim3(CENSUS_THREADS), (size_t)CENSUS_WAVES * nval * sizeof(double), ctx->stream, n, per_wg, ctx->ngroup,
                      ctx->nspecies, ctx->group.p, ctx->species.p, bead, cs.at<double>(part));
   return census_finish<RowsSum, double>(ctx, nwg, nval, cs.at<double>(part), cs.at<double>(out), h.data(), 0, nullptr, nullptr, nullptr);
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
   if (!ctxs || n < 1 || !ctxs[0]) return DDCMI_EINVAL;
   if (!ctxs[0]->group_) SETERR(ctxs[0], DDCMI_EINVAL, "ddcmi_group_%s: not the contexts of an in-process group: use ddcmi_%s", name, name);
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
/* the group entry of a pass that returns records (`what` names them): count_run(rank, r) leaves count[r] on every rank first, so that
 * a buffer that is too small stays untouched; with want_rec, cap the room for all of them, rec_run(rank, r, off) then puts rank r's
 * count[r] records off records into the caller's buffer: the ranks' blocks one behind the other in rank order */
template <class Check, class CountRun, class RecRun>
static int analysis_group_records(ddcmi_ctx **ctxs, int n, const char *name, const char *what, Check check, CountRun count_run, bool want_rec, int64_t cap,
                                  const int64_t *count, RecRun rec_run)
{
   int rc = analysis_group(ctxs, n, name, check, count_run);
   if (rc || !want_rec) return rc;
   std::vector<int64_t> off((size_t)n + 1, 0);
   for (int r = 0; r < n; r++) off[r + 1] = off[r] + count[r];
   if (cap < off[n]) SETERR(ctxs[0], DDCMI_EINVAL, "ddcmi_group_%s: capacity %lld < %lld %s", name, (long long)cap, (long long)off[n], what);
   const int64_t *o = off.data();
   return analysis_group(ctxs, n, name, [](ddcmi_ctx *, const char *) { return DDCMI_OK; }, [=](ddcmi_ctx *c, size_t r) { return rec_run(c, r, o[r]); });
}

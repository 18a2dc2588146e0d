/* ddcmi_chol.inl -- ANALYSIS type cholAnalysis on the device (cholAnalysis.c:109-163, cholAnalysis_eval): for every listed cholesterol
 * molecule how far the bead next to each ring triangle stands out of that triangle's plane (dR1, dR5), binned into two histograms,
 * with their sum and extremes.  Included from ddcmi.hip behind ddcmi_subset.inl.  A census pass (ddcmi_census_frame.inl): read-only,
 * no communication, no floating-point atomics, the same bytes when repeated, positions as a download returns them.
 *
 * It is the first pass per molecule, not per bead: a molecule's seven beads sit in unrelated slots after the cell sort, and on a
 * decomposed run other ranks may own some of them.  Halo slots are not read (what they hold between rebuilds depends on the step
 * plan); a molecule this rank owns in part comes back as fragments {mol, role, r}, which the caller merges over the ranks and
 * finishes on the host with the lane's own arithmetic (host/chol_math.h, shared with host/chol.c).
 *
 *   k_chol_gather   over the owned beads.  A bead whose gid lies outside [least, greatest listed gid] is skipped (the prefilter: the
 *                   C-ABI names beads by gid alone, so the host cannot tell their species); the others search the ascending
 *                   listed gids (gid_in_range, gid_find); a hit writes the wrapped position to table[mol][role] and a byte to
 *                   present[mol][role].  Every (mol, role) has one writer -- a gid is listed once and owned once -- so no atomics;
 *                   both arrays are zeroed on the stream first.
 *   k_chol_eval     one lane per molecule, census_split over the molecules.  Seven present: dR1, dR5 (chol_offsets_of), their bins
 *                   counted as k_census_kdist counts (wave_for_each_key, integer LDS adds), the doubles {sum, min, max} of each
 *                   into the wave's LDS row, rows and workgroups combined by RowsSumMinMax / k_census_final.  One to six present:
 *                   split[mol] = 1.  None: nothing.  A NaN offset (collinear beads) goes to bin 0, joins the sum and enters
 *                   neither extreme, as the reference's macros and comparisons have it.
 *   the fragments   the present (mol, role) of split molecules through the frame's compaction (CholFragSel): stable in (mol, role)
 *                   order, 32-byte records.
 * LDS of k_chol_eval: CENSUS_WAVES x 6 doubles, then 2 nbins + 1 counters (the last one counts the molecules done):
 * DDCMI_CHOL_LDS_BYTES(nbins) <= DDCMI_CHOL_MAX_LDS, i.e. nbins <= 8167. */

#define CHOL_FN __device__ __forceinline__
#define CHOL_RND(x) zd_rounded(x)
#include "../host/chol_math.h"
#undef CHOL_FN
#undef CHOL_RND

struct CholParms { double rmin, delta, L[3], invL[3]; int nbins, pbc; };

__global__ __launch_bounds__(256) void k_chol_gather(int n, CholParms cp, unsigned long long gmin, unsigned long long gmax, int nl, const double4 *__restrict__ pos,
                                                     const unsigned long long *__restrict__ gid, const unsigned long long *__restrict__ ids,
                                                     const int *__restrict__ perm, double *__restrict__ table, unsigned char *__restrict__ present)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   const unsigned long long g = gid[i];
   int at;
   if (!gid_in_range(g, gmin, gmax) || !gid_find(ids, 0, nl, g, &at)) return;
   const int slot = perm[at];
   if (slot < 0 || slot >= nl) return;      /* (the host's permutation: the stores stay in bounds whatever it holds) */
   double r[3];
   census_position(cp, pos[i], r);
   table[3 * (size_t)slot] = r[0]; table[3 * (size_t)slot + 1] = r[1]; table[3 * (size_t)slot + 2] = r[2];
   present[slot] = 1;
}

/* part_d: [nwg][6] doubles {sum, min, max} of dR1, then of dR5; part_c: [nwg][2 nbins + 1] 32-bit counts */
__global__ __launch_bounds__(CENSUS_THREADS) void k_chol_eval(int nmol, int per_wg, CholParms cp, const double *__restrict__ table,
                                                              const unsigned char *__restrict__ present, unsigned char *__restrict__ split,
                                                              double *__restrict__ part_d, unsigned *__restrict__ part_c)
{
   extern __shared__ double census_s[];      /* double [CENSUS_WAVES][6], then unsigned [2 nbins + 1] */
   const int nslot = 2 * cp.nbins + 1;
   unsigned *cnt_s = (unsigned *)(census_s + CENSUS_WAVES * 6);
   for (int k = threadIdx.x; k < CENSUS_WAVES * 6; k += CENSUS_THREADS) { const int q = k % 3; census_s[k] = q == 0 ? 0.0 : (q == 1 ? 1e300 : -1e300); }
   for (int k = threadIdx.x; k < nslot; k += CENSUS_THREADS) cnt_s[k] = 0u;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * 6;
   const int beg = blockIdx.x * per_wg, end = min(nmol, beg + per_wg);
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int m = base + (int)threadIdx.x;
      bool whole = false;
      double d[2] = {0.0, 0.0};
      int bin[2] = {-1, -1};
      if (m < end)
      {
         const unsigned char *pm = present + 7 * (size_t)m;
         int np = 0;
#pragma unroll
         for (int k = 0; k < 7; k++) np += pm[k] != 0;
         if (np == 7)
         {
            double r[21];
#pragma unroll
            for (int k = 0; k < 21; k++) r[k] = table[21 * (size_t)m + k];
            chol_offsets_of(cp.L, cp.invL, cp.pbc, r, &d[0], &d[1]);
            bin[0] = chol_bin(d[0], cp.rmin, cp.delta, cp.nbins);
            bin[1] = cp.nbins + chol_bin(d[1], cp.rmin, cp.delta, cp.nbins);
            whole = true;
         }
         else if (np > 0) split[m] = 1;
      }
      const unsigned long long done = __ballot(whole);
      if (done)      /* (uniform over the wave) */
      {
#pragma unroll
         for (int q = 0; q < 2; q++)
         {
            const bool ext = whole && d[q] == d[q];      /* a NaN enters neither extreme */
            const double sk = wave_sum_dpp(whole ? d[q] : 0.0), mn = wave_reduce_dpp<WaveMin>(ext ? d[q] : 1e300), mx = wave_reduce_dpp<WaveMax>(ext ? d[q] : -1e300);
            if ((threadIdx.x & 63) == 0)
            {
               double *r3 = row + 3 * q;
               r3[0] += sk;
               if (mn < r3[1]) r3[1] = mn;
               if (mx > r3[2]) r3[2] = mx;
            }
         }
         if ((threadIdx.x & 63) == 0) atomicAdd(&cnt_s[2 * cp.nbins], (unsigned)__popcll(done));      /* (integers: the order of the waves does not matter) */
      }
#pragma unroll
      for (int q = 0; q < 2; q++)
         wave_for_each_key(__ballot(bin[q] >= 0), bin[q], [&](int k, bool lead, bool, unsigned long long same) {
            if (lead) atomicAdd(&cnt_s[k], (unsigned)__popcll(same));
         });
   }
   __syncthreads();
   census_rows_to_part<RowsSumMinMax>(census_s, 6, part_d);
   unsigned *out_c = part_c + (size_t)blockIdx.x * nslot;
   for (int k = threadIdx.x; k < nslot; k += CENSUS_THREADS) out_c[k] = cnt_s[k];
}

/* the compaction's functor (k_compact_count, k_compact_pack) over the 7 nmol (mol, role) slots: the present ones of split molecules;
 * rec: nrec records of four 8-byte words {mol | role << 32, r[0], r[1], r[2]} (struct ddcmi_chol_fragment) */
struct CholFragSel
{
   const unsigned char *present, *split; const double *table; unsigned long long *rec;
   struct Item {};
   __device__ __forceinline__ bool selected(int s, Item &) const { return present[s] != 0 && split[s / 7] != 0; }
   __device__ __forceinline__ void store(int s, unsigned place, const Item &) const
   {
      unsigned long long *o = rec + 4 * (size_t)place;
      o[0] = (unsigned long long)(unsigned)(s / 7) | (unsigned long long)(unsigned)(s % 7) << 32;
      o[1] = (unsigned long long)__double_as_longlong(table[3 * (size_t)s]);
      o[2] = (unsigned long long)__double_as_longlong(table[3 * (size_t)s + 1]);
      o[3] = (unsigned long long)__double_as_longlong(table[3 * (size_t)s + 2]);
   }
};

/* ---- host side ---------------------------------------------------------- */
static_assert(sizeof(ddcmi_chol_fragment) == 32, "a fragment is 32 bytes: {int32 mol, role; double r[3]}");
/* the list in ascending gid order with the permutation back to 7 mol + role, kept with the context: a caller evaluates the same list
 * every eval_rate steps, and sorting it costs more than the pass.  Returns the first gid listed twice in *dup (false: none). */
static bool chol_list_prepare(ddcmi_ctx *ctx, int64_t nmol, const uint64_t *gid, uint64_t *dup)
{
   const size_t nl = 7 * (size_t)nmol;
   if (ctx->chol_list.size() != nl || (nl && memcmp(ctx->chol_list.data(), gid, nl * sizeof(uint64_t)) != 0))
   {
      std::vector<int> perm(nl);
      for (size_t k = 0; k < nl; k++) perm[k] = (int)k;
      std::sort(perm.begin(), perm.end(), [gid](int a, int b) { return gid[a] < gid[b] || (gid[a] == gid[b] && a < b); });
      std::vector<unsigned long long> ids(nl);
      for (size_t k = 0; k < nl; k++) ids[k] = gid[perm[k]];
      for (size_t k = 1; k < nl; k++)
         if (ids[k] == ids[k - 1]) { *dup = ids[k]; return true; }      /* (the kept list stays as it was) */
      ctx->chol_list.assign(gid, gid + nl);
      ctx->chol_sorted.swap(ids);
      ctx->chol_perm_h.swap(perm);
      ctx->chol_list_fresh = true;
   }
   return false;
}
static int chol_check(ddcmi_ctx *ctx, const char *fn, int64_t nmol, const uint64_t *gid, double rmin, double delta, int nbins, const void *counts,
                      const void *ndone, const void *stats, int64_t cap, const void *frag, const void *nfrag)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, nmol < 0 || nmol > (int64_t)(INT_MAX / 32), "%s: nmol = %lld", fn, (long long)nmol);
   ARGCHK(ctx, nmol > 0 && !gid, "%s: NULL gid with nmol = %lld", fn, (long long)nmol);
   ARGCHK(ctx, nbins < 1, "%s: nbins = %d", fn, nbins);
   ARGCHK(ctx, !std::isfinite(delta) || !(delta > 0.0), "%s: delta = %g, it must be finite and positive", fn, delta);
   ARGCHK(ctx, !std::isfinite(rmin), "%s: rmin = %g", fn, rmin);
   ARGCHK(ctx, nmol > 0 && (!counts || !ndone || !stats || !nfrag), "%s: NULL output array (counts %p, ndone %p, stats %p, nfrag %p)", fn, counts, ndone, stats, nfrag);
   ARGCHK(ctx, frag && cap < 0, "%s: cap = %lld", fn, (long long)cap);
   if ((rc = census_box_check(ctx, fn, 7))) return rc;
   if (DDCMI_CHOL_LDS_BYTES((long)nbins) > DDCMI_CHOL_MAX_LDS)
      SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d bins need %ld bytes of LDS, at most %d (8 per bin: %d bins)", fn, nbins, DDCMI_CHOL_LDS_BYTES((long)nbins),
             DDCMI_CHOL_MAX_LDS, DDCMI_CHOL_MAX_NBINS);
   uint64_t dup = 0;
   if (nmol > 0 && chol_list_prepare(ctx, nmol, gid, &dup)) SETERR(ctx, DDCMI_EINVAL, "%s: gid %llu is listed twice", fn, (unsigned long long)dup);
   return DDCMI_OK;
}
/* this rank's result; its fragments stay packed in ctx->chol_frag for chol_copy_fragments [sync] */
static int chol_one(ddcmi_ctx *ctx, int64_t nmol64, double rmin, double delta, int nbins, int64_t *counts, int64_t *ndone, double *stats, int64_t *nfrag)
{
   if (nmol64 == 0) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, nmol = (int)nmol64, nl = 7 * nmol, nslot = 2 * nbins + 1;
   *nfrag = 0; *ndone = 0; ctx->chol_nfrag = 0;
   for (int k = 0; k < 2 * nbins; k++) counts[k] = 0;
   for (int q = 0; q < 2; q++) { stats[3 * q] = 0.0; stats[3 * q + 1] = 1e300; stats[3 * q + 2] = -1e300; }
   if (n <= 0) return DDCMI_OK;      /* (a domain that holds no bead) */
   CholParms cp;
   cp.rmin = rmin; cp.delta = delta; cp.nbins = nbins; census_set_box(ctx, cp);
   for (int a = 0; a < 3; a++) cp.invL[a] = 1.0 / cp.L[a];
   int per_wg, nwg, per_wgf, nwgf;
   census_split(nmol, CENSUS_MAX_WG, &per_wg, &nwg);
   census_split(nl, CENSUS_MAX_WG, &per_wgf, &nwgf);
   /* chol_ids: the ascending gids; chol_int: perm[nl] | wg_count[nwgf] | wg_off[nwgf + 1]; chol_table: r[nl][3]; chol_flag: present[nl] | split[nmol] */
   const bool fresh = ctx->chol_list_fresh || ctx->chol_ids.cap < (size_t)nl || ctx->chol_int.cap < (size_t)nl + 2 * (size_t)nwgf + 1;
   ENSURE(ctx, ctx->chol_ids, (size_t)nl);
   ENSURE(ctx, ctx->chol_int, (size_t)nl + 2 * (size_t)nwgf + 1);
   ENSURE(ctx, ctx->chol_table, 3 * (size_t)nl);
   ENSURE(ctx, ctx->chol_flag, (size_t)nl + nmol);
   int *d_perm = ctx->chol_int.p;
   unsigned *d_cnt = (unsigned *)(d_perm + nl), *d_off = d_cnt + nwgf;
   unsigned char *d_present = ctx->chol_flag.p, *d_split = d_present + nl;
   if (fresh)
   {
      HIPCHK(ctx, hipMemcpyAsync(ctx->chol_ids.p, ctx->chol_sorted.data(), (size_t)nl * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipMemcpyAsync(d_perm, ctx->chol_perm_h.data(), (size_t)nl * sizeof(int), hipMemcpyHostToDevice, st));
      ctx->chol_list_fresh = false;
   }
   HIPCHK(ctx, hipMemsetAsync(ctx->chol_table.p, 0, 3 * (size_t)nl * sizeof(double), st));
   HIPCHK(ctx, hipMemsetAsync(ctx->chol_flag.p, 0, (size_t)nl + nmol, st));
   CensusScratch cs;
   const int s_pd = cs.seg(8, (size_t)nwg * 6), s_od = cs.seg(8, 6), s_oc = cs.seg(8, nslot), s_pc = cs.seg(4, (size_t)nwg * nslot);
   int rc = cs.ensure(ctx);
   if (rc) return rc;
   hipLaunchKernelGGL(k_chol_gather, dim3(cdiv(n, 256)), dim3(256), 0, st, n, cp, ctx->chol_sorted.front(), ctx->chol_sorted.back(), nl, ctx->pos.p,
                      (const unsigned long long *)ctx->gid.p, ctx->chol_ids.p, d_perm, ctx->chol_table.p, d_present);
   hipLaunchKernelGGL(k_chol_eval, dim3(nwg), dim3(CENSUS_THREADS), (size_t)DDCMI_CHOL_LDS_BYTES(nbins), st, nmol, per_wg, cp, ctx->chol_table.p, d_present, d_split,
                      cs.at<double>(s_pd), cs.at<unsigned>(s_pc));
   CholFragSel frags = {d_present, d_split, ctx->chol_table.p, nullptr};
   compact_count(st, nl, per_wgf, nwgf, frags, d_cnt, d_off);
   std::vector<long long> hc((size_t)nslot);      /* counts | ndone: an array and a word of the caller's */
   unsigned nf = 0u;
   if ((rc = census_finish<RowsSumMinMax, long long>(ctx, nwg, 6, cs.at<double>(s_pd), cs.at<double>(s_od), stats, nslot, cs.at<unsigned>(s_pc), cs.at<long long>(s_oc),
                                                      hc.data(), [&]() -> int {
                                                         HIPCHK(ctx, hipMemcpyAsync(&nf, d_off + nwgf, sizeof(unsigned), hipMemcpyDeviceToHost, st));
                                                         return DDCMI_OK;
                                                      }))) return rc;
   for (int k = 0; k < 2 * nbins; k++) counts[k] = hc[k];
   *ndone = hc[(size_t)2 * nbins];
   *nfrag = nf;
   if (nf == 0u) return DDCMI_OK;
   ctx->chol_nfrag = nf;
   ENSURE(ctx, ctx->chol_frag, 4 * (size_t)nf);
   frags.rec = ctx->chol_frag.p;
   compact_pack(st, nl, per_wgf, nwgf, frags, d_off, nf);
   HIPCHK(ctx, hipGetLastError());
   return DDCMI_OK;
}
/* the nf fragments chol_one left packed, into the caller's room [sync] */
static int chol_copy_fragments(ddcmi_ctx *ctx, int64_t nf, ddcmi_chol_fragment *frag)
{
   if (nf <= 0) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   HIPCHK(ctx, hipMemcpyAsync(frag, ctx->chol_frag.p, sizeof(ddcmi_chol_fragment) * (size_t)nf, hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   return DDCMI_OK;
}

extern "C" int ddcmi_chol_offsets(ddcmi_ctx *ctx, int64_t nmol, const uint64_t *gid, double rmin, double delta, int nbins, int64_t *counts, int64_t *ndone,
                                  double *stats, int64_t cap, ddcmi_chol_fragment *frag, int64_t *nfrag)
{
   return analysis_single(ctx, "chol_offsets", true,
                          [=](ddcmi_ctx *c, const char *fn) { return chol_check(c, fn, nmol, gid, rmin, delta, nbins, counts, ndone, stats, cap, frag, nfrag); },
                          [=](ddcmi_ctx *c) -> int {
                             int rc = chol_one(c, nmol, rmin, delta, nbins, counts, ndone, stats, nfrag);
                             if (rc || nmol == 0 || !frag) return rc;
                             if (cap < *nfrag) SETERR(c, DDCMI_EINVAL, "ddcmi_chol_offsets: capacity %lld < %lld fragments", (long long)cap, (long long)*nfrag);
                             return chol_copy_fragments(c, *nfrag, frag);
                          });
}
/* the fragments of this context's last ddcmi_chol_offsets, which stay packed on the device until its next one: a copy, no pass.
 * Legal for the contexts of an in-process group as well [sync] */
extern "C" int ddcmi_chol_fragments(ddcmi_ctx *ctx, int64_t cap, ddcmi_chol_fragment *frag, int64_t *nfrag)
{
   ARGCHK(ctx, !nfrag, "ddcmi_chol_fragments: NULL nfrag");
   *nfrag = ctx->chol_nfrag;
   if (!frag) return DDCMI_OK;
   if (cap < ctx->chol_nfrag) SETERR(ctx, DDCMI_EINVAL, "ddcmi_chol_fragments: capacity %lld < %lld fragments", (long long)cap, (long long)ctx->chol_nfrag);
   return chol_copy_fragments(ctx, ctx->chol_nfrag, frag);
}
/* in-process group: per-rank blocks, rank after rank (counts[r * 2 nbins ...], ndone[r], stats[r * 6 ...], nfrag[r]); with frag, the
 * domains' fragments one block behind the other in rank order, cap their sum's room */
extern "C" int ddcmi_group_chol_offsets(ddcmi_ctx **ctxs, int n, int64_t nmol, const uint64_t *gid, double rmin, double delta, int nbins, int64_t *counts,
                                        int64_t *ndone, double *stats, int64_t cap, ddcmi_chol_fragment *frag, int64_t *nfrag)
{
   return analysis_group_records(ctxs, n, "chol_offsets", "fragments",
                                 [=](ddcmi_ctx *c, const char *fn) { return chol_check(c, fn, nmol, gid, rmin, delta, nbins, counts, ndone, stats, cap, frag, nfrag); },
                                 [=](ddcmi_ctx *c, size_t r) { return chol_one(c, nmol, rmin, delta, nbins, counts + r * 2 * (size_t)nbins, ndone + r, stats + 6 * r, nfrag + r); },
                                 nmol != 0 && frag, cap, nfrag, [=](ddcmi_ctx *c, size_t r, int64_t off) { return chol_copy_fragments(c, nfrag[r], frag + off); });
}

/* ddcmi_track.inl -- ANALYSIS type FORCE_AVERAGE on the device (forceAverage.c:76-145, forceAverage_eval): running sums of the
 * force, the velocity or the position of the beads with listed gids, kept on the device between evaluations.  Included from ddcmi.hip
 * behind ddcmi_chol.inl.  Read-only with respect to the run like a census pass (ddcmi_census_frame.inl) -- no halo slot, no
 * communication, no atomics of any kind -- but unlike one it returns nothing: an evaluation is one launch on the context's stream and
 * the host does not wait; the sums come back when the window is read (ddcmi_track_read).
 *
 * The list is kept ascending and unique (track_ids, nu entries); the caller's order, duplicates included, lives on the host as
 * track_slot[k] = the place of the caller's k-th gid among the unique ones, and the read expands by it.
 *
 *   k_track_accumulate   over the owned beads, census_split over at most TRACK_MAX_WG workgroups.  A workgroup first stages pivots of
 *                   the list in LDS: every stride-th gid, stride the least power of two with nu / stride <= TRACK_LDS_IDS, so a list
 *                   of up to TRACK_LDS_IDS gids is staged whole (stride 1).  A bead whose gid lies outside [least, greatest listed
 *                   gid] (kernel arguments: scalar registers) is done after the 8-byte load of its gid.  The others search the
 *                   pivots in LDS for the last one <= gid and, with stride > 1, the stride gids behind it in global memory
 *                   (log2 stride dependent loads, not log2 nu).  Only a hit loads its three components and does
 *                   sum[3 u .. 3 u + 2] += value, hits[u] += 1: a gid is owned by one bead of one rank, so slot u has one writer
 *                   in the launch, and launches on one stream are ordered -- a plain load, add and store.
 * The value is what a download returns at this point: the force arrays as they stand, the stored velocity, the slot's position
 * shifted once by the box side where it left a periodic box (census_position).
 * The accumulators belong to the rank, not to the bead: a tracked bead that migrates adds to its new owner's sums, and the window's
 * value is the sum of the ranks' partial sums.  Nothing travels in the migration records. */

#define TRACK_LDS_IDS 1024      /* pivots staged per workgroup: 8 KB of LDS */
#define TRACK_MAX_WG 512        /* two workgroups per CU: each stages the pivots once */

struct TrackBeads { const double4 *pos; const double *ax, *ay, *az; CensusBox box; };

template <int WHAT>      /* 0 force, 1 velocity (both: the arrays ax, ay, az), 2 position */
__global__ __launch_bounds__(CENSUS_THREADS) void k_track_accumulate(int n, int per_wg, unsigned long long gmin, unsigned long long gmax, int nu, int lstride,
                                                                     const unsigned long long *__restrict__ ids, const unsigned long long *__restrict__ gid,
                                                                     const TrackBeads b, double *__restrict__ sum, unsigned long long *__restrict__ hits)
{
   __shared__ unsigned long long piv_s[TRACK_LDS_IDS];
   const int stride = 1 << lstride, npiv = (nu + stride - 1) >> lstride;      /* <= TRACK_LDS_IDS (track_lstride) */
   for (int k = threadIdx.x; k < npiv; k += CENSUS_THREADS) piv_s[k] = ids[(size_t)k << lstride];
   __syncthreads();
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int i = beg + (int)threadIdx.x; i < end; i += CENSUS_THREADS)
   {
      const unsigned long long g = gid[i];
      if (!gid_in_range(g, gmin, gmax)) continue;
      int lo = 0, hi = npiv;      /* the first pivot > g; g >= gmin = piv_s[0], so it is not the first one */
      while (lo < hi)
      {
         const int mid = lo + ((hi - lo) >> 1);
         if (piv_s[mid] <= g) lo = mid + 1; else hi = mid;
      }
      int u = lo - 1;
      if (u < 0) continue;
      if (lstride == 0) { if (piv_s[u] != g) continue; }
      else
      {
         /* g is among the gids ids[a, e) behind its pivot, or not listed: where e < nu, ids[e] is the next pivot, and that is > g (the
          * pivot search), so "the first entry >= g lies in [a, e) and is g" says what "it lies in [a, nu) and is g" said.  (u is
          * written on a miss too: the bead is done then.) */
         const int a = u << lstride;
         if (!gid_find(ids, a, min(nu, a + stride), g, &u)) continue;
      }
      double v[3];
      if (WHAT == 2) census_position(b.box, b.pos[i], v);
      else { v[0] = b.ax[i]; v[1] = b.ay[i]; v[2] = b.az[i]; }
      double *s = sum + 3 * (size_t)u;
      s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
      hits[u] += 1ull;
   }
}

/* ---- host side ---------------------------------------------------------- */
static int track_lstride(size_t nu) { int l = 0; while (((nu + ((size_t)1 << l) - 1) >> l) > (size_t)TRACK_LDS_IDS) l++; return l; }
static int track_zero(ddcmi_ctx *ctx)
{
   const size_t nu = ctx->track_sorted.size();
   ctx->track_what = -1;
   if (nu == 0) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   HIPCHK(ctx, hipMemsetAsync(ctx->track_sum.p, 0, 3 * nu * sizeof(double), ctx->stream));
   HIPCHK(ctx, hipMemsetAsync(ctx->track_hits.p, 0, nu * sizeof(unsigned long long), ctx->stream));
   return DDCMI_OK;
}

/* Legal for the contexts of an in-process group as well, like the two calls below: nothing here is collective. */
extern "C" int ddcmi_track_set(ddcmi_ctx *ctx, int64_t n, const uint64_t *gid)
{
   ARGCHK(ctx, n < 0, "ddcmi_track_set: n = %lld", (long long)n);
   ARGCHK(ctx, n > 0 && !gid, "ddcmi_track_set: NULL gid with n = %lld", (long long)n);
   if (n > (int64_t)DDCMI_TRACK_MAX_IDS) SETERR(ctx, DDCMI_EUNSUPPORTED, "ddcmi_track_set: %lld gids, at most %d are tracked", (long long)n, DDCMI_TRACK_MAX_IDS);
   (void)hipSetDevice(ctx->device);
   if (n == 0)
   {
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      /* (a launch that reads the buffers may still be queued) */
      ctx->track_list.clear(); ctx->track_sorted.clear(); ctx->track_slot.clear(); ctx->track_what = -1;
      ctx->track_ids.release(); ctx->track_sum.release(); ctx->track_hits.release();
      return DDCMI_OK;
   }
   std::vector<unsigned long long> ids(gid, gid + n);
   std::sort(ids.begin(), ids.end());
   ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
   std::vector<int> slot((size_t)n);
   for (int64_t k = 0; k < n; k++) slot[k] = (int)(std::lower_bound(ids.begin(), ids.end(), (unsigned long long)gid[k]) - ids.begin());
   const size_t nu = ids.size();
   ENSURE(ctx, ctx->track_ids, nu);
   ENSURE(ctx, ctx->track_sum, 3 * nu);
   ENSURE(ctx, ctx->track_hits, nu);
   ctx->track_list.assign(gid, gid + n);
   ctx->track_sorted.swap(ids);
   ctx->track_slot.swap(slot);
   HIPCHK(ctx, hipMemcpyAsync(ctx->track_ids.p, ctx->track_sorted.data(), nu * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
   return track_zero(ctx);
}

extern "C" int ddcmi_track_accumulate(ddcmi_ctx *ctx, int what)
{
   ARGCHK(ctx, what < 0 || what > 2, "ddcmi_track_accumulate: what = %d (0 force, 1 velocity, 2 position)", what);
   if (ctx->track_sorted.empty()) return DDCMI_OK;
   int rc = census_state_check(ctx, "ddcmi_track_accumulate");
   if (rc) return rc;
   ARGCHK(ctx, ctx->track_what >= 0 && ctx->track_what != what, "ddcmi_track_accumulate: what = %d, and this window holds sums of what = %d: a window averages one quantity "
          "(ddcmi_track_read with reset, or ddcmi_track_set, begins the next one)", what, ctx->track_what);
   const int n = ctx->nloc;
   if (what == 0 && n > 0 && (!ctx->forces_valid || ctx->fx.cap < (size_t)n))
      SETERR(ctx, DDCMI_EINVAL, "ddcmi_track_accumulate needs forces: call ddcmi_eval_forces first (firstEnergyCall, masters.c:579)");
   if (what == 2 && n > 0 && !ctx->have_box) SETERR(ctx, DDCMI_EINVAL, "ddcmi_track_accumulate needs a box (ddcmi_set_box)");
   ctx->track_what = what;
   if (n <= 0) return DDCMI_OK;      /* (a domain that holds no bead) */
   (void)hipSetDevice(ctx->device);
   const int nu = (int)ctx->track_sorted.size();
   int per_wg, nwg;
   census_split(n, TRACK_MAX_WG, &per_wg, &nwg);
   TrackBeads b;
   b.pos = ctx->pos.p; census_set_box(ctx, b.box);
   if (what == 0) { b.ax = ctx->fx.p; b.ay = ctx->fy.p; b.az = ctx->fz.p; }
   else { b.ax = ctx->vx.p; b.ay = ctx->vy.p; b.az = ctx->vz.p; }
   const auto k = what == 2 ? k_track_accumulate<2> : what == 1 ? k_track_accumulate<1> : k_track_accumulate<0>;
   hipLaunchKernelGGL(k, dim3(nwg), dim3(CENSUS_THREADS), 0, ctx->stream, n, per_wg, ctx->track_sorted.front(), ctx->track_sorted.back(), nu, track_lstride((size_t)nu),
                      ctx->track_ids.p, (const unsigned long long *)ctx->gid.p, b, ctx->track_sum.p, ctx->track_hits.p);
   HIPCHK(ctx, hipGetLastError());
   return DDCMI_OK;
}

extern "C" int ddcmi_track_read(ddcmi_ctx *ctx, int64_t n, double *sum, int64_t *hits, int reset)
{
   ARGCHK(ctx, n != (int64_t)ctx->track_list.size(), "ddcmi_track_read: n = %lld, the tracked list has %lld gids", (long long)n, (long long)ctx->track_list.size());
   ARGCHK(ctx, n > 0 && (!sum || !hits), "ddcmi_track_read: NULL output array (sum %p, hits %p)", (const void *)sum, (const void *)hits);
   if (n == 0) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   int rc = ddcmi_agree_poll(ctx);
   if (rc) return rc;
   const size_t nu = ctx->track_sorted.size();
   std::vector<double> hs(3 * nu);
   std::vector<unsigned long long> hh(nu);
   HIPCHK(ctx, hipMemcpyAsync(hs.data(), ctx->track_sum.p, 3 * nu * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipMemcpyAsync(hh.data(), ctx->track_hits.p, nu * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   for (int64_t k = 0; k < n; k++)
   {
      const size_t u = (size_t)ctx->track_slot[k];
      sum[3 * k] = hs[3 * u]; sum[3 * k + 1] = hs[3 * u + 1]; sum[3 * k + 2] = hs[3 * u + 2];
      hits[k] = (int64_t)hh[u];
   }
   return reset ? track_zero(ctx) : DDCMI_OK;
}

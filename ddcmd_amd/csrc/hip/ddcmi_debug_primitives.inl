/* ddcmi_debug_primitives.inl -- TEST-ONLY entry points (include/ddcmi_test.h) that run the device primitives every kernel shares on a test's own
 * numbers: the four reciprocals of ddcmi_internal.h and the bare double-precision seeds under them, the wave scan / maximum / row sum of
 * ddcmi.hip, lean_effective of ddcmi_nonbond.inl, ddcmi_scan_exclusive of scan.hip and the two in-cell sorts.  Part of the ONE translation
 * unit ddcmi.hip, included last: the hooks call the very __device__ functions and launch the very kernels the product does, and change
 * none of them.  Like ddcmi_debug_wave_reduce each hook allocates, copies in, launches once, copies out and frees. [sync] */
template <int W>
__global__ __launch_bounds__(256) void k_debug_recip(int n, const double *__restrict__ in, double *__restrict__ out)
{
   const int i = blockIdx.x * 256 + threadIdx.x;
   if (i >= n) return;
   const double x = in[i];
   out[i] = W == 0 ? rsqrt_f64(x) : W == 1 ? rcp_f64(x) : W == 2 ? rsqrt_f64_pair(x) : W == 3 ? rcp_f64_pair(x) : W == 4 ? __builtin_amdgcn_rsq(x) : __builtin_amdgcn_rcp(x);
}
extern "C" int ddcmi_debug_recip(int which, int n, const double *in, double *out)
{
   if (which < 0 || which > 5 || n < 1 || n > (1 << 24) || !in || !out) return DDCMI_EINVAL;
   double *d = nullptr;
   if (hipMalloc((void **)&d, 2 * (size_t)n * sizeof(double)) != hipSuccess) return DDCMI_ENOMEM;
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d, in, (size_t)n * sizeof(double), hipMemcpyHostToDevice) == hipSuccess)
   {
      const dim3 g(cdiv(n, 256)), b(256);
      switch (which)
      {
         case 0: hipLaunchKernelGGL(k_debug_recip<0>, g, b, 0, 0, n, d, d + n); break;
         case 1: hipLaunchKernelGGL(k_debug_recip<1>, g, b, 0, 0, n, d, d + n); break;
         case 2: hipLaunchKernelGGL(k_debug_recip<2>, g, b, 0, 0, n, d, d + n); break;
         case 3: hipLaunchKernelGGL(k_debug_recip<3>, g, b, 0, 0, n, d, d + n); break;
         case 4: hipLaunchKernelGGL(k_debug_recip<4>, g, b, 0, 0, n, d, d + n); break;
         default: hipLaunchKernelGGL(k_debug_recip<5>, g, b, 0, 0, n, d, d + n); break;
      }
      if (hipGetLastError() == hipSuccess && hipMemcpy(out, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}

/* one wave per set of 64 values, every lane's result stored: W = 0 wave_scan_inclusive_dpp, 1 wave_max_dpp (int), 2 row_sum_dpp (double),
 * 3 lean_effective (float; the lane is the thread, as k_nonbond calls it) */
template <int W>
__global__ __launch_bounds__(64) void k_debug_wave_ops(const void *__restrict__ in, void *__restrict__ out)
{
   const int lane = threadIdx.x;
   const size_t i = (size_t)blockIdx.x * 64 + lane;
   if (W == 0) ((int *)out)[i] = wave_scan_inclusive_dpp(((const int *)in)[i]);
   else if (W == 1) ((int *)out)[i] = wave_max_dpp(((const int *)in)[i]);
   else if (W == 2) ((double *)out)[i] = row_sum_dpp(((const double *)in)[i]);
   else ((float *)out)[i] = lean_effective(((const float *)in)[i], lane);
}
extern "C" int ddcmi_debug_wave_ops(int which, int nsets, const void *in, void *out)
{
   if (which < 0 || which > 3 || nsets < 1 || nsets > 65535 || !in || !out) return DDCMI_EINVAL;
   const size_t nb = (size_t)nsets * 64 * (which == 2 ? sizeof(double) : 4);
   char *d = nullptr;
   if (hipMalloc((void **)&d, 2 * nb) != hipSuccess) return DDCMI_ENOMEM;
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d, in, nb, hipMemcpyHostToDevice) == hipSuccess)
   {
      const dim3 g(nsets), b(64);
      switch (which)
      {
         case 0: hipLaunchKernelGGL(k_debug_wave_ops<0>, g, b, 0, 0, (const void *)d, (void *)(d + nb)); break;
         case 1: hipLaunchKernelGGL(k_debug_wave_ops<1>, g, b, 0, 0, (const void *)d, (void *)(d + nb)); break;
         case 2: hipLaunchKernelGGL(k_debug_wave_ops<2>, g, b, 0, 0, (const void *)d, (void *)(d + nb)); break;
         default: hipLaunchKernelGGL(k_debug_wave_ops<3>, g, b, 0, 0, (const void *)d, (void *)(d + nb)); break;
      }
      if (hipGetLastError() == hipSuccess && hipMemcpy(out, d + nb, nb, hipMemcpyDeviceToHost) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}

/* ddcmi_scan_exclusive as the rebuild calls it: on the context's stream, with the context's scan_tmp.  The device destination is n +
 * DDCMI_DEBUG_SCAN_GUARD ints long and starts as the caller's out[] (in place: in[] and, behind it, out[n ...]), so that the caller sees what
 * the scan left alone -- all of out[] where n <= 0, the guard behind element n otherwise */
extern "C" int ddcmi_debug_scan(ddcmi_ctx *ctx, int n, const int *in, int *out, int *total, int in_place)
{
   ARGCHK(ctx, n > (1 << 28), "ddcmi_debug_scan: n = %d is more than 2^28", n);
   ARGCHK(ctx, !out || (n > 0 && !in), "ddcmi_debug_scan: in or out is NULL");
   (void)hipSetDevice(ctx->device);
   const size_t nn = n > 0 ? (size_t)n : 0, nd = nn + DDCMI_DEBUG_SCAN_GUARD;
   int *d = nullptr;
   if (hipMalloc((void **)&d, (2 * nd + 1) * sizeof(int)) != hipSuccess) SETERR(ctx, DDCMI_ENOMEM, "ddcmi_debug_scan: device allocation of %zu ints failed", 2 * nd + 1);
   int *d_src = d, *d_dst = in_place ? d : d + nd, *d_tot = d + 2 * nd;
   const int poison = -123456789;      /* (a scan that forgets the total leaves this) */
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpyAsync(d_dst, out, nd * sizeof(int), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
       (nn == 0 || hipMemcpyAsync(d_src, in, nn * sizeof(int), hipMemcpyHostToDevice, ctx->stream) == hipSuccess) &&
       hipMemcpyAsync(d_tot, &poison, sizeof(int), hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
       (rc = ddcmi_scan_exclusive(ctx, d_src, d_dst, n, total ? d_tot : nullptr)) == DDCMI_OK)
   {
      rc = DDCMI_ENODEVICE;
      if (hipGetLastError() == hipSuccess && hipMemcpyAsync(out, d_dst, nd * sizeof(int), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
          (!total || hipMemcpyAsync(total, d_tot, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) == hipSuccess) &&
          hipStreamSynchronize(ctx->stream) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipStreamSynchronize(ctx->stream);
   (void)hipFree(d);
   if (rc == DDCMI_ENODEVICE) ctx->err = "ddcmi_debug_scan: a copy or a launch failed";
   return rc;
}

/* k_sort_cells (key == NULL) or k_sort_cells_key with the rebuild's launch shape.  The tables are checked on the host first: a cell outside
 * order[] or an entry of a cell that names no key would be an address */
extern "C" int ddcmi_debug_sort_cells(int ncell, const int *start, const int *cnt, int norder, int *order, const uint64_t *key, const int *key2)
{
   if (ncell < 1 || ncell > (1 << 20) || norder < 1 || norder > (1 << 24) || !start || !cnt || !order || (key2 && !key)) return DDCMI_EINVAL;
   for (int c = 0; c < ncell; c++)
   {
      if (start[c] < 0 || cnt[c] < 0 || start[c] > norder || cnt[c] > norder - start[c]) return DDCMI_EINVAL;
      if (key) for (int k = start[c]; k < start[c] + cnt[c]; k++) if (order[k] < 0 || order[k] >= norder) return DDCMI_EINVAL;
   }
   const size_t nk = key ? (size_t)norder : 0, nk2 = key2 ? (size_t)norder : 0;
   const size_t bytes = nk * sizeof(uint64_t) + ((size_t)2 * ncell + norder + nk2) * sizeof(int);
   char *d = nullptr;
   if (hipMalloc((void **)&d, bytes) != hipSuccess) return DDCMI_ENOMEM;
   uint64_t *d_key = (uint64_t *)d;
   int *d_start = (int *)(d + nk * sizeof(uint64_t)), *d_cnt = d_start + ncell, *d_order = d_cnt + ncell, *d_key2 = d_order + norder;
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d_start, start, (size_t)ncell * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_cnt, cnt, (size_t)ncell * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_order, order, (size_t)norder * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       (!key || hipMemcpy(d_key, key, nk * sizeof(uint64_t), hipMemcpyHostToDevice) == hipSuccess) &&
       (!key2 || hipMemcpy(d_key2, key2, nk2 * sizeof(int), hipMemcpyHostToDevice) == hipSuccess))
   {
      const int ncb = cdiv(ncell, 256);
      if (key) hipLaunchKernelGGL(k_sort_cells_key, dim3(ncb), dim3(256), 0, 0, ncell, d_start, d_cnt, d_order, d_key, key2 ? (const int *)d_key2 : (const int *)nullptr);
      else hipLaunchKernelGGL(k_sort_cells, dim3(ncb), dim3(256), 0, 0, ncell, d_start, d_cnt, d_order);
      if (hipGetLastError() == hipSuccess && hipMemcpy(order, d_order, (size_t)norder * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}

/* the census frame's stable compaction (k_compact_count, k_compact_scan, k_compact_pack of ddcmi_census_frame.inl, launched by the
 * product's compact_count / compact_pack over census_split(n, max_wg)) on the caller's 0 / 1 flags: the kept slots' indices in slot
 * order.  The device array of places is nrec + DDCMI_DEBUG_COMPACT_GUARD long and starts as the caller's */
struct DebugFlagSel
{
   const int *flags; int *places;
   struct Item {};
   __device__ __forceinline__ bool selected(int i, Item &) const { return flags[i] != 0; }
   __device__ __forceinline__ void store(int i, unsigned place, const Item &) const { places[place] = i; }
};
extern "C" int ddcmi_debug_compact(int n, const int *flags, int max_wg, int nrec, int *places, int *total)
{
   if (n < 1 || n > (1 << 24) || max_wg < 1 || max_wg > 2048 || nrec < 0 || nrec > (1 << 24) || !flags || !places || !total) return DDCMI_EINVAL;
   int per_wg, nwg;
   census_split(n, max_wg, &per_wg, &nwg);
   const size_t np = (size_t)nrec + DDCMI_DEBUG_COMPACT_GUARD;
   int *d = nullptr;
   if (hipMalloc((void **)&d, ((size_t)n + np + 2 * (size_t)nwg + 1) * sizeof(int)) != hipSuccess) return DDCMI_ENOMEM;
   int *d_flags = d, *d_places = d + n;
   unsigned *d_cnt = (unsigned *)(d_places + np), *d_off = d_cnt + nwg, t = 0u;
   const DebugFlagSel sel = {d_flags, d_places};
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d_flags, flags, (size_t)n * sizeof(int), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_places, places, np * sizeof(int), hipMemcpyHostToDevice) == hipSuccess)
   {
      compact_count((hipStream_t)0, n, per_wg, nwg, sel, d_cnt, d_off);
      compact_pack((hipStream_t)0, n, per_wg, nwg, sel, d_off, (unsigned)nrec);
      if (hipGetLastError() == hipSuccess && hipMemcpy(places, d_places, np * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess &&
          hipMemcpy(&t, d_off + nwg, sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess) { *total = (int)t; rc = DDCMI_OK; }
   }
   (void)hipFree(d);
   return rc;
}

/* gid_find of ddcmi_census_frame.inl over ids[lo, hi), one thread per query: the index of the query, -1 where it is not in the range.  I: the
 * index type of the call -- int as cholAnalysis and FORCE_AVERAGE (a sub-range: the gids behind a pivot) call it, long long as subsetWrite does */
template <class I>
__global__ __launch_bounds__(256) void k_debug_gid_find(I lo, I hi, const unsigned long long *__restrict__ ids, int nq, const unsigned long long *__restrict__ queries,
                                                        int *__restrict__ index)
{
   const int q = blockIdx.x * 256 + threadIdx.x;
   if (q >= nq) return;
   I at;
   index[q] = gid_find(ids, lo, hi, queries[q], &at) ? (int)at : -1;
}
extern "C" int ddcmi_debug_gid_find_in(int nids, const uint64_t *ids, int lo, int hi, int wide, int nq, const uint64_t *queries, int *index)
{
   if (nids < 1 || nids > (1 << 24) || lo < 0 || hi < lo || hi > nids || nq < 1 || nq > (1 << 24) || !ids || !queries || !index) return DDCMI_EINVAL;
   for (int k = 1; k < nids; k++) if (ids[k] < ids[k - 1]) return DDCMI_EINVAL;
   unsigned long long *d = nullptr;
   if (hipMalloc((void **)&d, ((size_t)nids + nq) * sizeof(unsigned long long) + (size_t)nq * sizeof(int)) != hipSuccess) return DDCMI_ENOMEM;
   unsigned long long *d_ids = d, *d_q = d + nids;
   int *d_index = (int *)(d_q + nq);
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d_ids, ids, (size_t)nids * sizeof(uint64_t), hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d_q, queries, (size_t)nq * sizeof(uint64_t), hipMemcpyHostToDevice) == hipSuccess)
   {
      if (wide) hipLaunchKernelGGL(k_debug_gid_find<long long>, dim3(cdiv(nq, 256)), dim3(256), 0, 0, (long long)lo, (long long)hi, d_ids, nq, d_q, d_index);
      else hipLaunchKernelGGL(k_debug_gid_find<int>, dim3(cdiv(nq, 256)), dim3(256), 0, 0, lo, hi, d_ids, nq, d_q, d_index);
      if (hipGetLastError() == hipSuccess && hipMemcpy(index, d_index, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}
extern "C" int ddcmi_debug_gid_find(int nids, const uint64_t *ids, int nq, const uint64_t *queries, int *index)
{
   return ddcmi_debug_gid_find_in(nids, ids, 0, nids, 0, nq, queries, index);
}

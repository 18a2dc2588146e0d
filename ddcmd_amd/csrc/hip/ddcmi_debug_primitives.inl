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

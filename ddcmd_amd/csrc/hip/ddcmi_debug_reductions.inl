/* ddcmi_debug_reductions.inl -- TEST-ONLY entry points (include/ddcmi_test.h) that run the cross-workgroup reductions on a test's own rows:
 * reduce_jobs_block through its three front ends (k_reduce_jobs with one and with two jobs, k_reduce_jobs_images) and through k_reduce_hist,
 * block_reduce_store / block_vmax_store, k_census_final and the plain finishers k_group_ke_sum / k_class_kinetic_sum.  (reduce_gather_row and
 * k_mol_sum live in bonded.hip, and so do their hooks.)  Part of the ONE translation unit ddcmi.hip, included last: the hooks launch the very
 * kernels of the product with the product's launch shapes and change none of them.  Every hook checks its arguments on the host -- a bad count
 * is DDCMI_EINVAL and never an address --, allocates, copies in, launches, copies out and frees.  Device outputs start as the caller's
 * arrays, so that the caller's poison shows what no kernel wrote. [sync] */
static bool debug_red_ok(hipError_t e) { return e == hipSuccess; }

extern "C" int ddcmi_debug_reduce_jobs(int nlaunch, const int *front, const int nrows[2], const int nv[2], const double *part0, const double *part1,
                                       const double disp_dt[2], const double disp0[2], double *out, double *disp)
{
   if (nlaunch < 1 || nlaunch > 64 || !front || !nrows || !nv || !part0 || !part1 || !disp_dt || !disp0 || !out || !disp) return DDCMI_EINVAL;
   for (int l = 0; l < nlaunch; l++) if (front[l] < 0 || front[l] > 2) return DDCMI_EINVAL;
   for (int q = 0; q < 2; q++)
   {
      if (nrows[q] < 1 || nrows[q] > (1 << 20)) return DDCMI_EINVAL;
      if (nv[q] != 0 && nv[q] != 3 && nv[q] != 7 && nv[q] != 8) return DDCMI_EINVAL;
      if (!(disp_dt[q] >= 0.0) || !(disp_dt[q] < 1e300) || (disp_dt[q] > 0.0 && nv[q] == 8)) return DDCMI_EINVAL;      /* (column 7 is a sum or a maximum, not both) */
   }
   const size_t n0 = (size_t)nrows[0] * 8, n1 = (size_t)nrows[1] * 8;
   double *d = nullptr;
   if (hipMalloc((void **)&d, (n0 + n1 + RED_TMP_DOUBLES + 16 + 2) * sizeof(double)) != hipSuccess) return DDCMI_ENOMEM;
   double *d_p0 = d, *d_p1 = d + n0, *d_tmp = d_p1 + n1, *d_out = d_tmp + RED_TMP_DOUBLES, *d_disp = d_out + 16;
   int rc = DDCMI_ENODEVICE;
   bool ok = debug_red_ok(hipMemcpy(d_p0, part0, n0 * sizeof(double), hipMemcpyHostToDevice)) &&
             debug_red_ok(hipMemcpy(d_p1, part1, n1 * sizeof(double), hipMemcpyHostToDevice)) &&
             debug_red_ok(hipMemset(d_tmp, 0, RED_TMP_DOUBLES * sizeof(double))) &&      /* (as ddcmi_create does it for red_tmp) */
             debug_red_ok(hipMemcpy(d_disp, disp0, 2 * sizeof(double), hipMemcpyHostToDevice));
   const RedJob j0 = {d_p0, nrows[0], nv[0], d_out, 0, disp_dt[0], d_disp};
   const RedJob j1 = {d_p1, nrows[1], nv[1], d_out + 8, 0, disp_dt[1], d_disp + 1};
   for (int l = 0; ok && l < nlaunch; l++)
   {
      ok = debug_red_ok(hipMemcpy(d_out, out + (size_t)16 * l, 16 * sizeof(double), hipMemcpyHostToDevice));
      if (!ok) break;
      if (front[l] == 0) hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 1), dim3(1024), 0, 0, j0, j0, (double *)nullptr, 0.0, d_tmp);
      else if (front[l] == 1) hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 2), dim3(1024), 0, 0, j0, j1, (double *)nullptr, 0.0, d_tmp);
      else
      {
         ImageJob im = {}; PackJob pk = {};      /* no image, nothing to pack: the launch is the two jobs' workgroups alone */
         hipLaunchKernelGGL(k_reduce_jobs_images, dim3(2 * RED_SPLIT + cdiv(im.nhalo, 1024)), dim3(1024), 0, 0, j0, j1, (double *)nullptr, 0.0, d_tmp, im, pk);
      }
      ok = debug_red_ok(hipGetLastError()) && debug_red_ok(hipMemcpy(out + (size_t)16 * l, d_out, 16 * sizeof(double), hipMemcpyDeviceToHost)) &&
           debug_red_ok(hipMemcpy(disp + (size_t)2 * l, d_disp, 2 * sizeof(double), hipMemcpyDeviceToHost));
   }
   if (ok) rc = DDCMI_OK;
   (void)hipFree(d);
   return rc;
}

extern "C" int ddcmi_debug_reduce_hist(int nflush, const int *nsteps, int nrows, long long stride, const double *pair, const double *kin, double *hist)
{
   if (nflush < 1 || nflush > 16 || !nsteps || nrows < 1 || nrows > 8192 || stride < (long long)nrows * 8 || stride > (1 << 17) || !pair || !kin || !hist) return DDCMI_EINVAL;
   for (int i = 0; i < nflush; i++) if (nsteps[i] < 1 || nsteps[i] > LEAN_W) return DDCMI_EINVAL;
   const size_t ring = (size_t)LEAN_W * (size_t)stride, nh = (size_t)LEAN_HW * LEAN_W;
   double *d = nullptr;
   if (hipMalloc((void **)&d, (2 * ring + nh + LEAN_TMP_DOUBLES) * sizeof(double)) != hipSuccess) return DDCMI_ENOMEM;
   double *d_pair = d, *d_kin = d + ring, *d_hist = d_kin + ring, *d_tmp = d_hist + nh;
   bool ok = debug_red_ok(lean_tmp_zero(d_tmp, 0)) && debug_red_ok(hipMemset(d_hist, 0xff, nh * sizeof(double)));
   size_t in_off = 0, h_off = 0;
   for (int i = 0; ok && i < nflush; i++)
   {
      const int np = nsteps[i];
      const size_t nin = (size_t)np * (size_t)stride, nout = (size_t)LEAN_HW * np;
      ok = debug_red_ok(hipMemcpy(d_pair, pair + in_off, nin * sizeof(double), hipMemcpyHostToDevice)) &&
           debug_red_ok(hipMemcpy(d_kin, kin + in_off, nin * sizeof(double), hipMemcpyHostToDevice)) &&
           debug_red_ok(hipMemcpy(d_hist, hist + h_off, nout * sizeof(double), hipMemcpyHostToDevice));
      if (!ok) break;
      const RedJob jf = {d_pair, nrows, 8, nullptr, 0, 0.0, nullptr};
      const RedJob jk = {d_kin, nrows, 7, nullptr, 0, 0.0, nullptr};
      lean_launch_hist(jf, jk, (size_t)stride, np, d_hist, d_tmp, 0);
      ok = debug_red_ok(hipGetLastError()) && debug_red_ok(hipMemcpy(hist + h_off, d_hist, nout * sizeof(double), hipMemcpyDeviceToHost));
      in_off += nin; h_off += nout;
   }
   (void)hipFree(d);
   return ok ? DDCMI_OK : DDCMI_ENODEVICE;
}

/* one workgroup of 256 threads per block of in[256][NV]: thread t's NV values through block_reduce_store<NV> into out[block][16] */
template <int NV>
__global__ __launch_bounds__(DDCMI_BLOCK) void k_debug_block_reduce(const double *__restrict__ in, double *__restrict__ out)
{
   const double *p = in + ((size_t)blockIdx.x * DDCMI_BLOCK + threadIdx.x) * NV;
   double v[NV];
#pragma unroll
   for (int k = 0; k < NV; k++) v[k] = p[k];
   block_reduce_store<NV>(v, out + (size_t)blockIdx.x * 16);
}
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_debug_block_vmax(const float *__restrict__ in, double *__restrict__ out)
{
   block_vmax_store<NW>(in[(size_t)blockIdx.x * NW * 64 + threadIdx.x], out + (size_t)blockIdx.x * 16);
}
extern "C" int ddcmi_debug_block_reduce(int which, int nblocks, const void *in, double *out)
{
   if (which < 0 || which > 4 || nblocks < 1 || nblocks > 4096 || !in || !out) return DDCMI_EINVAL;
   const int nvs[5] = {7, 3, KD_NV, 1, 1};
   const size_t nin = (size_t)nblocks * DDCMI_BLOCK * nvs[which] * (which < 3 ? sizeof(double) : sizeof(float)), nout = (size_t)nblocks * 16 * sizeof(double);
   if (which >= 3)      /* the maximum orders non-negative floats by their bit patterns: anything else is not its domain */
   {
      const float *f = (const float *)in;
      for (size_t i = 0; i < (size_t)nblocks * DDCMI_BLOCK; i++) if (!(f[i] >= 0.0f)) return DDCMI_EINVAL;
   }
   char *d = nullptr;
   if (hipMalloc((void **)&d, nin + nout + 16) != hipSuccess) return DDCMI_ENOMEM;
   double *d_out = (double *)d; const void *d_in = d + nout;
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d + nout, in, nin, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_out, out, nout, hipMemcpyHostToDevice) == hipSuccess)
   {
      const dim3 g(nblocks), b(DDCMI_BLOCK);
      switch (which)
      {
         case 0: hipLaunchKernelGGL(k_debug_block_reduce<7>, g, b, 0, 0, (const double *)d_in, d_out); break;
         case 1: hipLaunchKernelGGL(k_debug_block_reduce<3>, g, b, 0, 0, (const double *)d_in, d_out); break;
         case 2: hipLaunchKernelGGL(k_debug_block_reduce<KD_NV>, g, b, 0, 0, (const double *)d_in, d_out); break;
         case 3: hipLaunchKernelGGL(k_debug_block_vmax<4>, g, b, 0, 0, (const float *)d_in, d_out); break;
         default: hipLaunchKernelGGL(k_debug_block_vmax<DDCMI_BLOCK / 64>, g, b, 0, 0, (const float *)d_in, d_out); break;
      }
      if (hipGetLastError() == hipSuccess && hipMemcpy(out, d_out, nout, hipMemcpyDeviceToHost) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}

extern "C" int ddcmi_debug_census_final(int which, int nwg, int nd, const double *part_d, double *out_d, int nc, const unsigned *part_c, void *out_c)
{
   if (which < 0 || which > 2 || nwg < 1 || nwg > VAF_MAX_WG || nd < 0 || nc < 0 || nd > 65536 || nc > 65536 || nd + nc < 1) return DDCMI_EINVAL;
   if ((nd > 0 && (!part_d || !out_d)) || (nc > 0 && (!part_c || !out_c))) return DDCMI_EINVAL;
   const size_t b_pd = (size_t)nwg * nd * sizeof(double), b_od = (size_t)nd * sizeof(double), b_oc = (size_t)nc * 8, b_pc = (size_t)nwg * nc * sizeof(unsigned);
   char *d = nullptr;
   if (hipMalloc((void **)&d, b_pd + b_od + b_oc + b_pc + 16) != hipSuccess) return DDCMI_ENOMEM;
   double *d_pd = (double *)d, *d_od = (double *)(d + b_pd); char *d_oc = d + b_pd + b_od; unsigned *d_pc = (unsigned *)(d_oc + b_oc);
   int rc = DDCMI_ENODEVICE;
   if ((nd == 0 || (hipMemcpy(d_pd, part_d, b_pd, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_od, out_d, b_od, hipMemcpyHostToDevice) == hipSuccess)) &&
       (nc == 0 || (hipMemcpy(d_pc, part_c, b_pc, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_oc, out_c, b_oc, hipMemcpyHostToDevice) == hipSuccess)))
   {
      const dim3 g(cdiv(std::max(nd, nc), 64)), b(64);
      const double *pd = nd ? d_pd : nullptr; double *od = nd ? d_od : nullptr; const unsigned *pc = nc ? d_pc : nullptr;
      if (which == 0) hipLaunchKernelGGL((k_census_final<RowsSum, double>), g, b, 0, 0, nwg, nd, pd, od, nc, pc, nc ? (double *)d_oc : nullptr);
      else if (which == 1) hipLaunchKernelGGL((k_census_final<RowsSum, long long>), g, b, 0, 0, nwg, nd, pd, od, nc, pc, nc ? (long long *)d_oc : nullptr);
      else hipLaunchKernelGGL((k_census_final<RowsSumMinMax, long long>), g, b, 0, 0, nwg, nd, pd, od, nc, pc, nc ? (long long *)d_oc : nullptr);
      if (hipGetLastError() == hipSuccess && (nd == 0 || hipMemcpy(out_d, d_od, b_od, hipMemcpyDeviceToHost) == hipSuccess) &&
          (nc == 0 || hipMemcpy(out_c, d_oc, b_oc, hipMemcpyDeviceToHost) == hipSuccess)) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}

extern "C" int ddcmi_debug_kinetic_finish(int which, int n, const double *part, double *out)
{
   if (which < 0 || which > 1 || n < 1 || n > (which == 0 ? 32 : 64) || !part || !out) return DDCMI_EINVAL;
   const size_t nin = (size_t)GKE_BLOCKS * (which == 0 ? 2 * n : 16 * n), nout = which == 0 ? (size_t)2 * n : (size_t)KD_NV * n;
   double *d = nullptr;
   if (hipMalloc((void **)&d, (nin + nout) * sizeof(double)) != hipSuccess) return DDCMI_ENOMEM;
   int rc = DDCMI_ENODEVICE;
   if (hipMemcpy(d, part, nin * sizeof(double), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d + nin, out, nout * sizeof(double), hipMemcpyHostToDevice) == hipSuccess)
   {
      if (which == 0) hipLaunchKernelGGL(k_group_ke_sum, dim3(1), dim3(64), 0, 0, n, d, d + nin);
      else hipLaunchKernelGGL(k_class_kinetic_sum, dim3(cdiv(n * KD_NV, 64)), dim3(64), 0, 0, n, d, d + nin);
      if (hipGetLastError() == hipSuccess && hipMemcpy(out, d + nin, nout * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess) rc = DDCMI_OK;
   }
   (void)hipFree(d);
   return rc;
}

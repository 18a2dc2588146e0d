/* ddcmi_analysis.inl -- ANALYSIS type PAIRCORRELATION on the device (paircorrelation.c:354-457, paircorrelation_eval_geom):
 * a histogram of pair distances by species pair, read-only with respect to the run.  Included from ddcmi.hip, behind the
 * multi-domain path (it uses the halo plan of the last rebuild).
 *
 * What is counted: for every bead i this rank owns and every OTHER bead j (owned or halo) with rmin <= r < rmax
 * (rmax = rmin + nbins delta_r), the ordered pair (i, j) when species(i) <= species(j), in bin k of combo comboIndex(a, b).
 * Over the ranks this is the reference's nBonds exactly: a like pair is met from both ends (2), an unlike one from the end of
 * lower species (1).  The counts are integers, so the result does not depend on the order of the atomics.
 *
 * The search is the analysis's own -- the force list only promises pairs up to the cut-off, and the step's paths stay as
 * they are: the beads are binned into cells of edge >= rmax (counting sort: k_pc_count, scan.hip's scan, k_pc_scatter) and
 * every owned bead walks the 3x3x3 stencil (k_pc_hist).  One domain: periodic axes wrap (cell indices modulo the cell count,
 * distances by minimum image; fewer than three cells on an axis visit each distinct cell once), open axes clamp.  A decomposed
 * rank: its owned beads plus the halo of the last rebuild with CURRENT positions -- owned sources of periodic self-images
 * shifted, received beads brought by one exchange of {x, y, z, species} into buffers of the analysis's own along the per-step
 * halo's messages (the run's send / receive buffers, tags and flags are not touched); no wrapping, every axis clamps.
 * Histogram: ncombo x nbins u32 counters in LDS per workgroup (in passes over slices of the combos when they do not fit
 * PC_LDS_WORDS), flushed with u64 global atomics; bins beyond PC_LDS_WORDS, or a cell occupancy that could overflow a u32
 * counter, take the global-atomic path. */

#define PC_THREADS 256
#define PC_LDS_WORDS 12288      /* 48 KB of u32 counters per workgroup: three workgroups per CU */
#define PC_TARGET_WG 2048       /* workgroups of the histogram launch at large sizes (each flushes its counters once) */

struct PcGrid
{
   double lo[3], inv[3], L[3];      /* cell grid origin, 1/cell edge; L: box sides of the minimum image (wrap axes) */
   int nc[3];
   int wrap;                        /* bit a: axis a is periodic on one domain (cells modulo nc, minimum image) */
};
struct PcArgs
{
   double rmin, rmax, delta_r, lrmin, ldelta;      /* ldelta: ddcMD's logDelta */
   int nbins, ns, logscale, c0, c1;                /* combos [c0, c1) this pass counts */
};

__device__ __forceinline__ int pc_axis(double x, double lo, double inv, int nc, bool wrap)
{
   double t = (x - lo) * inv;
   t = fmin(fmax(t, -1.0e9), 1.0e9);      /* (NaN -> -1e9: the first cell) */
   int c = (int)floor(t);
   if (wrap) { c %= nc; if (c < 0) c += nc; }
   else c = min(max(c, 0), nc - 1);
   return c;
}
__device__ __forceinline__ int pc_cell_of(const PcGrid &g, double x, double y, double z)
{
   const int cx = pc_axis(x, g.lo[0], g.inv[0], g.nc[0], g.wrap & 1);
   const int cy = pc_axis(y, g.lo[1], g.inv[1], g.nc[1], g.wrap & 2);
   const int cz = pc_axis(z, g.lo[2], g.inv[2], g.nc[2], g.wrap & 4);
   return cx + g.nc[0] * (cy + g.nc[1] * cz);
}

/* the analysis's records {x, y, z, w}: w = species of an owned bead, -1 - species of a halo bead (j only) */
__global__ void k_pc_gather(int nloc, int nhalo, const double4 *__restrict__ pos, const int *__restrict__ species, const int *__restrict__ halo_src,
                            const int *__restrict__ halo_shift, double L0, double L1, double L2, const double *__restrict__ recv, double4 *__restrict__ out)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i < nloc)
   {
      const double4 p = pos[i];
      out[i] = make_double4(p.x, p.y, p.z, (double)species[i]);
   }
   else if (i < nloc + nhalo)
   {
      const int h = i - nloc, s = halo_src[h];
      double4 q;
      if (s >= 0)
      {
         /* periodic self-image: its owner's current position, shifted (k_halo_update's arithmetic) */
         const int code = halo_shift[h];
         const double4 p = pos[s];
         q.x = p.x + (double)(code % 3 - 1) * L0;
         q.y = p.y + (double)((code / 3) % 3 - 1) * L1;
         q.z = p.z + (double)(code / 9 - 1) * L2;
         q.w = -1.0 - (double)species[s];
      }
      else
      {
         const double *r = recv + 4 * (size_t)(-1 - s);
         q = make_double4(r[0], r[1], r[2], -1.0 - r[3]);
      }
      out[i] = q;
   }
}
/* the halo send lists with the sender's shift (k_pack_halo) and the species instead of the tag word */
__global__ void k_pc_pack(int nsend, DirTab dt, const unsigned *__restrict__ send_map, double L0, double L1, double L2, const double4 *__restrict__ pos,
                          const int *__restrict__ species, double *__restrict__ out)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k >= nsend) return;
   const unsigned m = send_map[k];
   const int i = (int)(m & 0x7ffffffu), code = (int)(m >> 27);
   const double4 p = pos[i];
   double *o = out + (size_t)k * 4;
   o[0] = p.x + dt.shift[code][0] * L0;
   o[1] = p.y + dt.shift[code][1] * L1;
   o[2] = p.z + dt.shift[code][2] * L2;
   o[3] = (double)species[i];
}
/* cell counts of the records, and this rank's beads per species (LDS counters, one flush per workgroup) */
__global__ __launch_bounds__(PC_THREADS) void k_pc_count(PcGrid g, int n, int ns, const double4 *__restrict__ rec, int *cnt, unsigned long long *nbeads)
{
   extern __shared__ unsigned sp_s[];
   for (int s = threadIdx.x; s < ns; s += PC_THREADS) sp_s[s] = 0u;
   __syncthreads();
   for (int i = blockIdx.x * PC_THREADS + threadIdx.x; i < n; i += gridDim.x * PC_THREADS)
   {
      const double4 p = rec[i];
      atomicAdd(&cnt[pc_cell_of(g, p.x, p.y, p.z)], 1);
      if (p.w >= 0.0) atomicAdd(&sp_s[(int)p.w], 1u);
   }
   __syncthreads();
   for (int s = threadIdx.x; s < ns; s += PC_THREADS)
      if (sp_s[s]) atomicAdd(&nbeads[s], (unsigned long long)sp_s[s]);
}
__global__ __launch_bounds__(PC_THREADS) void k_pc_scatter(PcGrid g, int n, const double4 *__restrict__ rec, int *fill, double4 *__restrict__ out)
{
   const int i = blockIdx.x * PC_THREADS + threadIdx.x;
   if (i >= n) return;
   const double4 p = rec[i];
   out[atomicAdd(&fill[pc_cell_of(g, p.x, p.y, p.z)], 1)] = p;      /* (order inside a cell is arbitrary: the counts are not) */
}
/* largest cell occupancy: bounds what one workgroup's u32 counters can receive */
__global__ __launch_bounds__(PC_THREADS) void k_pc_maxcell(int ncell, const int *__restrict__ cnt, int *mx)
{
   int m = 0;
   for (int c = blockIdx.x * PC_THREADS + threadIdx.x; c < ncell; c += gridDim.x * PC_THREADS) m = max(m, cnt[c]);
   for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
   if ((threadIdx.x & 63) == 0) atomicMax(mx, m);
}

/* the histogram: thread = one record of the cell-sorted array (owned beads count, halo beads are partners only); the threads of
 * a wave share their cell and with it the stencil, whose records they read at the same addresses */
template <bool LDS>
__global__ __launch_bounds__(PC_THREADS) void k_pc_hist(PcGrid g, PcArgs a, int n, int per_wg, const double4 *__restrict__ rec, const int *__restrict__ start,
                                                        unsigned long long *out)
{
   extern __shared__ unsigned h_s[];
   const int nsl = (a.c1 - a.c0) * a.nbins;
   if (LDS)
   {
      for (int k = threadIdx.x; k < nsl; k += PC_THREADS) h_s[k] = 0u;
      __syncthreads();
   }
   const double rmin2 = a.rmin * a.rmin, rmax2 = a.rmax * a.rmax;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int k = beg + (int)threadIdx.x; k < end; k += PC_THREADS)
   {
      const double4 p = rec[k];
      if (p.w < 0.0) continue;
      const int si = (int)p.w;
      int cc[3] = {pc_axis(p.x, g.lo[0], g.inv[0], g.nc[0], g.wrap & 1), pc_axis(p.y, g.lo[1], g.inv[1], g.nc[1], g.wrap & 2),
                   pc_axis(p.z, g.lo[2], g.inv[2], g.nc[2], g.wrap & 4)};
      int off[3][3], noff[3];
#pragma unroll
      for (int ax = 0; ax < 3; ax++)
      {
         const int nc = g.nc[ax];
         noff[ax] = 0;
         if ((g.wrap >> ax) & 1)
         {
            /* each distinct neighbour cell once: 3 cells or more -> c-1, c, c+1 modulo nc; 2 -> both; 1 -> itself */
            if (nc >= 3) { off[ax][0] = (cc[ax] + nc - 1) % nc; off[ax][1] = cc[ax]; off[ax][2] = (cc[ax] + 1) % nc; noff[ax] = 3; }
            else { for (int q = 0; q < nc; q++) off[ax][q] = q; noff[ax] = nc; }
         }
         else
            for (int d = -1; d <= 1; d++) if (cc[ax] + d >= 0 && cc[ax] + d < nc) off[ax][noff[ax]++] = cc[ax] + d;
      }
      for (int oz = 0; oz < noff[2]; oz++)
         for (int oy = 0; oy < noff[1]; oy++)
            for (int ox = 0; ox < noff[0]; ox++)
            {
               const int c = off[0][ox] + g.nc[0] * (off[1][oy] + g.nc[1] * off[2][oz]);
               const int j1 = start[c + 1];
               for (int j = start[c]; j < j1; j++)
               {
                  if (j == k) continue;
                  const double4 q = rec[j];
                  const int sj = q.w >= 0.0 ? (int)q.w : (int)(-1.0 - q.w);
                  if (si > sj) continue;
                  double dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                  if (g.wrap & 1) dx -= g.L[0] * rint(dx / g.L[0]);
                  if (g.wrap & 2) dy -= g.L[1] * rint(dy / g.L[1]);
                  if (g.wrap & 4) dz -= g.L[2] * rint(dz / g.L[2]);
                  const double r2 = dx * dx + dy * dy + dz * dz;
                  if (r2 >= rmax2 * 1.0000001 || r2 < rmin2 * 0.9999999) continue;      /* (coarse cut first; the exact one on r below) */
                  const double r = sqrt(r2);
                  if (r < a.rmin || r >= a.rmax) continue;
                  const int b = a.logscale ? (int)((log10(r) - a.lrmin) / a.ldelta) : (int)((r - a.rmin) / a.delta_r);
                  if (b < 0 || b >= a.nbins) continue;
                  const int combo = (sj - si) + a.ns * si - (si * (si - 1)) / 2;      /* comboIndex (paircorrelation.c) with si <= sj */
                  if (combo < a.c0 || combo >= a.c1) continue;
                  if (LDS) atomicAdd(&h_s[(combo - a.c0) * a.nbins + b], 1u);
                  else atomicAdd(&out[(size_t)combo * a.nbins + b], 1ull);
               }
            }
   }
   if (LDS)
   {
      __syncthreads();
      unsigned long long *o = out + (size_t)a.c0 * a.nbins;
      for (int k = threadIdx.x; k < nsl; k += PC_THREADS)
         if (h_s[k]) atomicAdd(&o[k], (unsigned long long)h_s[k]);
   }
}

/* ---- host side ---------------------------------------------------------- */
struct PcReq { double rmin, delta_r; int nbins, log_scale, nspecies; };

/* every argument check of the entry, before anything collective happens (a refused call changes nothing) */
static int pc_check(ddcmi_ctx *ctx, const PcReq &q, const void *counts, const void *nbeads)
{
   ARGCHK(ctx, ctx->nloc <= 0 && !decomposed(ctx), "ddcmi_pair_correlation needs an uploaded state (ddcmi_upload_state)");
   ARGCHK(ctx, !ctx->have_box, "ddcmi_pair_correlation needs a box (ddcmi_set_box)");
   ARGCHK(ctx, q.nbins <= 0, "ddcmi_pair_correlation: nbins = %d must be positive", q.nbins);
   ARGCHK(ctx, !std::isfinite(q.delta_r) || !(q.delta_r > 0.0), "ddcmi_pair_correlation: delta_r = %g must be finite and positive", q.delta_r);
   ARGCHK(ctx, !std::isfinite(q.rmin) || q.rmin < 0.0, "ddcmi_pair_correlation: rmin = %g must be finite and not negative", q.rmin);
   ARGCHK(ctx, q.log_scale && !(q.rmin > 0.0), "ddcmi_pair_correlation: log bins need rmin > 0 (rmin = %g)", q.rmin);
   ARGCHK(ctx, q.nspecies != ctx->nspecies, "ddcmi_pair_correlation: nspecies = %d, the context has %d species", q.nspecies, ctx->nspecies);
   ARGCHK(ctx, !counts || !nbeads, "ddcmi_pair_correlation: NULL output array (counts %p, nbeads %p)", counts, nbeads);
   const long long ncombo = (long long)q.nspecies * (q.nspecies + 1) / 2;
   ARGCHK(ctx, ncombo * q.nbins > (long long)INT32_MAX || q.nspecies > 16384, "ddcmi_pair_correlation: %lld combos x %d bins is too large", ncombo, q.nbins);
   const double rmax = q.rmin + q.nbins * q.delta_r;
   ARGCHK(ctx, !std::isfinite(rmax), "ddcmi_pair_correlation: rmax = rmin + nbins delta_r is not finite");
   double half = INFINITY;
   for (int a = 0; a < 3; a++) if ((ctx->pbc >> a) & 1) half = std::min(half, 0.5 * ctx->h[4 * a]);
   ARGCHK(ctx, rmax > half, "ddcmi_pair_correlation: rmax = %g exceeds half the shortest periodic box side, %g", rmax, half);
   if (decomposed(ctx) && ctx->nranks > 1)
   {
      ARGCHK(ctx, rmax > ctx->rmax, "ddcmi_pair_correlation: rmax = %g exceeds the potential's cut-off %g, the reach of a decomposed run's halo", rmax, ctx->rmax);
      ARGCHK(ctx, !ctx->list_valid, "ddcmi_pair_correlation: a decomposed run needs its first list build (ddcmi_eval_forces) for the halo");
   }
   return DDCMI_OK;
}
static bool pc_one_domain(const ddcmi_ctx *ctx) { return ctx->nranks == 1; }      /* (a loopback rank owns every bead too) */
/* the halo send of the analysis's records: pack into pc_send, receive into pc_recv (4 doubles per bead) */
static int pc_pack(ddcmi_ctx *ctx)
{
   if (pc_one_domain(ctx)) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   ENSURE(ctx, ctx->pc_send, 4 * (size_t)std::max(ctx->nsend, 1));
   ENSURE(ctx, ctx->pc_recv, 4 * (size_t)std::max(ctx->nrecv, 1));
   if (ctx->nsend > 0)
      hipLaunchKernelGGL(k_pc_pack, dim3(cdiv(ctx->nsend, 256)), dim3(256), 0, ctx->stream, ctx->nsend, mg_dirtab(ctx), ctx->send_map.p,
                         ctx->gp.L[0], ctx->gp.L[1], ctx->gp.L[2], ctx->pos.p, ctx->species.p, ctx->pc_send.p);
   return DDCMI_OK;
}
/* the rest on this rank once pc_recv holds the received beads: grid, sort, histogram, copy out [sync] */
static int pc_eval(ddcmi_ctx *ctx, const PcReq &q, int64_t *counts, int64_t *nbeads)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const bool one = pc_one_domain(ctx);
   const int nloc = ctx->nloc, nhalo = one ? 0 : ctx->nhalo, n = nloc + nhalo;
   const int ns = q.nspecies, ncombo = ns * (ns + 1) / 2;
   const size_t nhist = (size_t)ncombo * q.nbins;
   const double rmax = q.rmin + q.nbins * q.delta_r;
   /* cells of edge >= rmax (with a margin of rounding), at most about two per record */
   PcGrid g;
   double ext[3];
   g.wrap = 0;
   for (int a = 0; a < 3; a++)
   {
      const double L = ctx->h[4 * a];
      g.L[a] = L;
      if (one)
      {
         g.lo[a] = -0.5 * L; ext[a] = L;      /* (the box is centred on the origin) */
         if ((ctx->pbc >> a) & 1) g.wrap |= 1 << a;
      }
      else
      {
         const double W = L / ctx->pgrid[a];
         g.lo[a] = -0.5 * L + ctx->pcoord[a] * W - rmax; ext[a] = W + 2.0 * rmax;
      }
      const double m = floor(ext[a] / (rmax * (1.0 + 1e-12)));
      g.nc[a] = (int)std::max(1.0, std::min(m, 1.0e6));
   }
   while ((double)g.nc[0] * g.nc[1] * g.nc[2] > 2.0 * n + 1024.0)
   {
      int a = 0;
      for (int b = 1; b < 3; b++) if (g.nc[b] > g.nc[a]) a = b;
      g.nc[a] = std::max(1, g.nc[a] / 2);
   }
   for (int a = 0; a < 3; a++) g.inv[a] = g.nc[a] / ext[a];
   const int ncell = g.nc[0] * g.nc[1] * g.nc[2];
   PcArgs pa;
   pa.rmin = q.rmin; pa.rmax = rmax; pa.delta_r = q.delta_r; pa.nbins = q.nbins; pa.ns = ns; pa.logscale = q.log_scale;
   pa.lrmin = q.log_scale ? log10(q.rmin) : 0.0;
   pa.ldelta = q.log_scale ? (log10(rmax) - log10(q.rmin)) / (double)q.nbins : 0.0;
   ENSURE(ctx, ctx->pc_rec, (size_t)std::max(n, 1));
   ENSURE(ctx, ctx->pc_sorted, (size_t)std::max(n, 1));
   ENSURE(ctx, ctx->pc_cnt, (size_t)ncell + 2);
   ENSURE(ctx, ctx->pc_start, (size_t)ncell + 2);
   ENSURE(ctx, ctx->pc_hist, nhist + (size_t)ns);
   unsigned long long *d_nb = ctx->pc_hist.p + nhist;
   HIPCHK(ctx, hipMemsetAsync(ctx->pc_cnt.p, 0, ((size_t)ncell + 2) * sizeof(int), st));      /* [ncell]: the scan's end, [ncell + 1]: the largest cell */
   HIPCHK(ctx, hipMemsetAsync(ctx->pc_hist.p, 0, (nhist + ns) * sizeof(unsigned long long), st));
   int maxcell = 0;
   if (n > 0)
   {
      hipLaunchKernelGGL(k_pc_gather, dim3(cdiv(n, 256)), dim3(256), 0, st, nloc, nhalo, ctx->pos.p, ctx->species.p, ctx->halo_src.p, ctx->halo_shift.p,
                         ctx->gp.L[0], ctx->gp.L[1], ctx->gp.L[2], ctx->pc_recv.p, ctx->pc_rec.p);
      hipLaunchKernelGGL(k_pc_count, dim3(std::min(cdiv(n, PC_THREADS), 1024)), dim3(PC_THREADS), ns * sizeof(unsigned), st, g, n, ns, ctx->pc_rec.p, ctx->pc_cnt.p, d_nb);
      hipLaunchKernelGGL(k_pc_maxcell, dim3(std::min(cdiv(ncell, PC_THREADS), 256)), dim3(PC_THREADS), 0, st, ncell, ctx->pc_cnt.p, ctx->pc_cnt.p + ncell + 1);
      int rc = ddcmi_scan_exclusive(ctx, ctx->pc_cnt.p, ctx->pc_start.p, ncell + 1, nullptr);      /* [ncell] = n */
      if (rc) return rc;
      HIPCHK(ctx, hipMemcpyAsync(&maxcell, ctx->pc_cnt.p + ncell + 1, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(ctx->pc_cnt.p, ctx->pc_start.p, (size_t)ncell * sizeof(int), hipMemcpyDeviceToDevice, st));      /* the fill pointers */
      hipLaunchKernelGGL(k_pc_scatter, dim3(cdiv(n, PC_THREADS)), dim3(PC_THREADS), 0, st, g, n, ctx->pc_rec.p, ctx->pc_cnt.p, ctx->pc_sorted.p);
      HIPCHK(ctx, hipStreamSynchronize(st));
      /* records per workgroup: ~PC_TARGET_WG workgroups, fewer records where a u32 counter could overflow (<= per_wg x 27 x maxcell) */
      const double cand = 27.0 * std::max(maxcell, 1);
      long long per_wg = (long long)cdiv(cdiv(n, PC_TARGET_WG), PC_THREADS) * PC_THREADS;
      while (per_wg > PC_THREADS && (double)per_wg * cand >= 4294967295.0) per_wg -= PC_THREADS;
      const bool lds = q.nbins <= PC_LDS_WORDS && (double)per_wg * cand < 4294967295.0;
      const int nwg = cdiv(n, (long)per_wg);
      if (lds)
      {
         const int per_pass = PC_LDS_WORDS / q.nbins;      /* combos per slice */
         for (int c0 = 0; c0 < ncombo; c0 += per_pass)
         {
            pa.c0 = c0; pa.c1 = std::min(ncombo, c0 + per_pass);
            const size_t lds_b = (size_t)(pa.c1 - pa.c0) * q.nbins * sizeof(unsigned);
            hipLaunchKernelGGL(k_pc_hist<true>, dim3(nwg), dim3(PC_THREADS), lds_b, st, g, pa, n, (int)per_wg, ctx->pc_sorted.p, ctx->pc_start.p, ctx->pc_hist.p);
         }
      }
      else
      {
         pa.c0 = 0; pa.c1 = ncombo;
         hipLaunchKernelGGL(k_pc_hist<false>, dim3(nwg), dim3(PC_THREADS), 0, st, g, pa, n, (int)per_wg, ctx->pc_sorted.p, ctx->pc_start.p, ctx->pc_hist.p);
      }
      HIPCHK(ctx, hipGetLastError());
   }
   HIPCHK(ctx, hipMemcpyAsync(counts, ctx->pc_hist.p, nhist * sizeof(int64_t), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipMemcpyAsync(nbeads, d_nb, (size_t)ns * sizeof(int64_t), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}

extern "C" int ddcmi_pair_correlation(ddcmi_ctx *ctx, double rmin, double delta_r, int nbins, int log_scale, int nspecies, int64_t *counts, int64_t *nbeads)
{
   const PcReq q = {rmin, delta_r, nbins, log_scale, nspecies};
   return analysis_single(ctx, "pair_correlation", true, [=](ddcmi_ctx *c, const char *) { return pc_check(c, q, counts, nbeads); },
                          [=](ddcmi_ctx *c) {
                             int rc;
                             if (!pc_one_domain(c))
                             {
                                /* collective: the received beads' current positions, along the per-step halo's messages */
                                if ((rc = pc_pack(c))) return rc;
                                if (mg_transport(c) && (rc = mg_xchg_halo(c, c->pc_send.p, c->pc_recv.p, 4, c->stream))) return rc;
                             }
                             return pc_eval(c, q, counts, nbeads);
                          });
}

/* in-process group: per-rank results, rank after rank (counts[r * ncombo * nbins ...], nbeads[r * nspecies ...]) */
extern "C" int ddcmi_group_pair_correlation(ddcmi_ctx **ctxs, int n, double rmin, double delta_r, int nbins, int log_scale, int nspecies,
                                            int64_t *counts, int64_t *nbeads)
{
   const PcReq q = {rmin, delta_r, nbins, log_scale, nspecies};
   const size_t nhist = (size_t)nspecies * (nspecies + 1) / 2 * nbins;
   return analysis_group(ctxs, n, "pair_correlation", [=](ddcmi_ctx *c, const char *) { return pc_check(c, q, counts, nbeads); },
                         [](ddcmi_group *g) {
                            int rc;
                            if (g->ranks[0]->nranks > 1)
                            {
                               for (ddcmi_ctx *c : g->ranks) if ((rc = pc_pack(c))) return rc;
                               if ((rc = group_exchange(g, 4, [](const ddcmi_ctx *c) { return group_halo_side(c, c->pc_send.p, c->pc_recv.p); }))) return rc;
                            }
                            return (int)DDCMI_OK;
                         },
                         [=](ddcmi_ctx *c, size_t r) { return pc_eval(c, q, counts + r * nhist, nbeads + r * (size_t)nspecies); });
}

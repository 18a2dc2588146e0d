/* ddcmi_census.inl -- ANALYSIS types vcmWrite and zdensity on the device (vcmWrite.c:95-110, zdensity.c:66-151): one read-only pass
 * over the owned beads each.  Included from ddcmi.hip behind ddcmi_vaf.inl, whose wave reduction (vaf_add_classes, wave_sum_dpp) and
 * second stage (k_vaf_final) both passes use.
 *
 * Both read the state ddcmi_download_state returns, change nothing of the run, need no communication (the caller adds the ranks'
 * results) and repeat bit for bit: a workgroup owns a contiguous range of slots, a wave adds its 64 beads key by key into its own
 * LDS row -- a ballot picks the lanes that share the first pending lane's key, wave_sum_dpp adds them with the other lanes at zero,
 * that one lane adds the sum into the row: one writer per row at a time, no bank conflict, no atomic -- the workgroup adds its
 * waves' rows in wave order, a second launch adds the workgroups' rows in workgroup order.  No floating-point atomics.
 *
 * Momentum (k_census_momentum): four values per class, {m vx, m vy, m vz, m}.  m is ctx->d_mass[species]: the mass ddcmi_set_species
 * took, whose reciprocal (d_invmass) the integrator's kick multiplies the force with and which its kinetic energy uses -- the
 * reference's ((ATOMTYPE_PARMS *)species->parm)->mass.  Classes as in ddcmi_vaf.inl: 0 the system, 1 + g, 1 + ngroup + s.
 *
 * Z histogram (k_census_zdensity<SMEAR>), derived in DESIGN.md ("zdensity: the shape of the histogram kernel"):
 *   SMEAR = false  one bin per bead, weight 1: the key's lanes are COUNTED (popcount of the ballot) and the count goes into the
 *                  workgroup's one row of 32-bit integers by an integer LDS add; workgroup partials are 32-bit (a workgroup holds
 *                  fewer than 2^32 beads), the second stage adds them in 64 bits and converts once: exact at any bead count.
 *   SMEAR = true   two (bin, weight) pairs per bead, the lower bin's pass first, then the upper bin's (the reference's kk = 0, 1);
 *                  per-wave rows of doubles: CENSUS_WAVES x 8 B of LDS per bin, hence CENSUS_MAX_NZ.
 * The per-bead arithmetic is the reference's, operation by operation, with every product kept from contraction into an FMA
 * (zd_rounded: the library is built with -ffp-contract=fast), so that a float64 restatement on the host lands in the same bin at an edge.  The position is the
 * one ddcmi_download_state hands out: slot position, shifted once by the box side where it left a periodic box since the last
 * rebuild (k_export_pos); the reference bins its positions as they are, and so does this -- no further wrap.  A coordinate outside
 * the box reaches the reference's clamp: a label read as unsigned that is >= nz goes to nz - 1 (negative t below -1 included;
 * -1 < t < 0 truncates to bin 0).  The conversion to int saturates at +-2^30 (C leaves it undefined there), NaN goes to -2^30. */

#define CENSUS_THREADS 256
#define CENSUS_WAVES (CENSUS_THREADS / 64)
#define CENSUS_MAX_WG 1024
#define CENSUS_MAX_CLASS 512     /* CENSUS_WAVES rows x 4 values x 8 B = 128 B of LDS per class: 64 KB */
#define CENSUS_MAX_NZ 2048       /* CENSUS_WAVES rows x 8 B = 32 B of LDS per bin: 64 KB */

__global__ __launch_bounds__(CENSUS_THREADS) void k_census_momentum(int n, int per_wg, int ngroup, int nspecies, const double *__restrict__ vx,
                                                                    const double *__restrict__ vy, const double *__restrict__ vz, const int *__restrict__ group,
                                                                    const int *__restrict__ species, const double *__restrict__ massv, double *__restrict__ part)
{
   extern __shared__ double census_s[];      /* [CENSUS_WAVES][nclass][4] */
   const int nval = 4 * (1 + ngroup + nspecies);
   for (int k = threadIdx.x; k < CENSUS_WAVES * nval; k += CENSUS_THREADS) census_s[k] = 0.0;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * nval;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   double sys[4] = {0.0, 0.0, 0.0, 0.0};      /* the system's sums: per lane over the range, one reduction at the end */
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int i = base + (int)threadIdx.x;
      const bool have = i < end;
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      int g = 0, s = 0;
      if (have)
      {
         g = min(max(group[i], 0), ngroup - 1); s = min(max(species[i], 0), nspecies - 1);      /* (checked at the upload: the LDS rows stay in bounds whatever the arrays hold) */
         const double m = massv[s];
         v[0] = m * vx[i]; v[1] = m * vy[i]; v[2] = m * vz[i]; v[3] = m;
      }
#pragma unroll
      for (int q = 0; q < 4; q++) sys[q] += v[q];
      const unsigned long long pending = __ballot(have);
      vaf_add_classes<4>(pending, 1 + g, v, row);
      vaf_add_classes<4>(pending, 1 + ngroup + s, v, row);
   }
#pragma unroll
   for (int q = 0; q < 4; q++) sys[q] = wave_sum_dpp(sys[q]);
   if ((threadIdx.x & 63) == 0) { row[0] = sys[0]; row[1] = sys[1]; row[2] = sys[2]; row[3] = sys[3]; }
   __syncthreads();
   double *out = part + (size_t)blockIdx.x * nval;
   for (int k = threadIdx.x; k < nval; k += CENSUS_THREADS)
   {
      double t = census_s[k];
#pragma unroll
      for (int w = 1; w < CENSUS_WAVES; w++) t += census_s[(size_t)w * nval + k];
      out[k] = t;
   }
}

/* zdensity_output's constants (zdensity.c:66-81), formed on the host in the reference's operations */
struct ZdParms
{
   int nz, method, wrap;              /* method: 0 impulse, 1 hat; wrap: the box is periodic along z */
   double L;                          /* bbox.z */
   double deltai, scaled_corner;      /* nz / L, corner.z * deltai */
   double half, inv;                  /* lSmearHalf.z, lSmearInv.z */
};
__device__ __forceinline__ int zd_int(double x)      /* (int)x, saturating at +-2^30; NaN: -2^30 */
{
   const double lim = 1073741824.0;
   return x >= lim ? (int)lim : (x > -lim ? (int)x : -(int)lim);
}
__device__ __forceinline__ unsigned zd_label(int ig, int nz) { const unsigned l = (unsigned)ig; return l >= (unsigned)nz ? (unsigned)(nz - 1) : l; }
/* a product that stays a product: with -ffp-contract=fast the back end fuses a multiplication into the addition that uses it
 * whatever the source says; a value that went through an (empty) asm statement is no multiplication to it any more */
__device__ __forceinline__ double zd_rounded(double x) { asm volatile("" : "+v"(x)); return x; }
/* r.z of zdensity.c:90 from the slot's z */
__device__ __forceinline__ double zd_t(const ZdParms &zp, double z)
{
   if (zp.wrap) { if (z > 0.5 * zp.L) z -= zp.L; if (z < -0.5 * zp.L) z += zp.L; }      /* k_export_pos */
   const double a = zd_rounded(z * zp.deltai);
   return a - zp.scaled_corner;
}
/* zdensity.c:105-133: the two bins and weights of a smeared bead */
__device__ __forceinline__ void zd_smear(const ZdParms &zp, double t, unsigned label[2], double w[2])
{
   const double fl = floor(t + 0.5);
   double delta = fl - t;
   delta = delta < zp.half ? delta : zp.half;
   delta = delta > -zp.half ? delta : -zp.half;
   const int iw = zd_int(fl);
   int ig0 = iw - 1, ig1 = iw;
   if (ig0 == -1) ig0 = zp.nz - 1;
   if (ig1 == zp.nz) ig1 = 0;
   if (zp.method == 1)
   {
      const double a = (2 * delta) * zp.inv, b = zd_rounded(fabs(delta) * zp.inv), c = 1.0 - b, d = zd_rounded(a * c);
      w[0] = 0.5 + d;
   }
   else
   {
      const double a = zd_rounded(delta * zp.inv);
      w[0] = 0.5 + a;
   }
   w[1] = 1.0 - w[0];
   label[0] = zd_label(ig0, zp.nz); label[1] = zd_label(ig1, zp.nz);
}
template <bool SMEAR>
__global__ __launch_bounds__(CENSUS_THREADS) void k_census_zdensity(int n, int per_wg, ZdParms zp, const double4 *__restrict__ pos, void *__restrict__ part_)
{
   extern __shared__ double census_s[];      /* SMEAR: double [CENSUS_WAVES][nz]; otherwise unsigned [nz] */
   unsigned *cnt_s = (unsigned *)census_s;
   const int nz = zp.nz, lane = threadIdx.x & 63;
   if (SMEAR) for (int k = threadIdx.x; k < CENSUS_WAVES * nz; k += CENSUS_THREADS) census_s[k] = 0.0;
   else for (int k = threadIdx.x; k < nz; k += CENSUS_THREADS) cnt_s[k] = 0u;
   __syncthreads();
   double *row = census_s + (size_t)(threadIdx.x >> 6) * nz;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the wave operations) */
   {
      const int i = base + (int)threadIdx.x;
      const bool have = i < end;
      unsigned label[2] = {0u, 0u};
      double w[2] = {0.0, 0.0};
      if (have)
      {
         const double t = zd_t(zp, pos[i].z);
         if (SMEAR) zd_smear(zp, t, label, w);
         else label[0] = zd_label(zd_int(t), nz);
      }
#pragma unroll
      for (int kk = 0; kk < (SMEAR ? 2 : 1); kk++)
      {
         unsigned long long pending = __ballot(have && (!SMEAR || !(w[kk] < 1e-20)));
         while (pending)
         {
            const int lead = __ffsll((long long)pending) - 1;
            const unsigned k = (unsigned)__shfl((int)label[kk], lead, 64);
            const bool mine = (pending >> lane & 1ull) && label[kk] == k;
            const unsigned long long same = __ballot(mine);
            if (SMEAR)
            {
               const double sw = wave_sum_dpp(mine ? w[kk] : 0.0);
               if (lane == lead) row[k] += sw;
            }
            else if (lane == lead) atomicAdd(&cnt_s[k], (unsigned)__popcll(same));      /* (integers: the order of the waves does not matter) */
            pending &= ~same;
         }
      }
   }
   __syncthreads();
   if (SMEAR)
   {
      double *out = (double *)part_ + (size_t)blockIdx.x * nz;
      for (int k = threadIdx.x; k < nz; k += CENSUS_THREADS)
      {
         double t = census_s[k];
#pragma unroll
         for (int wv = 1; wv < CENSUS_WAVES; wv++) t += census_s[(size_t)wv * nz + k];
         out[k] = t;
      }
   }
   else
   {
      unsigned *out = (unsigned *)part_ + (size_t)blockIdx.x * nz;
      for (int k = threadIdx.x; k < nz; k += CENSUS_THREADS) out[k] = cnt_s[k];
   }
}
/* the workgroups' counts in 64-bit integers, converted once: out[k] = (double) sum over w of part[w][k] */
__global__ void k_census_final_counts(int nwg, int nval, const unsigned *__restrict__ part, double *__restrict__ out)
{
   const int k = blockIdx.x * blockDim.x + threadIdx.x;
   if (k >= nval) return;
   unsigned long long t = 0ull;
   for (int w = 0; w < nwg; w++) t += part[(size_t)w * nval + k];
   out[k] = (double)t;
}

/* ---- host side ---------------------------------------------------------- */
static int census_state_check(ddcmi_ctx *ctx, const char *fn)
{
   ARGCHK(ctx, ctx->nloc <= 0 && !decomposed(ctx), "%s needs an uploaded state (ddcmi_upload_state)", fn);
   ARGCHK(ctx, ctx->nloc > 0 && ctx->vx.cap < (size_t)ctx->nloc, "%s needs an uploaded state (ddcmi_upload_state)", fn);
   return DDCMI_OK;
}
static int census_momentum_check(ddcmi_ctx *ctx, const char *fn, int ngroup, int nspecies, const void *mv, const void *m)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, ngroup != ctx->ngroup, "%s: ngroup = %d, the context has %d groups", fn, ngroup, ctx->ngroup);
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, !mv || !m, "%s: NULL output array (mv %p, m %p)", fn, mv, m);
   if (1 + ngroup + nspecies > CENSUS_MAX_CLASS) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d classes, at most %d", fn, 1 + ngroup + nspecies, CENSUS_MAX_CLASS);
   return DDCMI_OK;
}
static int census_zdensity_check(ddcmi_ctx *ctx, const char *fn, int nz, int smear_method, const void *density)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, !density, "%s: NULL output array", fn);
   ARGCHK(ctx, nz < 1, "%s: nz = %d", fn, nz);
   ARGCHK(ctx, smear_method != 0 && smear_method != 1, "%s: smear_method = %d (0 impulse, 1 hat)", fn, smear_method);
   if (nz > CENSUS_MAX_NZ) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: nz = %d, at most %d", fn, nz, CENSUS_MAX_NZ);
   const int off[6] = {1, 2, 3, 5, 6, 7};
   for (int k = 0; k < 6; k++)
      if (fabs(ctx->h[off[k]]) > 1e-10) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: only orthorhombic boxes are supported (h[%d]=%g)", fn, off[k], ctx->h[off[k]]);
   if (!(ctx->h[8] > 0.0)) SETERR(ctx, DDCMI_EINVAL, "%s needs a box (ddcmi_set_box)", fn);
   return DDCMI_OK;
}
/* slots per workgroup: whole blocks of CENSUS_THREADS, at most about CENSUS_MAX_WG workgroups, every one of them with beads */
static void census_split(int n, int *per_wg, int *nwg)
{
   *per_wg = cdiv(cdiv(n, CENSUS_MAX_WG), CENSUS_THREADS) * CENSUS_THREADS;
   *nwg = cdiv(n, *per_wg);
}
/* this rank's sums [sync] */
static int census_momentum_one(ddcmi_ctx *ctx, double *mv, double *m)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, nclass = 1 + ctx->ngroup + ctx->nspecies, nval = 4 * nclass;
   if (n <= 0) { for (int c = 0; c < nclass; c++) { mv[3 * c] = mv[3 * c + 1] = mv[3 * c + 2] = 0.0; m[c] = 0.0; } return DDCMI_OK; }      /* (a domain that holds no bead) */
   int per_wg, nwg;
   census_split(n, &per_wg, &nwg);
   ENSURE(ctx, ctx->census_part, (size_t)(nwg + 1) * nval);
   double *d_out = ctx->census_part.p + (size_t)nwg * nval;
   hipLaunchKernelGGL(k_census_momentum, dim3(nwg), dim3(CENSUS_THREADS), (size_t)CENSUS_WAVES * nval * sizeof(double), st, n, per_wg, ctx->ngroup, ctx->nspecies,
                      ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->group.p, ctx->species.p, ctx->d_mass.p, ctx->census_part.p);
   hipLaunchKernelGGL(k_vaf_final, dim3(cdiv(nval, 64)), dim3(64), 0, st, nwg, nval, ctx->census_part.p, d_out);
   HIPCHK(ctx, hipGetLastError());
   std::vector<double> h((size_t)nval);
   HIPCHK(ctx, hipMemcpyAsync(h.data(), d_out, (size_t)nval * sizeof(double), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   for (int c = 0; c < nclass; c++) { mv[3 * c] = h[4 * c]; mv[3 * c + 1] = h[4 * c + 1]; mv[3 * c + 2] = h[4 * c + 2]; m[c] = h[4 * c + 3]; }
   return DDCMI_OK;
}
static int census_zdensity_one(ddcmi_ctx *ctx, int nz, double smear_radius, int smear_method, double *density)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc;
   if (n <= 0) { for (int k = 0; k < nz; k++) density[k] = 0.0; return DDCMI_OK; }      /* (a domain that holds no bead) */
   const bool smear = smear_radius > 0.0;
   ZdParms zp;
   zp.nz = nz; zp.method = smear_method; zp.wrap = (ctx->pbc >> 2) & 1;
   zp.L = ctx->h[8];
   const double corner = ctx->h[8] * -0.5;      /* box->corner = h0 * reducedcorner (box.c:69), reducedcorner = -0.5 on this path */
   zp.deltai = nz / zp.L;
   zp.scaled_corner = corner * zp.deltai;
   zp.half = zp.inv = 0.0;
   if (smear)
   {
      const double a = 2.0 * smear_radius, b = zp.L / (1.0 * nz), lSmear = a < b ? a : b;
      zp.inv = 1.0 / lSmear; zp.half = 0.5 * lSmear;
   }
   int per_wg, nwg;
   census_split(n, &per_wg, &nwg);
   ENSURE(ctx, ctx->census_part, (size_t)(nwg + 1) * nz);      /* (the counts' 32-bit partials take half of the room) */
   double *d_out = ctx->census_part.p + (size_t)nwg * nz;
   if (smear)
   {
      hipLaunchKernelGGL(k_census_zdensity<true>, dim3(nwg), dim3(CENSUS_THREADS), (size_t)CENSUS_WAVES * nz * sizeof(double), st, n, per_wg, zp, ctx->pos.p, (void *)ctx->census_part.p);
      hipLaunchKernelGGL(k_vaf_final, dim3(cdiv(nz, 64)), dim3(64), 0, st, nwg, nz, ctx->census_part.p, d_out);
   }
   else
   {
      hipLaunchKernelGGL(k_census_zdensity<false>, dim3(nwg), dim3(CENSUS_THREADS), (size_t)nz * sizeof(unsigned), st, n, per_wg, zp, ctx->pos.p, (void *)ctx->census_part.p);
      hipLaunchKernelGGL(k_census_final_counts, dim3(cdiv(nz, 64)), dim3(64), 0, st, nwg, nz, (const unsigned *)ctx->census_part.p, d_out);
   }
   HIPCHK(ctx, hipGetLastError());
   HIPCHK(ctx, hipMemcpyAsync(density, d_out, (size_t)nz * sizeof(double), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}

extern "C" int ddcmi_momentum_by_class(ddcmi_ctx *ctx, int ngroup, int nspecies, double *mv, double *m)
{
   if (!ctx) return DDCMI_EINVAL;
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group: use ddcmi_group_momentum_by_class");
   int rc = census_momentum_check(ctx, "ddcmi_momentum_by_class", ngroup, nspecies, mv, m);
   if (rc) return rc;
   (void)hipSetDevice(ctx->device);
   if ((rc = ddcmi_agree_poll(ctx))) return rc;
   return census_momentum_one(ctx, mv, m);
}
extern "C" int ddcmi_zdensity(ddcmi_ctx *ctx, int nz, double smear_radius, int smear_method, double *density)
{
   if (!ctx) return DDCMI_EINVAL;
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group: use ddcmi_group_zdensity");
   int rc = census_zdensity_check(ctx, "ddcmi_zdensity", nz, smear_method, density);
   if (rc) return rc;
   (void)hipSetDevice(ctx->device);
   if ((rc = ddcmi_agree_poll(ctx))) return rc;
   return census_zdensity_one(ctx, nz, smear_radius, smear_method, density);
}

/* in-process group: per-rank blocks, rank after rank (mv[r * 3 nclass ...], m[r * nclass ...]; density[r * nz ...]) */
extern "C" int ddcmi_group_momentum_by_class(ddcmi_ctx **ctxs, int n, int ngroup, int nspecies, double *mv, double *m)
{
   if (!ctxs || n < 1 || !ctxs[0] || !ctxs[0]->group_) return DDCMI_EINVAL;
   ddcmi_group *g = ctxs[0]->group_;
   ARGCHK(ctxs[0], n != (int)g->ranks.size(), "ddcmi_group_momentum_by_class: n = %d, the group has %d domains", n, (int)g->ranks.size());
   int rc;
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = census_momentum_check(c, "ddcmi_group_momentum_by_class", ngroup, nspecies, mv, m))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   const size_t nclass = (size_t)1 + ngroup + nspecies;
   for (size_t r = 0; r < g->ranks.size(); r++)
      if ((rc = census_momentum_one(g->ranks[r], mv + r * 3 * nclass, m + r * nclass))) { if (r) ctxs[0]->err = g->ranks[r]->err; return rc; }
   return DDCMI_OK;
}
extern "C" int ddcmi_group_zdensity(ddcmi_ctx **ctxs, int n, int nz, double smear_radius, int smear_method, double *density)
{
   if (!ctxs || n < 1 || !ctxs[0] || !ctxs[0]->group_) return DDCMI_EINVAL;
   ddcmi_group *g = ctxs[0]->group_;
   ARGCHK(ctxs[0], n != (int)g->ranks.size(), "ddcmi_group_zdensity: n = %d, the group has %d domains", n, (int)g->ranks.size());
   int rc;
   for (ddcmi_ctx *c : g->ranks)
      if ((rc = census_zdensity_check(c, "ddcmi_group_zdensity", nz, smear_method, density))) { if (c != ctxs[0]) ctxs[0]->err = c->err; return rc; }
   for (size_t r = 0; r < g->ranks.size(); r++)
      if ((rc = census_zdensity_one(g->ranks[r], nz, smear_radius, smear_method, density + r * (size_t)nz))) { if (r) ctxs[0]->err = g->ranks[r]->err; return rc; }
   return DDCMI_OK;
}

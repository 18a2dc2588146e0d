/* ddcmi_thermalize.inl -- TRANSFORM type THERMALIZE on the device (thermalize.c, thermalizeTransform.c): new velocities for the owned beads,
 * drawn (BOLTZMANN) or rescaled (RESCALE).  Included from ddcmi.hip behind ddcmi_census.inl, whose frame it uses.  Only vx, vy, vz of
 * the owned slots change: positions, lists, forces_valid and the VAF records stay.  Classes: select 0 one class, 1 the species, 2 the groups
 * (getIndex, thermalize.c:271-289); a class temperature < 0 leaves BOLTZMANN's class alone, <= 0 scales RESCALE's by 1.  The mass is
 * ctx->d_mass[species], the one the integrator's kick uses (ddcmi_momentum_by_class).
 *
 * BOLTZMANN (thermalize_boltzmann, thermalize.c:103-125; k_thermalize_boltzmann): one lane per bead, nothing shared.  The bead's stream is
 * prand48_init((loop % 10000000 + 1) * gid, seed, 0x1234512345ab) (random.c:370-386) restated word by word, the uniforms are erand48's 48-bit
 * LCG in integers (X <- 0x5DEECE66D X + 0xB mod 2^48, u = X 2^-48: exact in a double), the normals three calls of gasdev0 (random.c:100-112):
 * the polar rejection loop, v2 * fac returned, no second deviate kept.  v1 = 2 u - 1 is exact; v1 v1 and v2 v2 are rounded once each and
 * kept from contraction (zd_rounded: the library is built with -ffp-contract=fast), their sum once more -- the operations of the
 * reference's C on a host without FMA, so that rsq >= 1 decides alike.  The loop makes lanes diverge: this is no per-step path.
 *
 * RESCALE (thermalize_rescale, thermalize.c:159-269): per class sum m v, sum m (class_sums_one<4> with MomentumBead: the pass of
 * ddcmi_momentum_by_class), then sum m |v - vcm|^2 and N (class_sums_one<2>), then v' = (v - vcm) vScale + vcmNew (k_thermalize_rescale).
 * The two sums follow the census passes' rules (per-wave partial sums, a fixed second stage, no floating-point atomics); the ranks' sums are
 * gathered and added in rank order on every rank (therm_reduce), so a decomposed run repeats bit for bit and all ranks scale alike.  vcm is
 * the quotient (sum m v) / (sum m) (the reference multiplies by the rounded reciprocal: one rounding more).  A class with N <= 1 or
 * sum m |v - vcm|^2 == 0 -- where the reference divides by zero -- is not written. */

#define THERM_THREADS 256
enum { THERM_BOLTZMANN = 0, THERM_RESCALE = 1, THERM_JUTTNER = 2 };

__device__ __forceinline__ int therm_class(int select, int s, int i, const int *__restrict__ group, int nclass)
{
   const int c = select == 0 ? 0 : (select == 1 ? s : group[i]);
   return min(max(c, 0), nclass - 1);      /* (checked at the upload: the tables stay in bounds whatever the arrays hold) */
}
/* erand48: the 48-bit LCG; X 2^-48 is exact */
__device__ __forceinline__ double therm_erand48(unsigned long long &x)
{
   x = (0x5DEECE66Dull * x + 0xBull) & 0xFFFFFFFFFFFFull;
   return (double)x * 0x1p-48;
}
/* prand48_init (random.c:370-386): seedVec as erand48 reads it, word 0 lowest */
__device__ __forceinline__ unsigned long long therm_prand48_init(unsigned long long gid, unsigned long long seed, unsigned long long callSite)
{
   seed ^= callSite;
   gid ^= seed;
   unsigned short sv[3] = {0, 0, 0};
   const unsigned short mask[4] = {0x000F, 0x00F0, 0x0F00, 0xF000};
#pragma unroll
   for (int ii = 0; ii < 4; ii++)
   {
      sv[0] += (unsigned short)(gid & mask[ii]); gid = gid >> 4;
      sv[1] += (unsigned short)(gid & mask[ii]); gid = gid >> 4;
      sv[2] += (unsigned short)(gid & mask[ii]);
   }
   return (unsigned long long)sv[0] | (unsigned long long)sv[1] << 16 | (unsigned long long)sv[2] << 32;
}
/* PROBE: the rejected draws of every bead go to rej[] (-1: the bead's class is left alone) and no velocity is written (ddcmi_debug_thermalize_rejects) */
template <bool PROBE>
__global__ __launch_bounds__(THERM_THREADS) void k_thermalize_boltzmann(int n, int select, int nclass, unsigned long long seed, unsigned long long loopmul,
                                                                        const double *__restrict__ temp, const double *__restrict__ massv, int nspecies,
                                                                        const int *__restrict__ species, const int *__restrict__ group,
                                                                        const uint64_t *__restrict__ gid, double *__restrict__ vx, double *__restrict__ vy,
                                                                        double *__restrict__ vz, int *__restrict__ rej)
{
   const int i = blockIdx.x * THERM_THREADS + threadIdx.x;
   if (i >= n) return;
   const int s = min(max(species[i], 0), nspecies - 1);
   const double T = temp[therm_class(select, s, i, group, nclass)];
   if (T < 0.0) { if (PROBE) rej[i] = -1; return; }      /* thermalize.c:113: not written at all */
   unsigned long long x = therm_prand48_init(loopmul * (unsigned long long)gid[i], seed, 0x1234512345abull);
   const double sigma = sqrt(T / massv[s]);      /* kB = 1 */
   double g[3];
   int nrej = 0;
#pragma unroll
   for (int k = 0; k < 3; k++)
   {
      double v2, rsq;
      for (;;)      /* gasdev0 */
      {
         const double v1 = 2.0 * therm_erand48(x) - 1.0;
         v2 = 2.0 * therm_erand48(x) - 1.0;
         rsq = zd_rounded(v1 * v1) + zd_rounded(v2 * v2);
         if (!(rsq >= 1.0 || rsq == 0.0)) break;
         nrej++;
      }
      const double fac = sqrt(-2.0 * log(rsq) / rsq);
      g[k] = v2 * fac;
   }
   if (PROBE) rej[i] = nrej;
   else { vx[i] = sigma * g[0]; vy[i] = sigma * g[1]; vz[i] = sigma * g[2]; }
}

/* m |v - vcm|^2 and 1 of a bead, vcm its class's (k_class_sums adds them for the system, every group, every species: the caller reads the
 * selected family's classes) */
struct ThermSpreadBead
{
   const double *vx, *vy, *vz, *massv, *vcm;      /* vcm[3 nclass] */
   const int *group;
   int select, nclass;
   __device__ __forceinline__ void load(int i, int s, double (&v)[2]) const
   {
      const int c = therm_class(select, s, i, group, nclass);
      const double x = vx[i] - vcm[3 * c], y = vy[i] - vcm[3 * c + 1], z = vz[i] - vcm[3 * c + 2];
      v[0] = massv[s] * (x * x + y * y + z * z); v[1] = 1.0;
   }
};
/* tab[8 c ..] = {vcm x y z, vScale, vcmNew x y z, apply}: thermalize.c:257-268 */
__global__ __launch_bounds__(THERM_THREADS) void k_thermalize_rescale(int n, int select, int nclass, int nspecies, const double *__restrict__ tab,
                                                                      const int *__restrict__ species, const int *__restrict__ group,
                                                                      double *__restrict__ vx, double *__restrict__ vy, double *__restrict__ vz)
{
   const int i = blockIdx.x * THERM_THREADS + threadIdx.x;
   if (i >= n) return;
   const int s = min(max(species[i], 0), nspecies - 1);
   const double *t = tab + 8 * therm_class(select, s, i, group, nclass);
   if (t[7] == 0.0) return;
   vx[i] = (vx[i] - t[0]) * t[3] + t[4];
   vy[i] = (vy[i] - t[1]) * t[3] + t[5];
   vz[i] = (vz[i] - t[2]) * t[3] + t[6];
}

/* ---- host side ---------------------------------------------------------- */
struct ThermReq { int method, select, ntemp; const double *temperature; uint64_t seed; int64_t loop; int keep_vcm; };
static int therm_nclass(const ddcmi_ctx *ctx, int select) { return select == 0 ? 1 : (select == 1 ? ctx->nspecies : ctx->ngroup); }
/* the selected family's class c among the classes of k_class_sums */
static int therm_census_class(const ddcmi_ctx *ctx, int select, int c) { return select == 0 ? 0 : (select == 1 ? 1 + ctx->ngroup + c : 1 + c); }
static unsigned long long therm_loopmul(int64_t loop) { return (unsigned long long)((loop % 10000000) + 1); }      /* thermalize.c:118 */

static int therm_check(ddcmi_ctx *ctx, const char *fn, const ThermReq &q)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, q.method < 0 || q.method > THERM_JUTTNER, "%s: method = %d (0 BOLTZMANN, 1 RESCALE)", fn, q.method);
   if (q.method == THERM_JUTTNER) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: method JUTTNER (relativistic) is not supported", fn);
   ARGCHK(ctx, q.select < 0 || q.select > 2, "%s: select = %d (0 global, 1 by species, 2 by group)", fn, q.select);
   const int nclass = therm_nclass(ctx, q.select);
   ARGCHK(ctx, nclass < 1, "%s: the context has no %s", fn, q.select == 1 ? "species" : "groups");
   ARGCHK(ctx, !q.temperature || q.ntemp < nclass, "%s: %d temperatures for %d classes", fn, q.temperature ? q.ntemp : 0, nclass);
   for (int k = 0; k < q.ntemp; k++) ARGCHK(ctx, std::isnan(q.temperature[k]), "%s: temperature[%d] is NaN", fn, k);
   if (q.method == THERM_RESCALE && 1 + ctx->ngroup + ctx->nspecies > census_max_class(4))
      SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d classes, at most %d", fn, 1 + ctx->ngroup + ctx->nspecies, census_max_class(4));
   return DDCMI_OK;
}
/* this rank's draw; rej: the probe's device array, or NULL [sync] */
static int therm_boltzmann_one(ddcmi_ctx *ctx, const ThermReq &q, int *rej)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, nclass = therm_nclass(ctx, q.select);
   if (n <= 0) return DDCMI_OK;      /* (a domain that holds no bead) */
   ENSURE(ctx, ctx->therm_tab, (size_t)nclass);
   HIPCHK(ctx, hipMemcpyAsync(ctx->therm_tab.p, q.temperature, (size_t)nclass * sizeof(double), hipMemcpyHostToDevice, st));
   const dim3 g(cdiv(n, THERM_THREADS)), b(THERM_THREADS);
   if (rej)
      hipLaunchKernelGGL(k_thermalize_boltzmann<true>, g, b, 0, st, n, q.select, nclass, (unsigned long long)q.seed, therm_loopmul(q.loop), ctx->therm_tab.p, ctx->d_mass.p,
                         ctx->nspecies, ctx->species.p, ctx->group.p, ctx->gid.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, rej);
   else
      hipLaunchKernelGGL(k_thermalize_boltzmann<false>, g, b, 0, st, n, q.select, nclass, (unsigned long long)q.seed, therm_loopmul(q.loop), ctx->therm_tab.p, ctx->d_mass.p,
                         ctx->nspecies, ctx->species.p, ctx->group.p, ctx->gid.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, (int *)nullptr);
   HIPCHK(ctx, hipGetLastError());
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}
/* glob = loc[0] + loc[1] + ... in rank order.  An in-process group hands every domain's sums; one context of a decomposed run hands its own
 * and gathers the others through its communicator (collective) */
static int therm_reduce(const std::vector<ddcmi_ctx *> &ranks, const std::vector<std::vector<double>> &loc, std::vector<double> &glob)
{
   ddcmi_ctx *ctx = ranks[0];
   const size_t nv = loc[0].size();
   const std::vector<double> *rows = loc.data();
   size_t nrows = loc.size();
   std::vector<std::vector<double>> got;
   if (ranks.size() == 1 && ctx->nranks > 1 && mg_transport(ctx))      /* (not exchanging(): a loopback rank owns every bead, its sums are the run's) */
   {
      std::vector<double> all((size_t)ctx->nranks * nv);
      const int rcg = mg_allgather_host_values(ctx, loc[0].data(), all.data(), nv, ctx->therm_tab);
      if (rcg) return rcg;
      for (int r = 0; r < ctx->nranks; r++) got.emplace_back(all.begin() + (size_t)r * nv, all.begin() + (size_t)(r + 1) * nv);
      rows = got.data(); nrows = got.size();
   }
   glob = rows[0];
   for (size_t r = 1; r < nrows; r++)
      for (size_t k = 0; k < nv; k++) glob[k] += rows[r][k];
   return DDCMI_OK;
}
static int therm_rescale(const std::vector<ddcmi_ctx *> &ranks, const ThermReq &q)
{
   ddcmi_ctx *c0 = ranks[0];
   const int nclass = therm_nclass(c0, q.select);
   int rc;
   std::vector<std::vector<double>> loc(ranks.size());
   std::vector<double> mom, spread, tab(8 * (size_t)nclass, 0.0), vcm(3 * (size_t)nclass, 0.0);
   /* sum m v and sum m (thermalize.c:193-215) */
   for (size_t r = 0; r < ranks.size(); r++)
   {
      ddcmi_ctx *c = ranks[r];
      const MomentumBead bead = {c->vx.p, c->vy.p, c->vz.p, c->d_mass.p};
      if ((rc = class_sums_one<4>(c, CENSUS_MAX_WG, bead, loc[r]))) { if (r) c0->err = c->err; return rc; }
   }
   if ((rc = therm_reduce(ranks, loc, mom))) return rc;
   for (int k = 0; k < nclass; k++)
   {
      const double *m = mom.data() + 4 * (size_t)therm_census_class(c0, q.select, k);
      if (m[3] > 0.0) for (int a = 0; a < 3; a++) vcm[3 * k + a] = m[a] / m[3];
   }
   /* sum m |v - vcm|^2 and N (thermalize.c:218-237) */
   for (size_t r = 0; r < ranks.size(); r++)
   {
      ddcmi_ctx *c = ranks[r];
      (void)hipSetDevice(c->device);
      ENSURE(c, c->therm_tab, 8 * (size_t)nclass);
      HIPCHK(c, hipMemcpyAsync(c->therm_tab.p, vcm.data(), vcm.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      const ThermSpreadBead bead = {c->vx.p, c->vy.p, c->vz.p, c->d_mass.p, c->therm_tab.p, c->group.p, q.select, nclass};
      if ((rc = class_sums_one<2>(c, CENSUS_MAX_WG, bead, loc[r]))) { if (r) c0->err = c->err; return rc; }
   }
   if ((rc = therm_reduce(ranks, loc, spread))) return rc;
   for (int k = 0; k < nclass; k++)
   {
      const double *sp = spread.data() + 2 * (size_t)therm_census_class(c0, q.select, k);
      double *t = tab.data() + 8 * (size_t)k;
      const double T = q.temperature[k];
      if (!(sp[1] > 1.0) || sp[0] == 0.0) continue;      /* the reference's 0/0 and x/0: the class keeps its bits */
      const double tempSum = sp[0] / (3.0 * (sp[1] - 1.0));
      const double vScale = T > 0.0 ? sqrt(T / tempSum) : 1.0;
      for (int a = 0; a < 3; a++) { t[a] = vcm[3 * k + a]; t[4 + a] = q.keep_vcm ? vcm[3 * k + a] : vcm[3 * k + a] * vScale; }
      t[3] = vScale; t[7] = 1.0;
   }
   for (ddcmi_ctx *c : ranks)
   {
      if (c->nloc <= 0) continue;
      (void)hipSetDevice(c->device);
      HIPCHK(c, hipMemcpyAsync(c->therm_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(k_thermalize_rescale, dim3(cdiv(c->nloc, THERM_THREADS)), dim3(THERM_THREADS), 0, c->stream, c->nloc, q.select, nclass, c->nspecies, c->therm_tab.p,
                         c->species.p, c->group.p, c->vx.p, c->vy.p, c->vz.p);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipStreamSynchronize(c->stream));
   }
   return DDCMI_OK;
}

extern "C" int ddcmi_thermalize(ddcmi_ctx *ctx, int method, int select, int ntemp, const double *temperature, uint64_t seed, int64_t loop, int keep_vcm)
{
   const ThermReq q = {method, select, ntemp, temperature, seed, loop, keep_vcm};
   return analysis_single(ctx, "thermalize", true, [=](ddcmi_ctx *c, const char *fn) { return therm_check(c, fn, q); },
                          [=](ddcmi_ctx *c) {
                             if (q.method == THERM_BOLTZMANN) return therm_boltzmann_one(c, q, nullptr);
                             return therm_rescale(std::vector<ddcmi_ctx *>(1, c), q);
                          });
}
/* in-process group: every domain draws for its own beads; RESCALE adds the domains' sums in rank order */
extern "C" int ddcmi_group_thermalize(ddcmi_ctx **ctxs, int n, int method, int select, int ntemp, const double *temperature, uint64_t seed, int64_t loop, int keep_vcm)
{
   const ThermReq q = {method, select, ntemp, temperature, seed, loop, keep_vcm};
   if (method == THERM_RESCALE)
   {
      int rc = analysis_group(ctxs, n, "thermalize", [=](ddcmi_ctx *c, const char *fn) { return therm_check(c, fn, q); }, [](ddcmi_ctx *, size_t) { return (int)DDCMI_OK; });
      if (rc) return rc;
      rc = therm_rescale(ctxs[0]->group_->ranks, q);
      return rc;
   }
   return analysis_group(ctxs, n, "thermalize", [=](ddcmi_ctx *c, const char *fn) { return therm_check(c, fn, q); },
                         [=](ddcmi_ctx *c, size_t) { return therm_boltzmann_one(c, q, nullptr); });
}
/* TEST-ONLY (include/ddcmi_test.h): what BOLTZMANN would do with this context's owned beads, in the order of ddcmi_download_particles, and no
 * velocity written -- gid[k] the bead, rejects[k] the draws its three gasdev0 calls rejected, -1 where its class is left alone [sync] */
extern "C" int ddcmi_debug_thermalize_rejects(ddcmi_ctx *ctx, int select, int ntemp, const double *temperature, uint64_t seed, int64_t loop, int cap, int *nout,
                                              uint64_t *gid, int *rejects)
{
   const ThermReq q = {THERM_BOLTZMANN, select, ntemp, temperature, seed, loop, 0};
   if (!ctx) return DDCMI_EINVAL;
   int rc = therm_check(ctx, "ddcmi_debug_thermalize_rejects", q);
   if (rc) return rc;
   ARGCHK(ctx, !nout || !gid || !rejects, "ddcmi_debug_thermalize_rejects: NULL output");
   *nout = ctx->nloc;
   ARGCHK(ctx, cap < ctx->nloc, "ddcmi_debug_thermalize_rejects: room for %d beads, the context owns %d", cap, ctx->nloc);
   if (ctx->nloc <= 0) return DDCMI_OK;
   (void)hipSetDevice(ctx->device);
   int *d = nullptr;
   if (hipMalloc((void **)&d, (size_t)ctx->nloc * sizeof(int)) != hipSuccess) SETERR(ctx, DDCMI_ENOMEM, "ddcmi_debug_thermalize_rejects: device allocation of %d ints failed", ctx->nloc);
   rc = therm_boltzmann_one(ctx, q, d);
   if (rc == DDCMI_OK && (hipMemcpy(rejects, d, (size_t)ctx->nloc * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
                          hipMemcpy(gid, ctx->gid.p, (size_t)ctx->nloc * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess))
   {
      ctx->err = "ddcmi_debug_thermalize_rejects: a copy failed";
      rc = DDCMI_ENODEVICE;
   }
   (void)hipFree(d);
   return rc;
}

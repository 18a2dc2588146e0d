/* ddcmi_vaf.inl -- ANALYSIS type VELOCITYAUTOCORRELATION on the device (velocityAutocorrelation.c:117-229,
 * velocityAutocorrelation_eval): sum v0.v and sum d.d over the owned beads, for the system, every group and every species.
 * Included from ddcmi.hip behind the multi-domain path.
 *
 * The reference record (the reference's REF {r, v}, velocityAutocorrelation.c:30, registered with particleRegisterinfo so that it
 * follows its bead): VafRec {v0[3], o[3]} per owned bead in slot order, ctx->vaf, allocated by the first ddcmi_vaf_origin.
 *   v0  the bead's velocity at the time origin.
 *   o   the ORIGIN of its displacement: d = (current position) - o.  The reference adds dt*v to REF.r in every drift loop
 *       (nglf.c:79-86, nglfconstraint.c:537-545); the device keeps positions continuous between rebuilds, so the sum of the drift
 *       moves IS the difference of positions, and no step kernel carries an accumulation.  o is corrected where the library moves
 *       a bead by something that is no drift, by exactly what that moved the bead:
 *         the wrap into the box at a rebuild    k_gather_state, k_mig_classify   o += p_wrapped - p
 *         the barostat's scaling                k_vaf_rescale in front of it      o  = s p - (p - o)
 *       ddcmi_upload_positions (host-integrator mode) places every bead at the image nearest to where it was: the whole host move
 *       counts, with no correction.
 * The record moves with its bead like the LCG64 streams: through k_gather_state's permutation, in the migration records of a
 * decomposed run (six more doubles while tracking is on: mig_width), through the growth of the owned arrays (mg_ensure_owned).
 * ddcmi_upload_state drops the records.
 *
 * The sample is k_class_sums<2, VafBead> of ddcmi_census_frame.inl ({v0.v, d.d} per bead) over at most VAF_MAX_WG workgroups. */

__global__ void k_vaf_origin(int n, const double4 *__restrict__ pos, const double *__restrict__ vx, const double *__restrict__ vy, const double *__restrict__ vz,
                             VafRec *__restrict__ vaf)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if (i >= n) return;
   const double4 p = pos[i];
   VafRec r;
   r.v0[0] = vx[i]; r.v0[1] = vy[i]; r.v0[2] = vz[i];
   r.o[0] = p.x; r.o[1] = p.y; r.o[2] = p.z;
   vaf[i] = r;
}
struct VafBead
{
   const double4 *pos; const double *vx, *vy, *vz; const VafRec *vaf;
   __device__ __forceinline__ void load(int i, int, double (&v)[2]) const
   {
      const double4 p = pos[i];
      const VafRec r = vaf[i];
      v[0] = r.v0[0] * vx[i] + r.v0[1] * vy[i] + r.v0[2] * vz[i];
      const double dx = p.x - r.o[0], dy = p.y - r.o[1], dz = p.z - r.o[2];
      v[1] = dx * dx + dy * dy + dz * dz;
   }
};

/* ---- host side ---------------------------------------------------------- */
static int vaf_origin_one(ddcmi_ctx *ctx)
{
   (void)hipSetDevice(ctx->device);
   const int n = ctx->nloc;
   /* room for what the owned arrays hold: a decomposed rank's beads arrive by migration (mg_ensure_owned grows the records with them) */
   const size_t cap = std::max((size_t)n, ctx->vx.cap) + 1;
   ENSURE(ctx, ctx->vaf, cap);
   if (decomposed(ctx)) ENSURE(ctx, ctx->vaf2, cap);
   if (n > 0)
      hipLaunchKernelGGL(k_vaf_origin, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, n, ctx->pos.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->vaf.p);
   HIPCHK(ctx, hipGetLastError());
   ctx->vaf_on = true;
   return DDCMI_OK;
}
static int vaf_sample_check(ddcmi_ctx *ctx, const char *fn, int ngroup, int nspecies, const void *vaf, const void *msd)
{
   ARGCHK(ctx, ctx->nloc <= 0 && !decomposed(ctx), "%s needs an uploaded state (ddcmi_upload_state)", fn);
   ARGCHK(ctx, !ctx->vaf_on, "%s: no time origin is set (ddcmi_vaf_origin)", fn);
   ARGCHK(ctx, ngroup != ctx->ngroup, "%s: ngroup = %d, the context has %d groups", fn, ngroup, ctx->ngroup);
   ARGCHK(ctx, nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, nspecies, ctx->nspecies);
   ARGCHK(ctx, !vaf || !msd, "%s: NULL output array (vaf %p, msd %p)", fn, vaf, msd);
   if (1 + ngroup + nspecies > census_max_class(2)) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d classes, at most %d", fn, 1 + ngroup + nspecies, census_max_class(2));
   return DDCMI_OK;
}
/* this rank's sums [sync] */
static int vaf_sample_one(ddcmi_ctx *ctx, double *vaf, double *msd)
{
   const VafBead bead = {ctx->pos.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->vaf.p};
   std::vector<double> h;
   int rc = class_sums_one<2>(ctx, VAF_MAX_WG, bead, h);
   if (rc) return rc;
   for (size_t c = 0; c < h.size() / 2; c++) { vaf[c] = h[2 * c]; msd[c] = h[2 * c + 1]; }
   return DDCMI_OK;
}
static int vaf_clear_one(ddcmi_ctx *ctx)
{
   (void)hipSetDevice(ctx->device);
   if (ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   ctx->vaf_on = false;
   ctx->vaf.release(); ctx->vaf2.release();
   return DDCMI_OK;
}
static int vaf_no_check(ddcmi_ctx *, const char *) { return DDCMI_OK; }

extern "C" int ddcmi_vaf_origin(ddcmi_ctx *ctx) { return analysis_single(ctx, "vaf_origin", false, census_state_check, vaf_origin_one); }
extern "C" int ddcmi_vaf_sample(ddcmi_ctx *ctx, int ngroup, int nspecies, double *vaf, double *msd)
{
   return analysis_single(ctx, "vaf_sample", true, [=](ddcmi_ctx *c, const char *fn) { return vaf_sample_check(c, fn, ngroup, nspecies, vaf, msd); },
                          [=](ddcmi_ctx *c) { return vaf_sample_one(c, vaf, msd); });
}
/* (one domain of a group without its records while the others send theirs: the migration records would differ in width) */
extern "C" int ddcmi_vaf_clear(ddcmi_ctx *ctx) { return analysis_single(ctx, "vaf_clear", false, vaf_no_check, vaf_clear_one); }

/* in-process group: every domain's origin; per-rank sums, rank after rank (vaf[r * nclass ...], msd[r * nclass ...]) */
extern "C" int ddcmi_group_vaf_origin(ddcmi_ctx **ctxs, int n)
{
   return analysis_group(ctxs, n, "vaf_origin", census_state_check, [](ddcmi_ctx *c, size_t) { return vaf_origin_one(c); });
}
extern "C" int ddcmi_group_vaf_clear(ddcmi_ctx **ctxs, int n)
{
   return analysis_group(ctxs, n, "vaf_clear", vaf_no_check, [](ddcmi_ctx *c, size_t) { return vaf_clear_one(c); });
}
extern "C" int ddcmi_group_vaf_sample(ddcmi_ctx **ctxs, int n, int ngroup, int nspecies, double *vaf, double *msd)
{
   const size_t nclass = (size_t)1 + ngroup + nspecies;
   return analysis_group(ctxs, n, "vaf_sample", [=](ddcmi_ctx *c, const char *fn) { return vaf_sample_check(c, fn, ngroup, nspecies, vaf, msd); },
                         [=](ddcmi_ctx *c, size_t r) { return vaf_sample_one(c, vaf + r * nclass, msd + r * nclass); });
}

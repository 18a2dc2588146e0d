/* analysis.c -- see analysis.h: the supported ANALYSIS types, one row of `types` each, and the driver's walks over a deck's list. */
#include "analysis.h"
#include "units.h"
#include "chol.h"
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <math.h>
#include <inttypes.h>
#include <sys/stat.h>
#include <time.h>

static int analysis_due(int rate, int64_t loop) { return rate > 0 && loop % rate == 0; }      /* TEST0 */
/* snapshot.<loop>/<filename>, opened for writing (rank 0) */
static FILE *snapshot_fopen(const SIMULATE *simulate, const char *filename, const char *where)
{
   char dir[512], path[1100];
   snprintf(dir, sizeof(dir), "snapshot.%012" PRId64, simulate->loop);      /* CreateSnapshotdir: the directory writeRestart uses */
   if (mkdir(dir, 0777) != 0 && errno != EEXIST) die(where, "cannot create the snapshot directory");
   snprintf(path, sizeof(path), "%s/%s", dir, filename);
   FILE *f = fopen(path, "w");
   if (!f) die(where, "cannot open the output file");
   return f;
}
static void sum_over_ranks(double *buf, int n, const char *where)      /* in rank order, the sum on every rank */
{ if (par.world > 1 && ddcmi_rdzv_allreduce_f64(par.rdzv, buf, n, 0) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv)); }
static void *zalloc(size_t n, size_t size) { void *p = calloc(n, size); if (!p) die("analysis", "out of memory"); return p; }
static void refuse_length(const ddcmi_analysis *an, char *msg, int msglen) { snprintf(msg, msglen, "ANALYSIS %s: length = %d", an->name, an->length); }

/* ------------------------------------------------------------------------- */
/* ANALYSIS type PAIRCORRELATION (paircorrelation.c: parms :68-135, eval_geom :354-457, output :460-520; analysis.c:133-153): the counts
 * come from the device (ddcmi_pair_correlation), are summed over the ranks (integers below 2^53: the double sum is exact, so every rank
 * count gives the same file) and accumulated on the host in the reference's order; rank 0 writes the file. */
typedef struct { int nsample; double *g, *buf; int64_t *cnt, *nb; } PCSTATE;
static void pc_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   int bad = msg[0] != 0;      /* the two range checks at the end speak only in a list without a refusal so far */
   char *m = NULL, *rs = NULL;
   object_get(obj, "delta_r", &an->delta_r, WITH_UNITS, 1, "1", "l", NULL);
   object_get(obj, "rmin", &an->rmin, WITH_UNITS, 1, "0", "l", NULL);
   object_get(obj, "method", &m, STRING, 1, "geom");
   object_get(obj, "rscale", &rs, STRING, 1, "normal");
   const char *method = m ? m : "", *rscale = rs ? rs : "";      /* "key = ;": present and empty */
   if (strcasecmp(method, "geom") == 0) an->method = 0;
   else if (strcasecmp(method, "grid") == 0) an->method = 1;
   else if (strcasecmp(method, "neighborList") == 0) an->method = 2;
   else { snprintf(msg, msglen, "ANALYSIS %s: unrecognized method \"%s\"", an->name, method); bad = 1; }
   if (strcasecmp(rscale, "normal") == 0) an->rscale_log = 0;
   else if (strcasecmp(rscale, "log") == 0) an->rscale_log = 1;
   else { snprintf(msg, msglen, "ANALYSIS %s: unrecognized rscale \"%s\"", an->name, rscale); bad = 1; }
   if (!bad && an->rscale_log && !(an->rmin > 0.0)) { snprintf(msg, msglen, "ANALYSIS %s: rscale = log needs rmin > 0", an->name); bad = 1; }
   if (!bad && an->length <= 0) refuse_length(an, msg, msglen);
   free(m); free(rs);
}
static void *pc_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   const size_t nh = (size_t)(s->nspecies * (s->nspecies + 1) / 2) * an->length;
   PCSTATE *p = zalloc(1, sizeof(PCSTATE));
   p->g = zalloc(nh, sizeof(double)); p->buf = zalloc(nh + s->nspecies, sizeof(double));
   p->cnt = zalloc(nh, sizeof(int64_t)); p->nb = zalloc(s->nspecies, sizeof(int64_t));
   return p;
}
static void pc_clear(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   const ddcmi_setup *s = simulate->setup;
   PCSTATE *p = state;
   memset(p->g, 0, sizeof(double) * (size_t)(s->nspecies * (s->nspecies + 1) / 2) * an->length);
   p->nsample = 0;
}
static int pc_combo(int i, int j, int ns) { int lo = i < j ? i : j, hi = i < j ? j : i; return (hi - lo) + ns * lo - (lo * (lo - 1)) / 2; }
static void pc_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   const ddcmi_setup *s = simulate->setup;
   PCSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const int ns = s->nspecies, nbins = an->length;
   const size_t nh = (size_t)(ns * (ns + 1) / 2) * nbins;
   if (ddcmi_pair_correlation(ctx, an->rmin, an->delta_r, nbins, an->rscale_log, ns, p->cnt, p->nb) != DDCMI_OK)
      die("paircorrelation_eval", ddcmi_last_error(ctx));
   for (size_t k = 0; k < nh; k++) p->buf[k] = (double)p->cnt[k];
   for (int t = 0; t < ns; t++) p->buf[nh + t] = (double)p->nb[t];
   sum_over_ranks(p->buf, (int)(nh + ns), "paircorrelation_eval");
   p->nsample += 1;
   for (int i = 0; i < ns; i++)
      for (int j = i; j < ns; j++)
      {
         const int l = pc_combo(i, j, ns);
         const double recipNiNj = 1.0 / (p->buf[nh + i] * p->buf[nh + j]);
         for (int k = 0; k < nbins; k++) { double nBonds = p->buf[(size_t)l * nbins + k]; nBonds *= recipNiNj; p->g[(size_t)l * nbins + k] += nBonds; }
      }
}
static void pc_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   const ddcmi_setup *s = simulate->setup;
   PCSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const int ns = s->nspecies, np = ns * (ns + 1) / 2, nbins = an->length;
   if (p->nsample == 0) { pc_clear(simulate, an, p); return; }
   if (par.rank == 0)
   {
      FILE *f = snapshot_fopen(simulate, an->filename, "paircorrelation_output");
      double h[9];
      if (ddcmi_get_box(ctx, h) != DDCMI_OK) die("paircorrelation_output", ddcmi_last_error(ctx));
      const double volume = h[0] * h[4] * h[8], sc = volume / p->nsample;
      const double rmin = an->rmin, dr = an->delta_r, rmax = rmin + nbins * dr;
      const double logDelta = an->rscale_log ? (log10(rmax) - log10(rmin)) / (nbins * 1.0) : 0.0;
      double *left = malloc(sizeof(double) * nbins), *right = malloc(sizeof(double) * nbins);
      for (int k = 0; k < nbins; k++)
      {
         if (an->rscale_log) left[k] = pow(10, log10(rmin) + k * logDelta);
         else { left[k] = rmin + k * dr; right[k] = rmin + (k + 1) * dr; }
      }
      if (an->rscale_log) { for (int k = 0; k + 1 < nbins; k++) right[k] = left[k + 1]; right[nbins - 1] = rmax; }
      for (int k = 0; k < nbins; k++)
      {
         const double dv = 4.0 * M_PI / 3.0 * (right[k] * right[k] * right[k] - left[k] * left[k] * left[k]);
         for (int l = 0; l < np; l++) p->g[k + (size_t)nbins * l] *= sc / dv;
      }
      fprintf(f, "# rmin = %f Ang; delta_r = %f Ang; length = %d; eval_rate = %d; outputrate = %d;\n", units_convert(rmin, NULL, "Angstrom"),
              units_convert(dr, NULL, "Angstrom"), nbins, an->eval_rate, an->outputrate);
      fprintf(f, "# nsample = %d;\n", p->nsample);
      fprintf(f, "# r(Ang) ");
      for (int l = 0; l < np; l++)
      {
         int ti = -1, tj = -1;
         for (int i = 0; i < ns && ti < 0; i++) for (int j = i; j < ns; j++) if (pc_combo(i, j, ns) == l) { ti = i; tj = j; break; }      /* comboReverseIndex */
         fprintf(f, "%s-%s ", s->species_name[ti], s->species_name[tj]);
      }
      fprintf(f, "\n");
      for (int k = 0; k < nbins; k++)
      {
         fprintf(f, "%f ", units_convert(0.5 * (left[k] + right[k]), NULL, "Angstrom"));
         for (int l = 0; l < np; l++) fprintf(f, "%e ", p->g[k + (size_t)nbins * l]);
         fprintf(f, "\n");
      }
      fclose(f);
      free(left); free(right);
   }
   pc_clear(simulate, an, p);
}
static void pc_free(void *state) { PCSTATE *p = state; free(p->g); free(p->buf); free(p->cnt); free(p->nb); free(p); }

/* ANALYSIS type VELOCITYAUTOCORRELATION (velocityAutocorrelation.c: parms :59-60, eval :117-229, output :230-327): the state machine of
 * the reference -- last, nsample, vaf0 / msd0 of the current window, vaf_ / msd_ accumulated over the windows -- over the device's sums
 * (ddcmi_vaf_origin / ddcmi_vaf_sample).  Every class is kept ([1 + ngroup + nspecies] blocks of length + 1); the output leaves out
 * the group block of a single group and the species block of a single species, as the reference does.  The sums over the ranks go
 * by ddcmi_rdzv_allreduce_f64, in rank order.  A restart begins with a fresh origin (last = 0).  There is no clear: the startup
 * evaluation stays and sets the first origin. */
typedef struct { int last, nsample, ncl, len; double *vaf0, *msd0, *vaf_, *msd_, *buf; } VAFSTATE;
static void vaf_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen) { (void)obj; if (an->length < 1) refuse_length(an, msg, msglen); }
static void *vaf_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   VAFSTATE *p = zalloc(1, sizeof(VAFSTATE));
   p->len = an->length; p->ncl = 1 + (s->ngroup > 0 ? s->ngroup : 1) + s->nspecies;
   const size_t tot = (size_t)p->ncl * (p->len + 1);
   p->vaf0 = zalloc(tot, sizeof(double)); p->msd0 = zalloc(tot, sizeof(double));
   p->vaf_ = zalloc(tot, sizeof(double)); p->msd_ = zalloc(tot, sizeof(double)); p->buf = zalloc(2 * (size_t)p->ncl, sizeof(double));
   return p;
}
/* sample k of the current window: the global sums of every class */
static void vaf_take(SIMULATE *simulate, VAFSTATE *p, int k)
{
   const ddcmi_setup *s = simulate->setup;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   if (ddcmi_vaf_sample(ctx, s->ngroup > 0 ? s->ngroup : 1, s->nspecies, p->buf, p->buf + p->ncl) != DDCMI_OK) die("velocityAutocorrelation_eval", ddcmi_last_error(ctx));
   sum_over_ranks(p->buf, 2 * p->ncl, "velocityAutocorrelation_eval");
   for (int c = 0; c < p->ncl; c++) { p->vaf0[k + c * (p->len + 1)] = p->buf[c]; p->msd0[k + c * (p->len + 1)] = p->buf[p->ncl + c]; }
}
static void vaf_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)an;
   VAFSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const size_t tot = (size_t)p->ncl * (p->len + 1);
   int k = p->last;
   if (k > 0) vaf_take(simulate, p, k);
   if (k == p->len)
   {
      p->nsample++;
      for (size_t l = 0; l < tot; l++) { p->msd_[l] += p->msd0[l]; p->vaf_[l] += p->vaf0[l]; p->msd0[l] = 0.0; p->vaf0[l] = 0.0; }
      k = p->last = 0;
   }
   if (k == 0)
   {
      if (ddcmi_vaf_origin(ctx) != DDCMI_OK) die("velocityAutocorrelation_eval", ddcmi_last_error(ctx));
      vaf_take(simulate, p, 0);      /* sum v.v, and zero */
   }
   p->last++;
}
static void vaf_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   const ddcmi_setup *s = simulate->setup;
   VAFSTATE *p = state;
   const int len = p->len, eval_rate = an->eval_rate, outputrate = an->outputrate;
   if ((long long)p->nsample * len * eval_rate != outputrate) return;      /* (no file, no reset) */
   const int ng = s->ngroup > 0 ? s->ngroup : 1, ngroups = ng == 1 ? 0 : ng, nspecies = s->nspecies == 1 ? 0 : s->nspecies;
   if (par.rank == 0)
   {
      FILE *f = snapshot_fopen(simulate, an->filename, "velocityAutocorrelation_output");
      /* member counts of the whole system (sys->group[ii]->nMember, species likewise) */
      double *ngm = calloc(ng, sizeof(double)), *nsm = calloc(s->nspecies, sizeof(double));
      for (int i = 0; i < s->natoms; i++) { ngm[s->group ? s->group[i] : 0] += 1.0; nsm[s->species[i]] += 1.0; }
      const double nglobal = (double)simulate->system->nglobal;
      const double time_convert = units_convert(1.0, NULL, "t"), v2_convert = units_convert(1.0, NULL, "velocity^2"), r2_convert = units_convert(1.0, NULL, "l^2");
      fprintf(f, "%-33s", "#time (fs)  System vaf MSD");
      for (int ii = 0; ii < ngroups; ii++) { char temp[300]; snprintf(temp, sizeof(temp), "  Group %s vaf MSD", s->group_name[ii]); fprintf(f, "%-26s", temp); }
      for (int ii = 0; ii < nspecies; ii++) { char temp[300]; snprintf(temp, sizeof(temp), "  Species %s vaf MSD", s->species_name[ii]); fprintf(f, "%-26s", temp); }
      fprintf(f, " (vaf in Ang^2/fs^2; msd in Ang^2)\n");
      for (int k = 0; k <= len; k++)
      {
         const double time = time_convert * k * simulate->dt * eval_rate;
         fprintf(f, "%f", time);
         fprintf(f, " %e %e", (v2_convert * p->vaf_[k] / p->nsample) / nglobal, (r2_convert * p->msd_[k] / p->nsample) / nglobal);
         for (int ii = 0; ii < ngroups; ii++)
         {
            const int off = (1 + ii) * (len + 1);
            fprintf(f, " %e %e", (v2_convert * p->vaf_[k + off] / p->nsample) / ngm[ii], (r2_convert * p->msd_[k + off] / p->nsample) / ngm[ii]);
         }
         for (int ii = 0; ii < nspecies; ii++)
         {
            const int off = (1 + ng + ii) * (len + 1);
            fprintf(f, " %e %e", (v2_convert * p->vaf_[k + off] / p->nsample) / nsm[ii], (r2_convert * p->msd_[k + off] / p->nsample) / nsm[ii]);
         }
         fprintf(f, "\n");
      }
      fclose(f);
      free(ngm); free(nsm);
   }
   memset(p->vaf_, 0, sizeof(double) * (size_t)p->ncl * (len + 1));
   memset(p->msd_, 0, sizeof(double) * (size_t)p->ncl * (len + 1));
   p->nsample = 0;
}
static void vaf_free(void *state) { VAFSTATE *p = state; free(p->vaf0); free(p->msd0); free(p->vaf_); free(p->msd_); free(p->buf); free(p); }

/* ANALYSIS type vcmWrite (vcmWrite.c: parms :23-64, output :71-136, close :142-146): the centre-of-mass velocity of the system, of
 * every group and of every species -- every block, a single group's and a single species' too -- one line per output into a file of
 * the run directory that rank 0 opens for append, with a header line, at init.  The sums come from the device
 * (ddcmi_momentum_by_class) and are added over the ranks in rank order.  eval does nothing; there is no clear. */
#define LOOP_WIDTH 12      /* loopFormatSize: the width printinfo writes the data file's loop column with (plugin.c) */
typedef struct { FILE *file; int ng, ncl; double *buf; } VCMSTATE;
static void vcm_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen) { (void)obj; (void)an; (void)msg; (void)msglen; }
static void *vcm_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   VCMSTATE *p = zalloc(1, sizeof(VCMSTATE));
   p->ng = s->ngroup > 0 ? s->ngroup : 1; p->ncl = 1 + p->ng + s->nspecies;
   p->buf = zalloc(4 * (size_t)p->ncl, sizeof(double));
   if (par.rank == 0)
   {
      p->file = fopen(an->filename, "a");
      if (!p->file) die("vcmWrite_parms", "cannot open the output file");
      char fmt[32]; snprintf(fmt, sizeof(fmt), "-%%%ds %%14s", LOOP_WIDTH);      /* (the reference's format as it stands, its leading '-' outside the conversion) */
      fprintf(p->file, fmt, "#loop", "time(fs)");
      fprintf(p->file, "%-51s", "     System vx vy vz (Ang/fs)");
      for (int ii = 0; ii < p->ng; ii++)
      {
         char temp[300]; snprintf(temp, sizeof(temp), "     Group %s vx vy vz (Ang/fs)", s->ngroup > 0 ? s->group_name[ii] : "group");
         fprintf(p->file, "%-51s", temp);
      }
      for (int ii = 0; ii < s->nspecies; ii++)
      {
         char temp[300]; snprintf(temp, sizeof(temp), "     Species %s vx vy vz (Ang/fs)", s->species_name[ii]);
         fprintf(p->file, "%-51s", temp);
      }
      fprintf(p->file, "\n");
      fflush(p->file);
   }
   return p;
}
static void vcm_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state) { (void)simulate; (void)an; (void)state; }
static void vcm_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)an;
   VCMSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   double *mv = p->buf, *m = p->buf + 3 * p->ncl;
   if (ddcmi_momentum_by_class(ctx, p->ng, simulate->setup->nspecies, mv, m) != DDCMI_OK) die("vcmWrite_output", ddcmi_last_error(ctx));
   sum_over_ranks(p->buf, 4 * p->ncl, "vcmWrite_output");
   if (par.rank != 0) return;
   const double time = units_convert(1.0, NULL, "fs") * simulate->time, velocity_convert = units_convert(1.0, NULL, "Ang/fs");
   fprintf(p->file, "%*" PRId64, LOOP_WIDTH, simulate->loop);
   fprintf(p->file, " %16.6f", time);
   for (int ii = 0; ii < p->ncl; ii++)
   {
      double v[3] = {mv[3 * ii], mv[3 * ii + 1], mv[3 * ii + 2]};
      if (m[ii] > 0.0) { const double r = 1 / m[ii]; v[0] *= r; v[1] *= r; v[2] *= r; }      /* VSCALE(vmsum[ii], 1/msum[ii]) */
      for (int a = 0; a < 3; a++) v[a] *= velocity_convert;
      fprintf(p->file, " %16.6e %16.6e %16.6e", v[0], v[1], v[2]);
   }
   fprintf(p->file, "\n");
   fflush(p->file);
}
static void vcm_free(void *state) { VCMSTATE *p = state; if (p->file) fclose(p->file); free(p->buf); free(p); }

/* ANALYSIS type zdensity (zdensity.c: parms :36-50, output :56-175): the beads' density profile along z, orthorhombic boxes.  The
 * histogram comes from the device (ddcmi_zdensity: at most 2048 bins), is added over the ranks in rank order, and rank 0 writes
 * snapshot.<loop>/<filename>.  eval does nothing; there is no clear.  nz < 1 (the reference writes an empty file) is refused. */
typedef struct { double *density; } ZDSTATE;
static void zd_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   char *sm = NULL;
   object_get(obj, "nz", &an->nz, INT, 1, "0");
   object_get(obj, "smearRadius", &an->smear_radius, WITH_UNITS, 1, "0", "l", NULL);
   object_get(obj, "smearMethod", &sm, STRING, 1, "impulse");
   an->smear_method = sm && strcasecmp(sm, "hat") == 0;      /* anything else is impulse */
   free(sm);
   if (an->nz < 1) snprintf(msg, msglen, "ANALYSIS %s: nz = %d", an->name, an->nz);
}
static void *zd_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   (void)simulate;
   ZDSTATE *p = zalloc(1, sizeof(ZDSTATE));
   p->density = zalloc(an->nz, sizeof(double));
   return p;
}
static void zd_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state) { (void)simulate; (void)an; (void)state; }
static void zd_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   ZDSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const int nz = an->nz;
   if (ddcmi_zdensity(ctx, nz, an->smear_radius, an->smear_method, p->density) != DDCMI_OK) die("zdensity_output", ddcmi_last_error(ctx));
   sum_over_ranks(p->density, nz, "zdensity_output");
   if (par.rank != 0) return;
   FILE *f = snapshot_fopen(simulate, an->filename, "zdensity_output");
   double h[9];
   if (ddcmi_get_box(ctx, h) != DDCMI_OK) die("zdensity_output", ddcmi_last_error(ctx));
   const double lc = units_convert(1.0, NULL, "Angstrom");
   const double boxVol = (h[0] * h[4] * h[8]) * lc * lc * lc, bz = h[8];
   for (int ii = 0; ii < nz; ii++)
   {
      const double z = ((ii + 0.5) * (bz / nz)) / (bz);
      const double dens = p->density[ii] * (nz / boxVol);
      fprintf(f, "%f %f %f\n", z, dens, p->density[ii]);
   }
   fclose(f);
}
static void zd_free(void *state) { ZDSTATE *p = state; free(p->density); free(p); }

/* ANALYSIS type KINETICENERGYDISTN (kineticEnergyDistn.c: parms :45-93, eval :157-188, output :98-155, clear :189-203): per BIN object of
 * distGroups the histogram of one species' kinetic energies.  Every evaluation comes from the device (ddcmi_kinetic_energy_distn: all
 * groups in one pass), is combined over the ranks -- the counts and the sum of K added in rank order (integers below 2^53: exact),
 * the minima and maxima by a maximum over the ranks -- and accumulated until the output, where rank 0 writes
 * snapshot.<loop>/<BIN name>_kDist.data per group and one line of kinetic.data (opened for append, with a header line, at init; the
 * time stays in internal units, as in the reference), and everything is cleared.  The startup evaluation is cleared as well. */
typedef struct { FILE *file; int nd, nbt; int *nbins, *map; double *emin, *emax; int64_t *cnt, *tal; double *stats, *buf, *acc, *accmin, *accmax; } KDSTATE;
static void kd_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   char **names = NULL;
   const int nd = object_getv(obj, "distGroups", (void **)&names, STRING, IGNORE_IF_NOT_FOUND);
   an->ndist = nd > 0 ? nd : 0;
   an->dist = zalloc(an->ndist > 0 ? an->ndist : 1, sizeof(ddcmi_kdist_group));
   long nbt = 0;
   for (int j = 0; j < an->ndist; j++)
   {
      ddcmi_kdist_group *b = &an->dist[j];
      b->name = names[j];
      const OBJECT *og = object_find(b->name, "BIN");
      if (!og) { b->species = strdup(""); b->nbins = 1; snprintf(msg, msglen, "ANALYSIS %s: distGroups names %s, and there is no BIN object of that name", an->name, b->name); continue; }
      object_get(og, "species", &b->species, STRING, 1, "");
      if (!b->species) b->species = strdup("");
      object_get(og, "emin", &b->emin, WITH_UNITS, 1, "0", "energy", NULL);
      object_get(og, "emax", &b->emax, WITH_UNITS, 1, "0", "energy", NULL);
      object_get(og, "nBins", &b->nbins, INT, 1, "1");
      if (b->nbins < 1) snprintf(msg, msglen, "ANALYSIS %s: BIN %s: nBins = %d", an->name, b->name, b->nbins);
      else if (!isfinite(b->emin) || !isfinite(b->emax)) snprintf(msg, msglen, "ANALYSIS %s: BIN %s: emin = %g, emax = %g: not finite", an->name, b->name, b->emin, b->emax);
      else if (!(b->emax > b->emin)) snprintf(msg, msglen, "ANALYSIS %s: BIN %s: emax = %g <= emin = %g", an->name, b->name, b->emax, b->emin);
      for (int i = 0; i < j; i++)      /* the reference's assert(mapS2D[i] == -1) */
         if (b->species[0] && an->dist[i].species && strcmp(an->dist[i].species, b->species) == 0)
         { snprintf(msg, msglen, "ANALYSIS %s: species %s is claimed by BIN %s and by BIN %s", an->name, b->species, an->dist[i].name, b->name); break; }
      nbt += b->nbins > 0 ? b->nbins : 0;
   }
   free(names);
   if (DDCMI_KDIST_LDS_BYTES((long)an->ndist, nbt) > DDCMI_KDIST_MAX_LDS)
      snprintf(msg, msglen, "ANALYSIS %s: %ld bins in %d groups need %ld bytes of the device's LDS, at most %d (4 per bin, 108 per group)", an->name, nbt, an->ndist,
               DDCMI_KDIST_LDS_BYTES((long)an->ndist, nbt), DDCMI_KDIST_MAX_LDS);
}
static void kd_clear(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)simulate; (void)an;
   KDSTATE *p = state;
   memset(p->acc, 0, sizeof(double) * (size_t)(p->nbt + 4 * p->nd));
   for (int g = 0; g < p->nd; g++) { p->accmin[g] = 1e300; p->accmax[g] = 0.0; }
}
static void *kd_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   KDSTATE *p = zalloc(1, sizeof(KDSTATE));
   const int nd = p->nd = an->ndist;
   p->nbins = zalloc(nd + 1, sizeof(int)); p->emin = zalloc(nd + 1, sizeof(double)); p->emax = zalloc(nd + 1, sizeof(double));
   p->map = zalloc(s->nspecies + 1, sizeof(int));
   for (int i = 0; i < s->nspecies; i++) p->map[i] = -1;
   for (int j = 0; j < nd; j++)
   {
      p->nbins[j] = an->dist[j].nbins; p->emin[j] = an->dist[j].emin; p->emax[j] = an->dist[j].emax;
      p->nbt += an->dist[j].nbins;
      for (int i = 0; i < s->nspecies; i++)
         if (strcmp(an->dist[j].species, s->species_name[i]) == 0) { p->map[i] = j; break; }      /* (a BIN of a species the system lacks stays empty) */
   }
   const size_t nv = (size_t)p->nbt + 4 * nd;
   p->cnt = zalloc(p->nbt + 1, sizeof(int64_t)); p->tal = zalloc(3 * nd + 1, sizeof(int64_t)); p->stats = zalloc(3 * nd + 1, sizeof(double));
   p->buf = zalloc(nv + 2 * nd + 1, sizeof(double)); p->acc = zalloc(nv + 1, sizeof(double));
   p->accmin = zalloc(nd + 1, sizeof(double)); p->accmax = zalloc(nd + 1, sizeof(double));
   kd_clear(simulate, an, p);
   if (par.rank == 0)
   {
      p->file = fopen("kinetic.data", "a");
      if (!p->file) die("kineticEnergyDistn_parms", "cannot open kinetic.data");
      fprintf(p->file, "# loop  time(fs)   \n");
      fflush(p->file);
   }
   return p;
}
static void kd_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)an;
   KDSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const int nd = p->nd, nbt = p->nbt, nv = nbt + 4 * nd;
   if (nd == 0) return;
   if (ddcmi_kinetic_energy_distn(ctx, simulate->setup->nspecies, nd, p->emin, p->emax, p->nbins, p->map, p->cnt, p->tal, p->stats) != DDCMI_OK)
      die("kineticEnergyDistn_eval", ddcmi_last_error(ctx));
   double *mm = p->buf + nv;      /* {-min, max} of every group: both go by a maximum over the ranks */
   for (int k = 0; k < nbt; k++) p->buf[k] = (double)p->cnt[k];
   for (int g = 0; g < nd; g++)
   {
      for (int q = 0; q < 3; q++) p->buf[nbt + 4 * g + q] = (double)p->tal[3 * g + q];
      p->buf[nbt + 4 * g + 3] = p->stats[3 * g];
      mm[g] = -p->stats[3 * g + 1]; mm[nd + g] = p->stats[3 * g + 2];
   }
   sum_over_ranks(p->buf, nv, "kineticEnergyDistn_eval");
   if (par.world > 1 && ddcmi_rdzv_allreduce_f64(par.rdzv, mm, 2 * nd, 1) != DDCMI_OK) die("kineticEnergyDistn_eval", ddcmi_rdzv_last_error(par.rdzv));
   for (int k = 0; k < nv; k++) p->acc[k] += p->buf[k];
   for (int g = 0; g < nd; g++)
   {
      if (-mm[g] < p->accmin[g]) p->accmin[g] = -mm[g];
      if (mm[nd + g] > p->accmax[g]) p->accmax[g] = mm[nd + g];
   }
}
static void kd_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   KDSTATE *p = state;
   if (par.rank == 0)
   {
      const double eC = units_convert(1.0, NULL, "eV");
      int off = 0;
      for (int i = 0; i < p->nd; i++)
      {
         char filename[600];
         snprintf(filename, sizeof(filename), "%s_kDist.data", an->dist[i].name);
         FILE *f = snapshot_fopen(simulate, filename, "kineticEnergyDistn_output");
         fprintf(f, "%-14s %14s %14s\n", "# Energy (eV)", "pdf (1/eV)", "cnt");
         const double *t = p->acc + p->nbt + 4 * i;      /* cntTotal, subCnt, supCnt, sum K */
         const double cntTotal = t[0], minValue = p->emin[i], delta = (p->emax[i] - p->emin[i]) / p->nbins[i];
         for (int j = 0; j < p->nbins[i]; j++)
         {
            const double cnt = p->acc[off + j];
            const double energy = ((j + 0.5) * delta + minValue) * eC;
            const double pdf = cnt / (cntTotal * delta) / eC;
            fprintf(f, "%e %e %e\n", energy, pdf, cnt);
         }
         fclose(f);
         off += p->nbins[i];
         const double ave = cntTotal ? t[3] / cntTotal : 0.0;
         fprintf(p->file, "%*" PRId64, LOOP_WIDTH, simulate->loop);
         fprintf(p->file, " %16.6f ", simulate->time);
         fprintf(p->file, "%12.6f %12.8f %12.8f %4.0f %4.0f %8.0f ", ave * eC, p->accmin[i] * eC, p->accmax[i] * eC, t[1], t[2], cntTotal);
      }
      fprintf(p->file, "\n");
      fflush(p->file);
   }
   kd_clear(simulate, an, p);
}
static void kd_free(void *state)
{
   KDSTATE *p = state;
   if (p->file) fclose(p->file);
   free(p->nbins); free(p->map); free(p->emin); free(p->emax); free(p->cnt); free(p->tal); free(p->stats); free(p->buf); free(p->acc); free(p->accmin); free(p->accmax); free(p);
}

/* ANALYSIS type DSF | DynamicStructureFactor | Dynamic_Structure_Factor (dsf.c: parms :33-96, eval :127-217, output :98-124, close
 * :219-231, addKvectors :234-269): the time series of the charge-density modes rho(k, t) = (1/N) sum q_j exp(i k.r_j) over the beads of
 * one species (or all), N their global count, on the axis-aligned wave vectors k = m b_a of an orthorhombic box.  Every m > 0 of the
 * list adds (0,0,m), (0,m,0), (m,0,0), in that order and as often as it is listed.  Every evaluation comes from the device
 * (ddcmi_charge_density_modes: all m up to the largest in one pass), is added over the ranks in rank order together with the count,
 * divided by the global count where that is positive, and buffered with the loop and the driver's time; output writes the buffered
 * rows into a file of the run directory that rank 0 opens for append, with a header line, at init, and so does an evaluation that
 * finds outputrate / eval_rate + 1 rows buffered.  There is no clear: the startup sample is kept.  What is still buffered at the end
 * of the run is written before the file is closed.  What the reference leaves to an abort, an assert or a division by zero is
 * refused at load: no `m` key, eval_rate < 1 or outputrate < 1, a species the system lacks (deck.c), a largest m above
 * DDCMI_DSF_MAX_M. */
typedef struct { FILE *file; int nk, mmax, nbuf, nbufmax, *axis, *mk, *select; int64_t *loop; double *time, *buffer, *rho; } DSFSTATE;
static void dsf_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   an->nm = object_testforkeyword(obj, "m") ? object_getv(obj, "m", (void **)&an->m, INT, IGNORE_IF_NOT_FOUND) : 0;
   if (an->nm < 0) an->nm = 0;
   if (object_testforkeyword(obj, "species")) object_get(obj, "species", &an->dsf_species, STRING, 1, "");
   if (an->dsf_species && !an->dsf_species[0]) { free(an->dsf_species); an->dsf_species = NULL; }      /* "species = ;" */
   if (an->dsf_species && !object_testforkeyword(obj, "filename"))
   {
      char name[600];
      snprintf(name, sizeof(name), "rho_k_%s.data", an->dsf_species);
      free(an->filename); an->filename = strdup(name);
   }
   int mmax = 0;
   for (int i = 0; i < an->nm; i++) if (an->m[i] > mmax) mmax = an->m[i];
   if (an->nm < 1) snprintf(msg, msglen, "ANALYSIS %s: no m key (the list of wave numbers)", an->name);
   else if (an->eval_rate < 1 || an->outputrate < 1) snprintf(msg, msglen, "ANALYSIS %s: eval_rate = %d, outputrate = %d: both must be at least 1", an->name, an->eval_rate, an->outputrate);
   else if (mmax > DDCMI_DSF_MAX_M) snprintf(msg, msglen, "ANALYSIS %s: m = %d, the device takes at most %d", an->name, mmax, DDCMI_DSF_MAX_M);
}
static void dsf_write(DSFSTATE *p)      /* dsf_output */
{
   if (par.rank == 0)
   {
      for (int ii = 0; ii < p->nbuf; ii++)
      {
         fprintf(p->file, "%8.8d %16.6f", (int)p->loop[ii], p->time[ii]);
         for (int jj = 0; jj < p->nk; jj++) fprintf(p->file, "   %13.6e %13.6e", p->buffer[2 * ((size_t)ii * p->nk + jj)], p->buffer[2 * ((size_t)ii * p->nk + jj) + 1]);
         fprintf(p->file, "\n");
      }
      fflush(p->file);
   }
   p->nbuf = 0;
}
static void *dsf_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   DSFSTATE *p = zalloc(1, sizeof(DSFSTATE));
   p->axis = zalloc(3 * (size_t)an->nm + 1, sizeof(int)); p->mk = zalloc(3 * (size_t)an->nm + 1, sizeof(int));
   for (int i = 0; i < an->nm; i++)
   {
      if (an->m[i] <= 0) continue;      /* addKvectors finds no vector */
      if (an->m[i] > p->mmax) p->mmax = an->m[i];
      for (int a = 2; a >= 0; a--) { p->axis[p->nk] = a; p->mk[p->nk] = an->m[i]; p->nk++; }      /* (0,0,m), (0,m,0), (m,0,0) */
   }
   if (an->dsf_species)
   {
      p->select = zalloc(s->nspecies + 1, sizeof(int));
      for (int i = 0; i < s->nspecies; i++) p->select[i] = strcmp(an->dsf_species, s->species_name[i]) == 0;
   }
   p->nbufmax = an->outputrate / an->eval_rate + 1;
   p->loop = zalloc(p->nbufmax, sizeof(int64_t)); p->time = zalloc(p->nbufmax, sizeof(double));
   p->buffer = zalloc(2 * (size_t)p->nbufmax * p->nk + 1, sizeof(double));
   p->rho = zalloc(6 * (size_t)(p->mmax > 0 ? p->mmax : 1) + 1, sizeof(double));
   if (par.rank == 0)
   {
      p->file = fopen(an->filename, "a");
      if (!p->file) die("dsf_parms", "cannot open the output file");
      fprintf(p->file, "%-8s %16s", "#loop", "time");
      for (int ii = 0; ii < p->nk; ii++)
      {
         char tmp[256];
         const int a = p->axis[ii], m = p->mk[ii];
         snprintf(tmp, sizeof(tmp), "    (%d,%d,%d)", a == 0 ? m : 0, a == 1 ? m : 0, a == 2 ? m : 0);
         fprintf(p->file, "%-30s", tmp);
      }
      fprintf(p->file, "\n");
      fflush(p->file);
   }
   return p;
}
static void dsf_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)an;
   DSFSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   if (p->nbuf >= p->nbufmax) dsf_write(p);
   const int nv = 6 * p->mmax;
   int64_t count = 0;
   if (p->mmax > 0 && ddcmi_charge_density_modes(ctx, simulate->setup->nspecies, p->select, p->mmax, p->rho, &count) != DDCMI_OK)
      die("dsf_eval", ddcmi_last_error(ctx));
   p->rho[nv] = (double)count;      /* (an integer below 2^53: the double sum is exact) */
   sum_over_ranks(p->rho, nv + 1, "dsf_eval");
   const double countSum = p->rho[nv];
   double *row = p->buffer + 2 * (size_t)p->nbuf * p->nk;
   for (int ii = 0; ii < p->nk; ii++)
      for (int q = 0; q < 2; q++)
      {
         double v = p->rho[2 * ((size_t)p->axis[ii] * p->mmax + (p->mk[ii] - 1)) + q];
         if (countSum > 0) v /= countSum;
         row[2 * ii + q] = v;
      }
   p->loop[p->nbuf] = simulate->loop;
   p->time[p->nbuf] = simulate->time;
   p->nbuf++;
}
static void dsf_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state) { (void)simulate; (void)an; dsf_write(state); }
static void dsf_free(void *state)      /* dsf_close */
{
   DSFSTATE *p = state;
   dsf_write(p);
   if (p->file) fclose(p->file);
   free(p->axis); free(p->mk); free(p->select); free(p->loop); free(p->time); free(p->buffer); free(p->rho); free(p);
}

/* ANALYSIS type subsetWrite | subset_write with format = binaryCharmm (subsetWrite.c: parms :62-168, subsetWriteBinaryCharmm :409-522,
 * rejectParticle :532-564; pinfo.c; write_fileheader, io.c:352-404): a trajectory frame of the beads a filter selects.  eval does
 * nothing, as in the reference.  At outputrate every rank takes its records from the device (ddcmi_subset_records: selected, compacted
 * and packed there, 24 bytes per selected bead), the counts are gathered, then the blocks on rank 0 in rank order, and rank 0 writes
 * snapshot.<loop>/<filename>#000000 -- header, then the records -- under a temporary name and renames it.  One file whatever nfiles
 * says.  The other formats (pio, ovito) carry a per-bead potential energy that the device does not keep: deck.c leaves those objects
 * unsupported.  Refused at load where the reference would crash: modulus < 1 (a division by zero), a species the system lacks, a pinfo
 * range beyond 4 bytes (deck.c).
 * pinfo (pinfoEncodeInit / pinfoEncode): the distinct group names and the distinct species names in index order; every species has the
 * type ATOM on this path, so pinfo = gMap[group] + sMap[species] * nGroups.  The reference leaves gMap / sMap of a repeated name
 * unset; here it is the index of the name's first occurrence, the object pinfoDecode's lookup by name would return.
 * misc_info: the pieces of the reference's PioSet(file, "misc_info", ...) calls in their order, joined by one blank (pio.c is not part
 * of the reference tree; the blank is how its other headers read). */
int ddcmi_pinfo_fits(int ngroups, int nspecies, int ntypes)
{
   if (ngroups < 1 || nspecies < 1 || ntypes < 1) return 1;
   return (double)ngroups * (double)nspecies * (double)ntypes <= 4294967295.0;
}
typedef struct { ddcmi_subset_filter f; int *include; uint32_t *gterm, *sterm; int nug, nus; char **ugname, **usname; char *info; } SWSTATE;
static void sw_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   static const char *const rkey[6] = {"xmin", "xmax", "ymin", "ymax", "zmin", "zmax"};
   static const char *const vkey[6] = {"vxmin", "vxmax", "vymin", "vymax", "vzmin", "vzmax"};
   char buf[32];
   object_get(obj, "nfiles", &an->sw_nfiles, INT, 1, "0");
   object_get(obj, "modulus", &an->sw_modulus, INT, 1, "1");
   if (object_testforkeyword(obj, "idList"))
   {
      an->sw_nid = object_getv(obj, "idList", (void **)&an->sw_idlist, U64, IGNORE_IF_NOT_FOUND);
      if (an->sw_nid < 0) an->sw_nid = 0;
      if (!an->sw_idlist) an->sw_idlist = zalloc(1, sizeof(uint64_t));      /* "idList = ;": a list without a member selects nothing */
      for (int i = 1; i < an->sw_nid; i++)      /* qsort(compareGid) */
      {
         const uint64_t v = an->sw_idlist[i];
         int j = i;
         for (; j > 0 && an->sw_idlist[j - 1] > v; j--) an->sw_idlist[j] = an->sw_idlist[j - 1];
         an->sw_idlist[j] = v;
      }
   }
   object_get(obj, "idmin", &an->sw_idmin, U64, 1, "0");
   snprintf(buf, sizeof(buf), "%" PRIu64, (uint64_t)UINT64_MAX);      /* gid_max */
   object_get(obj, "idmax", &an->sw_idmax, U64, 1, buf);
   object_get(obj, "odd", &an->sw_odd, INT, 1, "0");
   object_get(obj, "lengthUnit", &an->sw_length_unit, LITERAL, 1, "Ang");
   if (an->sw_length_unit)      /* (a literal keeps the blanks around it) */
   {
      char *b = an->sw_length_unit, *e = b + strlen(b);
      while (*b == ' ' || *b == '\t' || *b == '\n') b++;
      while (e > b && (e[-1] == ' ' || e[-1] == '\t' || e[-1] == '\n')) e--;
      memmove(an->sw_length_unit, b, (size_t)(e - b)); an->sw_length_unit[e - b] = 0;
   }
   if (!an->sw_length_unit || !an->sw_length_unit[0]) { free(an->sw_length_unit); an->sw_length_unit = strdup("Ang"); }
   if (object_testforkeyword(obj, "species"))
   {
      an->sw_nspecies = object_getv(obj, "species", (void **)&an->sw_species, STRING, IGNORE_IF_NOT_FOUND);
      if (an->sw_nspecies < 0) an->sw_nspecies = 0;
   }
   for (int k = 0; k < 6; k++)
   {
      double *r = (k & 1) ? &an->sw_rmax[k / 2] : &an->sw_rmin[k / 2], *v = (k & 1) ? &an->sw_vmax[k / 2] : &an->sw_vmin[k / 2];
      if (object_testforkeyword(obj, rkey[k])) { object_get(obj, rkey[k], r, WITH_UNITS, 1, "0", "l", NULL); an->sw_given |= 1 << k; }
      if (object_testforkeyword(obj, vkey[k])) { object_get(obj, vkey[k], v, WITH_UNITS, 1, "0", "l/t", NULL); an->sw_given |= 1 << (6 + k); }
   }
   const double cL = units_convert(1.0, NULL, an->sw_length_unit);
   if (an->sw_modulus < 1) snprintf(msg, msglen, "ANALYSIS %s: modulus = %d, it must be at least 1", an->name, an->sw_modulus);
   else if (!isfinite(cL) || cL == 0.0) snprintf(msg, msglen, "ANALYSIS %s: lengthUnit = %s gives no finite conversion factor", an->name, an->sw_length_unit);
}
/* the distinct names of list[n] in order, and every entry's index among them (a repeated name: its first occurrence's) */
static int sw_unique(int n, char *const *list, char **uniq, int *map)
{
   int nu = 0;
   for (int i = 0; i < n; i++)
   {
      int k = 0;
      while (k < nu && strcmp(uniq[k], list[i]) != 0) k++;
      if (k == nu) uniq[nu++] = list[i];
      map[i] = k;
   }
   return nu;
}
static void *sw_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   SWSTATE *p = zalloc(1, sizeof(SWSTATE));
   const int ng = s->ngroup > 0 ? s->ngroup : 1, ns = s->nspecies;
   static char one_group[] = "group";
   char *one[1] = {one_group};
   char *const *gnames = s->ngroup > 0 ? s->group_name : one;
   p->ugname = zalloc(ng, sizeof(char *)); p->usname = zalloc(ns + 1, sizeof(char *));
   int *gmap = zalloc(ng, sizeof(int)), *smap = zalloc(ns + 1, sizeof(int));
   p->nug = sw_unique(ng, gnames, p->ugname, gmap);
   p->nus = sw_unique(ns, s->species_name, p->usname, smap);
   if (s->ngroup <= 0) p->ugname[0] = one_group;
   p->gterm = zalloc(ng, sizeof(uint32_t)); p->sterm = zalloc(ns + 1, sizeof(uint32_t)); p->include = zalloc(ns + 1, sizeof(int));
   for (int g = 0; g < ng; g++) p->gterm[g] = (uint32_t)gmap[g];
   const uint32_t kSType = 0;      /* the one type, ATOM */
   for (int i = 0; i < ns; i++) p->sterm[i] = ((uint32_t)smap[i] + kSType) * (uint32_t)p->nug + kSType * (uint32_t)p->nus;      /* pinfoEncode */
   free(gmap); free(smap);
   for (int i = 0; i < ns; i++)
   {
      p->include[i] = an->sw_nspecies <= 0;
      for (int k = 0; k < an->sw_nspecies; k++) if (strcmp(an->sw_species[k], s->species_name[i]) == 0) p->include[i] = 1;
   }
   ddcmi_subset_filter *f = &p->f;
   f->idmin = an->sw_idmin; f->idmax = an->sw_idmax; f->modulus = an->sw_modulus; f->odd = an->sw_odd;
   for (int a = 0; a < 3; a++) { f->rmin[a] = an->sw_rmin[a]; f->rmax[a] = an->sw_rmax[a]; f->vmin[a] = an->sw_vmin[a]; f->vmax[a] = an->sw_vmax[a]; }
   f->nspecies = ns; f->ngroup = ng; f->include_species = p->include; f->group_term = p->gterm; f->species_term = p->sterm;
   f->nid = an->sw_idlist ? an->sw_nid : 0; f->idlist = an->sw_idlist;
   f->cL = units_convert(1.0, NULL, an->sw_length_unit);
   /* _parms_info, subsetWrite.c:149-166 */
   const double lc = units_convert(1.0, NULL, "Angstrom"), vc = units_convert(1.0, NULL, "Angstrom/fs");
   char string[1024];
   snprintf(string, 1023, "idmin = %" PRIu64 "; idmax = %" PRIu64 "; modulus = %d; odd = %d;\n"
            "xmin = %f Ang; xmax = %f Ang;\n" "ymin = %f Ang; ymax = %f Ang;\n" "zmin = %f Ang; zmax = %f Ang;\n"
            "vxmin = %f Ang/fs; vxmax = %f Ang/fs;\n" "vymin = %f Ang/fs; vymax = %f Ang/fs;\n" "vzmin = %f Ang/fs; vzmax = %f Ang/fs;\n",
            an->sw_idmin, an->sw_idmax, an->sw_modulus, an->sw_odd, an->sw_rmin[0] * lc, an->sw_rmax[0] * lc, an->sw_rmin[1] * lc, an->sw_rmax[1] * lc,
            an->sw_rmin[2] * lc, an->sw_rmax[2] * lc, an->sw_vmin[0] * vc, an->sw_vmax[0] * vc, an->sw_vmin[1] * vc, an->sw_vmax[1] * vc,
            an->sw_vmin[2] * vc, an->sw_vmax[2] * vc);
   p->info = strdup(string);
   return p;
}
static void sw_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state) { (void)simulate; (void)an; (void)state; }
static void sw_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   SWSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const char *where = "subsetWrite_output";
   double h[9];
   if (ddcmi_get_box(ctx, h) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   for (int a = 0; a < 3; a++) p->f.corner[a] = h[4 * a] * -0.5;      /* box->corner = h0 * reducedcorner, reducedcorner = -0.5 on this path */
   int64_t n = 0;
   if (ddcmi_subset_records(ctx, &p->f, 0, NULL, &n) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   int64_t *cnt = zalloc(par.world, sizeof(int64_t));
   cnt[0] = n;
   if (par.world > 1 && ddcmi_rdzv_allgather(par.rdzv, &n, cnt, sizeof(int64_t)) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
   int64_t tot = 0;
   for (int r = 0; r < par.world; r++) tot += cnt[r];
   ddcmi_subset_record *rec = zalloc((size_t)(par.rank == 0 ? tot : n) + 1, sizeof(ddcmi_subset_record));
   int64_t got = 0;
   if (n > 0 && ddcmi_subset_records(ctx, &p->f, n, rec, &got) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   if (n > 0 && got != n) die(where, "the filter selected another number of beads the second time");
   if (par.world > 1 && par.rank != 0)
   {
      const int peer = 0; const void *sb = rec; const size_t sbytes = sizeof(ddcmi_subset_record) * (size_t)n;
      if (ddcmi_rdzv_exchange(par.rdzv, n > 0 ? 1 : 0, &peer, &sb, &sbytes, 0, NULL, NULL, NULL) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
   }
   else if (par.world > 1)
   {
      int *peer = zalloc(par.world, sizeof(int)); void **rb = zalloc(par.world, sizeof(void *)); size_t *rbytes = zalloc(par.world, sizeof(size_t));
      int nr = 0; size_t off = (size_t)n;
      for (int r = 1; r < par.world; r++)
      {
         if (cnt[r] > 0) { peer[nr] = r; rb[nr] = rec + off; rbytes[nr] = sizeof(ddcmi_subset_record) * (size_t)cnt[r]; nr++; }
         off += (size_t)cnt[r];
      }
      if (ddcmi_rdzv_exchange(par.rdzv, 0, NULL, NULL, NULL, nr, peer, rb, rbytes) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
      free(peer); free(rb); free(rbytes);
   }
   if (par.rank == 0)
   {
      char name[700], tmpname[720], dir[512], path[1300], tmppath[1300];
      snprintf(name, sizeof(name), "%s#000000", an->filename);
      snprintf(tmpname, sizeof(tmpname), "%s.tmp", name);
      FILE *f = snapshot_fopen(simulate, tmpname, where);
      time_t now = time(NULL);
      char stamp[64];
      strftime(stamp, sizeof(stamp), "%Y-%m-%d-%H:%M:%S", localtime(&now));
      int key;
      memcpy(&key, "1234", 4);
      const double cLen = units_convert(1.0, NULL, "l");
      const char *u = an->sw_length_unit;
      /* write_fileheader */
      fprintf(f, "subset FILEHEADER {type=MULTILINE; datatype=FIXRECORDBINARY; checksum=NONE; create_time=%s; run_id=0x%08x;\n", stamp, 0u);
      fprintf(f, "code_version=%s; srcpath=libddcmi;\n", ddcmi_version());
      fprintf(f, "loop=%" PRId64 "; time=%f fs;\n", simulate->loop, units_convert(simulate->time, NULL, "t"));
      fprintf(f, "nfiles=1; nrecord=%" PRIu64 "; lrec=%d; nfields=5; endian_key=%d;\n", (uint64_t)tot, (int)sizeof(ddcmi_subset_record), key);
      fprintf(f, "field_names=id pinfo rx ry  rz;\n");
      fprintf(f, "field_types= u8 u4 f4 f4 f4;\n");
      fprintf(f, "field_units=1 1 %s %s %s;\n", u, u, u);
      fprintf(f, "reducedcorner=%21.14f %21.14f %21.14f;\n", -0.5, -0.5, -0.5);
      fprintf(f, "h=%21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f Ang;\n",
              h[0] * cLen, h[1] * cLen, h[2] * cLen, h[3] * cLen, h[4] * cLen, h[5] * cLen, h[6] * cLen, h[7] * cLen, h[8] * cLen);
      fprintf(f, "random = NONE;\n nrandomFieldSize = 0;\n types = ATOM ;\n groups =");
      for (int g = 0; g < p->nug; g++) fprintf(f, " %s", p->ugname[g]);
      fprintf(f, " ;\n species =");
      for (int i = 0; i < p->nus; i++) fprintf(f, " %s", p->usname[i]);
      fprintf(f, " ;\n %s\n", p->info);
      fprintf(f, "}\n \n\n");
      if (tot > 0 && fwrite(rec, sizeof(ddcmi_subset_record), (size_t)tot, f) != (size_t)tot) die(where, "cannot write the records");
      if (fclose(f) != 0) die(where, "cannot write the output file");
      snprintf(dir, sizeof(dir), "snapshot.%012" PRId64, simulate->loop);
      snprintf(path, sizeof(path), "%s/%s", dir, name);
      snprintf(tmppath, sizeof(tmppath), "%s/%s", dir, tmpname);
      if (rename(tmppath, path) != 0) die(where, "cannot rename the output file");
   }
   free(rec); free(cnt);
}
static void sw_free(void *state)
{
   SWSTATE *p = state;
   free(p->include); free(p->gterm); free(p->sterm); free(p->ugname); free(p->usname); free(p->info); free(p);
}

/* ANALYSIS type COARSEGRAIN (coarsegrain.c: parms :80-119, eval :242-448, output :449-583, clear :585-597; matched by its head in any
 * case, analysis.c:162): per (grid cell, species) the sums {number, mass, K, momentum} of the beads, averaged over the evaluations of an
 * output window.  Every evaluation comes from the device (ddcmi_coarsegrain: this rank's non-empty entries in ascending (label, species)
 * order) and is merged into the rank's own table, which stays in that order; nsteps counts them.  At outputrate the ranks' tables are
 * gathered on rank 0 (the transport subsetWrite uses) and merged in rank order, duplicate keys added; rank 0 writes
 * snapshot.<loop>/<filename>#000000 -- the FILEHEADER of class cgrid, then one record per entry in ascending (label, species) (the
 * reference's order is its hash table's) -- under a temporary name and renames it; table and nsteps are cleared.  The startup sample is
 * cleared as well.  One file whatever nfiles says.  A record: u4 CRC-32 of the bytes behind it in native byte order; label and
 * species_index as unsigned integers of the fewest whole bytes that hold nx ny nz - 1 and nspecies - 1, MOST SIGNIFICANT BYTE FIRST
 * (bFieldPack lives in the reference's util submodule, which is not part of the reference tree: the order is fixed here); the f4
 * fields (float)(sum * convert * (1.0 / nsteps)), multiplied left to right in double.  U, virial and the virial tensor are per-atom
 * arrays the Martini path never fills: 0.0f.  Refused at load: nx, ny or nz < 1 (the reference divides by zero), no field_units key
 * (the reference aborts), outputMode outside 1 to 3, more keys than DDCMI_CG_MAX_KEYS (deck.c); outputMode = 3 divides by the species'
 * charge: deck.c leaves such an object unsupported. */
typedef struct { int nsteps; int64_t n, cap; ddcmi_cg_record *tab; char *info; } CGSTATE;
static void cg_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   object_get(obj, "nx", &an->cg_n[0], INT, 1, "0");
   object_get(obj, "ny", &an->cg_n[1], INT, 1, "0");
   object_get(obj, "nz", &an->cg_n[2], INT, 1, "0");
   object_get(obj, "outputMode", &an->cg_output_mode, INT, 1, "2");
   object_get(obj, "nfiles", &an->cg_nfiles, INT, 1, "0");
   object_get(obj, "smearRadius", &an->smear_radius, WITH_UNITS, 1, "0", "l", NULL);
   object_get(obj, "smearMethod", &an->cg_smear_string, STRING, 1, "impulse");
   if (!an->cg_smear_string) an->cg_smear_string = strdup("");
   an->smear_method = strcasecmp(an->cg_smear_string, "hat") == 0;      /* anything else is impulse */
   if (an->cg_n[0] < 1 || an->cg_n[1] < 1 || an->cg_n[2] < 1)
      snprintf(msg, msglen, "ANALYSIS %s: nx = %d, ny = %d, nz = %d: each must be at least 1", an->name, an->cg_n[0], an->cg_n[1], an->cg_n[2]);
   else if (!object_testforkeyword(obj, "field_units")) snprintf(msg, msglen, "ANALYSIS %s: no field_units key", an->name);
   else if (an->cg_output_mode < 1 || an->cg_output_mode > 3) snprintf(msg, msglen, "ANALYSIS %s: outputMode = %d (1, 2 or 3)", an->name, an->cg_output_mode);
   else if (!isfinite(an->smear_radius)) snprintf(msg, msglen, "ANALYSIS %s: smearRadius = %g: not finite", an->name, an->smear_radius);
   else if ((double)an->cg_n[0] * an->cg_n[1] * an->cg_n[2] > (double)DDCMI_CG_MAX_KEYS)
      snprintf(msg, msglen, "ANALYSIS %s: %d x %d x %d cells, the device takes at most %d keys", an->name, an->cg_n[0], an->cg_n[1], an->cg_n[2], DDCMI_CG_MAX_KEYS);
}
static void *cg_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   const ddcmi_setup *s = simulate->setup;
   CGSTATE *p = zalloc(1, sizeof(CGSTATE));
   size_t len = 256 + strlen(an->cg_smear_string);
   for (int j = 0; j < s->nspecies; j++) len += strlen(s->species_name[j]) + 1;
   p->info = zalloc(len, 1);
   snprintf(p->info, len, "nx = %d; ny = %d; nz=%d; smearRadius=%f; smearMethod=%s;\n       ouputrate=%d; eval_rate=%d; species=", an->cg_n[0], an->cg_n[1], an->cg_n[2],
            units_convert(an->smear_radius, NULL, "l"), an->cg_smear_string, an->outputrate, an->eval_rate);      /* (the reference's spelling) */
   for (int j = 0; j < s->nspecies; j++) { strcat(p->info, " "); strcat(p->info, s->species_name[j]); }
   strcat(p->info, ";");
   return p;
}
static void cg_clear(SIMULATE *simulate, const ddcmi_analysis *an, void *state) { (void)simulate; (void)an; CGSTATE *p = state; p->n = 0; p->nsteps = 0; }
static int cg_less(const ddcmi_cg_record *a, const ddcmi_cg_record *b) { return a->label < b->label || (a->label == b->label && a->species < b->species); }
/* tab[n] += add[m], both ascending in (label, species); an entry of both is tab's plus add's, field by field */
static void cg_merge(CGSTATE *p, const ddcmi_cg_record *add, int64_t m)
{
   if (m <= 0) return;
   ddcmi_cg_record *out = zalloc((size_t)(p->n + m), sizeof(ddcmi_cg_record));
   int64_t i = 0, j = 0, k = 0;
   while (i < p->n || j < m)
   {
      if (j >= m || (i < p->n && cg_less(&p->tab[i], &add[j]))) out[k++] = p->tab[i++];
      else if (i >= p->n || cg_less(&add[j], &p->tab[i])) out[k++] = add[j++];
      else
      {
         ddcmi_cg_record r = p->tab[i++];
         const ddcmi_cg_record *o = &add[j++];
         r.n += o->n; r.mass += o->mass;
         for (int a = 0; a < 3; a++) { r.K[a] += o->K[a]; r.p[a] += o->p[a]; }
         out[k++] = r;
      }
   }
   free(p->tab);
   p->tab = out; p->n = k; p->cap = k;
}
static void cg_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   CGSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const char *where = "coarsegrain_eval";
   const int ns = simulate->setup->nspecies;
   int64_t n = 0, got = 0;
   if (ddcmi_coarsegrain(ctx, an->cg_n[0], an->cg_n[1], an->cg_n[2], ns, an->smear_radius, an->smear_method, 0, NULL, &n) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   p->nsteps++;
   if (n <= 0) return;
   ddcmi_cg_record *rec = zalloc((size_t)n, sizeof(ddcmi_cg_record));
   if (ddcmi_coarsegrain(ctx, an->cg_n[0], an->cg_n[1], an->cg_n[2], ns, an->smear_radius, an->smear_method, n, rec, &got) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   if (got != n) die(where, "the grid held another number of entries the second time");
   cg_merge(p, rec, n);
   free(rec);
}
static int cg_field_size(uint64_t max) { int b = 1; while (b < 8 && (max >> (8 * b)) != 0) b++; return b; }      /* bFieldSize */
static void cg_pack_b(unsigned char *dst, int size, uint64_t v) { for (int k = 0; k < size; k++) dst[k] = (unsigned char)(v >> (8 * (size - 1 - k))); }
static void cg_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   CGSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const ddcmi_setup *s = simulate->setup;
   const char *where = "coarsegrain_output";
   /* the ranks' tables on rank 0, one block behind the other in rank order */
   const int64_t n = p->n;
   int64_t *cnt = zalloc(par.world, sizeof(int64_t));
   cnt[0] = n;
   if (par.world > 1 && ddcmi_rdzv_allgather(par.rdzv, &n, cnt, sizeof(int64_t)) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
   if (par.world > 1 && par.rank != 0)
   {
      const int peer = 0; const void *sb = p->tab; const size_t sbytes = sizeof(ddcmi_cg_record) * (size_t)n;
      if (ddcmi_rdzv_exchange(par.rdzv, n > 0 ? 1 : 0, &peer, &sb, &sbytes, 0, NULL, NULL, NULL) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
   }
   else if (par.world > 1)
   {
      int64_t tot = 0;
      for (int r = 1; r < par.world; r++) tot += cnt[r];
      ddcmi_cg_record *rec = zalloc((size_t)tot + 1, sizeof(ddcmi_cg_record));
      int *peer = zalloc(par.world, sizeof(int)); void **rb = zalloc(par.world, sizeof(void *)); size_t *rbytes = zalloc(par.world, sizeof(size_t));
      int nr = 0; size_t off = 0;
      for (int r = 1; r < par.world; r++)
      {
         if (cnt[r] > 0) { peer[nr] = r; rb[nr] = rec + off; rbytes[nr] = sizeof(ddcmi_cg_record) * (size_t)cnt[r]; nr++; }
         off += (size_t)cnt[r];
      }
      if (ddcmi_rdzv_exchange(par.rdzv, 0, NULL, NULL, NULL, nr, peer, rb, rbytes) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
      off = 0;
      for (int r = 1; r < par.world; r++) { cg_merge(p, rec + off, cnt[r]); off += (size_t)cnt[r]; }      /* rank order */
      free(peer); free(rb); free(rbytes); free(rec);
   }
   if (par.rank == 0)
   {
      const int mode = an->cg_output_mode, nf4 = mode == 1 ? 10 : 16, nfields = nf4 + 3;      /* the f4 fields behind checksum, label and species_index */
      const int lb = cg_field_size((uint64_t)an->cg_n[0] * an->cg_n[1] * an->cg_n[2] - 1), sb = cg_field_size((uint64_t)s->nspecies - 1);
      const int lrec = 4 + lb + sb + 4 * nf4;
      char name[700], tmpname[720], dir[512], path[1300], tmppath[1300];
      snprintf(name, sizeof(name), "%s#000000", an->filename);
      snprintf(tmpname, sizeof(tmpname), "%s.tmp", name);
      FILE *f = snapshot_fopen(simulate, tmpname, where);
      time_t now = time(NULL);
      char stamp[64];
      strftime(stamp, sizeof(stamp), "%Y-%m-%d-%H:%M:%S", localtime(&now));
      int key;
      memcpy(&key, "1234", 4);
      double h[9];
      if (ddcmi_get_box(ctx, h) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
      const double cLen = units_convert(1.0, NULL, "l");
      /* write_fileheader */
      fprintf(f, "cgrid FILEHEADER {type=MULTILINE; datatype=FIXRECORDBINARY; checksum=CRC32; create_time=%s; run_id=0x%08x;\n", stamp, 0u);
      fprintf(f, "code_version=%s; srcpath=libddcmi;\n", ddcmi_version());
      fprintf(f, "loop=%" PRId64 "; time=%f fs;\n", simulate->loop, units_convert(simulate->time, NULL, "t"));
      fprintf(f, "nfiles=1; nrecord=%" PRIu64 "; lrec=%d; nfields=%d; endian_key=%d;\n", (uint64_t)p->n, lrec, nfields, key);
      if (mode == 1)
      {
         fprintf(f, "field_names=checksum label species_index number_particles mass  Kx Ky Kz U virial px py pz;\n");
         fprintf(f, "field_types=u4 b%1u b%1u f4 f4 f4 f4 f4 f4 f4 f4 f4 f4;\n", (unsigned)lb, (unsigned)sb);
         fprintf(f, "field_units=1 1 1 1 amu eV eV eV eV eV amu*Angstrom/fs amu*Angstrom/fs amu*Angstrom/fs;\n");
      }
      else
      {
         fprintf(f, "field_names=checksum label species_index number_particles mass  Kx Ky Kz U virial px py pz vir_xx vir_yy vir_zz vir_xy vir_xz vir_yz;\n");
         fprintf(f, "field_types=u4 b%1u b%1u f4 f4 f4 f4 f4 f4 f4 f4 f4 f4 f4 f4 f4 f4 f4 f4;\n", (unsigned)lb, (unsigned)sb);
         fprintf(f, "field_units=1 1 1 1 amu eV eV eV eV eV amu*Angstrom/fs amu*Angstrom/fs amu*Angstrom/fs eV eV eV eV eV eV;\n");
      }
      fprintf(f, "reducedcorner=%21.14f %21.14f %21.14f;\n", -0.5, -0.5, -0.5);
      fprintf(f, "h=%21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f Ang;\n",
              h[0] * cLen, h[1] * cLen, h[2] * cLen, h[3] * cLen, h[4] * cLen, h[5] * cLen, h[6] * cLen, h[7] * cLen, h[8] * cLen);
      fprintf(f, "%s\n  nSamples = %d;\n", p->info, p->nsteps);
      fprintf(f, "}\n \n\n");
      const double mass_convert = units_convert(1.0, NULL, "amu"), energy_convert = units_convert(1.0, NULL, "eV");
      const double momentum_convert = units_convert(1.0, NULL, "amu*Angstrom/fs");
      const double nstepsInv = 1.0 / (p->nsteps * 1.0);
      unsigned char *line = zalloc((size_t)lrec, 1);
      for (int64_t k = 0; k < p->n; k++)
      {
         const ddcmi_cg_record *e = &p->tab[k];
         float v[16];
         int q = 0;
         memset(v, 0, sizeof(v));
         v[q++] = (float)(e->n * nstepsInv);
         v[q++] = (float)(e->mass * mass_convert * nstepsInv);
         for (int a = 0; a < 3; a++) v[q++] = (float)(e->K[a] * energy_convert * nstepsInv);
         q += 2;      /* U, virial */
         for (int a = 0; a < 3; a++) v[q++] = (float)(e->p[a] * momentum_convert * nstepsInv);
         cg_pack_b(line + 4, lb, (uint64_t)e->label);
         cg_pack_b(line + 4 + lb, sb, (uint64_t)e->species);
         memcpy(line + 4 + lb + sb, v, 4 * (size_t)nf4);
         const uint32_t crc = ddcmi_crc32(line + 4, (size_t)lrec - 4);
         memcpy(line, &crc, 4);
         if (fwrite(line, (size_t)lrec, 1, f) != 1) die(where, "cannot write the records");
      }
      free(line);
      if (fclose(f) != 0) die(where, "cannot write the output file");
      snprintf(dir, sizeof(dir), "snapshot.%012" PRId64, simulate->loop);
      snprintf(path, sizeof(path), "%s/%s", dir, name);
      snprintf(tmppath, sizeof(tmppath), "%s/%s", dir, tmpname);
      if (rename(tmppath, path) != 0) die(where, "cannot rename the output file");
   }
   free(cnt);
   cg_clear(simulate, an, p);
}
static void cg_free(void *state) { CGSTATE *p = state; free(p->tab); free(p->info); free(p); }

/* ANALYSIS type cholAnalysis (cholAnalysis.c: parms :41-71, eval :109-163, output :73-108): for every CHOL molecule how far the bead
 * next to each ring triangle stands out of that triangle's plane, dR1 and dR5, in two histograms with their sum and extremes.  Every
 * evaluation comes from the device (ddcmi_chol_offsets over the list the loader made, an->chol_gid); the ranks' counts and sums are
 * added in rank order, the extremes combined by a maximum over the ranks, the fragments of the molecules split over ranks gathered on
 * rank 0 in rank order (the transport subsetWrite uses) and those molecules completed there with the device lane's arithmetic
 * (ddcmi_chol_complete).  Rank 0 accumulates; at the output it appends one line to dataFilename in the run directory (opened for
 * append at init; the time stays in internal units, as in the reference) and writes snapshot.<loop>/<filename> under a temporary
 * name, renamed when complete; then everything is cleared.  The startup evaluation is cleared as well.  The reference's printf of
 * cnt1 and cnt3 to stdout is not restated: stdout belongs to rank 0's data lines.  A deck without a CHOL molecule is legal: 0/0 is
 * printed as C prints it. */
typedef struct { FILE *file; int nbins; double delta; int64_t *cnt, *acc; double stats[6], sum[2], min[2], max[2], *buf; ddcmi_chol_fragment *frag; int64_t fragcap; } CHSTATE;
static void ch_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   object_get(obj, "potentialName", &an->chol_potential, STRING, 1, "martini");
   object_get(obj, "dataFilename", &an->chol_data_filename, STRING, 1, "cholAnalysis.data");
   object_get(obj, "delta", &an->chol_delta, WITH_UNITS, 1, "0.1", "l", NULL);
   object_get(obj, "rmin", &an->chol_rmin, WITH_UNITS, 1, "0", "l", NULL);
   object_get(obj, "rmax", &an->chol_rmax, WITH_UNITS, 1, "0", "l", NULL);
   if (!an->chol_potential) an->chol_potential = strdup("");
   if (!an->chol_data_filename) an->chol_data_filename = strdup("");
   const OBJECT *pot = object_find(an->chol_potential, "POTENTIAL");      /* the reference's two asserts */
   char *ptype = NULL;
   if (pot) object_get(pot, "type", &ptype, STRING, 1, "");
   if (!pot) snprintf(msg, msglen, "ANALYSIS %s: potentialName = %s, and there is no POTENTIAL object of that name", an->name, an->chol_potential);
   else if (!ptype || strcmp(ptype, "MARTINI") != 0)
      snprintf(msg, msglen, "ANALYSIS %s: potentialName = %s is a POTENTIAL of type %s, not MARTINI", an->name, an->chol_potential, ptype ? ptype : "");
   free(ptype);
   const double q = (an->chol_rmax - an->chol_rmin) / an->chol_delta;
   an->chol_nbins = isfinite(q) && fabs(q) < 2e9 ? (int)lrint(q) : 0;
   if (an->chol_nbins < 1)
   {
      snprintf(msg, msglen, "ANALYSIS %s: rmin = %g, rmax = %g, delta = %g give %d bins (at least one is needed)", an->name, an->chol_rmin, an->chol_rmax, an->chol_delta,
               an->chol_nbins);
      return;
   }
   an->chol_delta = (an->chol_rmax - an->chol_rmin) / an->chol_nbins;
   if (an->chol_nbins > DDCMI_CHOL_MAX_NBINS)
      snprintf(msg, msglen, "ANALYSIS %s: %d bins need %ld bytes of the device's LDS, at most %d (8 per bin: %d bins)", an->name, an->chol_nbins,
               DDCMI_CHOL_LDS_BYTES((long)an->chol_nbins), DDCMI_CHOL_MAX_LDS, DDCMI_CHOL_MAX_NBINS);
   else if (!an->chol_data_filename[0] || !an->filename || !an->filename[0]) snprintf(msg, msglen, "ANALYSIS %s: an empty file name", an->name);
}
static void ch_clear(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)simulate; (void)an;
   CHSTATE *p = state;
   memset(p->acc, 0, sizeof(int64_t) * 2 * (size_t)p->nbins);
   for (int q = 0; q < 2; q++) { p->sum[q] = 0.0; p->min[q] = 1e300; p->max[q] = -1e300; }
}
static void *ch_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   CHSTATE *p = zalloc(1, sizeof(CHSTATE));
   p->nbins = an->chol_nbins; p->delta = an->chol_delta;
   p->cnt = zalloc(2 * (size_t)p->nbins + 1, sizeof(int64_t)); p->acc = zalloc(2 * (size_t)p->nbins + 1, sizeof(int64_t));
   p->buf = zalloc(2 * (size_t)p->nbins + 8, sizeof(double));
   p->fragcap = 64; p->frag = zalloc((size_t)p->fragcap, sizeof(ddcmi_chol_fragment));
   ch_clear(simulate, an, p);
   if (par.rank == 0)
   {
      p->file = fopen(an->chol_data_filename, "a");
      if (!p->file) die("cholAnalysis_parms", "cannot open the data file");
   }
   return p;
}
static void ch_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   CHSTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   const char *where = "cholAnalysis_eval";
   const int nb2 = 2 * p->nbins, nmol = an->chol_nmol;
   int64_t ndone = 0, nfrag = 0;
   memset(p->cnt, 0, sizeof(int64_t) * (size_t)nb2);
   for (int q = 0; q < 2; q++) { p->stats[3 * q] = 0.0; p->stats[3 * q + 1] = 1e300; p->stats[3 * q + 2] = -1e300; }
   if (ddcmi_chol_offsets(ctx, nmol, an->chol_gid, an->chol_rmin, p->delta, p->nbins, p->cnt, &ndone, p->stats, 0, NULL, &nfrag) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   if (nfrag > p->fragcap)
   {
      free(p->frag);
      p->fragcap = nfrag + nfrag / 4; p->frag = zalloc((size_t)p->fragcap, sizeof(ddcmi_chol_fragment));
   }
   /* (the fragments stay packed on the device: a copy, not a second pass) */
   if (nfrag > 0 && ddcmi_chol_fragments(ctx, p->fragcap, p->frag, &nfrag) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   /* counts, ndone and the two sums added in rank order (the integers stay below 2^53: exact); {-min, max} by a maximum */
   double *mm = p->buf + nb2 + 3;
   for (int k = 0; k < nb2; k++) p->buf[k] = (double)p->cnt[k];
   p->buf[nb2] = (double)ndone; p->buf[nb2 + 1] = p->stats[0]; p->buf[nb2 + 2] = p->stats[3];
   mm[0] = -p->stats[1]; mm[1] = p->stats[2]; mm[2] = -p->stats[4]; mm[3] = p->stats[5];
   sum_over_ranks(p->buf, nb2 + 3, where);
   if (par.world > 1 && ddcmi_rdzv_allreduce_f64(par.rdzv, mm, 4, 1) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
   /* the ranks' fragments on rank 0, one block behind the other in rank order */
   ddcmi_chol_fragment *all = p->frag;
   int64_t nall = nfrag;
   if (par.world > 1)
   {
      int64_t *cnt = zalloc(par.world, sizeof(int64_t));
      if (ddcmi_rdzv_allgather(par.rdzv, &nfrag, cnt, sizeof(int64_t)) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
      if (par.rank != 0)
      {
         const int peer = 0; const void *sb = p->frag; const size_t sbytes = sizeof(ddcmi_chol_fragment) * (size_t)nfrag;
         if (ddcmi_rdzv_exchange(par.rdzv, nfrag > 0 ? 1 : 0, &peer, &sb, &sbytes, 0, NULL, NULL, NULL) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
      }
      else
      {
         nall = 0;
         for (int r = 0; r < par.world; r++) nall += cnt[r];
         all = zalloc((size_t)nall + 1, sizeof(ddcmi_chol_fragment));
         memcpy(all, p->frag, sizeof(ddcmi_chol_fragment) * (size_t)nfrag);
         int *peer = zalloc(par.world, sizeof(int)); void **rb = zalloc(par.world, sizeof(void *)); size_t *rbytes = zalloc(par.world, sizeof(size_t));
         int nr = 0; size_t off = (size_t)nfrag;
         for (int r = 1; r < par.world; r++)
         {
            if (cnt[r] > 0) { peer[nr] = r; rb[nr] = all + off; rbytes[nr] = sizeof(ddcmi_chol_fragment) * (size_t)cnt[r]; nr++; }
            off += (size_t)cnt[r];
         }
         if (ddcmi_rdzv_exchange(par.rdzv, 0, NULL, NULL, NULL, nr, peer, rb, rbytes) != DDCMI_OK) die(where, ddcmi_rdzv_last_error(par.rdzv));
         free(peer); free(rb); free(rbytes);
      }
      free(cnt);
   }
   if (par.rank == 0)
   {
      for (int k = 0; k < nb2; k++) p->cnt[k] = (int64_t)p->buf[k];
      ndone = (int64_t)p->buf[nb2];
      double st[6] = {p->buf[nb2 + 1], -mm[0], mm[1], p->buf[nb2 + 2], -mm[2], mm[3]};
      double h[9];
      char err[512] = "";
      if (ddcmi_get_box(ctx, h) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
      const double L[3] = {h[0], h[4], h[8]};
      if (ddcmi_chol_complete(nall, all, nmol, an->chol_gid, L, simulate->setup->pbc, an->chol_rmin, p->delta, p->nbins, p->cnt, &ndone, st, err, sizeof(err)) != 0)
         die(where, err);
      if (ndone != nmol)
      {
         snprintf(err, sizeof(err), "%" PRId64 " of the %d CHOL molecules were found: a listed bead is owned by no rank", ndone, nmol);
         die(where, err);
      }
      for (int k = 0; k < nb2; k++) p->acc[k] += p->cnt[k];
      for (int q = 0; q < 2; q++)
      {
         p->sum[q] += st[3 * q];
         if (st[3 * q + 1] < p->min[q]) p->min[q] = st[3 * q + 1];
         if (st[3 * q + 2] > p->max[q]) p->max[q] = st[3 * q + 2];
      }
   }
   if (all != p->frag) free(all);
}
static void ch_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   CHSTATE *p = state;
   const char *where = "cholAnalysis_output";
   if (par.rank == 0)
   {
      const double lc = units_convert(1.0, NULL, "Angstrom");
      int64_t cnt1 = 0, cnt3 = 0;
      for (int i = 0; i < p->nbins; i++) { cnt1 += p->acc[i]; cnt3 += p->acc[i + p->nbins]; }
      const double ave1 = p->sum[0] / (double)cnt1, ave5 = p->sum[1] / (double)cnt1;      /* both by cnt1, as the reference does */
      fprintf(p->file, "%" PRId64 " %f %f %f %f %f %f %f\n", simulate->loop, simulate->time, p->min[0] * lc, p->max[0] * lc, ave1 * lc, p->min[1] * lc, p->max[1] * lc,
              ave5 * lc);
      fflush(p->file);
      char tmpname[700], dir[512], path[1300], tmppath[1300];
      snprintf(tmpname, sizeof(tmpname), "%s.tmp", an->filename);
      FILE *f = snapshot_fopen(simulate, tmpname, where);
      for (int i = 0; i < p->nbins; i++)
      {
         const double r = (an->chol_rmin + (i + 0.5) * p->delta);
         fprintf(f, " %e %e %e\n", r * lc, (double)p->acc[i] / lc * (1.0 / ((double)cnt1 * p->delta)), (double)p->acc[i + p->nbins] / lc * (1.0 / ((double)cnt3 * p->delta)));
      }
      if (fclose(f) != 0) die(where, "cannot write the output file");
      snprintf(dir, sizeof(dir), "snapshot.%012" PRId64, simulate->loop);
      snprintf(path, sizeof(path), "%s/%s", dir, an->filename);
      snprintf(tmppath, sizeof(tmppath), "%s/%s", dir, tmpname);
      if (rename(tmppath, path) != 0) die(where, "cannot rename the output file");
   }
   ch_clear(simulate, an, p);
}
static void ch_free(void *state)
{
   CHSTATE *p = state;
   if (p->file) fclose(p->file);
   free(p->cnt); free(p->acc); free(p->buf); free(p->frag); free(p);
}

/* ANALYSIS type FORCE_AVERAGE (forceAverage.c: parms :28-73, eval :76-145, output :148-190, clear :193-205): the time average of the
 * force, the velocity or the position of the beads idParticle lists, one line per window appended to `filename` in the run directory
 * (opened for append, with the header line, at init).  The running sums live on the device (ddcmi_track_set / _accumulate / _read):
 * an evaluation is one launch and counts the sample, and the host does not wait.  At the output, under the reference's gate
 * nSnapSum * eval_rate >= outputrate, every rank reads its partial sums; they are added over the ranks in rank order, every gid's
 * hits over the ranks must equal nSnapSum, rank 0 writes the line in internal units (the reference's conversions are commented out)
 * and everything is cleared.  The startup evaluation is cleared as well.
 * A context tracks one list.  Several FORCE_AVERAGE objects take turns: the object whose list is on the device is fa_owner, and an
 * object that evaluates while another one owns the device first moves the owner's sums to the owner's host accumulators (one read
 * with reset) and sets its own list.  A deck with one such object never reads between two outputs.  The host adds whole device
 * sums; with objects that alternate at every evaluation each device sum is one sample, so the bits are those of one running sum. */
typedef struct { FILE *file; int n, nsnap; double *sum, *buf; int64_t *hits, *part; } FASTATE;
static FASTATE *fa_owner = NULL;
static void fa_parms(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen)
{
   char *dt = NULL;
   object_get(obj, "eval_rate", &an->eval_rate, INT, 1, "1");       /* forceAverage_parms' defaults, not analysis_init's 0 */
   object_get(obj, "outputrate", &an->outputrate, INT, 1, "1");
   object_get(obj, "data_type", &dt, STRING, 1, "force");
   an->fa_nid = object_getv(obj, "idParticle", (void **)&an->fa_gid, U64, IGNORE_IF_NOT_FOUND);
   const char *data_type = dt ? dt : "";
   if (strcasecmp(data_type, "force") == 0) an->fa_what = 0;
   else if (strcasecmp(data_type, "velocity") == 0) an->fa_what = 1;
   else if (strcasecmp(data_type, "position") == 0) an->fa_what = 2;
   else snprintf(msg, msglen, "ANALYSIS %s: data_type = %s is none of force, velocity, position", an->name, data_type);      /* the reference's exit(19) */
   if (!an->fa_gid || an->fa_nid < 0)
   {
      an->fa_nid = 0;
      snprintf(msg, msglen, "ANALYSIS %s: no idParticle key (the gids of the beads to follow)", an->name);      /* ABORT_IF_NOT_FOUND */
   }
   else if (an->fa_nid > DDCMI_TRACK_MAX_IDS) snprintf(msg, msglen, "ANALYSIS %s: idParticle lists %d gids, the device tracks at most %d", an->name, an->fa_nid, DDCMI_TRACK_MAX_IDS);
   else if (an->eval_rate < 1) snprintf(msg, msglen, "ANALYSIS %s: eval_rate = %d, it must be at least 1", an->name, an->eval_rate);
   else if (!an->filename || !an->filename[0]) snprintf(msg, msglen, "ANALYSIS %s: an empty file name", an->name);
   free(dt);
}
/* the device's sums into the owner's host accumulators, and the device's cleared */
static void fa_spill(SIMULATE *simulate, const char *where)
{
   FASTATE *p = fa_owner;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   if (!p) return;
   if (ddcmi_track_read(ctx, p->n, p->buf, p->part, 1) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   for (int k = 0; k < 3 * p->n; k++) p->sum[k] += p->buf[k];
   for (int k = 0; k < p->n; k++) p->hits[k] += p->part[k];
}
static void fa_acquire(SIMULATE *simulate, const ddcmi_analysis *an, FASTATE *p, const char *where)
{
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   if (fa_owner == p) return;
   fa_spill(simulate, where);
   fa_owner = NULL;
   if (ddcmi_track_set(ctx, an->fa_nid, an->fa_gid) != DDCMI_OK) die(where, ddcmi_last_error(ctx));
   fa_owner = p;
}
static void fa_clear(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   (void)an;
   FASTATE *p = state;
   if (fa_owner == p) fa_spill(simulate, "forceAverage_clear");
   memset(p->sum, 0, sizeof(double) * 3 * (size_t)p->n);
   memset(p->hits, 0, sizeof(int64_t) * (size_t)p->n);
   p->nsnap = 0;
}
static void *fa_init(SIMULATE *simulate, const ddcmi_analysis *an)
{
   FASTATE *p = zalloc(1, sizeof(FASTATE));
   p->n = an->fa_nid;
   p->sum = zalloc(3 * (size_t)p->n + 1, sizeof(double)); p->buf = zalloc(4 * (size_t)p->n + 1, sizeof(double));
   p->hits = zalloc((size_t)p->n + 1, sizeof(int64_t)); p->part = zalloc((size_t)p->n + 1, sizeof(int64_t));
   if (par.rank == 0)
   {
      p->file = fopen(an->filename, "a");
      if (!p->file) die("forceAverage_parms", "cannot open the output file");
      fprintf(p->file, "# loop  time  ");
      for (int i = 0; i < p->n; i++) fprintf(p->file, "%llu  ", (unsigned long long)an->fa_gid[i]);
      fprintf(p->file, "\n");
      fflush(p->file);
   }
   fa_acquire(simulate, an, p, "forceAverage_parms");
   return p;
}
static void fa_eval(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   FASTATE *p = state;
   ddcmi_ctx *ctx = simulate->accelerator->parms;
   fa_acquire(simulate, an, p, "forceAverage_eval");
   if (ddcmi_track_accumulate(ctx, an->fa_what) != DDCMI_OK) die("forceAverage_eval", ddcmi_last_error(ctx));
   p->nsnap++;
}
static void fa_output(SIMULATE *simulate, const ddcmi_analysis *an, void *state)
{
   FASTATE *p = state;
   const char *where = "forceAverage_output";
   if ((int64_t)p->nsnap * an->eval_rate < (int64_t)an->outputrate) return;
   if (fa_owner == p) fa_spill(simulate, where);
   const int n = p->n;
   for (int k = 0; k < 3 * n; k++) p->buf[k] = p->sum[k];
   for (int k = 0; k < n; k++) p->buf[3 * n + k] = (double)p->hits[k];      /* (below 2^53: exact) */
   sum_over_ranks(p->buf, 4 * n, where);
   for (int k = 0; k < n; k++)
      if (p->buf[3 * n + k] != (double)p->nsnap)
      {
         char err[256];
         snprintf(err, sizeof(err), "gid %llu was found %.0f times in %d evaluations: a tracked bead is owned by no rank, or by several", (unsigned long long)an->fa_gid[k],
                  p->buf[3 * n + k], p->nsnap);
         die(where, err);
      }
   if (par.rank == 0)
   {
      fprintf(p->file, "%12.12" PRIu64, (uint64_t)simulate->loop);      /* loopFormat() */
      fprintf(p->file, " %10.6f ", simulate->time);
      for (int k = 0; k < n; k++)
         fprintf(p->file, " %12.7f %12.7f %12.7f ", p->buf[3 * k] / (double)p->nsnap, p->buf[3 * k + 1] / (double)p->nsnap, p->buf[3 * k + 2] / (double)p->nsnap);
      fprintf(p->file, "\n");
      fflush(p->file);
   }
   fa_clear(simulate, an, p);
}
static void fa_free(void *state)
{
   FASTATE *p = state;
   if (fa_owner == p) fa_owner = NULL;      /* (the context's list goes with the context) */
   if (p->file) fclose(p->file);
   free(p->sum); free(p->buf); free(p->hits); free(p->part); free(p);
}

/* ------------------------------------------------------------------------- */
static const char *const dsf_heads[] = {"DynamicStructureFactor", "Dynamic_Structure_Factor", NULL};
static const ANALYSIS_TYPE types[] = {      /* indexed by enum ddcmi_analysis_kind; DDCMI_AN_NONE has no row */
   [DDCMI_AN_PAIRCORRELATION] = {"PAIRCORRELATION", DDCMI_AN_PAIRCORRELATION, "paircorrelation.dat", pc_parms, pc_init, pc_eval, pc_output, pc_clear, pc_free},
   [DDCMI_AN_VAF] = {"VELOCITYAUTOCORRELATION", DDCMI_AN_VAF, "vaf.dat", vaf_parms, vaf_init, vaf_eval, vaf_output, NULL, vaf_free},
   [DDCMI_AN_VCMWRITE] = {"vcmWrite", DDCMI_AN_VCMWRITE, "vcm.data", vcm_parms, vcm_init, vcm_eval, vcm_output, NULL, vcm_free, 1, "vcm_write"},
   [DDCMI_AN_ZDENSITY] = {"zdensity", DDCMI_AN_ZDENSITY, "zden.dat", zd_parms, zd_init, zd_eval, zd_output, NULL, zd_free, 1, NULL},
   [DDCMI_AN_KDIST] = {"KINETICENERGYDISTN", DDCMI_AN_KDIST, "kinetic.data", kd_parms, kd_init, kd_eval, kd_output, kd_clear, kd_free},
   [DDCMI_AN_DSF] = {"DSF", DDCMI_AN_DSF, "rho_k.data", dsf_parms, dsf_init, dsf_eval, dsf_output, NULL, dsf_free, 0, NULL, dsf_heads},
   [DDCMI_AN_SUBSETWRITE] = {"subsetWrite", DDCMI_AN_SUBSETWRITE, "subset", sw_parms, sw_init, sw_eval, sw_output, NULL, sw_free, 1, "subset_write"},
   [DDCMI_AN_COARSEGRAIN] = {"COARSEGRAIN", DDCMI_AN_COARSEGRAIN, "cgrid", cg_parms, cg_init, cg_eval, cg_output, cg_clear, cg_free},
   [DDCMI_AN_CHOL] = {"cholAnalysis", DDCMI_AN_CHOL, "cholAnalysis.distn", ch_parms, ch_init, ch_eval, ch_output, ch_clear, ch_free, 1, NULL},
   [DDCMI_AN_FORCEAVERAGE] = {"FORCE_AVERAGE", DDCMI_AN_FORCEAVERAGE, "force.dat", fa_parms, fa_init, fa_eval, fa_output, fa_clear, fa_free},
};
const ANALYSIS_TYPE *analysis_type_find(const char *type_name)
{
   for (size_t t = 1; t < sizeof(types) / sizeof(types[0]); t++)
   {
      const ANALYSIS_TYPE *row = &types[t];
      if (!row->full_name)
      {
         if (strncasecmp(type_name, row->prefix, strlen(row->prefix)) == 0) return row;
         for (const char *const *h = row->heads; h && *h; h++) if (strncasecmp(type_name, *h, strlen(*h)) == 0) return row;
      }
      else if (strcasecmp(type_name, row->prefix) == 0 || (row->alias && strcasecmp(type_name, row->alias) == 0)) return row;
   }
   return NULL;
}

/* the supported analyses of the running deck, in list order */
typedef struct { const ddcmi_analysis *an; const ANALYSIS_TYPE *row; void *state; } ANALYSIS;
static ANALYSIS *analyses = NULL;
static int nanalyses = 0;
void analysis_init_all(SIMULATE *simulate)
{
   const ddcmi_setup *s = simulate->setup;
   nanalyses = 0;
   analyses = zalloc(s->nanalysis + 1, sizeof(ANALYSIS));
   for (int a = 0; a < s->nanalysis; a++)
   {
      const ddcmi_analysis *an = &s->analysis[a];
      if (an->type != DDCMI_AN_NONE) analyses[nanalyses++] = (ANALYSIS){an, &types[an->type], types[an->type].init(simulate, an)};
      else if (par.rank == 0) fprintf(stderr, "ddcmi_md: ANALYSIS %s of type %s is not supported and is ignored\n", an->name, an->type_name ? an->type_name : "?");
   }
}
void analysis_startup_all(SIMULATE *simulate)
{
   for (ANALYSIS *A = analyses; A < analyses + nanalyses; A++)
   {
      if (analysis_due(A->an->eval_rate, simulate->loop)) A->row->eval(simulate, A->an, A->state);
      if (A->row->clear) A->row->clear(simulate, A->an, A->state);      /* PAIRCORRELATION discards that sample */
   }
}
int64_t analysis_next_stop(const SIMULATE *simulate, int64_t endLoop)
{
   for (const ANALYSIS *A = analyses; A < analyses + nanalyses; A++)
   {
      const int r[2] = {A->an->eval_rate, A->an->outputrate};
      for (int q = 0; q < 2; q++)
         if (r[q] > 0) { int64_t nx = (simulate->loop / r[q] + 1) * r[q]; if (nx < endLoop) endLoop = nx; }
   }
   return endLoop;
}
void analysis_do_all(SIMULATE *simulate)
{
   for (ANALYSIS *A = analyses; A < analyses + nanalyses; A++)
   {
      if (analysis_due(A->an->eval_rate, simulate->loop)) A->row->eval(simulate, A->an, A->state);
      if (analysis_due(A->an->outputrate, simulate->loop)) A->row->output(simulate, A->an, A->state);
   }
}
void analysis_free_all(void)
{
   for (ANALYSIS *A = analyses; A < analyses + nanalyses; A++) A->row->free(A->state);
   free(analyses); analyses = NULL; nanalyses = 0;
}

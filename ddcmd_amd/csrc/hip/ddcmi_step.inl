/* ddcmi_step.inl -- host side of a force evaluation and of an NGLF step: launch_forces, step_pre / step_post, ddcmi_step_nglf.
 * Part of the ONE translation unit ddcmi.hip (kernels, templates and the static helpers they share), included there in this order. */
/* ------------------------------------------------------------------------- */
/* defer_reduce: the caller (a time step) folds the nonbonded reduction and the final
 * energies into the launch that reduces the kinetic terms */
/* LDS of one k_nonbond workgroup.  Fixed layout (neighbourhoods of up to NB_ZOFF/16 beads: every Martini system): {x,y} [capl] at
 * address 0, z [capl] at NB_ZOFF -- and whatever else fits goes into the GAP between them, which used to be wasted (4 KB beside a
 * water neighbourhood, 9 KB beside the bilayer's): the fused step's rows of kinetic sums at its top, the pair table at its bottom.
 * The pair table is the direct one (32 bytes per class pair) or, where that would cost the second workgroup per CU (or fit no CU at
 * all), the two-level one (one byte per class pair + the distinct entries).  Types and shifted-copy flags that the list entries do
 * not carry ride in the staged z (k_nonbond): no per-bead byte arrays. */
static NbLds nb_lds_layout(const ddcmi_ctx *ctx, bool fused)
{
   const size_t capl = (size_t)ctx->stage_cap + 2;
   const size_t rows = ((NB_THREADS / 64) * 8 + 2) * sizeof(double);      /* the waves' rows of kinetic sums + (lean step) the displacement bound handed from wave 0 to the others */
   const size_t npair = (size_t)ctx->nnb * ctx->nnb;
   const size_t direct = npair * sizeof(double4), level = (size_t)ctx->nlvl * sizeof(double4) + ((npair + 15) & ~(size_t)15);
   auto lay = [&](size_t table, bool lvl)
   {
      NbLds l;
      l.lvl = lvl; l.zfix = capl * 16 <= NB_ZOFF;
      /* (while it stages, the kernel keeps its cell tables and slot -> cell map where the positions will lie -- 2 (NRC + 8) + 16 ints and
       * 2 bytes per staged bead from address 0: the table, loaded before the staging, must start behind them) */
      const size_t scratch = ((2 * (NRC + 8) + 16) * sizeof(int) + ((NRC + 15) & ~15) + 2 * capl + 15) & ~(size_t)15;      /* cell tables, image cells' shift codes, the slot -> cell map */
      size_t gap_lo = std::max(capl * 16, scratch), gap_hi = l.zfix ? NB_ZOFF : 0, end = l.zfix ? NB_ZOFF + capl * 8 : capl * 24;
      l.ke_off = 0;
      if (fused)
      {
         if (l.zfix && gap_lo + rows <= gap_hi) { gap_hi -= rows; l.ke_off = (int)gap_hi; }
         else { end = (end + 7) & ~(size_t)7; l.ke_off = (int)end; end += rows; }
      }
      if (l.zfix && gap_lo + table <= gap_hi) l.tab_off = (int)gap_lo;
      else { end = (end + 15) & ~(size_t)15; l.tab_off = (int)end; end += table; }
      l.total = end;
      l.wgs = end > 160 * 1024 ? 0 : (int)std::min<size_t>(2, (160 * 1024) / end);
      return l;
   };
   const NbLds d = lay(direct, false);
   if (ctx->nlvl <= 0) return d;
   const NbLds v = lay(level, true);
   return (ctx->force_lvl || v.wgs > d.wgs) ? v : d;
}
/* ---- which path a force evaluation takes: the shared conditions, then ONE plan (plan_forces) ---- */
static bool mg_pack_ready(const ddcmi_ctx *ctx);
static bool ddcmi_mg_pack_job(const ddcmi_ctx *ctx, PackJob *pk);
/* every group is FREE or BERENDSEN: the integrator's pass is one kick + drift (Berendsen: host scalars from the temperature last published) */
static bool groups_plain(const ddcmi_ctx *ctx)
{
   for (int g = 0; g < ctx->ngroup; g++) if (ctx->gtype[g] != DDCMI_FREE && ctx->gtype[g] != DDCMI_BERENDSEN) return false;
   return true;
}
/* the step is the pair kernel only (+ the bonded kernels in front of it, which take a received partner out of the receive buffer too:
 * k_bonded_gather's bead()): restraints, constraint groups and the barostat want every halo bead in pos[]; bit 128 of
 * excludePotentialTerm takes the pair kernel away; updateRate == 0 puts a host round trip between the steps */
static bool pair_kernel_only(const ddcmi_ctx *ctx) { return ctx->nrest == 0 && ctx->ncgroup == 0 && !(ctx->baro_beta > 0.0) && (ctx->excludePotentialTerm & 128) == 0 && ctx->updateRate > 0; }
/* Three questions rest on these two and differ on purpose:
 *   fuse_ok       groups_plain, no constraint groups, no barostat, the pair kernel on -- but restraints and updateRate == 0 are welcome;
 *   lean_capable  groups_plain AND pair_kernel_only (so: no restraints), owned beads, not a domain of an in-process group;
 *   direct_halo   pair_kernel_only, whatever the groups (a LANGEVIN rank stages directly in front of the split kernels) -- and a transport,
 *                 and a halo of received beads only (nself_images == 0). */
/* may the integrator's pass ride in the pair kernel (k_nonbond<..., FUSE>)?  The force must be complete when the list walk ends and the
 * step must need nothing between the force and the drift (bonded terms, restraints and charges are no obstacle: their kernels run in
 * front of the pair kernel, the excluded-pair loop ends before the epilogue).  DDCMI_NO_FUSED_STEP=1: never */
static bool fuse_ok(const ddcmi_ctx *ctx)
{
   static const bool off = getenv("DDCMI_NO_FUSED_STEP") != nullptr;
   return !off && ctx->nloc > 0 && !ctx->group_ && (ctx->excludePotentialTerm & 128) == 0 && ctx->ncgroup == 0 && !(ctx->baro_beta > 0.0) && groups_plain(ctx);
}
/* may this context run lean steps (ddcmi_ctx::lean_pending)?  Its step is the fused pair kernel and nothing else.  DDCMI_NO_LEAN_STEP=1: never */
static bool lean_capable(const ddcmi_ctx *ctx) { return !ctx->no_lean && !ctx->group_ && ctx->nloc > 0 && pair_kernel_only(ctx) && groups_plain(ctx); }
/* a single domain's periodic images are staged by the pair kernel from their owners (NbTileArgs::self_img): nothing reads the image records
 * between two rebuilds, and nothing refreshes them -- where the step can be lean; elsewhere the reduction launch of every step refreshes
 * them on the side and the staging keeps its shorter path (the bilayer: 4 us per pair kernel).  DDCMI_NO_SELF_IMAGES=1: never. */
static bool self_images(const ddcmi_ctx *ctx) { return !ctx->no_self_img && !has_peers(ctx) && lean_capable(ctx) && ctx->nhalo > 0 && ctx->stage_cap + 2 < 4096; }
/* direct halo staging (ddcmi_ctx::halo_in_recv): the pair kernel takes the received beads out of the exchange's receive buffer, no update
 * launch -- for halos of received beads only, needed by the pair kernel only.  DDCMI_NO_DIRECT_HALO=1: never */
static bool direct_halo(const ddcmi_ctx *ctx) { return !ctx->no_direct_halo && exchanging(ctx) && !ctx->group_ && !ctx->halo_overlap && ctx->nself_images == 0 && pair_kernel_only(ctx) && ctx->stage_cap + 2 < 4096; }
/* The plan of one force evaluation, from the context as it stands and the caller's wishes: may_fuse, the integrator's pass may ride
 * in the pair kernel (with time step dt); may_lean, the step could be lean.  No side effects: launch_forces executes it. */
static StepPlan plan_forces(const ddcmi_ctx *ctx, bool may_fuse, bool may_lean, double dt)
{
   StepPlan p = {};
   const bool peers = has_peers(ctx), at_owners = self_images(ctx);
   p.direct = direct_halo(ctx);
   /* the received beads' displacement since the rebuild: measured by the update launch of a decomposed run whose pair kernel may end its rows early */
   p.hdisp = !p.direct && ctx->shell_skip && ctx->nhalo > 0 && decomposed(ctx);
   /* (no refresh after a rebuild: it made the images from these very positions; and never on a rank of a transport whose halo is marked fresh --
    * its last exchange or its rebuild placed every image and halo bead, and the receive buffer may hold velocities or nothing by now) */
   if (peers && !ctx->halo_fresh) p.halo = p.direct ? HALO_DIRECT : ctx->halo_overlap ? HALO_OVERLAP : HALO_UPDATE;
   else if (at_owners) p.halo = HALO_AT_OWNERS;
   else if (ctx->nhalo > 0 && !ctx->images_fresh && !(peers && !ctx->group_)) p.halo = HALO_IMAGES;
   if ((ctx->excludePotentialTerm & 128) != 0) return p;
   p.lds = nb_lds_layout(ctx, may_fuse);
   p.fused = may_fuse;
   if (may_fuse)
   {
      /* the integrator's pass rides in the pair kernel only with the fixed layout, and never at the price of the second workgroup per CU */
      const NbLds plain = nb_lds_layout(ctx, false);
      if (!(p.lds.zfix && p.lds.wgs >= plain.wgs && p.lds.wgs > 0)) { p.fused = false; p.lds = plain; }
   }
   /* lean: the fused launch, every tile in ONE launch, the images found at their owners (a decomposed rank: its halo staged directly; its
    * next exchange packs its messages by a launch of its own, mg_pack3, instead of riding in the reduction launch) */
   p.lean = may_lean && p.fused && ctx->ntile_class[1] <= 0 && (peers ? p.direct : (ctx->nhalo == 0 || at_owners)) && ctx->lean_pending < LEAN_W &&
            ctx->lean_since < LEAN_W && (ctx->lean_since == 0 || ctx->lean_dt == dt);
   if (p.fused && !p.lean)
      p.red = (ctx->nhalo > 0 && !peers && !at_owners) ? RED_IMAGES : (peers && !ctx->halo_overlap && mg_pack_ready(ctx)) ? RED_PACK : RED_PLAIN;
   return p;
}
/* test entry point (ddcmi_test.h): the plan of the evaluation out[0] back from the last one */
extern "C" int ddcmi_debug_step_plan(ddcmi_ctx *ctx, int out[8])
{
   if (!ctx || !out || out[0] < 0 || out[0] >= 16 || out[0] >= ctx->nplan) return DDCMI_EINVAL;
   const StepPlan &p = ctx->plan_ring[(ctx->nplan - 1 - out[0]) % 16];
   const int v[8] = {p.halo, p.fused, p.lean, p.lds.lvl, p.lds.zfix, p.red, p.hdisp, p.direct};
   memcpy(out, v, sizeof(v));
   return DDCMI_OK;
}

/* ---- launch_forces and its pieces ---- */
static void launch_halo_update(ddcmi_ctx *ctx, hipStream_t st, bool hdisp)
{
   /* (hdisp: the word of this step's parity is the one this step's pair kernel reads) */
   if (ctx->nhalo > 0)
      hipLaunchKernelGGL(k_halo_update, dim3(cdiv(ctx->nhalo, HU_PER)), dim3(HU_THREADS), 0, st, ctx->nloc, ctx->nhalo, ctx->halo_src.p, ctx->halo_shift.p,
                         ctx->gp.L[0], ctx->gp.L[1], ctx->gp.L[2], ctx->pos.p, ctx->gid.p, false, ctx->hrecv3.p, ctx->hrecv5.p, (const int *)nullptr,
                         hdisp ? (unsigned long long *)(ctx->d_results + R_DISP + 1) : nullptr, (int)(ctx->loop & 1));
}
/* *pending: the refresh runs on the second stream, and ev_halo says when it is done */
static int refresh_halo(ddcmi_ctx *ctx, const StepPlan &p, bool *pending)
{
   hipStream_t st = ctx->stream;
   int rc;
   switch (p.halo)
   {
   case HALO_DIRECT: case HALO_UPDATE:
      if ((rc = ddcmi_mg_refresh_halo(ctx, st))) return rc;
      /* (direct: pos[nloc..] keeps the rebuild's records from here on; else the update places every received bead in pos[]) */
      ctx->halo_in_recv = p.halo == HALO_DIRECT;
      if (p.halo == HALO_UPDATE) launch_halo_update(ctx, st, p.hdisp);
      break;
   case HALO_OVERLAP:
      if (!ctx->stream2) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));      /* (the rebuild's interior search may have made it already) */
      if (!ctx->ev_drift)
      {
         HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_drift, hipEventDisableTiming));
         HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_halo, hipEventDisableTiming));
      }
      HIPCHK(ctx, hipEventRecord(ctx->ev_drift, st));                  /* positions of this step are final */
      HIPCHK(ctx, hipStreamWaitEvent(ctx->stream2, ctx->ev_drift, 0));
      if ((rc = ddcmi_mg_refresh_halo(ctx, ctx->stream2))) return rc;
      launch_halo_update(ctx, ctx->stream2, p.hdisp);
      HIPCHK(ctx, hipEventRecord(ctx->ev_halo, ctx->stream2));
      *pending = true;
      break;
   case HALO_IMAGES: launch_halo_update(ctx, st, p.hdisp); break;
   case HALO_NONE: case HALO_AT_OWNERS: break;
   }
   return DDCMI_OK;
}
/* fb: the bonded kernels' force records, or null */
static NbTileArgs nb_tile_args(const ddcmi_ctx *ctx, const StepPlan &p, double4 *fb)
{
   NbTileArgs na;
   na.ntile = ctx->ntile; na.stage_stride = ctx->stage_cap; na.nlj = ctx->nnb;
   na.cap = ctx->stage_cap + 2;      /* + sentinel slot 0, kept even so every LDS array stays 16-byte aligned */
   na.cell_start_o = ctx->cell_start_o.p; na.stage_idx = ctx->stage_idx.p; na.tile_nstage = ctx->tile_nstage.p;
   na.cell_start = ctx->cell_start.p; na.cell_cnt = ctx->cell_cnt.p;
   na.tile_base = ctx->tile_base.p; na.tile_width = ctx->tile_width.p; na.tile_rows = ctx->tile_rows.p;
   na.nbr16 = ctx->nbr16.p; na.nbr_cnt = ctx->nbr_cnt.p; na.perm = ctx->tile_perm.p;
   na.tile_work = ctx->tile_work.p; na.halo_shift = ctx->halo_shift.p; na.nloc = ctx->nloc;
   na.disp = ctx->shell_skip ? ctx->d_results + R_DISP : nullptr; na.nbr_cum = ctx->nbr_cum.p; na.sh_r0sq = ctx->sh_r0sq; na.sh_step = ctx->sh_step;
   na.sh_reach[0] = -1e300;
   for (int sq = 1; sq < NSHELL; sq++) na.sh_reach[sq] = sqrt(ctx->sh_r0sq + (double)(sq - 1) * ctx->sh_step) * (1.0 - 1e-4) - ctx->rmax;
   na.hdisp = p.hdisp ? ctx->d_results + R_DISP + 1 + (int)(ctx->loop & 1) : nullptr;
   na.hrecv3 = ctx->halo_in_recv ? ctx->hrecv3.p : nullptr; na.halo_src = ctx->halo_src.p;
   na.halo_full_walk = (p.direct && ctx->shell_skip) ? 1 : 0;
   na.lvlidx = ctx->d_lvlidx.p; na.nlvl = ctx->nlvl; na.tab_off = p.lds.tab_off;
   na.fb = fb;
   na.self_img = p.halo == HALO_AT_OWNERS ? 1 : 0; na.vring_w = nullptr; na.vring_dt = ctx->lean_dt;
   na.vring = (na.disp && ctx->lean_since > 0) ? ctx->d_vring.p : nullptr; na.vring_n = ctx->lean_since;
   return na;
}
/* timing (ddcmi_ctx::timing): an event pair around a pair launch; *close is the second one, null where nothing is timed */
static int timing_open(ddcmi_ctx *ctx, bool fused, hipEvent_t *close)
{
   *close = nullptr;
   if (!ctx->timing) return DDCMI_OK;
   if (ctx->ev_used + 2 > ctx->ev.size())
   {
      size_t old = ctx->ev.size();
      ctx->ev.resize(old + 256);
      for (size_t k = old; k < ctx->ev.size(); k++) HIPCHK(ctx, hipEventCreate(&ctx->ev[k]));
   }
   hipEvent_t e0 = ctx->ev[ctx->ev_used++];
   *close = ctx->ev[ctx->ev_used++];
   ctx->ev_fused.resize(ctx->ev.size() / 2);
   ctx->ev_fused[ctx->ev_used / 2 - 1] = fused ? 1 : 0;
   HIPCHK(ctx, hipEventRecord(e0, ctx->stream));
   return DDCMI_OK;
}
static int timing_close(ddcmi_ctx *ctx, hipEvent_t close) { if (close) HIPCHK(ctx, hipEventRecord(close, ctx->stream)); return DDCMI_OK; }
/* one k_nonbond launch.  Q: charges; PS: the list entries carry the shifted-copy bit (pack_type 2); Z: NB_ZOFF, the fixed LDS layout
 * ({x,y} at 0, z at NB_ZOFF: neighbourhoods of up to NB_ZOFF/16 beads, which is every Martini system), or 0, the run-time layout;
 * F: the integrator's pass rides; L: the pair table in two levels */
template <bool Q, bool PS, int Z, bool F, bool L>
static int launch_nonbond(ddcmi_ctx *ctx, int grid, size_t lds, const NbTileArgs &na, double *partials, const FuseArgs &fa)
{
   const void *fn = (const void *)k_nonbond<Q, PS, PS, NB_THREADS, NB_WPE, NB_CH, Z, F, L>;
   size_t sb = 0;
   if (!lds_starts_at_zero(ctx->device, fn, &sb))
      SETERR(ctx, DDCMI_EUNSUPPORTED, "k_nonbond was built with %zu bytes of static LDS: its staged arrays no longer start at LDS address 0 (toolchain change) -- rebuild libddcmi.so with a compiler that gives it none", sb);
   HIPCHK(ctx, dyn_lds_limit(ctx->device, fn, (int)lds));
   hipLaunchKernelGGL((k_nonbond<Q, PS, PS, NB_THREADS, NB_WPE, NB_CH, Z, F, L>), dim3(grid), dim3(NB_THREADS), lds, ctx->stream, ctx->gp, na, ctx->npad, ctx->pos.p, ctx->d_kqtab.p,
                      ctx->excl16.p, ctx->excl_cnt.p, L ? ctx->d_lvltab.p : ctx->d_ljtab.p, ctx->rmax * ctx->rmax, ctx->krf, ctx->crf, ctx->keR,
                      ctx->fx.p, ctx->fy.p, ctx->fz.p, partials, fa);
   return DDCMI_OK;
}
/* the instantiations that exist: fused ones with the fixed layout only (plan_forces sees to it), plain ones with either */
template <bool Q, bool PS>
static int launch_nonbond_as(ddcmi_ctx *ctx, const StepPlan &p, int grid, const NbTileArgs &na, double *partials, const FuseArgs &fa)
{
   const size_t lds = p.lds.total;
   if (p.fused) return p.lds.lvl ? launch_nonbond<Q, PS, NB_ZOFF, true, true>(ctx, grid, lds, na, partials, fa) : launch_nonbond<Q, PS, NB_ZOFF, true, false>(ctx, grid, lds, na, partials, fa);
   if (p.lds.zfix) return p.lds.lvl ? launch_nonbond<Q, PS, NB_ZOFF, false, true>(ctx, grid, lds, na, partials, fa) : launch_nonbond<Q, PS, NB_ZOFF, false, false>(ctx, grid, lds, na, partials, fa);
   return p.lds.lvl ? launch_nonbond<Q, PS, 0, false, true>(ctx, grid, lds, na, partials, fa) : launch_nonbond<Q, PS, 0, false, false>(ctx, grid, lds, na, partials, fa);
}
/* the pair kernel's side of a force evaluation.  Bonded terms and restraints FIRST, into a zeroed array of force records (ddcmi_ctx::fb):
 * the pair kernel then finishes every bead's force in ONE place -- in memory (plain launch: f = f_pair + f_bonded) or in registers in
 * front of the integrator's pass (FUSE), so that systems with bonded terms take the fused step too.  Both kinds of launch form the same
 * sum, so the fused and the split step stay bit for bit alike, and both hand the records back zeroed: no launch is ever spent on
 * clearing them. */
static int launch_pair_forces(ddcmi_ctx *ctx, const StepPlan &p, bool defer_reduce, const FuseArgs *fuse, bool halo_pending)
{
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc;
   const bool has_bonded = (ctx->nbond + ctx->nangle + ctx->ntors + ctx->nrest) > 0;
   int rc;
   FuseArgs fa;
   memset(&fa, 0, sizeof(fa));
   if (p.fused) { fa = *fuse; fa.ke_off = p.lds.ke_off; }
   if (has_bonded && n == 0)
      /* a domain that holds no bead at the moment: no bonded launch -- and the sums of the last one it ran must not be reported again
       * (forces were never affected.  tools/soak_migration_r06.py lipid) */
      HIPCHK(ctx, hipMemsetAsync(ctx->d_results + R_SCR_BOND, 0, (R_SCR_MOLV - R_SCR_BOND) * sizeof(double), st));
   if (has_bonded && n > 0)
   {
      if (halo_pending) { HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_halo, 0)); halo_pending = false; }      /* bonded partners may be halo beads */
      /* (the record array: all zero -- every pair launch hands back zeroed what it consumed; a grown array is cleared once) */
      if (ctx->fb.cap < (size_t)ctx->npad) { if (ctx->fb.ensure(ctx->npad)) SETERR(ctx, DDCMI_ENOMEM, "bonded force records"); ctx->fb_zeroed = 0; }
      if (ctx->fb_zeroed < ctx->fb.cap) { HIPCHK(ctx, hipMemsetAsync(ctx->fb.p, 0, ctx->fb.cap * sizeof(double4), st)); ctx->fb_zeroed = ctx->fb.cap; }
      ctx->fb_zeroed = 0;      /* (until the pair launches below have consumed the records) */
      if ((rc = ddcmi_launch_bonded(ctx, ctx->fb.p, p.lean ? ctx->lean_pending : -1))) return rc;      /* (lean: the kernels' sums wait in the step's slot of the ring) */
   }
   if (p.lds.wgs <= 0) SETERR(ctx, DDCMI_EUNSUPPORTED, "nonbonded kernel needs %zu bytes of LDS (> 160 KiB)", p.lds.total);
   NbTileArgs na = nb_tile_args(ctx, p, (has_bonded && n > 0) ? ctx->fb.p : nullptr);
   double *partials = ctx->partials.p;
   if (p.lean)
   {
      /* the step's rows of sums go to its slot of the ring, its largest |v|^2 to its word */
      const size_t stride = (size_t)(ctx->nitems + 8) * 8;
      if (ctx->lean_pending > 0 && stride != ctx->lean_stride) SETERR(ctx, DDCMI_EINVAL, "internal: the lean steps' rows changed size without a flush");
      ctx->lean_stride = stride;
      ENSURE(ctx, ctx->lean_part, stride * LEAN_W); ENSURE(ctx, ctx->lean_kpart, stride * LEAN_W);
      partials = ctx->lean_part.p + stride * ctx->lean_pending;
      fa.kpartials = ctx->lean_kpart.p + stride * ctx->lean_pending;
      ctx->lean_dt = fa.dt; na.vring_dt = fa.dt;
      if (na.disp) na.vring_w = ctx->d_vring.p + (size_t)LEAN_VSTRIDE * ctx->lean_since;
      ctx->lean_since++;
   }
   /* class 0: tiles with all-owned neighbourhoods (every tile on a single domain);
    * class 1: tiles that stage image/halo beads, after the halo exchange */
   RoctxRange rng_nb("CHARMM_NONBOND");      /* martiniNonBond, bioMartini.c:989-1122 */
   const bool useq = ctx->has_charge, shbit = ctx->pack_type == 2;
   for (int cls = 0; cls < 2; cls++)
   {
      if (cls == 1 && halo_pending) { HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_halo, 0)); halo_pending = false; }
      if (ctx->ntile_class[cls] <= 0) continue;
      const double *hd_keep = na.hdisp;
      if (cls == 0 && halo_pending) na.hdisp = nullptr;      /* (tiles that stage owned beads only, while the exchange still writes the word) */
      const int grid = 8 * std::max(ctx->sched_longest[cls], 1);
      na.sched = ctx->sched.p + 16 * cls;
      hipEvent_t e1;
      if ((rc = timing_open(ctx, p.fused, &e1))) return rc;
      rc = useq ? (shbit ? launch_nonbond_as<true, true>(ctx, p, grid, na, partials, fa) : launch_nonbond_as<true, false>(ctx, p, grid, na, partials, fa))
                : (shbit ? launch_nonbond_as<false, true>(ctx, p, grid, na, partials, fa) : launch_nonbond_as<false, false>(ctx, p, grid, na, partials, fa));
      if (rc || (rc = timing_close(ctx, e1))) return rc;
      na.hdisp = hd_keep;
   }
   if (na.fb) ctx->fb_zeroed = ctx->fb.cap;
   if (ctx->timing) { ctx->t_launches++; if (p.fused) ctx->t_launches_fused++; }          /* per force evaluation: the event pairs of both classes add up */
   /* the final energies are formed in the same launch (the bonded kernels' sums are complete: they ran first) */
   if (!defer_reduce)
   {
      RedJob j0 = {ctx->partials.p, ctx->nitems, 8, ctx->d_results + R_NB_LJ, 1};
      hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 1), dim3(1024), 0, st, j0, j0, ctx->d_results, ctx->self_ele, ctx->red_tmp.p);
   }
   ctx->forces_valid = true;
   return DDCMI_OK;
}
/* plans the evaluation (ddcmi_ctx::plan keeps the plan for the caller and the tests) and executes it.  fuse: the integrator's pass may
 * ride in the pair kernel; may_lean: the caller could run this step lean */
static int launch_forces(ddcmi_ctx *ctx, bool defer_reduce = false, const FuseArgs *fuse = nullptr, bool may_lean = false)
{
   RoctxRange rng_force("DDCENERGY P_FORCE");      /* ddcenergy.c:160-238 */
   const StepPlan p = ctx->plan = ctx->plan_ring[ctx->nplan++ % 16] = plan_forces(ctx, fuse != nullptr, may_lean, fuse ? fuse->dt : 0.0);
   hipStream_t st = ctx->stream;
   bool halo_pending = false;
   int rc;
   if ((rc = refresh_halo(ctx, p, &halo_pending))) return rc;
   ctx->images_fresh = false;
   if ((ctx->excludePotentialTerm & 128) == 0) return launch_pair_forces(ctx, p, defer_reduce, fuse, halo_pending);
   /* no pair kernel: zeroed forces, the bonded kernels add to them */
   if (!defer_reduce) HIPCHK(ctx, hipMemsetAsync(ctx->d_results, 0, 8 * sizeof(double), st));
   hipLaunchKernelGGL(k_zero3, dim3(cdiv(ctx->nloc, 256)), dim3(256), 0, st, ctx->nloc, ctx->fx.p, ctx->fy.p, ctx->fz.p);
   if (halo_pending) HIPCHK(ctx, hipStreamWaitEvent(st, ctx->ev_halo, 0));      /* bonded partners may be halo beads */
   if ((rc = ddcmi_launch_bonded(ctx))) return rc;
   if (!defer_reduce) hipLaunchKernelGGL(k_finish_energy, dim3(1), dim3(64), 0, st, ctx->d_results, 0.0);
   ctx->forces_valid = true;
   return DDCMI_OK;
}

/* the scratch of k_reduce_hist, zeroed once when it is made (every launch leaves its tickets at zero), and the launch itself: shared with
 * ddcmi_debug_reduce_hist (include/ddcmi_test.h), so that the test runs on this layout and not on a restatement of it */
static hipError_t lean_tmp_zero(double *tmp, hipStream_t st) { return hipMemsetAsync(tmp, 0, LEAN_TMP_DOUBLES * sizeof(double), st); }
static void lean_launch_hist(const RedJob &jf, const RedJob &jk, size_t stride, int np, double *hist, double *tmp, hipStream_t st)
{
   hipLaunchKernelGGL(k_reduce_hist, dim3(RED_SPLIT, 2 * np), dim3(1024), 0, st, jf, jk, stride, hist, tmp);
}
/* the lean steps' pending sums, all in one launch (k_reduce_hist) */
int ddcmi_lean_flush(ddcmi_ctx *ctx)
{
   if (ctx->lean_pending <= 0) return DDCMI_OK;
   const int np = ctx->lean_pending;
   ctx->lean_pending = 0;
   if (!ctx->lean_tmp.p)
   {
      ENSURE(ctx, ctx->lean_tmp, LEAN_TMP_DOUBLES); ENSURE(ctx, ctx->lean_hist, (size_t)LEAN_HW * LEAN_W);
      HIPCHK(ctx, hipMemsetAsync(ctx->lean_hist.p, 0, (size_t)LEAN_HW * LEAN_W * sizeof(double), ctx->stream));
      HIPCHK(ctx, lean_tmp_zero(ctx->lean_tmp.p, ctx->stream));
   }
   RedJob jf = {ctx->lean_part.p, ctx->nitems, 8, nullptr, 0, 0.0, nullptr};
   RedJob jk = {ctx->lean_kpart.p, ctx->nitems, 7, nullptr, 0, 0.0, nullptr};
   lean_launch_hist(jf, jk, ctx->lean_stride, np, ctx->lean_hist.p, ctx->lean_tmp.p, ctx->stream);
   if ((ctx->nbond + ctx->nangle + ctx->ntors) > 0) { int rcb = ddcmi_lean_flush_bonded(ctx, np); if (rcb) return rcb; }
   ctx->lean_hist_n = np;
   return DDCMI_OK;
}
/* test entry point (ddcmi_test.h): the sums of the lean steps of the last flush, LEAN_HW = 32 per step: pair kernel {lj, ele, virial xx yy zz xy xz yz} as
 * the full list counts them (x 2), {rk, tion xx yy zz xy xz yz}, 0, the bonded kernels' {e_bond, e_angle, e_tors, e_impr, virial xx yy zz xy xz yz}, 0 ... */
extern "C" int ddcmi_debug_lean_history(ddcmi_ctx *ctx, int *nsteps, double *sums)
{
   if (!ctx || !nsteps || !sums) return DDCMI_EINVAL;
   (void)hipSetDevice(ctx->device);
   int rc = ddcmi_lean_flush(ctx);
   if (rc) return rc;
   *nsteps = ctx->lean_hist_n;
   if (ctx->lean_hist_n > 0)
   {
      HIPCHK(ctx, hipMemcpyAsync(sums, ctx->lean_hist.p, (size_t)LEAN_HW * ctx->lean_hist_n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   }
   return DDCMI_OK;
}
/* test entry point: the displacement bound's base word and the lean steps' words (largest |v|^2 per step since the rebuild) */
extern "C" int ddcmi_debug_disp(ddcmi_ctx *ctx, double *disp, float *ring, int *nring)
{
   if (!ctx || !disp || !ring || !nring) return DDCMI_EINVAL;
   (void)hipSetDevice(ctx->device);
   unsigned w[LEAN_W * LEAN_VSTRIDE];
   memset(w, 0, sizeof(w));
   HIPCHK(ctx, hipMemcpyAsync(disp, ctx->d_results + R_DISP, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
   if (ctx->d_vring.p) HIPCHK(ctx, hipMemcpyAsync(w, ctx->d_vring.p, sizeof(w), hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   *nring = ctx->lean_since;
   for (int q = 0; q < LEAN_W; q++) memcpy(ring + q, w + q * LEAN_VSTRIDE, sizeof(float));
   return DDCMI_OK;
}
static int fetch_results(ddcmi_ctx *ctx)
{
   RoctxRange rng_e("EVAL_ETYPE");      /* energyInfo.c:75-148 */
   { int rcl = ddcmi_lean_flush(ctx); if (rcl) return rcl; }
   { int rca = ddcmi_agree_poll(ctx); if (rca) return rca; }      /* (a peer whose rebuild failed: say so instead of waiting behind an exchange it never joins) */
   HIPCHK(ctx, hipMemcpyAsync(ctx->h_results, ctx->d_results, R_SIZE * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   return DDCMI_OK;
}

extern "C" int ddcmi_eval_forces(ddcmi_ctx *ctx, double *energies, double *virial)
{
   if (!ctx) return DDCMI_EINVAL;
   (void)hipSetDevice(ctx->device);
   int rc;
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group evaluate forces with ddcmi_group_eval_forces");
   /* new species or nonbonded parameters under an uploaded state (ddcmi_set_species / ddcmi_set_nonbonded without a new upload): the class tables, the
    * beads' tags and with them the list are rebuilt before anything is evaluated with the old ones */
   if (ctx->tables_dirty && ctx->nloc > 0 && (rc = nb_tables(ctx))) return rc;
   if (!ctx->list_valid) { if ((rc = ddcmi_build_list(ctx))) return rc; ctx->images_fresh = true; }
   if ((rc = launch_forces(ctx))) return rc;
   ctx->molv_valid = false;
   if ((rc = fetch_results(ctx))) return rc;
   if (energies) for (int k = 0; k < DDCMI_NE; k++) energies[k] = ctx->h_results[R_E + k];
   if (virial) for (int k = 0; k < 6; k++) virial[k] = ctx->h_results[R_VIR + k];
   return DDCMI_OK;
}

/* the velocity updates' per-group data of a step that has no thermostat, no noise (the counter-based stream, seed 0), no kinds and no scaling;
 * front_lambda starts from it */
static GroupLambda identity_lambda()
{
   GroupLambda lam;
   memset(&lam, 0, sizeof(lam));
   for (int g = 0; g < 32; g++) lam.v[g] = lam.a[g] = 1.0;
   lam.scale[0] = lam.scale[1] = lam.scale[2] = 1.0;
   return lam;
}
/* BACK half kick (do_kick) + the workgroups' kinetic terms into kpartials */
static int launch_kick_ke(ddcmi_ctx *ctx, double dt, int do_kick, const GroupLambda &lam)
{
   const int nblk = cdiv(ctx->nloc, DDCMI_BLOCK * KE_PER);
   ENSURE(ctx, ctx->kpartials, (size_t)(nblk + 8) * 8);
   hipLaunchKernelGGL(k_kick_ke, dim3(std::max(nblk, 1)), dim3(DDCMI_BLOCK), 0, ctx->stream, ctx->nloc, dt, ctx->d_invmass.p, ctx->d_mass.p, ctx->species.p,
                      ctx->fx.p, ctx->fy.p, ctx->fz.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->kpartials.p, do_kick, ctx->group.p, lam, ctx->gid.p);
   return DDCMI_OK;
}
/* kinetic_terms (+ the BACK half kick); with_forces: the same launch also reduces the
 * nonbonded partials of the force evaluation just queued and forms the final energies */
static int launch_kinetic(ddcmi_ctx *ctx, double dt, int do_kick, bool with_forces = false, const GroupLambda *gk = nullptr, bool then_drift = false)
{
   RoctxRange rng_ke("KINETIC_TERMS");      /* energy.c:48-163 */
   GroupLambda plain;
   if (!gk) { plain = identity_lambda(); gk = &plain; }
   int rc, n = ctx->nloc, nblk = cdiv(n, DDCMI_BLOCK * KE_PER);
   if (then_drift)
   {
      ENSURE(ctx, ctx->kpartials, (size_t)(nblk + 8) * 8);
      if (gk->scale[0] != 1.0 || gk->scale[1] != 1.0 || gk->scale[2] != 1.0) ctx->shell_skip = false;      /* (scaled positions: not a plain drift) */
      hipLaunchKernelGGL(k_kick_ke_drift, dim3(std::max(nblk, 1)), dim3(DDCMI_BLOCK), 0, ctx->stream, n, dt, ctx->d_invmass.p, ctx->d_mass.p, ctx->species.p, ctx->group.p, *gk,
                         ctx->fx.p, ctx->fy.p, ctx->fz.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->pos.p, ctx->kpartials.p, ctx->gid.p);
   }
   else if ((rc = launch_kick_ke(ctx, dt, do_kick, *gk))) return rc;
   RedJob jk = {ctx->kpartials.p, nblk, 7, ctx->d_results + R_RK, 0, then_drift ? dt : 0.0, ctx->d_results + R_DISP};      /* (+ the drift's share of the displacement bound) */
   if (with_forces)
   {
      const bool nb_on = (ctx->excludePotentialTerm & 128) == 0;
      const double self = nb_on ? ctx->self_ele : 0.0;
      RedJob jf = {ctx->partials.p, nb_on ? ctx->nitems : 0, 8, ctx->d_results + R_NB_LJ, 1};
      hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 2), dim3(1024), 0, ctx->stream, jf, jk, ctx->d_results, self, ctx->red_tmp.p);
   }
   else
      hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 1), dim3(1024), 0, ctx->stream, jk, jk, ctx->d_results, 0.0, ctx->red_tmp.p);
   return DDCMI_OK;
}

/* berendsen_Update FRONT_TIMESTEP (berendsen.c:30-62), host scalar logic */
static void berendsen_update(ddcmi_ctx *ctx, double dt_half)
{
   for (int g = 0; g < ctx->ngroup; g++)
   {
      if (ctx->gtype[g] != DDCMI_BERENDSEN) continue;
      ctx->gTsum[g] += ctx->gT[g];
      ctx->gnT[g] += 1;
      double Tave = ctx->gTsum[g] / ctx->gnT[g];
      double ratio = (Tave == 0) ? 0 : ctx->gTeq[g] / Tave;
      if (ctx->gtau[g] != 0) ctx->glambda[g] = sqrt(1 + (2.0 * dt_half / ctx->gtau[g]) * (ratio - 1));
      else ctx->glambda[g] = sqrt(ratio);
      ctx->gdoScaling[g] = 0;
      if (ctx->loop % ctx->ginterval[g] == 0) { ctx->gTsum[g] = 0; ctx->gnT[g] = 0; ctx->gdoScaling[g] = 1; }
   }
}

/* nglf.c:74-95: FRONT half kick + drift, clock advance */
static GroupLambda front_lambda(const ddcmi_ctx *ctx, double dt)
{
   GroupLambda lam = identity_lambda();
   lam.seed = ctx->rng_seed;
   lam.lcg = ctx->lcg_on ? ctx->lcg.p : nullptr;
   /* the FRONT update of a step sees the loop count before its increment, the BACK update the one after */
   lam.counter_front = 2ull * (unsigned long long)ctx->loop;
   lam.counter_back = 2ull * (unsigned long long)ctx->loop + 1ull;
   const double dt_half = 0.5 * dt;
   for (int g = 0; g < 32; g++)
   {
      /* lambda applies at the FRONT kick when doScaling is set (berendsen.c:74-80) */
      if (g < ctx->ngroup && ctx->gtype[g] == DDCMI_BERENDSEN && ctx->gdoScaling[g]) lam.v[g] = ctx->glambda[g];
      const int kind = g < ctx->ngroup ? ctx->gtype[g] : DDCMI_FREE;
      if (kind == DDCMI_FROZEN || kind == DDCMI_FIXEDVELOCITY || kind == DDCMI_QUENCH) lam.kind_mask |= 1u << g;
      if (kind == DDCMI_FROZEN) lam.frozen_mask |= 1u << g;
      if (kind == DDCMI_QUENCH) lam.quench_mask |= 1u << g;
      if (kind == DDCMI_FIXEDVELOCITY && (size_t)g < ctx->gvset.size() && ctx->gvset[g])
      {
         lam.fixset_mask |= 1u << g;
         for (int k = 0; k < 3; k++) lam.vw[g][k] = ctx->gvel[3 * g + k];
      }
      if (g < ctx->ngroup && ctx->gtype[g] == DDCMI_LANGEVIN)
      {
         lam.lang_mask |= 1u << g;
         lam.a[g] = exp(-dt_half / ctx->gtau[g]);
         lam.dfac[g] = sqrt(2.0 * dt_half * ctx->gTeq[g] / ctx->gtau[g]);          /* kB = 1 in internal units */
         if ((size_t)(3 * g + 2) < ctx->gvcm.size() && (ctx->gvcm[3 * g] != 0.0 || ctx->gvcm[3 * g + 1] != 0.0 || ctx->gvcm[3 * g + 2] != 0.0))
         {
            lam.vcm_mask |= 1u << g;
            for (int k = 0; k < 3; k++) lam.vw[g][k] = (1.0 - lam.a[g]) * ctx->gvcm[3 * g + k];
         }
      }
   }
   return lam;
}
/* The FRONT half of a step in phases, so that a decomposed run can put its exchanges between them (one context: step_pre
 * calls them back to back, the transport's collectives in between; an in-process group: ddcmi_group_step_nglf calls each
 * phase for every domain and moves the data itself):
 *   a  barostat: this rank's sums of the last force evaluation -- virial diagonal and molecular term -- to the host
 *      (+ {P, F} of the split molecules on the device)                       -> all-reduce
 *   b  barostat: pressures, scale factors, box; FRONT half kick (+ drift unless constraints follow)
 *                                                                            -> velocity halo (constraints only)
 *   c  constraints: FRONT solve, drift; clock */
int ddcmi_mg_refresh_vel(ddcmi_ctx *ctx);
static int step_pre_a(ddcmi_ctx *ctx)
{
   if (ctx->drift_done || !(ctx->baro_beta > 0.0)) return DDCMI_OK;
   /* nglfconstraint.c:527-536 + changeVolume (:64-84): semi-isotropic Berendsen barostat from the molecular
    * pressure of the last force evaluation, at the TARGET temperature */
   int rcb;
   if (!ctx->molv_valid && (rcb = ddcmi_launch_mol_virial(ctx))) return rcb;     /* first step after ddcmi_eval_forces */
   if ((rcb = fetch_results(ctx))) return rcb;
   const double *mv = ctx->h_results + R_SCR_MOLV;       /* zero unless molecule lists are set */
   ctx->baro_sums[0] = ctx->h_results[R_VIR + DDCMI_XX]; ctx->baro_sums[1] = ctx->h_results[R_VIR + DDCMI_YY]; ctx->baro_sums[2] = ctx->h_results[R_VIR + DDCMI_ZZ];
   ctx->baro_sums[3] = mv[0]; ctx->baro_sums[4] = mv[1]; ctx->baro_sums[5] = mv[2];
   ctx->baro_sums[6] = (double)ctx->nloc;
   return DDCMI_OK;
}
/* k_kick_drift's one call site */
static void launch_kick_drift(ddcmi_ctx *ctx, double dt, const GroupLambda &lam, KickDrift mode, double *vpart = nullptr)
{
   const auto k = mode == SCALE_KICK ? k_kick_drift<SCALE_KICK> : mode == DRIFT_ONLY ? k_kick_drift<DRIFT_ONLY> : k_kick_drift<KICK_DRIFT>;
   hipLaunchKernelGGL(k, dim3(cdiv(ctx->nloc, 256)), dim3(256), 0, ctx->stream, ctx->nloc, dt, ctx->d_invmass.p, ctx->species.p, ctx->group.p, lam, ctx->gid.p,
                      ctx->fx.p, ctx->fy.p, ctx->fz.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->pos.p, vpart);
}
static int step_pre_b(ddcmi_ctx *ctx, double dt)
{
   int n = ctx->nloc, nb = cdiv(n, 256);
   if (ctx->drift_done) return DDCMI_OK;
   GroupLambda lam = front_lambda(ctx, dt);
   if (ctx->baro_beta > 0.0)
   {
      int rcb;
      double split[3];
      if ((rcb = ddcmi_mol_split_term(ctx, split))) return rcb;      /* (P/M) o F of the molecules with atoms on several ranks, from the summed {P, F} */
      const double nmol = ctx->nmol_total > 0 ? (double)ctx->nmol_total : ctx->baro_sums[6];
      const double vol = ctx->h[0] * ctx->h[4] * ctx->h[8], NkT = nmol * ctx->baro_T;
      double pxx = (ctx->baro_sums[0] - (ctx->baro_sums[3] - split[0]) + NkT) / vol - ctx->baro_P0;
      double pyy = (ctx->baro_sums[1] - (ctx->baro_sums[4] - split[1]) + NkT) / vol - ctx->baro_P0;
      double pzz = (ctx->baro_sums[2] - (ctx->baro_sums[5] - split[2]) + NkT) / vol - ctx->baro_P0;
      ctx->pmol[0] = pxx + ctx->baro_P0; ctx->pmol[1] = pyy + ctx->baro_P0; ctx->pmol[2] = pzz + ctx->baro_P0;
      const double btt = ctx->baro_beta * dt / ctx->baro_tau;
      double pl = 0.5 * (pxx + pyy);
      if (ctx->baro_iso) pl = pzz = (1.0 / 3.0) * (pxx + pyy + pzz);          /* molecularPressureGPU.cu:211 */
      double l[3] = {cbrt(1.0 + pl * btt), cbrt(1.0 + pl * btt), cbrt(1.0 + pzz * btt)};
      for (int a = 0; a < 3; a++)
      {
         if (fabs(l[a] - 1.0) < 1e-14) l[a] = 1.0;          /* box.c:44 */
         lam.scale[a] = l[a];
         ctx->h[4 * a] *= l[a];
         ctx->gp.L[a] = ctx->h[4 * a];
      }
   }
   if (ctx->vaf_on && n > 0 && (lam.scale[0] != 1.0 || lam.scale[1] != 1.0 || lam.scale[2] != 1.0))
      /* the scaling is no displacement (scalePositionsByBoxChange leaves v0[].r alone): the origins move by what it moves the beads */
      hipLaunchKernelGGL(k_vaf_rescale, dim3(nb), dim3(256), 0, ctx->stream, n, lam.scale[0], lam.scale[1], lam.scale[2], ctx->pos.p, ctx->vaf.p);
   if (ctx->ncgroup > 0 && ctx->nhalo > 0 && (lam.scale[0] != 1.0 || lam.scale[1] != 1.0 || lam.scale[2] != 1.0))
      /* the FRONT solve reads the (scaled) positions of partners that are image / halo beads: adjustPosn for them too (an image
       * r + L goes to lambda r + lambda L, its place in the scaled box); the position halo after the drift replaces them */
      hipLaunchKernelGGL(k_scale_pos, dim3(cdiv(ctx->nhalo, 256)), dim3(256), 0, ctx->stream, ctx->nhalo, lam.scale[0], lam.scale[1], lam.scale[2], ctx->pos.p + n);
   /* the displacement bound of the shell-limited walk follows a plain kick + drift only: the barostat's scaling and the drift behind a
    * constraint solve move beads by more than dt |v| of this kernel */
   if (ctx->ncgroup > 0 || lam.scale[0] != 1.0 || lam.scale[1] != 1.0 || lam.scale[2] != 1.0) ctx->shell_skip = false;
   if (n > 0 && ctx->ncgroup > 0)
      /* nglfconstraint.c:538-553: FRONT kick, velocityConstraintOld(FRONT) at the (scaled) positions, drift */
      launch_kick_drift(ctx, dt, lam, SCALE_KICK);
   else if (n > 0)
   {
      double *vpart = nullptr;
      if (ctx->shell_skip) { ENSURE(ctx, ctx->kpartials, (size_t)(nb + 8) * 8); vpart = ctx->kpartials.p; }
      launch_kick_drift(ctx, dt, lam, KICK_DRIFT, vpart);
      if (vpart)
      {
         RedJob jd = {vpart, nb, 0, nullptr, 0, dt, ctx->d_results + R_DISP};      /* D += dt max |v| */
         hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 1), dim3(1024), 0, ctx->stream, jd, jd, ctx->d_results, 0.0, ctx->red_tmp.p);
      }
   }
   return DDCMI_OK;
}
static int step_pre_c(ddcmi_ctx *ctx, double dt)
{
   if (!ctx->drift_done && ctx->ncgroup > 0)
   {
      int rcc;
      if ((rcc = ddcmi_launch_constraints(ctx, dt, 0))) return rcc;
      if (ctx->nloc > 0) launch_kick_drift(ctx, dt, front_lambda(ctx, dt), DRIFT_ONLY);
   }
   ctx->drift_done = false;             /* else: the previous step's last kernel already did this kick + drift */
   ctx->time += dt;
   ctx->loop += 1;
   ctx->halo_fresh = false;
   return DDCMI_OK;
}
/* do the constraint solves of this context need its neighbours' velocities? */
static inline bool cons_exchange(const ddcmi_ctx *ctx) { return ctx->ncgroup > 0 && ctx->cons_gid && decomposed(ctx); }
static int step_pre(ddcmi_ctx *ctx, double dt)
{
   int rc;
   if ((rc = step_pre_a(ctx))) return rc;
   if (!ctx->drift_done && ctx->baro_beta > 0.0 && decomposed(ctx))
   {
      if ((rc = mg_allreduce_host_values(ctx, ctx->baro_sums, 7))) return rc;
      if (ctx->nsplit > 0 && (rc = mg_allreduce_device(ctx, ctx->mol_red.p, 6 * (size_t)ctx->nsplit))) return rc;
   }
   const bool had_drift = ctx->drift_done;
   if ((rc = step_pre_b(ctx, dt))) return rc;
   if (!had_drift && cons_exchange(ctx) && (rc = ddcmi_mg_refresh_vel(ctx))) return rc;
   return step_pre_c(ctx, dt);
}
static int step_post_cons_b(ddcmi_ctx *ctx, double dt)
{
   int rc;
   if ((rc = ddcmi_launch_constraints(ctx, dt, 1))) return rc;
   GroupLambda lam = front_lambda(ctx, dt);
   return launch_kinetic(ctx, dt, 0, true, &lam, false);
}
/* behind a plain force launch: BACK kick, kinetic terms, the forces' reduction and the coming step's FRONT kick + drift in one kernel */
static int kick_ke_then_drift(ddcmi_ctx *ctx, double dt, const GroupLambda &lam)
{
   const int rc = launch_kinetic(ctx, dt, 1, true, &lam, true);
   if (!rc) ctx->drift_done = true;
   return rc;
}
/* nglf.c:97-108: ddcenergy, BACK half kick, kinetic_terms, group Update */
static int step_post(ddcmi_ctx *ctx, double dt, bool more_steps)
{
   int rc;
   bool fuse = more_steps && fuse_ok(ctx);
   GroupLambda lam_f;
   if (fuse)
   {
      berendsen_update(ctx, 0.5 * dt);     /* host scalars only: nothing of this step's device results enters */
      lam_f = front_lambda(ctx, dt);
      for (int g = 1; g < ctx->ngroup; g++) fuse &= lam_f.v[g] == lam_f.v[0];      /* one scale factor for every bead */
      if (!fuse)
      {
         /* (groups with different Berendsen factors this step: the split kernels, with the factors just formed) */
         if ((rc = launch_forces(ctx, true))) return rc;
         return kick_ke_then_drift(ctx, dt, lam_f);
      }
   }
   if (fuse)
   {
      /* forces, BACK kick, kinetic terms, FRONT kick and drift in ONE pass: the pair kernel's epilogue is k_kick_ke_drift */
      FuseArgs fa;
      memset(&fa, 0, sizeof(fa));
      fa.dt = dt;
      fa.lam = ctx->ngroup > 0 ? lam_f.v[0] : 1.0;
      fa.invmass = ctx->d_invmass.p; fa.massv = ctx->d_mass.p;
      fa.vx = ctx->vx.p; fa.vy = ctx->vy.p; fa.vz = ctx->vz.p;
      ENSURE(ctx, ctx->kpartials, (size_t)(std::max(ctx->nitems, cdiv(ctx->nloc, DDCMI_BLOCK * KE_PER)) + 8) * 8);
      ENSURE(ctx, ctx->pos2, (size_t)ctx->nloc + ctx->nhalo);      /* (the size ddcmi_bl_reserve_halo gave both buffers: no reallocation here) */
      if (ctx->nhalo > 0 && has_peers(ctx) && ctx->fuse_tags_of != ctx->nrebuild)
      {
         /* received halo beads keep their tag word where they lie (k_halo_update rewrites x y z only): both buffers need it
          * (the periodic images of a single domain are whole copies of their owners' records) */
         HIPCHK(ctx, hipMemcpyAsync(ctx->pos2.p + ctx->nloc, ctx->pos.p + ctx->nloc, (size_t)ctx->nhalo * sizeof(double4), hipMemcpyDeviceToDevice, ctx->stream));
         ctx->fuse_tags_of = ctx->nrebuild;
      }
      fa.pos_new = ctx->pos2.p; fa.kpartials = ctx->kpartials.p;
      if ((rc = launch_forces(ctx, true, &fa, lean_capable(ctx)))) return rc;
      const StepPlan &p = ctx->plan;
      if (!p.fused) return kick_ke_then_drift(ctx, dt, lam_f);      /* (the launch kept the plain kernel: LDS layout; the kick follows as usual) */
      ctx->drift_done = true;
      std::swap(ctx->pos, ctx->pos2);
      if (p.lean)
      {
         /* the kernel has left the step's rows of sums in the ring, moved the displacement bound on and will find the images at their owners */
         ctx->lean_pending++;
         return ctx->lean_pending >= LEAN_W ? ddcmi_lean_flush(ctx) : DDCMI_OK;
      }
      RedJob jf = {ctx->partials.p, ctx->nitems, 8, ctx->d_results + R_NB_LJ, 1};
      RedJob jk = {ctx->kpartials.p, ctx->nitems, 7, ctx->d_results + R_RK, 0, dt, ctx->d_results + R_DISP};      /* + this drift's share of the displacement bound */
      if (p.red == RED_PLAIN)
         hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 2), dim3(1024), 0, ctx->stream, jf, jk, ctx->d_results, ctx->self_ele, ctx->red_tmp.p);
      else
      {
         /* on the side, in the same launch: the periodic images at the drifted positions, which the next force evaluation finds fresh -- or
          * this rank's halo messages packed from the drifted positions, so that the next step's exchange starts with the sends */
         PackJob pk;
         ImageJob im;
         memset(&pk, 0, sizeof(pk)); memset(&im, 0, sizeof(im));
         if (p.red == RED_IMAGES) im = ImageJob{ctx->nloc, ctx->nhalo, ctx->halo_src.p, ctx->halo_shift.p, ctx->gp.L[0], ctx->gp.L[1], ctx->gp.L[2], ctx->pos.p};
         else ddcmi_mg_pack_job(ctx, &pk);
         hipLaunchKernelGGL(k_reduce_jobs_images, dim3(2 * RED_SPLIT + cdiv(im.nhalo + pk.nsend, 1024)), dim3(1024), 0, ctx->stream, jf, jk, ctx->d_results, ctx->self_ele, ctx->red_tmp.p, im, pk);
         (p.red == RED_IMAGES ? ctx->images_fresh : ctx->pack_fresh) = true;
      }
      return DDCMI_OK;
   }
   if ((rc = launch_forces(ctx, true))) return rc;
   berendsen_update(ctx, 0.5 * dt);     /* host scalars only: nothing of this step's device results enters */
   GroupLambda lam = front_lambda(ctx, dt);
   if (ctx->baro_beta > 0.0)      /* from this step's forces, for the next step's barostat */
   {
      if ((rc = ddcmi_launch_mol_virial(ctx))) return rc;
      ctx->molv_valid = true;
   }
   if (ctx->ncgroup > 0)
   {
      /* nglfconstraint.c:567-571: BACK kick, velocityConstraintOld(BACK), then kinetic_terms (a decomposed run puts the
       * velocity halo between the kick and the solve: step_post_cons_b) */
      if (ctx->nloc > 0 && (rc = launch_kick_ke(ctx, dt, 1, lam))) return rc;
      if (ctx->group_) return DDCMI_OK;      /* the group driver exchanges the velocities of all domains, then calls step_post_cons_b */
      if (cons_exchange(ctx) && (rc = ddcmi_mg_refresh_vel(ctx))) return rc;
      return step_post_cons_b(ctx, dt);
   }
   if (more_steps && ctx->nloc > 0 && !(ctx->baro_beta > 0.0))      /* the barostat needs this step's virial before the next drift */
      return kick_ke_then_drift(ctx, dt, lam);
   return launch_kinetic(ctx, dt, 1, true, &lam, false);
}

/* updateRate == 0: does this domain's list need a rebuild?  (neighborCheck; one host
 * round trip per step, as the reference pays an MPI_Allreduce per step in this mode) */
int ddcmi_displacement_check(ddcmi_ctx *ctx, int *need)
{
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, nblk = cdiv(std::max(n, 1), DDCMI_BLOCK);
   *need = 1;
   { int rca = ddcmi_agree_poll(ctx); if (rca) return rca; }      /* (this path waits on the host every step: a peer whose rebuild failed is reported here, not after the mailbox's timeout) */
   if (!ctx->list_valid || ctx->pos0.cap < (size_t)n) return DDCMI_OK;
   *need = 0;
   if (n == 0)
   {
      if (decomposed(ctx) && !ctx->group_) { double z[4] = {0, 0, 0, 0}; return mg_allreduce_host_values(ctx, z, 4); }      /* an empty domain still takes part in the collective */
      return DDCMI_OK;
   }
   ENSURE(ctx, ctx->kpartials, (size_t)(nblk + 8) * 8);
   ENSURE(ctx, ctx->disp, 16);
   HIPCHK(ctx, hipMemsetAsync(ctx->disp.p, 0, 16 * sizeof(double), st));
   hipLaunchKernelGGL(k_disp_sum, dim3(nblk), dim3(DDCMI_BLOCK), 0, st, n, ctx->pos.p, ctx->pos0.p, ctx->kpartials.p);
   RedJob js = {ctx->kpartials.p, nblk, 3, ctx->disp.p, 0};
   hipLaunchKernelGGL(k_reduce_jobs, dim3(RED_SPLIT, 1), dim3(1024), 0, st, js, js, ctx->d_results, 0.0, ctx->red_tmp.p);
   if (decomposed(ctx))
   {
      /* neighborCheck measures every particle of a rank -- halo included -- against ONE mean displacement; here a rank
       * sees only its owned beads, and domains that each subtracted their own centroid would never count the drift of
       * one domain against its neighbour (shear, flow across a face).  With a transport the mean is the global one
       * (all-reduced sums); an in-process group subtracts nothing (conservative: a uniform drift then costs rebuilds,
       * never a stale list). */
      double hs[4] = {0, 0, 0, 0};
      if (!ctx->group_)
      {
         HIPCHK(ctx, hipMemcpyAsync(hs, ctx->disp.p, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
         HIPCHK(ctx, hipStreamSynchronize(st));
         hs[3] = (double)n;
         int rca = mg_allreduce_host_values(ctx, hs, 4);
         if (rca) return rca;
         const double w = hs[3] > 0.0 ? (double)n / hs[3] : 0.0;      /* k_disp_max divides by this rank's bead count */
         for (int k = 0; k < 3; k++) hs[k] *= w;
      }
      HIPCHK(ctx, hipMemcpyAsync(ctx->disp.p, hs, 3 * sizeof(double), hipMemcpyHostToDevice, st));
   }
   hipLaunchKernelGGL(k_disp_max, dim3(nblk), dim3(DDCMI_BLOCK), 0, st, n, ctx->pos.p, ctx->pos0.p, ctx->disp.p, (unsigned long long *)(ctx->disp.p + 4));
   double d2max = 0.0;
   HIPCHK(ctx, hipMemcpyAsync(&d2max, ctx->disp.p + 4, sizeof(double), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   *need = (2.0 * sqrt(d2max) < ctx->deltaR) ? 0 : 1;
   return DDCMI_OK;
}
/* nglfconstraint's barostat and velocity constraints given by caller-order indices are solved per domain: with several
 * domains each rank would scale its own box from its local virial and solve constraint groups without their halo
 * partners -- silently wrong physics.  Checked where the decomposition is set up AND at every step call, whatever the
 * call order.  The gid forms carry the cross-domain sums and the velocity halo. */
static int mg_check_one_domain_features(ddcmi_ctx *ctx)
{
   if (ctx->nranks > 1 && ((ctx->baro_beta > 0.0 && !ctx->mol_gid) || (ctx->ncgroup > 0 && !ctx->cons_gid)))
      SETERR(ctx, DDCMI_EUNSUPPORTED, "%d domains: the barostat and the velocity constraints (NGLFCONSTRAINT) work on a single domain unless the molecules and the "
             "constraint groups are named by gid (ddcmi_set_molecule_lists_gid, ddcmi_set_constraints_gid)", ctx->nranks);
   return DDCMI_OK;
}
/* FROZEN / FIXEDVELOCITY / QUENCH groups beside constraint groups or a barostat: the constraint solver would move frozen beads and
 * overwrite set velocities; the pairing is refused at the step, before anything moves */
static int kinds_pairing_check(ddcmi_ctx *ctx)
{
   if (!(ctx->ncgroup > 0 || ctx->baro_beta > 0.0)) return DDCMI_OK;
   for (int g = 0; g < ctx->ngroup; g++)
      if (ctx->gtype[g] == DDCMI_FROZEN || ctx->gtype[g] == DDCMI_FIXEDVELOCITY || ctx->gtype[g] == DDCMI_QUENCH)
         SETERR(ctx, DDCMI_EUNSUPPORTED, "group %d is FROZEN, FIXEDVELOCITY or QUENCH (kind %d): such groups are not supported together with %s", g, ctx->gtype[g],
                ctx->ncgroup > 0 ? "constraint groups (NGLFCONSTRAINT)" : "a barostat");
   return DDCMI_OK;
}
static int rebuild_due(ddcmi_ctx *ctx, bool *due)
{
   if (!ctx->list_valid) { *due = true; return DDCMI_OK; }
   if (ctx->updateRate > 0) { *due = (ctx->loop % ctx->updateRate == 0); return DDCMI_OK; }
   int need = 0, rc = ddcmi_displacement_check(ctx, &need);
   if (rc) return rc;
   if (exchanging(ctx))
   {
      /* check4updateNeighbor (ddcUpdateAll.c:56): anyone needs a rebuild -> everyone rebuilds */
      double v = (double)need;
      if ((rc = ddcmi_comm_allreduce_sum(ctx, &v, 1))) return rc;
      need = v > 0.0;
   }
   *due = need != 0;
   return DDCMI_OK;
}

extern "C" int ddcmi_step_nglf(ddcmi_ctx *ctx, double dt, int nsteps)
{
   ARGCHK(ctx, nsteps < 0, "ddcmi_step_nglf: %d steps", nsteps);
   ARGCHK(ctx, !std::isfinite(dt), "ddcmi_step_nglf: the time step dt = %g is not finite", dt);
   if (!ctx->forces_valid) SETERR(ctx, DDCMI_EINVAL, "ddcmi_step_nglf needs forces: call ddcmi_eval_forces first (firstEnergyCall, masters.c:579)");
   if (ctx->group_) SETERR(ctx, DDCMI_EINVAL, "contexts of an in-process group are stepped with ddcmi_group_step_nglf");
   (void)hipSetDevice(ctx->device);
   int rc;
   if ((rc = mg_check_one_domain_features(ctx))) return rc;
   if ((rc = kinds_pairing_check(ctx))) return rc;
   if (ctx->baro_beta > 0.0 && ctx->nmol_total == 0 && decomposed(ctx)) SETERR(ctx, DDCMI_EINVAL, "the barostat of a decomposed run needs the molecule count: ddcmi_set_molecule_lists_gid");
   if (ctx->baro_beta > 0.0 && ctx->nmol_total == 0)
      for (int m = 0; m < ctx->nmoltype; m++)
         if (ctx->mol_nspecies[m] > 1) SETERR(ctx, DDCMI_EINVAL, "the barostat acts on the molecular pressure: molecule type %d has %d beads, call ddcmi_set_molecule_lists first", m, ctx->mol_nspecies[m]);
   for (int s = 0; s < nsteps; s++)
   {
      RoctxRange rng_step("MDSTEP");      /* nglf.c:67-112 */
      if ((rc = step_pre(ctx, dt))) return rc;
      /* ddcUpdateAll.c:64-71: rebuild when loop % updateRate == 0, or (updateRate == 0) when neighborCheck asks */
      bool due = false;
      if ((rc = rebuild_due(ctx, &due))) return rc;
      if (due) { RoctxRange rng_upd("UPDATEALL PAIRLIST"); if ((rc = ddcmi_build_list(ctx))) return rc; ctx->images_fresh = true; }      /* (nothing moves between here and this step's forces; ddcUpdateAll.c:120-156) */
      if ((rc = step_post(ctx, dt, s + 1 < nsteps))) return rc;
   }
   return DDCMI_OK;
}


/* ddcmi_subset.inl -- ANALYSIS type subsetWrite, format binaryCharmm, on the device (subsetWrite.c:409-522, subsetWriteBinaryCharmm;
 * rejectParticle :532-564): the beads a filter selects, packed as the file's 24-byte records {uint64 gid, uint32 pinfo, float r[3]} in
 * a device buffer of the context and copied out once -- 24 bytes per selected bead, never the state.  Included from ddcmi.hip behind
 * ddcmi_dsf.inl.  A census pass (ddcmi_census_frame.inl): read-only, no communication, no atomics, the same bytes when repeated.
 *
 * The filter (subset_selected) is rejectParticle's, comparison by comparison and in its order: gid < idmin, gid > idmax,
 * gid % modulus != 0, odd && gid % 2 == 0, r > max and r < min per axis, v likewise (strict: a bead on a bound stays, and so does one
 * whose coordinate is NaN), the species' include flag, and membership in the ascending idList (gid_find).  Positions are the ones a
 * download returns (census_position), velocities the slots'.  A record's pinfo is group_term[group] + species_term[species] (pinfoEncode, pinfo.c:119-126, split by the caller into
 * the two tables), its coordinates (float)((r - corner) * cL): one subtraction and one multiplication in double, one rounding to float.
 *
 * Shape: the frame's stable compaction in slot order (k_compact_count, k_compact_scan, k_compact_pack with SubsetSel), the order of
 * ddcmi_download_particles.  The total comes back first (one word); the records only when the caller's buffer takes them. */

struct SubsetParms
{
   unsigned long long idmin, idmax, modulus;
   long long nid;      /* < 0: no idList */
   int odd, pbc, nspecies, ngroup;
   double lo[3], hi[3], vlo[3], vhi[3], L[3], corner[3], cL;
};
/* what the kernels read of a bead */
struct SubsetBeads
{
   const double4 *pos; const double *vx, *vy, *vz; const unsigned long long *gid; const int *species, *group;
   const unsigned *include, *group_term, *species_term; const unsigned long long *ids;
};

/* rejectParticle, negated; r: the wrapped position, s: the (clamped) species */
__device__ __forceinline__ bool subset_selected(const SubsetParms &sp, const SubsetBeads &b, int i, double (&r)[3], int &s)
{
   const unsigned long long gid = b.gid[i];
   census_position(sp, b.pos[i], r);
   const double v[3] = {b.vx[i], b.vy[i], b.vz[i]};
   s = min(max(b.species[i], 0), sp.nspecies - 1);      /* (checked at the upload: the reads stay in bounds whatever the array holds) */
   if (gid < sp.idmin) return false;
   if (gid > sp.idmax) return false;
   if (gid % sp.modulus != 0) return false;
   if (sp.odd && gid % 2 == 0) return false;
#pragma unroll
   for (int a = 0; a < 3; a++) if (r[a] > sp.hi[a]) return false;
#pragma unroll
   for (int a = 0; a < 3; a++) if (r[a] < sp.lo[a]) return false;
#pragma unroll
   for (int a = 0; a < 3; a++) if (v[a] > sp.vhi[a]) return false;
#pragma unroll
   for (int a = 0; a < 3; a++) if (v[a] < sp.vlo[a]) return false;
   if (b.include[s] == 0) return false;
   long long at;
   return sp.nid < 0 || gid_find(b.ids, 0ll, sp.nid, gid, &at);
}

/* the compaction's functor (k_compact_count, k_compact_pack): the predicate hands r and s on to the store, three 8-byte stores into
 * rec, nrec records of three 8-byte words */
struct SubsetSel
{
   SubsetParms sp; SubsetBeads b; unsigned long long *rec;
   struct Item { double r[3]; int s; };
   __device__ __forceinline__ bool selected(int i, Item &it) const { return subset_selected(sp, b, i, it.r, it.s); }
   __device__ __forceinline__ void store(int i, unsigned place, const Item &it) const
   {
      const int g = min(max(b.group[i], 0), sp.ngroup - 1);
      const unsigned pinfo = b.group_term[g] + b.species_term[it.s];
      const float f0 = (float)((it.r[0] - sp.corner[0]) * sp.cL), f1 = (float)((it.r[1] - sp.corner[1]) * sp.cL), f2 = (float)((it.r[2] - sp.corner[2]) * sp.cL);
      unsigned long long *o = rec + 3 * (size_t)place;
      o[0] = b.gid[i];
      o[1] = (unsigned long long)pinfo | (unsigned long long)__float_as_uint(f0) << 32;
      o[2] = (unsigned long long)__float_as_uint(f1) | (unsigned long long)__float_as_uint(f2) << 32;
   }
};

/* ---- host side ---------------------------------------------------------- */
static_assert(sizeof(ddcmi_subset_record) == 24, "a binaryCharmm record is 24 bytes");
static int subset_check(ddcmi_ctx *ctx, const char *fn, const ddcmi_subset_filter *f, int64_t cap, const void *rec, const void *count)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, !f || !count, "%s: NULL argument (filter %p, count %p)", fn, (const void *)f, count);
   ARGCHK(ctx, rec && cap < 0, "%s: cap = %lld", fn, (long long)cap);
   ARGCHK(ctx, f->modulus < 1, "%s: modulus = %d, it must be at least 1", fn, f->modulus);
   ARGCHK(ctx, f->nid < 0 || (f->nid > 0 && !f->idlist), "%s: nid = %lld, idlist %p", fn, (long long)f->nid, (const void *)f->idlist);
   for (int64_t k = 1; k < f->nid; k++)
      if (f->idlist[k] < f->idlist[k - 1])
         SETERR(ctx, DDCMI_EINVAL, "%s: the idList is not ascending (entry %lld = %llu behind %llu)", fn, (long long)k, (unsigned long long)f->idlist[k], (unsigned long long)f->idlist[k - 1]);
   ARGCHK(ctx, ctx->nspecies < 1, "%s needs the species (ddcmi_set_species)", fn);
   ARGCHK(ctx, f->nspecies < ctx->nspecies, "%s: nspecies = %d, the context's beads have species up to %d", fn, f->nspecies, ctx->nspecies - 1);
   ARGCHK(ctx, f->ngroup < std::max(ctx->ngroup, 1), "%s: ngroup = %d, the context's beads have groups up to %d", fn, f->ngroup, std::max(ctx->ngroup, 1) - 1);
   ARGCHK(ctx, !f->group_term || !f->species_term, "%s: NULL pinfo table (group_term %p, species_term %p)", fn, (const void *)f->group_term, (const void *)f->species_term);
   ARGCHK(ctx, !std::isfinite(f->cL), "%s: cL = %g", fn, f->cL);
   return census_box_check(ctx, fn, 7);
}
/* this rank's count and, with rec, its records [sync] */
static int subset_one(ddcmi_ctx *ctx, const ddcmi_subset_filter *f, int64_t cap, ddcmi_subset_record *rec, int64_t *count)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc, ns = f->nspecies, ng = f->ngroup;
   *count = 0;
   if (n <= 0) return DDCMI_OK;      /* (a domain that holds no bead) */
   int per_wg, nwg;
   census_split(n, CENSUS_MAX_WG, &per_wg, &nwg);
   SubsetParms sp;
   sp.idmin = f->idmin; sp.idmax = f->idmax; sp.modulus = (unsigned long long)f->modulus;
   sp.nid = f->idlist ? (long long)f->nid : -1;
   sp.odd = f->odd != 0; census_set_box(ctx, sp); sp.nspecies = ns; sp.ngroup = ng;
   for (int a = 0; a < 3; a++)
   {
      sp.lo[a] = f->rmin[a]; sp.hi[a] = f->rmax[a]; sp.vlo[a] = f->vmin[a]; sp.vhi[a] = f->vmax[a]; sp.corner[a] = f->corner[a];
   }
   sp.cL = f->cL;
   /* subset_tab: include[ns] | group_term[ng] | species_term[ns] | wg_count[nwg] | wg_off[nwg + 1] */
   std::vector<unsigned> tab((size_t)2 * ns + ng);
   for (int s = 0; s < ns; s++) { tab[s] = f->include_species ? f->include_species[s] != 0 : 1u; tab[(size_t)ns + ng + s] = f->species_term[s]; }
   for (int g = 0; g < ng; g++) tab[(size_t)ns + g] = f->group_term[g];
   ENSURE(ctx, ctx->subset_tab, tab.size() + 2 * (size_t)nwg + 1);
   ENSURE(ctx, ctx->subset_ids, (size_t)std::max<long long>(sp.nid, 0) + 1);
   unsigned *d_tab = ctx->subset_tab.p, *d_cnt = d_tab + tab.size(), *d_off = d_cnt + nwg;
   HIPCHK(ctx, hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(unsigned), hipMemcpyHostToDevice, st));
   if (sp.nid > 0) HIPCHK(ctx, hipMemcpyAsync(ctx->subset_ids.p, f->idlist, (size_t)sp.nid * sizeof(uint64_t), hipMemcpyHostToDevice, st));
   const SubsetBeads b = {ctx->pos.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, (const unsigned long long *)ctx->gid.p, ctx->species.p, ctx->group.p,
                          d_tab, d_tab + ns, d_tab + ns + ng, ctx->subset_ids.p};
   SubsetSel sel = {sp, b, nullptr};
   compact_count(st, n, per_wg, nwg, sel, d_cnt, d_off);
   HIPCHK(ctx, hipGetLastError());
   unsigned total = 0u;
   HIPCHK(ctx, hipMemcpyAsync(&total, d_off + nwg, sizeof(unsigned), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   *count = (int64_t)total;
   if (!rec) return DDCMI_OK;
   if (cap < (int64_t)total) SETERR(ctx, DDCMI_EINVAL, "ddcmi_subset_records: capacity %lld < %u selected beads", (long long)cap, total);
   if (total == 0u) return DDCMI_OK;
   ENSURE(ctx, ctx->subset_rec, 3 * (size_t)total);
   sel.rec = ctx->subset_rec.p;
   compact_pack(st, n, per_wg, nwg, sel, d_off, total);
   HIPCHK(ctx, hipGetLastError());
   HIPCHK(ctx, hipMemcpyAsync(rec, ctx->subset_rec.p, sizeof(ddcmi_subset_record) * (size_t)total, hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}

extern "C" int ddcmi_subset_records(ddcmi_ctx *ctx, const ddcmi_subset_filter *f, int64_t cap, ddcmi_subset_record *rec, int64_t *count)
{
   return analysis_single(ctx, "subset_records", true, [=](ddcmi_ctx *c, const char *fn) { return subset_check(c, fn, f, cap, rec, count); },
                          [=](ddcmi_ctx *c) { return subset_one(c, f, cap, rec, count); });
}
/* in-process group (analysis_group_records): count[r] of every domain; with rec, the domains' records in rank order, cap their sum's room */
extern "C" int ddcmi_group_subset_records(ddcmi_ctx **ctxs, int n, const ddcmi_subset_filter *f, int64_t cap, ddcmi_subset_record *rec, int64_t *count)
{
   return analysis_group_records(ctxs, n, "subset_records", "selected beads", [=](ddcmi_ctx *c, const char *fn) { return subset_check(c, fn, f, cap, rec, count); },
                                 [=](ddcmi_ctx *c, size_t r) { return subset_one(c, f, 0, nullptr, count + r); }, rec != nullptr, cap, count,
                                 [=](ddcmi_ctx *c, size_t r, int64_t off) { return subset_one(c, f, count[r], rec + off, count + r); });
}

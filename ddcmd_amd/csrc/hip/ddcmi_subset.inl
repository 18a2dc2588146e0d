/* ddcmi_subset.inl -- ANALYSIS type subsetWrite, format binaryCharmm, on the device (subsetWrite.c:409-522, subsetWriteBinaryCharmm;
 * rejectParticle :532-564): the beads a filter selects, packed as the file's 24-byte records {uint64 gid, uint32 pinfo, float r[3]} in
 * a device buffer of the context and copied out once -- 24 bytes per selected bead, never the state.  Included from ddcmi.hip behind
 * ddcmi_dsf.inl.  A census pass (ddcmi_census_frame.inl): read-only, no communication, no atomics, the same bytes when repeated.
 *
 * The filter (subset_selected) is rejectParticle's, comparison by comparison and in its order: gid < idmin, gid > idmax,
 * gid % modulus != 0, odd && gid % 2 == 0, r > max and r < min per axis, v likewise (strict: a bead on a bound stays, and so does one
 * whose coordinate is NaN), the species' include flag, and membership in the ascending idList by binary search.  Positions are the
 * ones a download returns (k_export_particles: the slot's, shifted once by the box side where it left a periodic box), velocities
 * the slots'.  A record's pinfo is group_term[group] + species_term[species] (pinfoEncode, pinfo.c:119-126, split by the caller into
 * the two tables), its coordinates (float)((r - corner) * cL): one subtraction and one multiplication in double, one rounding to float.
 *
 * Shape: a stable compaction in slot order, the order of ddcmi_download_particles.
 *   k_subset_count   a workgroup counts the selected beads of its census_split range: ballot and popcount per wave, the waves' counts
 *                    added through LDS.
 *   k_subset_scan    one wave: the exclusive scan of the (at most CENSUS_MAX_WG) counts, and their total behind it.
 *   k_subset_pack    the predicate again; a lane's place is the workgroup's offset + the selected beads of the blocks before this one
 *                    + those of the waves before its own (LDS) + the popcount of the ballot below its lane; three 8-byte stores.
 * The total comes back first (one word); the records only when the caller's buffer takes them. */

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

__device__ __forceinline__ bool subset_in_list(const unsigned long long *ids, long long nid, unsigned long long gid)
{
   long long lo = 0, hi = nid;      /* the first entry >= gid */
   while (lo < hi)
   {
      const long long mid = lo + ((hi - lo) >> 1);
      if (ids[mid] < gid) lo = mid + 1; else hi = mid;
   }
   return lo < nid && ids[lo] == gid;
}
/* rejectParticle, negated; r: the wrapped position, s: the (clamped) species */
__device__ __forceinline__ bool subset_selected(const SubsetParms &sp, const SubsetBeads &b, int i, double (&r)[3], int &s)
{
   const unsigned long long gid = b.gid[i];
   const double4 p4 = b.pos[i];
   r[0] = p4.x; r[1] = p4.y; r[2] = p4.z;
#pragma unroll
   for (int a = 0; a < 3; a++)
      if (sp.pbc >> a & 1) { if (r[a] > 0.5 * sp.L[a]) r[a] -= sp.L[a]; if (r[a] < -0.5 * sp.L[a]) r[a] += sp.L[a]; }      /* k_export_particles */
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
   if (sp.nid >= 0 && !subset_in_list(b.ids, sp.nid, gid)) return false;
   return true;
}

__global__ __launch_bounds__(CENSUS_THREADS) void k_subset_count(int n, int per_wg, SubsetParms sp, SubsetBeads b, unsigned *__restrict__ wg_count)
{
   __shared__ unsigned wave_s[CENSUS_WAVES];
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   unsigned mine = 0u;      /* the wave's count: the same in all its lanes */
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the ballot) */
   {
      const int i = base + (int)threadIdx.x;
      double r[3]; int s;
      const bool sel = i < end && subset_selected(sp, b, i, r, s);
      mine += (unsigned)__popcll(__ballot(sel));
   }
   if ((threadIdx.x & 63) == 0) wave_s[threadIdx.x >> 6] = mine;
   __syncthreads();
   if (threadIdx.x == 0)
   {
      unsigned t = 0u;
#pragma unroll
      for (int w = 0; w < CENSUS_WAVES; w++) t += wave_s[w];
      wg_count[blockIdx.x] = t;
   }
}
/* one wave: wg_off[k] = wg_count[0] + ... + wg_count[k - 1] for k <= nwg (wg_off[nwg]: the total); lane l takes the entries
 * [l chunk, (l + 1) chunk) */
__global__ __launch_bounds__(64) void k_subset_scan(int nwg, const unsigned *__restrict__ wg_count, unsigned *__restrict__ wg_off)
{
   const int lane = threadIdx.x, chunk = (nwg + 63) / 64;
   const int beg = min(lane * chunk, nwg), end = min(beg + chunk, nwg);
   unsigned t = 0u;
   for (int k = beg; k < end; k++) t += wg_count[k];
   unsigned incl = t;
#pragma unroll
   for (int d = 1; d < 64; d <<= 1)
   {
      const unsigned o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
   }
   unsigned run = incl - t;
   for (int k = beg; k < end; k++) { wg_off[k] = run; run += wg_count[k]; }
   if (lane == 63) wg_off[nwg] = incl;
}
/* rec: nrec records of three 8-byte words */
__global__ __launch_bounds__(CENSUS_THREADS) void k_subset_pack(int n, int per_wg, SubsetParms sp, SubsetBeads b, const unsigned *__restrict__ wg_off,
                                                                unsigned nrec, unsigned long long *__restrict__ rec)
{
   __shared__ unsigned wave_s[2][CENSUS_WAVES];      /* the waves' counts of this block of beads and of the next: one barrier per block */
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   const int beg = blockIdx.x * per_wg, end = min(n, beg + per_wg);
   unsigned run = wg_off[blockIdx.x];
   int par = 0;
   for (int base = beg; base < end; base += CENSUS_THREADS, par ^= 1)      /* (uniform trip count) */
   {
      const int i = base + (int)threadIdx.x;
      double r[3]; int s = 0;
      const bool sel = i < end && subset_selected(sp, b, i, r, s);
      const unsigned long long same = __ballot(sel);
      if (lane == 0) wave_s[par][wave] = (unsigned)__popcll(same);
      __syncthreads();
      unsigned before = 0u, all = 0u;
#pragma unroll
      for (int w = 0; w < CENSUS_WAVES; w++) { const unsigned c = wave_s[par][w]; all += c; if (w < wave) before += c; }
      const unsigned place = run + before + (unsigned)__popcll(same & ((1ull << lane) - 1ull));
      if (sel && place < nrec)      /* (place < nrec whenever the state is the one k_subset_count saw) */
      {
         const int g = min(max(b.group[i], 0), sp.ngroup - 1);
         const unsigned pinfo = b.group_term[g] + b.species_term[s];
         const float f0 = (float)((r[0] - sp.corner[0]) * sp.cL), f1 = (float)((r[1] - sp.corner[1]) * sp.cL), f2 = (float)((r[2] - sp.corner[2]) * sp.cL);
         unsigned long long *o = rec + 3 * (size_t)place;
         o[0] = b.gid[i];
         o[1] = (unsigned long long)pinfo | (unsigned long long)__float_as_uint(f0) << 32;
         o[2] = (unsigned long long)__float_as_uint(f1) | (unsigned long long)__float_as_uint(f2) << 32;
      }
      run += all;
   }
}

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
   const int off[6] = {1, 2, 3, 5, 6, 7};
   for (int k = 0; k < 6; k++)
      if (fabs(ctx->h[off[k]]) > 1e-10) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: only orthorhombic boxes are supported (h[%d]=%g)", fn, off[k], ctx->h[off[k]]);
   if (!(ctx->h[0] > 0.0) || !(ctx->h[4] > 0.0) || !(ctx->h[8] > 0.0)) SETERR(ctx, DDCMI_EINVAL, "%s needs a box (ddcmi_set_box)", fn);
   return DDCMI_OK;
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
   sp.odd = f->odd != 0; sp.pbc = ctx->pbc; sp.nspecies = ns; sp.ngroup = ng;
   for (int a = 0; a < 3; a++)
   {
      sp.lo[a] = f->rmin[a]; sp.hi[a] = f->rmax[a]; sp.vlo[a] = f->vmin[a]; sp.vhi[a] = f->vmax[a];
      sp.L[a] = ctx->h[4 * a]; sp.corner[a] = f->corner[a];
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
   hipLaunchKernelGGL(k_subset_count, dim3(nwg), dim3(CENSUS_THREADS), 0, st, n, per_wg, sp, b, d_cnt);
   hipLaunchKernelGGL(k_subset_scan, dim3(1), dim3(64), 0, st, nwg, d_cnt, d_off);
   HIPCHK(ctx, hipGetLastError());
   unsigned total = 0u;
   HIPCHK(ctx, hipMemcpyAsync(&total, d_off + nwg, sizeof(unsigned), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   *count = (int64_t)total;
   if (!rec) return DDCMI_OK;
   if (cap < (int64_t)total) SETERR(ctx, DDCMI_EINVAL, "ddcmi_subset_records: capacity %lld < %u selected beads", (long long)cap, total);
   if (total == 0u) return DDCMI_OK;
   ENSURE(ctx, ctx->subset_rec, 3 * (size_t)total);
   hipLaunchKernelGGL(k_subset_pack, dim3(nwg), dim3(CENSUS_THREADS), 0, st, n, per_wg, sp, b, d_off, total, ctx->subset_rec.p);
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
/* in-process group: count[r] of every domain; with rec, the domains' records one block behind the other in rank order, cap their sum's
 * room.  The counts of all domains come first, so that a buffer that is too small stays untouched. */
extern "C" int ddcmi_group_subset_records(ddcmi_ctx **ctxs, int n, const ddcmi_subset_filter *f, int64_t cap, ddcmi_subset_record *rec, int64_t *count)
{
   if (ctxs && n >= 1 && ctxs[0] && !ctxs[0]->group_)
      SETERR(ctxs[0], DDCMI_EINVAL, "ddcmi_group_subset_records: not the contexts of an in-process group: use ddcmi_subset_records");
   int rc = analysis_group(ctxs, n, "subset_records", [=](ddcmi_ctx *c, const char *fn) { return subset_check(c, fn, f, cap, rec, count); },
                           [=](ddcmi_ctx *c, size_t r) { return subset_one(c, f, 0, nullptr, count + r); });
   if (rc || !rec) return rc;
   int64_t total = 0;
   for (int r = 0; r < n; r++) total += count[r];
   if (cap < total) SETERR(ctxs[0], DDCMI_EINVAL, "ddcmi_group_subset_records: capacity %lld < %lld selected beads", (long long)cap, (long long)total);
   std::vector<int64_t> off((size_t)n, 0);
   for (int r = 1; r < n; r++) off[r] = off[r - 1] + count[r - 1];
   const int64_t *o = off.data();
   return analysis_group(ctxs, n, "subset_records", [](ddcmi_ctx *, const char *) { return DDCMI_OK; },
                         [=](ddcmi_ctx *c, size_t r) { return subset_one(c, f, count[r], rec + o[r], count + r); });
}

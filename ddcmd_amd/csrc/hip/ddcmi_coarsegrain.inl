/* ddcmi_coarsegrain.inl -- ANALYSIS type COARSEGRAIN on the device (coarsegrain.c:242-448, coarsegrain_eval): the sums {number, mass,
 * K[3], p[3]} of the owned beads per (grid cell, species) on an nx x ny x nz grid of an orthorhombic box, with the reference's optional
 * smearing over the eight cells around a bead, as the non-empty entries in ascending (label, species) order.  Included from ddcmi.hip
 * behind ddcmi_subset.inl.  A census pass (ddcmi_census_frame.inl): read-only, no communication, no floating-point atomics, the same
 * bytes when repeated.  U, virial and the virial tensor of the reference's record are per-atom arrays that the Martini path never
 * fills (docs/history_r1-r3.md, section 7): they are zero there and are not computed here.
 *
 * The key space, up to DDCMI_CG_MAX_KEYS (cell, species) pairs and sparsely occupied, fits no workgroup's LDS, so the census frame's
 * one row per wave does not stretch to it: the pass is a scatter by key, i.e. a stable sort and a segmented reduction.
 *   k_cg_keys        contribution slot * nc + corner (nc = 1, or 8 with smearing; corner = 4 ii + 2 jj + kk, the reference's loop order)
 *                    gets the 32-bit key label * nspecies + species and the value slot * 8 + corner; a corner the reference skips
 *                    (weight < 1e-20) gets the sentinel key, one above every real key.
 *   the sort         a stable LSD radix sort of the (key, value) pairs, 8 bits per pass, ceil(bits(sentinel) / 8) passes.  A pass:
 *                    k_cg_hist (a workgroup's digit counts over its census_split range, integer LDS adds), scan.hip's exclusive scan
 *                    over them in (digit, workgroup) order, k_cg_scatter (a lane's place: the scanned offset + the items of that digit
 *                    in the workgroup's earlier blocks + those in the earlier waves of its block (LDS) + those in the lower lanes
 *                    of its wave -- eight ballots give the lanes that share the digit, a popcount the rank: the ranking of
 *                    the frame's compaction, per digit).  Equal keys keep their order, so a segment lists its contributions
 *                    by ascending slot * 8 + corner.
 *   the segments     an item heads a segment when its key differs from the one before it; the heads go through the frame's
 *                    compaction (CgHeadSel).  The sentinel's items are the last segment: it is not a record.
 *   k_cg_reduce      segment s belongs to lane s % 64 of wave s / 64.  Up to CG_SHORT items: that lane adds them in order, starting
 *                    from +0.  More: the wave takes it, lane l adds items l, l + 64, ... in order, wave_sum_dpp combines the lanes.
 *                    The association is a function of the segment's length alone.  Every item recomputes its eight terms from the
 *                    bead (cg_item, the code that made its key), so that the sort carries 8 bytes per contribution; the lane writes
 *                    the 80-byte record.
 * Every term is a rounded product (zd_rounded keeps the back end from fusing it into the addition), in the reference's operations:
 * weight = (wx wy) wz, m, 0.5 m (v v) and m v times the weight.  The position is the one a download returns (census_coord);
 * r = x (n / L) - corner (n / L); the cells are the reference's ((int)r, or floor(r + 0.5) - 1 and floor(r + 0.5) with -1 -> n - 1
 * and n -> 0 on every axis, open ones too), then clamped into [0, n): a bead on the upper face, one the wrap leaves at L / 2, a NaN
 * (cell 0, as pc_axis). */

#define CG_SORT_MAX_WG 2048      /* workgroups of a sort pass: 256 counters each for the scan */
#define CG_SHORT 16              /* a segment of up to this many contributions is one lane's */
static_assert(CENSUS_THREADS == 256, "a sort pass has one thread per digit value");

struct CgParms
{
   int n[3], ns, pbc, smear, method, nc;      /* method: 0 impulse, 1 hat; nc: contributions per bead */
   unsigned sentinel;                         /* nx ny nz ns */
   double L[3], deltai[3], scaled_corner[3], half[3], inv[3];      /* coarsegrain.c:264-291, formed on the host */
};
struct CgBeads { const double4 *pos; const double *vx, *vy, *vz, *massv; const int *species; };

/* axis a: the cell and the weight of the lower (c = 0) or the upper (c = 1) of the two cells; without smearing the one cell, weight 1 */
__device__ __forceinline__ void cg_axis(const CgParms &cp, int a, double x, int c, int &ig, double &w)
{
   const int n = cp.n[a];
   const double r = zd_rounded(census_coord(cp, a, x) * cp.deltai[a]) - cp.scaled_corner[a];
   if (!cp.smear) { ig = zd_int(r); w = 1.0; }
   else
   {
      const double fl = floor(r + 0.5);
      double delta = fl - r;
      delta = delta < cp.half[a] ? delta : cp.half[a];
      delta = delta > -cp.half[a] ? delta : -cp.half[a];
      const int iw = zd_int(fl);
      double w0;
      if (cp.method == 1)
      {
         const double p = (2 * delta) * cp.inv[a], q = zd_rounded(fabs(delta) * cp.inv[a]), s = 1.0 - q, d = zd_rounded(p * s);
         w0 = 0.5 + d;
      }
      else w0 = 0.5 + zd_rounded(delta * cp.inv[a]);
      if (c == 0) { ig = iw - 1; if (ig == -1) ig = n - 1; w = w0; }
      else { ig = iw; if (ig == n) ig = 0; w = 1.0 - w0; }
   }
   ig = min(max(ig, 0), n - 1);
}
/* contribution `corner` of bead `slot`: its key, and whether the reference counts it */
__device__ __forceinline__ bool cg_key_of(const CgParms &cp, const CgBeads &b, int slot, int corner, unsigned &key, double &weight)
{
   const double4 p = b.pos[slot];
   int ix, iy, iz;
   double wx, wy, wz;
   cg_axis(cp, 0, p.x, corner >> 2 & 1, ix, wx);
   cg_axis(cp, 1, p.y, corner >> 1 & 1, iy, wy);
   cg_axis(cp, 2, p.z, corner & 1, iz, wz);
   weight = zd_rounded(wx * wy) * wz;
   const int s = min(max(b.species[slot], 0), cp.ns - 1);      /* (checked at the upload) */
   key = (unsigned)(iz + cp.n[2] * (iy + cp.n[1] * ix)) * (unsigned)cp.ns + (unsigned)s;      /* below sentinel <= 2^28 */
   return !(weight < 1e-20);
}
/* the eight terms of a counted contribution: weight times {1, m, Kx, Ky, Kz, px, py, pz} */
__device__ __forceinline__ void cg_item(const CgParms &cp, const CgBeads &b, int nloc, unsigned val, double (&v)[8])
{
   const int slot = min((int)(val >> 3), nloc - 1), corner = (int)(val & 7u);
   unsigned key;
   double w;
   (void)cg_key_of(cp, b, slot, corner, key, w);
   const int s = min(max(b.species[slot], 0), cp.ns - 1);
   const double m = b.massv[s], vx = b.vx[slot], vy = b.vy[slot], vz = b.vz[slot], hm = 0.5 * m;
   v[0] = w;
   v[1] = zd_rounded(w * m);
   v[2] = zd_rounded(w * zd_rounded(hm * zd_rounded(vx * vx)));
   v[3] = zd_rounded(w * zd_rounded(hm * zd_rounded(vy * vy)));
   v[4] = zd_rounded(w * zd_rounded(hm * zd_rounded(vz * vz)));
   v[5] = zd_rounded(w * zd_rounded(m * vx));
   v[6] = zd_rounded(w * zd_rounded(m * vy));
   v[7] = zd_rounded(w * zd_rounded(m * vz));
}

__global__ __launch_bounds__(CENSUS_THREADS) void k_cg_keys(int m, CgParms cp, CgBeads b, unsigned *__restrict__ key, unsigned *__restrict__ val)
{
   const int i = blockIdx.x * CENSUS_THREADS + threadIdx.x;
   if (i >= m) return;
   const int slot = i / cp.nc, corner = i - slot * cp.nc;
   unsigned k;
   double w;
   const bool counted = cg_key_of(cp, b, slot, corner, k, w);
   key[i] = counted ? k : cp.sentinel;
   val[i] = (unsigned)slot * 8u + (unsigned)corner;
}
/* hist[d][workgroup]: the items of the workgroup's range whose digit is d */
__global__ __launch_bounds__(CENSUS_THREADS) void k_cg_hist(int m, int per_wg, int shift, const unsigned *__restrict__ key, int *__restrict__ hist)
{
   __shared__ unsigned h_s[256];
   h_s[threadIdx.x] = 0u;
   __syncthreads();
   const int beg = blockIdx.x * per_wg, end = min(m, beg + per_wg);
   for (int i = beg + (int)threadIdx.x; i < end; i += CENSUS_THREADS) atomicAdd(&h_s[key[i] >> shift & 255u], 1u);      /* (integers: any order) */
   __syncthreads();
   hist[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (int)h_s[threadIdx.x];
}
/* off: the exclusive scan of hist.  An item goes behind every item of a lower digit, behind the items of its digit in earlier
 * workgroups, earlier blocks, earlier waves and lower lanes: stable */
__global__ __launch_bounds__(CENSUS_THREADS) void k_cg_scatter(int m, int per_wg, int shift, const unsigned *__restrict__ key, const unsigned *__restrict__ val,
                                                               const int *__restrict__ off, unsigned *__restrict__ key_out, unsigned *__restrict__ val_out)
{
   __shared__ unsigned base_s[256], wcnt_s[CENSUS_WAVES][256];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   base_s[threadIdx.x] = (unsigned)off[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
#pragma unroll
   for (int w = 0; w < CENSUS_WAVES; w++) wcnt_s[w][threadIdx.x] = 0u;
   __syncthreads();
   const int beg = blockIdx.x * per_wg, end = min(m, beg + per_wg);
   for (int base = beg; base < end; base += CENSUS_THREADS)      /* (uniform trip count: every lane reaches the ballots and the barriers) */
   {
      const int i = base + (int)threadIdx.x;
      const bool have = i < end;
      const unsigned k = have ? key[i] : 0u, v = have ? val[i] : 0u, d = k >> shift & 255u;
      unsigned long long same = __ballot(have);      /* the lanes with an item whose digit is this lane's */
#pragma unroll
      for (int q = 0; q < 8; q++)
      {
         const unsigned long long bal = __ballot(d >> q & 1u);
         same &= (d >> q & 1u) ? bal : ~bal;
      }
      const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
      if (have && rank == 0u) wcnt_s[wave][d] = (unsigned)__popcll(same);      /* (one writer per wave and digit) */
      __syncthreads();
      if (have)
      {
         unsigned place = base_s[d] + rank;
#pragma unroll
         for (int w = 0; w < CENSUS_WAVES; w++) if (w < wave) place += wcnt_s[w][d];
         if (place < (unsigned)m) { key_out[place] = k; val_out[place] = v; }      /* (place < m whenever hist counted these keys) */
      }
      __syncthreads();
      unsigned t = 0u;
#pragma unroll
      for (int w = 0; w < CENSUS_WAVES; w++) { t += wcnt_s[w][threadIdx.x]; wcnt_s[w][threadIdx.x] = 0u; }
      base_s[threadIdx.x] += t;
      __syncthreads();
   }
}
/* the compaction's functor (k_compact_count, k_compact_pack): item i of the sorted keys heads a segment; seg[place] = the head's
 * index, and item 0, always a head, leaves seg[nseg] = m, the end of the last segment */
struct CgHeadSel
{
   const unsigned *key; unsigned *seg; unsigned nseg, m;
   struct Item {};
   __device__ __forceinline__ bool selected(int i, Item &) const { return i == 0 || key[i] != key[i - 1]; }
   __device__ __forceinline__ void store(int i, unsigned place, const Item &) const
   {
      seg[place] = (unsigned)i;
      if (i == 0) seg[nseg] = m;
   }
};
/* rec: nrec records of ten 8-byte words {label, species, n, mass, K[3], p[3]}; seg[nrec] is the end of the last record's segment */
__global__ __launch_bounds__(CENSUS_THREADS) void k_cg_reduce(int nrec, int nloc, CgParms cp, CgBeads b, const unsigned *__restrict__ key, const unsigned *__restrict__ val,
                                                              const unsigned *__restrict__ seg, unsigned long long *__restrict__ rec)
{
   const int lane = threadIdx.x & 63;
   const int s = (blockIdx.x * CENSUS_WAVES + (int)(threadIdx.x >> 6)) * 64 + lane;
   const bool have = s < nrec;
   const unsigned beg = have ? seg[s] : 0u, end = have ? seg[s + 1] : 0u;
   const bool lng = have && end - beg > (unsigned)CG_SHORT;
   double acc[8], v[8];
#pragma unroll
   for (int q = 0; q < 8; q++) acc[q] = 0.0;
   if (have && !lng)
      for (unsigned i = beg; i < end; i++)
      {
         cg_item(cp, b, nloc, val[i], v);
#pragma unroll
         for (int q = 0; q < 8; q++) acc[q] += v[q];
      }
   for (unsigned long long pending = __ballot(lng); pending; pending &= pending - 1ull)      /* (uniform: every lane reaches the wave's sums) */
   {
      const int lead = __ffsll((long long)pending) - 1;
      const unsigned lb = __shfl(beg, lead, 64), le = __shfl(end, lead, 64);
      double t[8];
#pragma unroll
      for (int q = 0; q < 8; q++) t[q] = 0.0;
      for (unsigned i = lb + (unsigned)lane; i < le; i += 64u)
      {
         cg_item(cp, b, nloc, val[i], v);
#pragma unroll
         for (int q = 0; q < 8; q++) t[q] += v[q];
      }
#pragma unroll
      for (int q = 0; q < 8; q++) t[q] = wave_sum_dpp(t[q]);
      if (lane == lead)
      {
#pragma unroll
         for (int q = 0; q < 8; q++) acc[q] = t[q];
      }
   }
   if (!have) return;
   const unsigned k = key[beg];
   unsigned long long *o = rec + 10 * (size_t)s;
   o[0] = (unsigned long long)(k / (unsigned)cp.ns);
   o[1] = (unsigned long long)(k % (unsigned)cp.ns);
#pragma unroll
   for (int q = 0; q < 8; q++) o[2 + q] = (unsigned long long)__double_as_longlong(acc[q]);
}

/* ---- host side ---------------------------------------------------------- */
static_assert(sizeof(ddcmi_cg_record) == 80, "a coarse-grain record is 80 bytes");
struct CgReq { int n[3], nspecies; double smear_radius; int smear_method; };
static int cg_check(ddcmi_ctx *ctx, const char *fn, const CgReq &q, int64_t cap, const void *rec, const void *count)
{
   int rc = census_state_check(ctx, fn);
   if (rc) return rc;
   ARGCHK(ctx, !count, "%s: NULL count", fn);
   ARGCHK(ctx, rec && cap < 0, "%s: cap = %lld", fn, (long long)cap);
   ARGCHK(ctx, q.n[0] < 1 || q.n[1] < 1 || q.n[2] < 1, "%s: nx = %d, ny = %d, nz = %d: each must be at least 1", fn, q.n[0], q.n[1], q.n[2]);
   ARGCHK(ctx, ctx->nspecies < 1, "%s needs the species (ddcmi_set_species)", fn);
   ARGCHK(ctx, q.nspecies != ctx->nspecies, "%s: nspecies = %d, the context has %d species", fn, q.nspecies, ctx->nspecies);
   ARGCHK(ctx, q.smear_method != 0 && q.smear_method != 1, "%s: smear_method = %d (0 impulse, 1 hat)", fn, q.smear_method);
   ARGCHK(ctx, !std::isfinite(q.smear_radius), "%s: smear_radius = %g", fn, q.smear_radius);
   if ((rc = census_box_check(ctx, fn, 7, true))) return rc;
   const double nkeys = (double)q.n[0] * q.n[1] * q.n[2] * q.nspecies;
   if (nkeys > (double)DDCMI_CG_MAX_KEYS)
      SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d x %d x %d cells x %d species = %.0f keys, at most %d", fn, q.n[0], q.n[1], q.n[2], q.nspecies, nkeys, DDCMI_CG_MAX_KEYS);
   if ((long long)ctx->nloc * 8 >= (1ll << 31)) SETERR(ctx, DDCMI_EUNSUPPORTED, "%s: %d beads on one rank, fewer than 2^28", fn, ctx->nloc);
   return DDCMI_OK;
}
/* this rank's count and, with rec, its records [sync] */
static int cg_one(ddcmi_ctx *ctx, const CgReq &q, int64_t cap, ddcmi_cg_record *rec, int64_t *count)
{
   (void)hipSetDevice(ctx->device);
   hipStream_t st = ctx->stream;
   const int n = ctx->nloc;
   *count = 0;
   if (n <= 0) return DDCMI_OK;      /* (a domain that holds no bead) */
   CgParms cp;
   cp.ns = q.nspecies; census_set_box(ctx, cp); cp.smear = q.smear_radius > 0.0; cp.method = q.smear_method; cp.nc = cp.smear ? 8 : 1;
   cp.sentinel = (unsigned)q.n[0] * (unsigned)q.n[1] * (unsigned)q.n[2] * (unsigned)q.nspecies;
   for (int a = 0; a < 3; a++)
   {
      const double L = ctx->h[4 * a], corner = L * -0.5;      /* box->corner = h0 * reducedcorner, reducedcorner = -0.5 on this path */
      cp.n[a] = q.n[a];
      cp.deltai[a] = q.n[a] / L;
      cp.scaled_corner[a] = corner * cp.deltai[a];
      cp.half[a] = cp.inv[a] = 0.0;
      if (cp.smear)
      {
         const double s2 = 2.0 * q.smear_radius, cell = L / (1.0 * q.n[a]), lSmear = s2 < cell ? s2 : cell;
         cp.inv[a] = 1.0 / lSmear; cp.half[a] = 0.5 * lSmear;
      }
   }
   const int m = n * cp.nc;
   int bits = 0;
   while (bits < 32 && (cp.sentinel >> bits) != 0u) bits++;      /* the sentinel is the largest key */
   const int npass = (bits + 7) / 8;
   int per_wg, nwg;
   census_split(m, CG_SORT_MAX_WG, &per_wg, &nwg);
   /* cg_key, cg_val: two arrays of m each, the pass's source and its destination; cg_hist: hist[256][nwg] | off[256][nwg];
    * cg_cnt: wg_count[nwg] | wg_off[nwg + 1] */
   ENSURE(ctx, ctx->cg_key, 2 * (size_t)m);
   ENSURE(ctx, ctx->cg_val, 2 * (size_t)m);
   ENSURE(ctx, ctx->cg_hist, 2 * 256 * (size_t)nwg);
   ENSURE(ctx, ctx->cg_cnt, 2 * (size_t)nwg + 1);
   unsigned *key[2] = {ctx->cg_key.p, ctx->cg_key.p + m}, *val[2] = {ctx->cg_val.p, ctx->cg_val.p + m};
   int *d_hist = ctx->cg_hist.p, *d_off = d_hist + 256 * (size_t)nwg;
   unsigned *d_cnt = ctx->cg_cnt.p, *d_wgoff = d_cnt + nwg;
   const CgBeads b = {ctx->pos.p, ctx->vx.p, ctx->vy.p, ctx->vz.p, ctx->d_mass.p, ctx->species.p};
   hipLaunchKernelGGL(k_cg_keys, dim3(cdiv(m, CENSUS_THREADS)), dim3(CENSUS_THREADS), 0, st, m, cp, b, key[0], val[0]);
   int cur = 0;
   for (int p = 0; p < npass; p++, cur ^= 1)
   {
      hipLaunchKernelGGL(k_cg_hist, dim3(nwg), dim3(CENSUS_THREADS), 0, st, m, per_wg, 8 * p, key[cur], d_hist);
      int rc = ddcmi_scan_exclusive(ctx, d_hist, d_off, 256 * nwg, nullptr);
      if (rc) return rc;
      hipLaunchKernelGGL(k_cg_scatter, dim3(nwg), dim3(CENSUS_THREADS), 0, st, m, per_wg, 8 * p, key[cur], val[cur], d_off, key[cur ^ 1], val[cur ^ 1]);
   }
   CgHeadSel heads = {key[cur], nullptr, 0u, (unsigned)m};
   compact_count(st, m, per_wg, nwg, heads, d_cnt, d_wgoff);
   HIPCHK(ctx, hipGetLastError());
   unsigned nseg = 0u, last = 0u;
   HIPCHK(ctx, hipMemcpyAsync(&nseg, d_wgoff + nwg, sizeof(unsigned), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipMemcpyAsync(&last, key[cur] + (m - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   const unsigned nrec = nseg - (last == cp.sentinel ? 1u : 0u);      /* the skipped corners are the last segment */
   *count = (int64_t)nrec;
   if (!rec) return DDCMI_OK;
   if (cap < (int64_t)nrec) SETERR(ctx, DDCMI_EINVAL, "ddcmi_coarsegrain: capacity %lld < %u entries", (long long)cap, nrec);
   if (nrec == 0u) return DDCMI_OK;
   ENSURE(ctx, ctx->cg_seg, (size_t)nseg + 1);
   ENSURE(ctx, ctx->cg_rec, 10 * (size_t)nrec);
   heads.seg = ctx->cg_seg.p; heads.nseg = nseg;
   compact_pack(st, m, per_wg, nwg, heads, d_wgoff, nseg);
   hipLaunchKernelGGL(k_cg_reduce, dim3(cdiv((long)nrec, CENSUS_THREADS)), dim3(CENSUS_THREADS), 0, st, (int)nrec, n, cp, b, key[cur], val[cur], ctx->cg_seg.p, ctx->cg_rec.p);
   HIPCHK(ctx, hipGetLastError());
   HIPCHK(ctx, hipMemcpyAsync(rec, ctx->cg_rec.p, sizeof(ddcmi_cg_record) * (size_t)nrec, hipMemcpyDeviceToHost, st));
   HIPCHK(ctx, hipStreamSynchronize(st));
   return DDCMI_OK;
}

extern "C" int ddcmi_coarsegrain(ddcmi_ctx *ctx, int nx, int ny, int nz, int nspecies, double smear_radius, int smear_method, int64_t cap, ddcmi_cg_record *rec,
                                 int64_t *count)
{
   const CgReq q = {{nx, ny, nz}, nspecies, smear_radius, smear_method};
   return analysis_single(ctx, "coarsegrain", true, [=](ddcmi_ctx *c, const char *fn) { return cg_check(c, fn, q, cap, rec, count); },
                          [=](ddcmi_ctx *c) { return cg_one(c, q, cap, rec, count); });
}
/* in-process group (analysis_group_records): count[r] of every domain; with rec, the domains' records in rank order, cap their sum's room */
extern "C" int ddcmi_group_coarsegrain(ddcmi_ctx **ctxs, int n, int nx, int ny, int nz, int nspecies, double smear_radius, int smear_method, int64_t cap,
                                       ddcmi_cg_record *rec, int64_t *count)
{
   const CgReq q = {{nx, ny, nz}, nspecies, smear_radius, smear_method};
   return analysis_group_records(ctxs, n, "coarsegrain", "entries", [=](ddcmi_ctx *c, const char *fn) { return cg_check(c, fn, q, cap, rec, count); },
                                 [=](ddcmi_ctx *c, size_t r) { return cg_one(c, q, 0, nullptr, count + r); }, rec != nullptr, cap, count,
                                 [=](ddcmi_ctx *c, size_t r, int64_t off) { return cg_one(c, q, count[r], rec + off, count + r); });
}

/* ddcmi_test.h -- TEST-ONLY entry points of the device code.  NOT part of the drop-in boundary: libddcmi.so (what a ddcMD
 * maintainer links with -lddcmi) exports include/ddcmi.h and nothing else.  The functions below are exported by a second link
 * of the very same objects, libddcmi_test.so (ddcmd_amd/csrc/Makefile: same kernels, wider version script), which only
 * tests/ and tools/ load:
 *   ddcmi_group_*              in-process emulation of a px*py*pz decomposition on ONE GPU (the multi-domain path without RCCL)
 *   ddcmi_plan_*               the host logic of the halo exchange / domain directions, callable without a GPU (world-2 CPU tests)
 *   ddcmi_debug_branch_census  which rarely taken dihedral branches a test's geometry drives
 *   ddcmi_debug_bonded_layout  what the bonded kernels' lane layout decided for a test's term lists
 *   ddcmi_debug_step_plan      which path a context's force evaluations took (halo mode, fused, lean, LDS layout, reduction launch)
 *   ddcmi_debug_tile_items     the work items the pair kernel was launched with (tiles, row parts) and the owned beads of their tiles
 *   ddcmi_debug_wave_reduce    the transposed wave reduction of several sums against the one-sum reduction, on the test's own numbers
 *   ddcmi_debug_recip          the four reciprocal routines and the two bare double-precision seeds, on the test's own numbers
 *   ddcmi_debug_wave_ops       the wave's prefix sum, maximum and row sum and the decaying maximum of the lean steps' words, every lane's result
 *   ddcmi_debug_scan           the exclusive prefix sum of the rebuild on a context's stream and scratch array
 *   ddcmi_debug_sort_cells     the two in-cell sorts on the test's own cells and keys
 *   ddcmi_debug_thermalize_rejects  the rejected draws of every bead's BOLTZMANN stream
 *   ddcmi_debug_reduce_* / _block_reduce / _census_final / _kinetic_finish / _mol_sum  the cross-workgroup reductions on the test's own rows */
#ifndef DDCMI_TEST_H
#define DDCMI_TEST_H
#include "ddcmi.h"
#ifdef __cplusplus
extern "C" {
#endif
/* census of the rarely taken branches of the dihedral code since the last reset (bioCharmmCovalentEnergiesSorted.c:649-683,
 * 793-810): [0] torsion series (|sin phi| <= 1e-8), of these [1] delta < 1 deg, [2] delta > 179 deg, [3] any other delta;
 * [4] improper series; [5] improper difference wrapped by 2 pi; [6] cos phi clamped.  Counted per evaluation (a term is
 * evaluated once per atom it has).  Test aid: shows that a test's geometry really drives those branches. [sync] */
int ddcmi_debug_branch_census(unsigned long long out[8], int reset);
/* census of the lane layout ddcmi_set_bonded / ddcmi_set_bonded_gid made of the term lists, out[0] the light launch (bonds, func 2/10 angles), out[1] the
 * heavy one (func-1 angles, dihedrals): [0] lanes, [1] of these filler lanes (in front of a molecule's run that would straddle two workgroups), [2] row
 * patterns, [3] 16-byte pieces of the launch's table (at most 384: copied to LDS), [4] [5] distinct parameter sets of its two term kinds, [6] atoms'
 * lanes with the near bit (every partner a lane of the same workgroup at the distance of the atom numbers), waves of 64 lanes that hold an atom's
 * lane and [7] are all near (the wave reads its partners' records unasked) / [8] hold near and far atoms' lanes / [9] hold no near one, [10] whether
 * the context's last launch took the instantiation with the table in LDS (-1: none launched yet; DDCMI_NO_BONDED_LDS_TABLES=1 at ddcmi_create: never),
 * [11] 0.  Host numbers, kept where the tables are made: no device counter.  Test aid: shows that a test's molecules really drive each path. */
int ddcmi_debug_bonded_layout(ddcmi_ctx *ctx, int out[2][12]);
/* Host logic of the halo exchange (ddcSendRecvTables, ddcSendRecv.c:126-225), callable without a GPU.
 * ddcmi_plan_recv_counts: from the all-gathered per-direction send counts all_counts[nranks][27], what
 * this rank receives: recv_cnt[c] = what the rank in my direction opp(c) sends along ITS direction c.
 * ddcmi_plan_halo_layout: buffer layout (in beads) and message list of the per-step exchange -- remote
 * segments ordered by (peer rank, direction code) on both sides, so that each peer pair exchanges ONE
 * message: send_off/recv_off[28] = offset of direction c's segment (send: my direction; receive: the
 * SENDER's direction); msgs[0] = number of send messages, then {peer, offset, count} triples;
 * msgr likewise for the receives (room for 1 + 3*27 ints each).  loopback != 0: a single rank whose
 * periodic neighbours are itself exchanges with itself through the transport (test facility). */
int ddcmi_plan_recv_counts(int px, int py, int pz, int rank, int pbc, int loopback, const int *all_counts, int *recv_cnt);
int ddcmi_plan_halo_layout(int px, int py, int pz, int rank, int pbc, int loopback, const int send_cnt[27], const int recv_cnt[27],
                           int send_off[28], int recv_off[28], int *msgs, int *msgr);
/* host logic of the decomposition (domain.c:61-208 for a cubic lattice of domain
 * centres): destination rank and periodic shift of the 26 neighbour directions,
 * code = (dx+1)+3(dy+1)+9(dz+1); dest[27], shift[27*3]; dest = -1 where the box is open */
int ddcmi_plan_directions(int px, int py, int pz, int rank, int pbc, int *dest, int *shift);
/* in-process emulation of a px*py*pz decomposition (several contexts on one
 * device, halo/migration traffic by device copies): lets the whole multi-domain
 * path run on a single GPU.  Contexts of a group are driven only through these. */
int ddcmi_group_create(ddcmi_ctx **ctxs, int n, int px, int py, int pz);
int ddcmi_group_destroy(ddcmi_ctx **ctxs, int n);
int ddcmi_group_eval_forces(ddcmi_ctx **ctxs, int n);
int ddcmi_group_step_nglf(ddcmi_ctx **ctxs, int n, double dt, int nsteps);
/* ddcmi_group_temperatures for an in-process group (sums over its domains) */
int ddcmi_group_temperatures_all(ddcmi_ctx **ctxs, int n, double *Tgroup);
/* ddcmi_pair_correlation for an in-process group: every domain's own result, domain after domain -- counts[r*ncombo*nbins ...],
 * nbeads[r*nspecies ...] for domain r */
int ddcmi_group_pair_correlation(ddcmi_ctx **ctxs, int n, double rmin, double delta_r, int nbins, int log_scale, int nspecies,
                                 int64_t *counts, int64_t *nbeads);
/* ddcmi_vaf_origin / ddcmi_vaf_sample / ddcmi_vaf_clear for an in-process group: the origin (the clear) on every domain; every
 * domain's own sums, domain after domain -- vaf[r*nclass ...], msd[r*nclass ...] for domain r, nclass = 1 + ngroup + nspecies */
int ddcmi_group_vaf_origin(ddcmi_ctx **ctxs, int n);
int ddcmi_group_vaf_clear(ddcmi_ctx **ctxs, int n);
int ddcmi_group_vaf_sample(ddcmi_ctx **ctxs, int n, int ngroup, int nspecies, double *vaf, double *msd);
/* ddcmi_momentum_by_class / ddcmi_zdensity for an in-process group: every domain's own result, domain after domain --
 * mv[r*3*nclass ...], m[r*nclass ...] and density[r*nz ...] for domain r */
int ddcmi_group_momentum_by_class(ddcmi_ctx **ctxs, int n, int ngroup, int nspecies, double *mv, double *m);
int ddcmi_group_zdensity(ddcmi_ctx **ctxs, int n, int nz, double smear_radius, int smear_method, double *density);
/* ddcmi_kinetic_energy_distn for an in-process group: every domain's own result, domain after domain -- counts[r*nbt ...] (nbt the
 * sum of nbins), tallies[r*3*ndist ...], stats[r*3*ndist ...] for domain r */
int ddcmi_group_kinetic_energy_distn(ddcmi_ctx **ctxs, int n, int nspecies, int ndist, const double *emin, const double *emax, const int *nbins,
                                     const int *species_dist, int64_t *counts, int64_t *tallies, double *stats);
/* ddcmi_charge_density_modes for an in-process group: every domain's own result, domain after domain -- rho[r*6*mmax ...], count[r]
 * for domain r */
int ddcmi_group_charge_density_modes(ddcmi_ctx **ctxs, int n, int nspecies, const int *select, int mmax, double *rho, int64_t *count);
/* ddcmi_structure_modes for an in-process group: every domain's own result, domain after domain -- rho[r*2*nk ...], count[r] for
 * domain r */
int ddcmi_group_structure_modes(ddcmi_ctx **ctxs, int n, int nspecies, const int *select, int weight, int nk, const int32_t *kvec, double *rho,
                                int64_t *count);
/* ddcmi_subset_records for an in-process group: count[r] of every domain r; with rec, the domains' records one block behind the
 * other in rank order, cap the room for all of them (too small: DDCMI_EINVAL, the counts set, rec untouched) */
int ddcmi_group_subset_records(ddcmi_ctx **ctxs, int n, const ddcmi_subset_filter *filter, int64_t cap, ddcmi_subset_record *rec, int64_t *count);
/* ddcmi_coarsegrain for an in-process group: count[r] of every domain r; with rec, the domains' records one block behind the other in
 * rank order, cap the room for all of them (too small: DDCMI_EINVAL, the counts set, rec untouched) */
int ddcmi_group_coarsegrain(ddcmi_ctx **ctxs, int n, int nx, int ny, int nz, int nspecies, double smear_radius, int smear_method, int64_t cap,
                            ddcmi_cg_record *rec, int64_t *count);
/* ddcmi_chol_offsets for an in-process group: every domain's own result, domain after domain -- counts[r*2*nbins ...], ndone[r],
 * stats[r*6 ...], nfrag[r] for domain r; with frag, the domains' fragments one block behind the other in rank order, cap the room
 * for all of them (too small: DDCMI_EINVAL, everything else set, frag untouched) */
int ddcmi_group_chol_offsets(ddcmi_ctx **ctxs, int n, int64_t nmol, const uint64_t *gid, double rmin, double delta, int nbins, int64_t *counts,
                             int64_t *ndone, double *stats, int64_t cap, ddcmi_chol_fragment *frag, int64_t *nfrag);
/* ddcmi_thermalize for an in-process group: every domain's own beads; RESCALE adds the domains' sums in rank order */
int ddcmi_group_thermalize(ddcmi_ctx **ctxs, int n, int method, int select, int ntemp, const double *temperature, uint64_t seed, int64_t loop, int keep_vcm);
/* what ddcmi_thermalize's BOLTZMANN would do with this context's owned beads, without writing a velocity: in the order of
 * ddcmi_download_particles gid[k] and rejects[k], the draws the bead's three gasdev0 calls rejected (-1: its class has T < 0 and is left
 * alone); *nout = the owned beads, cap the room (too small: DDCMI_EINVAL with *nout set).  The very kernel of the product. [sync] */
int ddcmi_debug_thermalize_rejects(ddcmi_ctx *ctx, int select, int ntemp, const double *temperature, uint64_t seed, int64_t loop, int cap, int *nout,
                                   uint64_t *gid, int *rejects);
/* the lean step (a single domain of FREE beads without bonded terms: one launch per step, the second stage of its energy / virial /
 * kinetic sums formed for all pending steps at once): the sums of the steps of the last such launch, 32 doubles per step --
 * {lj, ele, virial xx yy zz xy xz yz} as the full list counts them (twice), {rk, tion xx yy zz xy xz yz}, 0, the bonded kernels'
 * {e_bond, e_angle, e_tors, e_impr, virial xx yy zz xy xz yz}, zeros.  Forms what is pending first.  sums: room for 32 steps. */
int ddcmi_debug_lean_history(ddcmi_ctx *ctx, int *nsteps, double *sums);
/* the plan of a force evaluation the context ran (one per ddcmi_eval_forces and per step).  out[0] on entry: which one, counted back from
 * the last (0; at most 15, and no more than the context has run: else DDCMI_EINVAL) -- only the last step of a ddcmi_step_nglf call knows
 * that no step follows and never fuses, so the steps that show the steady path lie behind it.  On return:
 * [0] how the halo reached the pair kernel: 0 nothing to refresh, 1 periodic images staged from their owners, 2 exchange + update launch,
 * 3 exchange alone, received beads staged from the receive buffer, 4 exchange + update launch on the second stream, 5 update launch alone
 * (a single domain's images; a domain of an in-process group, whose driver exchanged); [1] the integrator's pass rode in the pair kernel;
 * [2] the step was lean; [3] pair table in two levels; [4] fixed LDS layout ([3] [4]: 0 where no pair kernel ran); [5] the reduction launch
 * behind a fused launch that was not lean: 1 alone, 2 with the periodic images, 3 with the next exchange's messages (0: none of these);
 * [6] the update launch measured the received beads' displacement; [7] received beads are read from the receive buffer.  Host numbers. */
int ddcmi_debug_step_plan(ddcmi_ctx *ctx, int out[8]);
/* the displacement bound of the shell-limited walk: the word the reduction launches add to, and the lean steps' words since the rebuild (largest |v|^2 of each; ring[32]) */
int ddcmi_debug_disp(ddcmi_ctx *ctx, double *disp, float *ring, int *nring);
/* census of the pair kernel's work items after a list build, in launch order: item[q] = tile | part << 24 | (nparts - 1) << 27 as k_nonbond reads it
 * (a whole tile: part 0 of 1), nown[q] = owned beads of that tile; *nitems = their number.  Part p of n walks the rows [nown p / n, nown (p + 1) / n)
 * of the tile; how many lanes then share a bead's row follows from that count alone (tests/pair_split_systems.py restates it).  cap < *nitems:
 * DDCMI_EINVAL with *nitems set and the arrays untouched.  Host numbers (the schedule as it left for the device, the cell table): no device
 * counter.  Test aid: shows which lane splits and row parts a test's tiles really drive; DDCMI_DEBUG_HOOKS=1 DDCMI_DEBUG_TAIL=k at ddcmi_create
 * (k = 1, 2, 3, 4, 6, 8; anything else is refused there) cuts the last min(n, 1024 / k) tiles of each of the eight runs into k parts. [sync] */
int ddcmi_debug_tile_items(ddcmi_ctx *ctx, int cap, int *nitems, int *item, int *nown);

/* the wave reductions of the pair kernel's epilogue against each other, on the current device: nsets sets of in[64][n] doubles (lane-major, 1 <= n <= 16,
 * nsets <= 65535), one 64-thread workgroup each; single[set][k] = wave_sum_dpp of column k, multi[set][k] = what wave_sum_multi_dpp<n> of all
 * columns hands lane k.  The two must agree bit for bit. [sync] */
int ddcmi_debug_wave_reduce(int n, int nsets, const double *in, double *single, double *multi);

/* the device primitives the kernels share, each on the caller's numbers and on the current device (tests/test_gpu_device_primitives.py).  Arguments
 * out of range: DDCMI_EINVAL. [sync]
 * ddcmi_debug_recip: out[i] = f(in[i]), one thread per element, 1 <= n <= 2^24; which = 0 rsqrt_f64, 1 rcp_f64 (single-precision seed, two
 * Newton steps: the bonded kernels'), 2 rsqrt_f64_pair, 3 rcp_f64_pair (double-precision seed, one step: the pair kernel's), 4 the bare seed
 * v_rsq_f64, 5 the bare seed v_rcp_f64. */
int ddcmi_debug_recip(int which, int n, const double *in, double *out);
/* ddcmi_debug_wave_ops: nsets sets of 64 values (nsets <= 65535), one 64-thread workgroup each, out[set][lane] = what the lane got; which = 0
 * wave_scan_inclusive_dpp (int32), 1 wave_max_dpp (int32 >= 0), 2 row_sum_dpp (double), 3 lean_effective (float, the lane its own index). */
int ddcmi_debug_wave_ops(int which, int nsets, const void *in, void *out);
/* ddcmi_debug_scan: ddcmi_scan_exclusive of in[n] on the context's stream with the context's scratch array; the context needs no beads.  in_place != 0:
 * source and destination are one device array.  total == NULL: the scan is given no word for its total.  out has room for n +
 * DDCMI_DEBUG_SCAN_GUARD ints (n <= 0: for the guard alone): the device destination is that long, starts as the caller's out[] and comes back whole, so
 * that out[] shows what the scan left alone -- everything where n <= 0 (then *total = 0), the guard behind element n otherwise.  n <= 2^28. */
#define DDCMI_DEBUG_SCAN_GUARD 2048
int ddcmi_debug_scan(ddcmi_ctx *ctx, int n, const int *in, int *out, int *total, int in_place);
/* ddcmi_debug_sort_cells: the in-cell sort of the rebuild on order[norder]: cell c is order[start[c] ... start[c] + cnt[c]) (cells do not overlap;
 * a cell outside order[]: DDCMI_EINVAL).  key == NULL: k_sort_cells, ascending entries.  Otherwise k_sort_cells_key: the entries index key[norder]
 * (unsigned) and key2[norder] (may be NULL), ascending (key, key2, entry); an entry of a cell outside [0, norder): DDCMI_EINVAL.  What lies
 * between the cells is left alone.  ncell <= 2^20, norder <= 2^24. */
int ddcmi_debug_sort_cells(int ncell, const int *start, const int *cnt, int norder, int *order, const uint64_t *key, const int *key2);
/* ddcmi_debug_compact: the stable compaction the record-writing analyses share (count, scan, pack over the ranges of census_split(n, max_wg),
 * max_wg <= 2048) on flags[n]: places[k] = the index of the k-th non-zero flag for k < nrec, *total = their number.  places has room for nrec +
 * DDCMI_DEBUG_COMPACT_GUARD ints: the device array is that long, starts as the caller's and comes back whole, so that places[] shows what the
 * pack left alone -- with nrec below the total, everything from nrec on.  1 <= n <= 2^24, 0 <= nrec <= 2^24. */
#define DDCMI_DEBUG_COMPACT_GUARD 64
int ddcmi_debug_compact(int n, const int *flags, int max_wg, int nrec, int *places, int *total);
/* ddcmi_debug_gid_find: the search of an ascending gid list that subsetWrite's idList, cholAnalysis and FORCE_AVERAGE share, over ids[nids]
 * (not ascending: DDCMI_EINVAL): index[q] = where queries[q] stands in ids, -1 where it is not listed.  nids, nq <= 2^24. */
int ddcmi_debug_gid_find(int nids, const uint64_t *ids, int nq, const uint64_t *queries, int *index);
/* ddcmi_debug_gid_find_in: the same search over the sub-range ids[lo, hi), 0 <= lo <= hi <= nids, as FORCE_AVERAGE searches the gids behind a
 * pivot: index[q] is still the place in ids[], -1 where queries[q] is not in the range.  wide != 0: the instantiation with 64-bit indices, subsetWrite's. */
int ddcmi_debug_gid_find_in(int nids, const uint64_t *ids, int lo, int hi, int wide, int nq, const uint64_t *queries, int *index);

/* the cross-workgroup reductions, each on the caller's rows and on the current device (tests/test_gpu_reductions.py; tests/reductions.py restates
 * their orders).  The very kernels of the product with the product's launch shapes.  Arguments out of range: DDCMI_EINVAL.  Every output array
 * is also an input: the device array starts as the caller's, so that the caller's poison shows what no kernel wrote. [sync]
 * ddcmi_debug_reduce_jobs: reduce_jobs_block on two jobs of part_q[nrows[q]][8], nv[q] in {0, 3, 7, 8}, finish = 0, disp_dt[q] >= 0 (> 0: column 7
 * is a maximum and the job's displacement word, which starts as disp0[q], grows; not with nv = 8).  nlaunch <= 64 launches one after the other on ONE
 * scratch array, sized and zeroed as ddcmi_create does it: front[l] = 0 k_reduce_jobs with grid (RED_SPLIT, 1) on job 0 alone, 1 k_reduce_jobs
 * with grid (RED_SPLIT, 2), 2 k_reduce_jobs_images without images or messages.  out[l][q][8] and disp[l][q] are what launch l left (out[l] goes in
 * before launch l; the displacement words carry on from launch to launch).  1 <= nrows <= 2^20. */
int ddcmi_debug_reduce_jobs(int nlaunch, const int *front, const int nrows[2], const int nv[2], const double *part0, const double *part1,
                            const double disp_dt[2], const double disp0[2], double *out, double *disp);
/* ddcmi_debug_reduce_hist: k_reduce_hist as ddcmi_lean_flush launches it, nflush <= 16 flushes of nsteps[i] (1 ... 32) pending steps one after the
 * other on ONE scratch array, made and zeroed once by the code ddcmi_lean_flush uses.  Step q of a flush has its nrows rows of 8 doubles
 * q * stride doubles behind the flush's first (stride >= 8 nrows, nrows <= 8192, stride <= 2^17); pair[] (8 sums) and kin[] (7 sums) hold the
 * flushes' rings one behind the other, nsteps[i] * stride doubles each.  hist[]: 32 doubles per step, flush behind flush; flush i's
 * part goes in before its launch and comes back after it. */
int ddcmi_debug_reduce_hist(int nflush, const int *nsteps, int nrows, long long stride, const double *pair, const double *kin, double *hist);
/* ddcmi_debug_reduce_gather: k_reduce_gather on partials[10][pstride], nblocks <= pstride <= 2^20 values per row; out[24] = the words
 * [R_SCR_BOND, R_SCR_REST) of the results: {e_bond, virial xx yy zz xy xz yz, -}, {e_angle, 0 x 6, -}, {e_tors, e_impr, 0 x 6}.
 * ddcmi_debug_reduce_gather_hist: k_reduce_gather_hist on flushes of nsteps[i] steps, step q's ten rows 10 * pstride * q doubles behind the first
 * (pstride <= 2^13); partials[] and hist[] as for ddcmi_debug_reduce_hist (the sums are words 16 ... 25 of a step). */
int ddcmi_debug_reduce_gather(int nblocks, int pstride, const double *partials, double *out);
int ddcmi_debug_reduce_gather_hist(int nflush, const int *nsteps, int nblocks, int pstride, const double *partials, double *hist);
/* ddcmi_debug_block_reduce: one workgroup of 256 threads per block, nblocks <= 4096, out[nblocks][16].  which = 0, 1, 2: in[nblocks][256][NV]
 * doubles through block_reduce_store<NV, 4>, NV = 7, 3, 12 (KD_NV), into out[block][0 ... NV); which = 3, 4: in[nblocks][256] floats, none
 * negative or NaN, through block_vmax_store<4> / block_vmax_store<DDCMI_BLOCK / 64> into out[block][7]. */
int ddcmi_debug_block_reduce(int which, int nblocks, const void *in, double *out);
/* ddcmi_debug_census_final: k_census_final on part_d[nwg][nd] and part_c[nwg][nc] (either may be empty; nwg <= 2048, nd, nc <= 65536), grid of
 * 64-thread workgroups over the longer of the two; which = 0 <RowsSum, double> (out_c doubles), 1 <RowsSum, long long>, 2 <RowsSumMinMax, long long>
 * (out_c 64-bit integers). */
int ddcmi_debug_census_final(int which, int nwg, int nd, const double *part_d, double *out_d, int nc, const unsigned *part_c, void *out_c);
/* ddcmi_debug_kinetic_finish: which = 0 k_group_ke_sum on part[512][2 n] (n groups <= 32), out[2 n]; 1 k_class_kinetic_sum on part[512][n][16]
 * (n classes <= 64), out[n][12].  ddcmi_debug_mol_sum: k_mol_sum on part[nblk][3], out[3]; nblk <= 2^20. */
int ddcmi_debug_kinetic_finish(int which, int n, const double *part, double *out);
int ddcmi_debug_mol_sum(int nblk, const double *part, double *out);

/* roctx ranges opened so far (DDCMI_ROCTX=1: MDSTEP, DDCENERGY, CHARMM_NONBOND ... named like ptiming.h's regions; 0 without the variable) */
long ddcmi_debug_roctx_ranges(void);

#ifdef __cplusplus
}
#endif
#endif

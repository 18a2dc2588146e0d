/*
 * ddcmi.h -- C-ABI of libddcmi.so: the MI355X (gfx950) device side of ddcMD's
 * Martini MD inner loop.  Plain pointers and sizes only; the caller owns host
 * arrays, the library owns device memory.  Every call returns 0 on success or a
 * negative DDCMI_E* code; ddcmi_last_error() gives the message.  No exceptions,
 * no callbacks.  One host thread per context; all work is queued on the
 * context's HIP stream and only the calls marked [sync] wait for it.
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * /root/reference/src).  All quantities are in ddcMD internal units (bohr, fs,
 * Rydberg, e; kB = 1: ddcMD.c:71-73).  Particle arrays are in the CALLER's order
 * on both upload and download; the library keeps its own cell-sorted order
 * internally.
 */
#ifndef DDCMI_H
#define DDCMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ddcmi_ctx ddcmi_ctx;

enum
{
   DDCMI_OK = 0,
   DDCMI_ENODEVICE = -1,    /* no HIP device / HIP runtime error */
   DDCMI_EINVAL = -2,       /* bad argument or call order */
   DDCMI_ENOMEM = -3,
   DDCMI_EUNSUPPORTED = -4, /* e.g. non-orthorhombic box, box < 2*(rmax+deltaR) */
   DDCMI_ECOMM = -5         /* RCCL error */
};

/* energies[] slots of ddcmi_eval_forces / ddcmi_get_energies (BIOENERGIES,
 * bioCharmmParms.h; e->eion is slot DDCMI_E_TOTAL) */
enum { DDCMI_E_LJ = 0, DDCMI_E_ELE, DDCMI_E_BOND, DDCMI_E_ANGLE, DDCMI_E_TORS, DDCMI_E_IMPR, DDCMI_E_TOTAL, DDCMI_E_RESTRAINT, DDCMI_NE };
/* virial / tion component order (THREE_SMATRIX as summed in bioMartini.c:1098-1103) */
enum { DDCMI_XX = 0, DDCMI_YY, DDCMI_ZZ, DDCMI_XY, DDCMI_XZ, DDCMI_YZ };
/* download mask */
enum { DDCMI_POS = 1, DDCMI_VEL = 2, DDCMI_FORCE = 4 };
/* group kinds (a GROUP's velocityUpdate): free.c, berendsen.c, langevin.c, frozen.c, fixedVelocity.c, quench.c.
 * 3 is no kind: it stays refused (the deck loader files every other GROUP type under that number) */
enum { DDCMI_FREE = 0, DDCMI_BERENDSEN = 1, DDCMI_LANGEVIN = 2, DDCMI_FROZEN = 4, DDCMI_FIXEDVELOCITY = 5, DDCMI_QUENCH = 6 };

/* particle labels (gid_type = uint64_t, gid.h:13): MOL 32 | RESID 16 | GROUP 8 | ATOM 8 (bioGid.h:13-22).  The molecule id
 * (reOrgPairs, molecule lists), the residue runs of the bonded terms (charmmResidues) and the group:atom codes of the
 * bonded-pair lists are read off a label with these masks; tests/test_abi.py holds them against the reference's own header */
#define DDCMI_GID_MOLSHIFT   32
#define DDCMI_GID_ATMMASK    0x00000000000000ffull
#define DDCMI_GID_ATMGRPMASK 0x000000000000ffffull
#define DDCMI_GID_GRPMASK    0x000000000000ff00ull
#define DDCMI_GID_RESMASK    0x00000000ffff0000ull
#define DDCMI_GID_MOLMASK    0xffffffff00000000ull
#define DDCMI_GID_MOLRESMASK 0xffffffffffff0000ull

/* ---- context -------------------------------------------------------------
 * replaces accelerator_init / accelerator_getAccelerator (accelerator.c:10-56)
 * and the allocation half of allocSendGPUState / allocGPUBoxInfo
 * (gpuMemUtils.cu).  device = HIP device ordinal. */
int ddcmi_create(ddcmi_ctx **ctx, int device);
void ddcmi_destroy(ddcmi_ctx *ctx);
const char *ddcmi_last_error(const ddcmi_ctx *ctx);   /* ctx may be NULL: last create error */
int ddcmi_device_count(void);                          /* hipGetDeviceCount; 0 without a GPU */
const char *ddcmi_version(void);

/* ---- parameters ------------------------------------------------------------
 * Every setter checks what it is handed -- counts, NULL arrays, offsets (start at 0, never decrease), indices (not negative), constants (finite; rmax > 0,
 * deltaR >= 0, masses > 0, pbc in 0..7) -- and refuses with DDCMI_EINVAL and a message; a refused call changes nothing.  What only a rebuild can know is
 * checked there (molecule types against ddcmi_set_molecules, index-named terms / constraint pairs / molecules against the bead count of the upload).  Under
 * an uploaded state ddcmi_set_species also checks its count against the beads: a table that ends at or below the largest species id of the last
 * ddcmi_upload_state is refused (the kick would read past it); ddcmi_set_groups checks every group's kind and constants before it keeps any.  The
 * caller's promise that an array is as long as its count says cannot be checked.  New species or nonbonded parameters under an uploaded state invalidate
 * the forces on the device: the next ddcmi_eval_forces rebuilds the class tables, the beads' tags and the list (ddcmi_step_nglf asks for it). */
/* BOX h (row-major 3x3, orthorhombic) and pbc bitmask: allocGPUBoxInfo */
int ddcmi_set_box(ddcmi_ctx *ctx, const double h[9], int pbc);
/* SPECIES tables: mass, charge (ddcenergy.c:210), LJ type (getCGLJindexbySpecie
 * bioMartini.c:952), molecule type (molecule.c:56) */
int ddcmi_set_species(ddcmi_ctx *ctx, int nspecies, const double *mass, const double *charge,
                      const int *ljtype, const int *moltype);
/* martiniNonBondGPUParms (bioMartiniGPU.h:8): LJ table [nlj*nlj] {sigma,eps,shift},
 * rmax ("cutoff"), keR = ke/epsilon_r, krf, crf (bioMartini.c:1234-1245) */
int ddcmi_set_nonbonded(ddcmi_ctx *ctx, int nlj, const double *sigma, const double *eps, const double *shift,
                        double rmax, double keR, double krf, double crf);
/* reOrgPairs inputs (bioMartini.c:1392-1485): per molecule type nSpecies and the
 * bpairList (atmgrp codes) of its ownership residue.  nmoltype = 0: no MOLECULECLASS */
int ddcmi_set_molecules(ddcmi_ctx *ctx, int nmoltype, const int *mol_nspecies, const int *bpair_off,
                        const int *bpairI, const int *bpairJ);
/* martiniBondGPUParms (bioMartiniGPU.h:9): bonded terms as lists over CALLER-order
 * atom indices.  angle func 1/2/10 = resAngleSorted/resAngleCosineSorted/
 * resAngleRestrainSorted; tors func 1/2 = resTorsionSorted/resImproperSorted
 * (bioCharmmCovalentEnergiesSorted.c).  excludePotentialTerm: bioCharmmParms.h:25-28 */
int ddcmi_set_bonded(ddcmi_ctx *ctx,
                     int nbond, const int *bond_ij, const double *bond_kb, const double *bond_b0,
                     int nangle, const int *angle_ijk, const int *angle_func, const double *angle_k, const double *angle_t0,
                     int ntors, const int *tors_ijkl, const int *tors_func, const int *tors_n, const double *tors_k, const double *tors_delta,
                     int excludePotentialTerm);
/* The same terms with atoms named by gid (gid_type, gid.h), for decomposed runs where a
 * bead's index does not survive migration: every rank passes the GLOBAL term list.  At
 * each list rebuild a rank finds the owned or halo copy of every term atom; it evaluates
 * the terms of the atoms it owns and keeps those atoms' forces, so no force is sent back,
 * and a term's energy and virial are booked by the owner of its first atom: the sums over
 * ranks count every term once.  This replaces the whole-molecule ownership of
 * ddcRuleMartini (bioMartiniRule.c:64-85): a partner further than rmax+deltaR from the
 * owning domain is an error at the rebuild. */
int ddcmi_set_bonded_gid(ddcmi_ctx *ctx,
                         int nbond, const uint64_t *bond_gid, const double *bond_kb, const double *bond_b0,
                         int nangle, const uint64_t *angle_gid, const int *angle_func, const double *angle_k, const double *angle_t0,
                         int ntors, const uint64_t *tors_gid, const int *tors_func, const int *tors_n, const double *tors_k, const double *tors_delta,
                         int excludePotentialTerm);
/* POTENTIAL type=RESTRAINT (restraint.c:259-361; restraintGPU.cu): harmonic position restraints on the
 * beads with the listed gids.  fc[3n] = fcx fcy fcz switches, r0[3n] = x0 y0 z0 as fractions of the box,
 * kb[n]; origin 0: the box is centred on the origin (r0*L - L/2).  Energy lands in DDCMI_E_RESTRAINT
 * and in DDCMI_E_TOTAL.  n = 0 removes them.  fc takes any int (the force scales with fc, the virial with
 * fc^2).  A bead may carry several restraints: their forces add.  A gid that no bead carries is accepted
 * and contributes nothing -- no force, energy or virial -- like a restraintMap entry of -1 in the reference. */
int ddcmi_set_restraints(ddcmi_ctx *ctx, int n, const uint64_t *gid, const int *fc, const double *r0, const double *kb, int origin);
/* NEIGHBOR deltaR (neighbor.c:49) and DDC updateRate (ddc.c:96).  updateRate = 0: rebuild when
 * neighborCheck (neighbor.c:117-208) finds 2*max displacement >= deltaR (one host round trip per step) */
int ddcmi_set_neighbor(ddcmi_ctx *ctx, double deltaR, int updateRate);
/* GROUP objects (group.c:48-90): type DDCMI_FREE / DDCMI_BERENDSEN{Teq,tau,interval} /
 * DDCMI_LANGEVIN{Teq,tau} (langevin.c:92-128, constant Teq, vcm = 0).  Teq in internal energy units
 * (kB = 1).  The Langevin noise is a counter-based normal stream keyed by (seed, gid, loop): the
 * reference's per-particle LCG64 states are not reproduced -- statistical parity only.
 * DDCMI_FROZEN / DDCMI_FIXEDVELOCITY / DDCMI_QUENCH: Teq, tau and interval of such a group are ignored (neither
 * checked nor used).  With a = (dt/2)/m and f the force the call sees, at FRONT and at BACK (nglf.c:74-108):
 *   FROZEN         the bead does not move and its stored velocity never changes (frozen.c saves v, zeroes it for the drift and puts it
 *                  back): the stored velocity still enters the kinetic terms, the group's temperature and every analysis
 *   FIXEDVELOCITY  v = the group's vector where one is set (ddcmi_set_group_velocity); else nothing: the bead coasts (fixedVelocity.c)
 *   QUENCH         per component: if (v f < 0) v = 0; then v += a f (quench.c; a product, strict <)
 * A step of a context that has one of these three kinds together with constraint groups or a barostat is refused (DDCMI_EUNSUPPORTED). */
int ddcmi_set_groups(ddcmi_ctx *ctx, int ngroup, const int *type, const double *Teq, const double *tau, const int *interval);
/* LANGEVIN groups, the rest of langevin_velocityUpdate (langevin.c:92-128): `vcm`, the velocity the friction relaxes towards
 * (:106,167; v = vcm + a (v - vcm) + c f + d g), per group, [3 ngroup], internal units; after ddcmi_set_groups (which resets it
 * to zero).  And Teq as a function of time (`Teq_dynamics = EXPLICIT_TIME`, :49,84-85): langevin_Update re-evaluates the group's
 * equation once per step on the host; here the host does the same between calls of ddcmi_step_nglf with ddcmi_set_group_temperature
 * (the equation grammar is simutil's eq_parse, which the reference tree does not hold: the deck loader takes constants). */
int ddcmi_set_group_vcm(ddcmi_ctx *ctx, int ngroup, const double *vcm);
int ddcmi_set_group_temperature(ddcmi_ctx *ctx, int group, double Teq);
/* FIXEDVELOCITY groups: set[g] != 0: the group's beads get v[3 g ..] (internal units) at every FRONT and BACK update; set[g] == 0: the
 * group has no `v` key and its beads coast.  Entries of groups of other kinds are checked and ignored.  Comes after ddcmi_set_groups (which
 * resets it: no vector set) with its group count, and checks every value for finiteness before it keeps any: a refused call changes nothing. */
int ddcmi_set_group_velocity(ddcmi_ctx *ctx, int ngroup, const int *set, const double *v /* [3 ngroup] */);
/* INTEGRATOR type=NGLFCONSTRAINT (nglfconstraint.c:510-574): NGLF plus a semi-isotropic Berendsen
 * barostat (changeVolume, :64-84) driven by the molecular pressure of the last force evaluation at the
 * target temperature T: lambda_xy = cbrt(1 + beta dt/tau ((Pxx+Pyy)/2 - P0)), lambda_z likewise from Pzz;
 * box and positions scaled before the FRONT kick.  beta = 0 switches it off.  Costs one host round trip per step
 * (decomposed runs: one all-reduce of the virial and the molecular terms, ddcmi_set_molecule_lists_gid).  Without ddcmi_set_molecule_lists every bead is its own molecule.  Internal units. */
int ddcmi_set_barostat(ddcmi_ctx *ctx, double T, double P0, double beta, double tau);
/* on: ONE scale factor for the three axes, from the mean of Pxx, Pyy, Pzz -- what the reference's GPU integrator
 * NGLFGPULANGEVIN applies (changeVolumeGPUisotropic, molecularPressureGPU.cu:204-239); off (default): changeVolume's
 * semi-isotropic form */
int ddcmi_set_barostat_isotropic(ddcmi_ctx *ctx, int on);
/* current box (it changes under the barostat) */
int ddcmi_get_box(const ddcmi_ctx *ctx, double h[9]);
/* the molecular pressure (xx, yy, zz; molecularPressure.c:57-67) the barostat acted on in the last step */
int ddcmi_get_barostat_pressure(const ddcmi_ctx *ctx, double p[3]);
/* Molecules for the barostat's molecular virial (molecularVirial, molecularPressure.c:23-56):
 * nmol_total = N in the N kB T term; the nmulti molecules of two or more beads are listed as caller-order
 * atom indices, molecule m = mol_atoms[mol_off[m] .. mol_off[m+1]).  One domain. */
int ddcmi_set_molecule_lists(ddcmi_ctx *ctx, long nmol_total, int nmulti, const int *mol_off, const int *mol_atoms);
/* The same with atoms named by gid, for decomposed runs (every rank passes the GLOBAL lists; mol_mass[m] = total mass of
 * molecule m).  Beads migrate one by one, so a molecule may have atoms on several ranks: each rank sums over the atoms it
 * owns; the centre of mass and total force of such SPLIT molecules are completed by an all-reduce of six doubles per split
 * molecule in every step the barostat acts, together with the virial.  No limit on the molecule's extent. */
int ddcmi_set_molecule_lists_gid(ddcmi_ctx *ctx, long nmol_total, int nmulti, const int *mol_off, const uint64_t *mol_atom_gid, const double *mol_mass);
/* nglfconstraint's velocity constraints (velocityConstraintOld/resMoveConsOld, nglfconstraint.c:180-264,
 * 438-455; groups from genConstraint, bioMartini.c:300-445).  Group g holds the pairs
 * [pair_off[g], pair_off[g+1]) in the order the reference sweeps them; pairI/pairJ are caller-order atom
 * indices, dist the constrained lengths (internal units).  Groups must not share atoms.  With groups set,
 * every step runs FRONT kick -> constraint ((r + dt v)^2 = d^2) -> drift -> forces -> BACK kick ->
 * constraint (r.v = 0) -> kinetic terms.  Gauss-Seidel sweeps to |rvab dt| < 1e-12, at most 500, as the
 * reference.  The constraint virial is not booked (the reference computes and drops it).  Caller-order indices: one domain
 * (decomposed runs: ddcmi_set_constraints_gid). */
int ddcmi_set_constraints(ddcmi_ctx *ctx, int ngroups, const int *pair_off, const int *pairI, const int *pairJ, const double *dist);
/* The same groups with atoms named by gid, for decomposed runs (every rank passes the GLOBAL list): at each rebuild a rank
 * finds the owned or halo copy of every group atom; a rank that owns an atom of a group solves the whole group -- positions of
 * the partners from the position halo, their velocities from a velocity halo exchanged before each of the two solves of a
 * step -- and keeps the velocities of the atoms it owns.  A partner further than rmax+deltaR from the owning domain is an
 * error at the rebuild. */
int ddcmi_set_constraints_gid(ddcmi_ctx *ctx, int ngroups, const int *pair_off, const uint64_t *pairI, const uint64_t *pairJ, const double *dist);
/* largest sweep count of any group since the last reset, and how many group solves hit the 500-sweep cap */
int ddcmi_constraint_stats(ddcmi_ctx *ctx, int *max_sweeps, int *unconverged, int reset);
/* RANDOM seed (random.c:44-60) for the Langevin noise */
int ddcmi_set_random(ddcmi_ctx *ctx, uint64_t seed);
/* RANDOM type LCG64 (lcg64.c, random.c:135-160): Langevin groups draw from the reference's own per-particle streams -- three
 * unit normals per half kick by gasdev3d over lcg64_2 -- instead of the counter-based one.  n LCG64_PARM records
 * {state, multID, prime} (lcg64.h:8-12) in the caller order of the last ddcmi_upload_state, which they must follow (and, in a
 * decomposed run, precede the first list build); what a particle without a random field gets is lcg64_default's business
 * (deck.c restates it for the atoms reader).  The records travel with their beads: through the sorts of a rebuild and, in a
 * decomposed run, inside the migration records (particleRegisterinfo of random->parmsArray, random.c:72-76).  n = 0: back to
 * the counter-based stream.  ddcmi_get_random_lcg64 returns the advanced states (collection_write.c:157-161) in caller
 * order -- in the order of ddcmi_download_particles for a decomposed run, whose beads have no caller order left. [sync] */
int ddcmi_set_random_lcg64(ddcmi_ctx *ctx, int n, const uint64_t *state, const uint32_t *multID, const uint32_t *prime);
int ddcmi_get_random_lcg64(ddcmi_ctx *ctx, int n, uint64_t *state, uint32_t *multID, uint32_t *prime);
/* SIMULATE loop/time (simulate.c:146,155) */
int ddcmi_set_clock(ddcmi_ctx *ctx, int64_t loop, double time);

/* ---- state ----------------------------------------------------------------- */
/* allocSendGPUState + sendGPUState + sendForceVelocityToGPU (gpuMemUtils.h):
 * nlocal particles in caller order.  v may be NULL (zero). [sync] */
int ddcmi_upload_state(ddcmi_ctx *ctx, int nlocal,
                       const double *rx, const double *ry, const double *rz,
                       const double *vx, const double *vy, const double *vz,
                       const uint64_t *gid, const int *species, const int *group);
/* sendGPUState between list rebuilds (gpuMemUtils.cu; martiniGPU1 with a CPU integrator, bioMartini.cu:157): new
 * positions (and velocities, if not NULL) of the SAME particles in caller order; the neighbour list stays valid.
 * A position that was wrapped into the box on the host is taken at its periodic image nearest to where the bead
 * was (the device keeps positions continuous between rebuilds). */
int ddcmi_upload_positions(ddcmi_ctx *ctx, const double *rx, const double *ry, const double *rz,
                           const double *vx, const double *vy, const double *vz);
/* sendHostState / sendForceVelocityToHost / sendPosnToHost: any pointer may be
 * NULL; positions come back wrapped into the box like backInBox_fast
 * (nglf.c:90). [sync] */
int ddcmi_download_state(ddcmi_ctx *ctx, int mask,
                         double *rx, double *ry, double *rz,
                         double *vx, double *vy, double *vz,
                         double *fx, double *fy, double *fz);
int ddcmi_nlocal(const ddcmi_ctx *ctx);

/* ---- hot path -------------------------------------------------------------- */
/* constructList (nlistGPU.cu:1459; hook ddcUpdateAll.c:136-139): wrap, bin-sort,
 * image atoms, full neighbour list within rmax+deltaR, exclusion split. [sync] */
int ddcmi_build_list(ddcmi_ctx *ctx);
/* martiniGPU1 (bioMartini.cu:146-171) = zeroGPUForceEnergyBuffers + charmmPairGPU
 * + charmmConvalentGPU: forces on the device, energies[DDCMI_NE], virial[6].
 * Builds the list first when none exists.  [sync] */
int ddcmi_eval_forces(ddcmi_ctx *ctx, double *energies, double *virial);
/* nglfGPU (nglfGPU.cu:511; CPU contract nglf.c:67-112): nsteps velocity-Verlet
 * steps fully on the device incl. rebuild every updateRate loops and
 * kinetic_terms each step.  Not synchronising except at rebuilds. */
int ddcmi_step_nglf(ddcmi_ctx *ctx, double dt, int nsteps);
/* sendForceEnergyToHost + kineticGPU: energies/virial of the last force
 * evaluation, rk and tion[6] of the last kinetic_terms. [sync] */
int ddcmi_get_energies(ddcmi_ctx *ctx, double *energies, double *virial, double *rk, double *tion);
/* kinetic_terms (energy.c:48-163) on the current velocities. [sync] */
int ddcmi_kinetic(ddcmi_ctx *ctx, double *rk, double *tion);
/* the per-group (by_species = 0) or per-species (1) copies of kinetic_terms and the thermal flux, energy.c:104-147:
 * out[12 c + k] for class c = {rk, tion xx yy zz xy xz yz, mass, number, J x y z} over this rank's beads, J = sum (K + U) v - S v / 2
 * with the per-atom U and S this path leaves at zero (ddcenergy.c:152-154, bioMartini.c:1111-1120); the classes' J add up to
 * e->thermal_flux.  nclass must be the context's group / species count.  For print steps. [sync] */
int ddcmi_kinetic_detail(ddcmi_ctx *ctx, int by_species, int nclass, double *out);
/* eval_energyInfo group branch (energyInfo.c:118-141): refresh the per-group
 * temperatures Berendsen reads; returns them in Tgroup[ngroup] if not NULL.  With an
 * RCCL communicator the sums are all-reduced first (collective call). [sync] */
int ddcmi_group_temperatures(ddcmi_ctx *ctx, double *Tgroup);
int ddcmi_get_clock(const ddcmi_ctx *ctx, int64_t *loop, double *time);
int ddcmi_sync(ddcmi_ctx *ctx);

/* ---- analysis -------------------------------------------------------------- */
/* paircorrelation_eval_geom (paircorrelation.c:354-457) on the device: this rank's counts of ordered pairs (i owned here, j any
 * other bead) with rmin <= r < rmin + nbins*delta_r, species(i) <= species(j), in combo-major order
 * counts[comboIndex(a,b)*nbins + k] (ncombo = nspecies(nspecies+1)/2), and this rank's beads per species in nbeads[nspecies].
 * log_scale: ddcMD's rscale = log (rmin > 0).  Sums over ranks are the global histogram exactly.  rmax must not exceed half
 * the shortest periodic box side, and on a decomposed run the potential's cut-off.  Collective on a decomposed context.  Reads
 * the current positions (those ddcmi_download_state returns) and changes nothing of the run. [sync] */
int ddcmi_pair_correlation(ddcmi_ctx *ctx, double rmin, double delta_r, int nbins, int log_scale,
                           int nspecies, int64_t *counts, int64_t *nbeads);
/* ANALYSIS VELOCITYAUTOCORRELATION (velocityAutocorrelation.c) on the device.  Every owned bead carries a reference record -- its
 * velocity at the time origin and its displacement since, the sum of the drift moves dt*v (the reference's REF {r, v},
 * velocityAutocorrelation.c:30, kept up in nglf.c:79-86): wraps into the box and the barostat's scaling do not count, and the
 * record follows its bead through rebuilds and migration between ranks.  Off until the first origin; with it off nothing of a
 * run differs.  ddcmi_upload_state drops the records.
 * ddcmi_vaf_origin (velocityAutocorrelation.c:193-199): the current state becomes the time origin of every owned bead, v0 = v,
 * d = 0; switches tracking on.  On a decomposed run every rank calls it at the same point of the run. */
int ddcmi_vaf_origin(ddcmi_ctx *ctx);
/* velocityAutocorrelation_eval's sums (velocityAutocorrelation.c:152-179) over this rank's beads, in internal units:
 * vaf[c] = sum v0.v, msd[c] = sum d.d for class c = 0 the system, 1 + g group g, 1 + ngroup + s species s ([1 + ngroup + nspecies]
 * each; the reference's "a single group / species has no block" rule is the output's).  ngroup and nspecies must be the
 * context's.  Sums over ranks are the global sums; no communication.  Right after an origin: sum v.v and exactly 0.  Refused
 * without an origin.  Two identical runs give identical bits.  Changes nothing of the run. [sync] */
int ddcmi_vaf_sample(ddcmi_ctx *ctx, int ngroup, int nspecies, double *vaf, double *msd);
/* tracking off, the records released (the reference has no counterpart: its v0 lives as long as the analysis).  On a decomposed
 * run every rank calls it at the same point of the run, as with the origin: the migration records carry the reference record
 * while tracking is on, and sender and receiver must agree on that. */
int ddcmi_vaf_clear(ddcmi_ctx *ctx);
/* ANALYSIS vcmWrite, zdensity, KINETICENERGYDISTN, DSF and subsetWrite on the device: one read-only pass over the owned beads each.  All read the state that a download
 * returns at this point of the run, change nothing of it (a run with calls and one without are bit for bit the same), need no
 * communication and give identical bits when repeated; a domain that holds no bead gives zeros.
 * vcmWrite_output's sums (vcmWrite.c:95-110) over this rank's beads, internal units: mv[3 c .. 3 c + 2] = sum m v, m[c] = sum m, class c = 0 the
 * system, 1 + g group g, 1 + ngroup + s species s ([1 + ngroup + nspecies] classes, at most 512).  m is the species' mass of
 * ddcmi_set_species, the one the integrator's kick uses.  ngroup and nspecies must be the context's.  Sums over ranks are the global
 * sums; no communication.  Changes nothing of the run. [sync] */
int ddcmi_momentum_by_class(ddcmi_ctx *ctx, int ngroup, int nspecies, double *mv, double *m);
/* zdensity_output's histogram (zdensity.c:66-151) over this rank's beads: density[nz] weights, 1 <= nz <= 2048.  smear_radius <= 0: one bin per bead,
 * weight 1 (the sums are integers, exact at any bead count).  smear_radius > 0 (internal length): two neighbouring bins per bead,
 * smear_method 0 impulse, 1 hat.  The positions are binned as a download returns them, without a further wrap: a bead outside
 * the box lands where the reference's clamp puts it (bin nz - 1 in general).  Sums over ranks are the global histogram. [sync] */
int ddcmi_zdensity(ddcmi_ctx *ctx, int nz, double smear_radius, int smear_method, double *density);
/* ANALYSIS KINETICENERGYDISTN on the device: kineticEnergyDistn_eval's loop (kineticEnergyDistn.c:157-188) over this rank's beads, for
 * all ndist histograms ("groups") in one read-only pass under the rules above.  Group g has nbins[g] bins of width
 * delta = (emax[g] - emin[g]) / nbins[g] from emin[g] (internal energy units; finite, emax > emin, nbins >= 1); species_dist[nspecies]
 * names the group of each species, or -1 (two species may share a group).  A bead of group g has K = (0.5 mass)((vx vx + vy vy) + vz vz),
 * every operation rounded once as the reference's C does, mass the species' mass of ddcmi_set_species, and goes
 *    K < emin: tallies[3 g + 1] (subCnt);   K >= emax, +inf included: tallies[3 g + 2] (supCnt);
 *    otherwise counts[off(g) + min((int)((K - emin)/delta), nbins - 1)], off(g) = nbins[0] + ... + nbins[g - 1]
 * (the quotient of a K just below emax may round up to nbins: the last bin, where the reference asserts).  tallies[3 g] counts every
 * bead of the group (cntTotal); stats[3 g .. 3 g + 2] = {sum K, min K, max K}, the extremes starting at the reference's 1e300 and 0.0,
 * which a group without beads returns.  A bead whose K is NaN is counted in cntTotal and joins the sum, and enters no bin, neither
 * outer count, neither extreme.  Counts are exact 64-bit integers; over ranks, add counts and sums and take the minimum of the
 * minima and the maximum of the maxima.  nspecies must be the context's.  ndist = 0 is valid and touches nothing.  The bins of all
 * groups share one workgroup's LDS: DDCMI_KDIST_LDS_BYTES(ndist, sum of nbins) <= DDCMI_KDIST_MAX_LDS, else DDCMI_EUNSUPPORTED
 * (16357 bins for one group; 8192 and more for up to 303 groups). [sync] */
#define DDCMI_KDIST_MAX_LDS 65536
#define DDCMI_KDIST_LDS_BYTES(ndist, nbins_total) (4 * ((nbins_total) + 3 * (ndist)) + 96 * (ndist))
int ddcmi_kinetic_energy_distn(ddcmi_ctx *ctx, int nspecies, int ndist, const double *emin, const double *emax, const int *nbins,
                               const int *species_dist, int64_t *counts, int64_t *tallies, double *stats);
/* ANALYSIS DSF / DynamicStructureFactor on the device: dsf_eval's local sums (dsf.c:160-205) over this rank's beads for the axis-aligned
 * wave vectors k = m b_a of an orthorhombic box, in one read-only pass under the rules above.  rho[3][mmax][2]: for axis a (0 x, 1 y,
 * 2 z) and m = 1 .. mmax the {re, im} of sum q_j c^m, c = exp(i 2 pi r_a / L_a), over the owned beads whose species is selected --
 * select[nspecies], nonzero: takes part; NULL: every species.  q is the species' charge of ddcmi_set_species.  *count: the selected
 * owned beads.  Over ranks, add rho and the counts; the division by the global count (dsf.c:210-212) is the caller's.  The positions
 * are those a download returns, without a further wrap: the phase is periodic, so a bead outside the box contributes correctly.
 * nspecies must be the context's; 1 <= mmax <= DDCMI_DSF_MAX_M, above it DDCMI_EUNSUPPORTED.  A domain that holds no bead, or a
 * select without a member, gives zeros and count 0. [sync] */
#define DDCMI_DSF_MAX_M 256
int ddcmi_charge_density_modes(ddcmi_ctx *ctx, int nspecies, const int *select, int mmax, double *rho, int64_t *count);
/* The density modes of ANALYSIS SSF (ssf.c:91-120) on any list of integer wave vectors, on the device, in one read-only pass under the
 * rules above: rho[l] = {re, im} of sum w_j exp(i 2 pi (n_x x_j / L_x + n_y y_j / L_y + n_z z_j / L_z)), (n_x, n_y, n_z) = kvec[l] (signed),
 * over the owned beads whose species is selected -- select[nspecies], nonzero: takes part; NULL: every species.  weight 0: w = 1 (ssf.c);
 * weight 1: w the species' charge of ddcmi_set_species (DSF's weight).  *count: the selected owned beads.  Over ranks, add rho and the
 * counts.  Positions and phase reduction are ddcmi_charge_density_modes': the position a download returns without a further wrap,
 * t = r / L less its nearest integer, the phase n . t in turns less its nearest integer, one sincospi.  The value of a wave vector
 * does not depend on the list: it has the same bits wherever it stands, whatever else the list holds (duplicates and (0,0,0) -- the
 * sum of w -- included) and whatever nk is.  Orthorhombic boxes; 1 <= nk <= DDCMI_SM_MAX_K and |component| <= DDCMI_SM_MAX_N, above
 * them DDCMI_EUNSUPPORTED.  nspecies must be the context's.  A domain that holds no bead, or a select without a member, gives zeros and
 * count 0. [sync] */
#define DDCMI_SM_MAX_N 1024
#define DDCMI_SM_MAX_K 4096
int ddcmi_structure_modes(ddcmi_ctx *ctx, int nspecies, const int *select, int weight, int nk, const int32_t *kvec, double *rho, int64_t *count);
/* ANALYSIS subsetWrite, format binaryCharmm, on the device (subsetWrite.c:409-522): the owned beads a filter selects as the file's
 * 24-byte records, in one read-only pass under the rules above.  The filter is rejectParticle's (subsetWrite.c:532-564), in its order
 * and with its comparisons: a bead is dropped if gid < idmin, gid > idmax, gid % modulus != 0, odd and gid even, r_a > rmax[a] or
 * r_a < rmin[a], v_a > vmax[a] or v_a < vmin[a] (strict: a bead on a bound is kept, and a NaN coordinate passes), include_species[its
 * species] == 0 (NULL: every species), or -- with an idlist -- its gid is not among the nid ascending entries (binary search on the
 * device; idlist NULL and nid 0: no list).  Internal units; positions and velocities are those a download returns (wrapped).  A
 * record is {gid, pinfo = group_term[group] + species_term[species], (float)((r_a - corner[a]) * cL)}: the difference and the product
 * in double, rounded once; the two tables are pinfoEncode (pinfo.c:119-126) split by the caller.  nspecies and ngroup are the tables'
 * lengths and must cover the context's species and groups (a context without groups has the one group 0).
 * *count: this rank's selected beads, always.  rec NULL: nothing else.  Otherwise the records in the order of
 * ddcmi_download_particles (a stable compaction) if cap >= *count; with a smaller cap DDCMI_EINVAL, *count set and rec untouched.
 * The records are packed in a device buffer of the context and copied once: 24 * count bytes cross, not the state.  Over ranks,
 * concatenate.  Refused: modulus < 1, an idlist that is not ascending, tables shorter than the context's ids, a cL that is not finite
 * (DDCMI_EINVAL); a box that is not orthorhombic (DDCMI_EUNSUPPORTED). [sync] */
typedef struct ddcmi_subset_filter
{
   uint64_t idmin, idmax;
   int modulus, odd;
   double rmin[3], rmax[3], vmin[3], vmax[3];
   int nspecies, ngroup;
   const int *include_species;
   const uint32_t *group_term, *species_term;
   int64_t nid;
   const uint64_t *idlist;
   double corner[3], cL;
} ddcmi_subset_filter;
typedef struct ddcmi_subset_record { uint64_t gid; uint32_t pinfo; float r[3]; } ddcmi_subset_record;      /* 24 bytes: the file's record */
int ddcmi_subset_records(ddcmi_ctx *ctx, const ddcmi_subset_filter *filter, int64_t cap, ddcmi_subset_record *rec, int64_t *count);
/* ANALYSIS COARSEGRAIN on the device (coarsegrain.c:242-448, coarsegrain_eval): one evaluation's sums over this rank's owned beads per
 * (grid cell, species) of an nx x ny x nz grid of the orthorhombic box, in one read-only pass under the rules above, as the non-empty
 * entries in ascending (label, species) order; label = igz + nz (igy + ny igx).  Internal units: n the sum of the weights, mass of
 * weight m, K[a] of weight 0.5 m v_a v_a, p[a] of weight m v_a; m is the species' mass of ddcmi_set_species.  smear_radius <= 0: the
 * one cell (int)r_a per axis, r_a = x_a (n_a / L_a) - corner_a (n_a / L_a), weight 1.  Otherwise the reference's two cells per axis
 * (floor(r_a + 0.5) - 1 and floor(r_a + 0.5), -1 -> n_a - 1 and n_a -> 0 on every axis, open ones too), lSmear = min(2 smear_radius,
 * L_a / n_a), weights by smear_method 0 (impulse) or 1 (hat), corner weight (wx wy) wz, corners below 1e-20 skipped.  Positions are
 * those a download returns (wrapped).  Where the reference runs off its grid, a cell index outside [0, n_a) is clamped into it (a
 * bead on the upper face, a NaN: cell 0).  U, virial and the virial tensor of the reference's record are zero on the Martini path and
 * are not computed.  Every sum is added in an order that depends only on the set of contributions (stable radix sort by key, then a
 * segmented reduction whose association depends only on the segment's length): no floating-point atomics, identical bytes when repeated.
 * *count: this rank's entries, always.  rec NULL: nothing else.  Otherwise the records, cap their room: cap < *count is DDCMI_EINVAL
 * and leaves rec untouched.  The records are formed in a device buffer of the context and copied once.  Over ranks, merge by key.
 * Refused: n_a < 1, an nspecies that is not the context's, no state or no box, a smear_method other than 0 or 1, a smear_radius that is
 * not finite (DDCMI_EINVAL); a box that is not orthorhombic, nx ny nz nspecies > DDCMI_CG_MAX_KEYS (DDCMI_EUNSUPPORTED).  A domain
 * that holds no bead gives count 0. [sync] */
#define DDCMI_CG_MAX_KEYS (1 << 28)      /* bounds the sort key label * nspecies + species and the sentinel one above it: 32 bits hold it, four 8-bit passes sort it */
typedef struct ddcmi_cg_record { int64_t label; int32_t species; int32_t pad; double n, mass, K[3], p[3]; } ddcmi_cg_record;      /* 80 bytes */
int ddcmi_coarsegrain(ddcmi_ctx *ctx, int nx, int ny, int nz, int nspecies, double smear_radius, int smear_method, int64_t cap, ddcmi_cg_record *rec,
                      int64_t *count);
/* ANALYSIS cholAnalysis on the device (cholAnalysis.c:109-163, cholAnalysis_eval): for each of nmol listed molecules -- gid[7 m + role],
 * roles 0..6 the first seven beads of a CHOL residue in gid order, the list in any molecule order -- the ring-plane offsets, in one
 * read-only pass under the rules above.  With b(i,j) the nearest image of r_j - r_i (the rint form, open axes not wrapped):
 *    A = b(0,1), B = b(0,2), C = b(0,3), D = b(4,5), E = b(4,3), F = b(4,6)
 *    dR1 = ((B x C) . A) / |B x C|,   dR5 = -((E x F) . D) / |E x F|
 * every operation rounded once, in the reference's order.  A molecule all of whose seven beads this rank owns is counted:
 * counts[ibin(dR1)]++, counts[nbins + ibin(dR5)]++ with ibin(d) = (int)MIN(MAX((d - rmin) / delta, 0), nbins - 1) (a NaN: bin 0),
 * (*ndone)++, stats[0..2] = {sum, min, max} of dR1 and stats[3..5] of dR5; the extremes start at the reference's 1e300 and -1e300
 * and a NaN joins the sum and neither extreme.  A molecule of which this rank owns one to six beads is returned as fragments
 * {mol, role, r} in (mol, role) order -- mol the index in the list, r the position a download returns; halo beads are never read --
 * and a molecule it owns nothing of leaves no trace.  *nfrag: this rank's fragments, always.  frag NULL: nothing else.  Otherwise the
 * fragments if cap >= *nfrag; with a smaller cap DDCMI_EINVAL, *nfrag (and counts, ndone, stats) set and frag untouched.  Over ranks:
 * add counts and ndone, add the sums in rank order, minimum of the minima, maximum of the maxima, concatenate the fragments in rank
 * order and complete the split molecules on the host with the lane's own arithmetic (ddcmi_chol_complete of the host layer).
 * Internal units.  nmol = 0 is valid and touches nothing.  DDCMI_EINVAL, nothing changed: nmol < 0, a NULL array with a positive
 * count, nbins < 1, a delta that is not finite and positive, an rmin that is not finite, a gid listed twice, no state or no box.
 * DDCMI_EUNSUPPORTED: a box that is not orthorhombic; nbins > DDCMI_CHOL_MAX_NBINS (the two histograms share one workgroup's LDS
 * with the workgroup's partial sums: DDCMI_CHOL_LDS_BYTES(nbins) <= DDCMI_CHOL_MAX_LDS). [sync] */
#define DDCMI_CHOL_MAX_LDS 65536
#define DDCMI_CHOL_LDS_BYTES(nbins) (4 * (2 * (nbins) + 1) + 196)
#define DDCMI_CHOL_MAX_NBINS 8167
typedef struct ddcmi_chol_fragment { int32_t mol, role; double r[3]; } ddcmi_chol_fragment;      /* 32 bytes */
int ddcmi_chol_offsets(ddcmi_ctx *ctx, int64_t nmol, const uint64_t *gid /* [7 nmol], roles 0..6 */, double rmin, double delta, int nbins,
                       int64_t *counts /* [2 nbins] */, int64_t *ndone, double *stats /* {sum,min,max} of dR1, then of dR5 */,
                       int64_t cap, ddcmi_chol_fragment *frag, int64_t *nfrag);
/* The fragments of this context's last ddcmi_chol_offsets once more: they stay packed in a device buffer of the context until its next
 * ddcmi_chol_offsets, so a caller asks for the count first (frag NULL above) and fetches them here without a second pass.  *nfrag:
 * their number, always; frag NULL: nothing else; cap < *nfrag: DDCMI_EINVAL and frag untouched. [sync] */
int ddcmi_chol_fragments(ddcmi_ctx *ctx, int64_t cap, ddcmi_chol_fragment *frag, int64_t *nfrag);
/* ANALYSIS FORCE_AVERAGE on the device (forceAverage.c:76-145): running sums of the force, the velocity or the position of the beads
 * with listed gids, which stay on the device from one evaluation to the next -- an evaluation is one small launch and no host wait.
 * The three calls are not collective and are legal for the contexts of an in-process group as well.
 * ddcmi_track_set: the n tracked gids in the caller's order; any order, duplicates (the reference searches once per list entry) and
 * gids above 2^32 are legal.  The context keeps the list ascending and unique on the device and the caller's order on the host.  A
 * new list clears the accumulators; n = 0 removes the list and frees its buffers.  n > DDCMI_TRACK_MAX_IDS: DDCMI_EUNSUPPORTED (the
 * device buffers, 40 bytes per gid, stay below 40 MB).  n < 0, or a NULL list with n > 0: DDCMI_EINVAL, nothing changed. */
#define DDCMI_TRACK_MAX_IDS (1 << 20)
int ddcmi_track_set(ddcmi_ctx *ctx, int64_t n, const uint64_t *gid);
/* forceAverage_eval: one pass over this rank's owned beads; the bead that carries a listed gid adds its three components to that
 * gid's running sum and 1 to its 64-bit hit count.  what 0: the force of the last force evaluation, 1: the stored velocity, 2: the
 * position -- each the bits ddcmi_download_state returns at this point (the position wrapped as it wraps).  One gid has one owner,
 * so one lane writes a slot: a plain load, add and store, no atomics.  Asynchronous on the context's stream, no communication; it
 * changes nothing of the run and is legal at any point between steps, like the passes above.  A domain that holds no bead, or a
 * context without a list, does nothing and succeeds.  DDCMI_EINVAL, nothing changed: a what other than 0, 1, 2; no uploaded state;
 * what = 0 without a valid force evaluation (ddcmi_step_nglf's refusal); a what other than the one the window already holds -- a
 * window, from one clearing of the accumulators to the next, averages one quantity. */
int ddcmi_track_accumulate(ddcmi_ctx *ctx, int what /*0 force, 1 velocity, 2 position*/);
/* this rank's sums and hit counts in the caller's order, sum[3 k .. 3 k + 2] and hits[k] for the k-th listed gid (duplicates get
 * equal values); n must be the list's length.  reset != 0 then zeroes the accumulators: the next window.  The accumulators belong to
 * the rank, not to the bead: a tracked bead that migrates goes on adding at its new owner, and nothing travels with it.  A gid no
 * owned bead carried has sum 0 and hits 0 here; over the ranks the hits of a gid that exists add up to the number of accumulations,
 * and the window's sum is the ranks' sums added in rank order. [sync] */
int ddcmi_track_read(ddcmi_ctx *ctx, int64_t n, double *sum /* [3 n] */, int64_t *hits /* [n] */, int reset);

/* ---- transforms ------------------------------------------------------------ */
/* TRANSFORM type THERMALIZE on the device (thermalize.c:83-269): new velocities for the owned beads.  Only the velocities change --
 * positions, lists, the validity of the forces and the VAF records stay -- and the call is legal whenever a state is uploaded; kinetic
 * terms read before it are stale (ddcmi_kinetic forms them anew).  select 0: one class, temperature[0]; 1: by species; 2: by group
 * (getIndex, :271-289); ntemp must cover the classes of the select.  Temperatures in internal energy units (kB = 1).  The mass is the
 * species' mass of ddcmi_set_species, the one the integrator's kick uses.
 * method 0 BOLTZMANN (thermalize_boltzmann, :103-125): v = sqrt(T / m) g, g three normals of gasdev0 (random.c:100-112) on the bead's own
 *    erand48 stream prand48_init((loop % 10000000 + 1) * gid, seed, 0x1234512345ab) (random.c:370-386), reproduced operation by operation:
 *    a bead's velocity depends on its gid, its mass, T, seed and loop alone -- not on the decomposition, and loop and loop + 10000000 draw
 *    alike.  A bead whose class has T < 0 is not written.  keep_vcm is ignored.
 * method 1 RESCALE (thermalize_rescale, :159-269): per class vcm = sum m v / sum m, tempSum = sum m |v - vcm|^2 / (3 (N - 1)),
 *    v' = (v - vcm) vScale + vcmNew, vScale = sqrt(T / tempSum) or 1 where T <= 0, vcmNew = vcm (keep_vcm != 0) or vcm vScale.  The sums
 *    follow the census passes' rules (no floating-point atomics, identical bits when repeated); on a decomposed run the call is collective
 *    and every rank adds the ranks' sums in rank order.  A class with N <= 1 or tempSum == 0, where the reference divides by zero, is not
 *    written.  At most 512 classes (1 + groups + species, as ddcmi_momentum_by_class): more is DDCMI_EUNSUPPORTED.
 * method 2 JUTTNER (relativistic): DDCMI_EUNSUPPORTED.
 * DDCMI_EINVAL: no uploaded state, a method or select out of range, ntemp below the number of classes, a NaN temperature. [sync] */
int ddcmi_thermalize(ddcmi_ctx *ctx, int method /*0 BOLTZMANN, 1 RESCALE*/, int select /*0 global, 1 by species, 2 by group*/,
                     int ntemp, const double *temperature /*internal energy units, kB = 1; < 0: leave this class alone*/,
                     uint64_t seed, int64_t loop, int keep_vcm);

/* ---- introspection / measurement ------------------------------------------- */
/* list statistics of the last build: stats[0]=stored full-list entries,
 * [1]=excluded-list entries, [2]=ELL width, [3]=image (halo) atoms, [4]=cells,
 * [5]=rebuild count */
int ddcmi_list_stats(const ddcmi_ctx *ctx, int64_t stats[8]);
/* the per-step halo exchange of a decomposed run, as laid out at the last rebuild (ddcSendRecvTables, ddcSendRecv.c:41):
 * stats[0]=beads this rank sends per step, [1]=beads it receives, [2]/[3]=messages sent/received (one per peer),
 * [4]=RCCL version code (ncclGetVersion), [5]=transport (0 none, 1 RCCL, 2 host-staged TCP, 3 RCCL loopback), [6]=ranks, [7]=rank */
int ddcmi_comm_stats(const ddcmi_ctx *ctx, int64_t stats[8]);
/* the same exchange peer by peer: returns the number of peers (one message each way per step) and fills up to cap of them --
 * peer rank, beads sent to it and received from it per step (x 24 B on the wire; 2x2x2 bricks: seven peers over seven xGMI links) */
int ddcmi_comm_peer_stats(const ddcmi_ctx *ctx, int cap, int *peer, int64_t *send_beads, int64_t *recv_beads);
/* Copy the full neighbour list out as CSR over caller-order indices (image atoms
 * are mapped back to their source atom). start[nlocal+1]; j may be NULL to query
 * the size (returned through *nentries).  which: 0 kept, 1 excluded. [sync] */
int ddcmi_get_list(ddcmi_ctx *ctx, int which, int *start, int *j, int64_t *nentries);
/* HIP-event timing of the nonbonded kernel on the context's stream:
 * enable, run, then read {launch count, total ms}.  [sync] on read */
int ddcmi_timing_enable(ddcmi_ctx *ctx, int on);
int ddcmi_timing_read(ddcmi_ctx *ctx, int64_t *launches, double *total_ms, int reset);
/* of what the last ddcmi_timing_read returned: the launches (and their time) whose epilogue was the integrator's pass -- between
 * print steps ddcmi_step_nglf runs BACK kick, kinetic_terms, FRONT kick and drift (nglf.c:74-104) inside the pair kernel when
 * the force is complete at the end of the list walk (no bonded terms, restraints, constraints, barostat, charges) */
int ddcmi_timing_fused(ddcmi_ctx *ctx, int64_t *launches, double *total_ms);
/* native stream handle (hipStream_t) for callers that time with their own events */
void *ddcmi_stream(ddcmi_ctx *ctx);

/* ---- multi-GPU: spatial decomposition over RCCL ----------------------------
 * replaces ddc_init / ddcAssignment / ddcSendRecvTables / ddcUpdate (ddc.c,
 * ddcAssignment.c, ddcSendRecv.c, ddcUpdate.c).  The caller distributes the
 * 128-byte id produced on rank 0 (MPI_Bcast in ddcMD, torch.distributed in
 * bench.py).  With a full list no force return (ddcUpdateForce) is needed. */
int ddcmi_comm_unique_id(char id[128]);
int ddcmi_comm_init(ddcmi_ctx *ctx, int rank, int nranks, const char id[128], int px, int py, int pz);
/* energyInfo.c:9-63 allreduce(): sum the 24-double ETYPE block across ranks */
int ddcmi_comm_allreduce_sum(ddcmi_ctx *ctx, double *values, int n);
/* Preflight of a fresh communicator (RCCL or host transport), right behind ddcmi_comm_init[_host] and before any timing: ONE grouped
 * exchange of a known pattern along every direction the brick plan names (the peers, matching and grouping of ddcUpdate's halo
 * exchange, ddcUpdate.c:56-85 / ddcSendRecv.c:126-225), one 24-double sum all-reduce (energyInfo.c:37) and one int all-gather (the
 * rebuild's count round), each verified on the receiver.  Collective.  On a mismatch, or when timeout_s (<= 0: 60 s) passes without
 * completion, the call returns DDCMI_ECOMM on EVERY rank and ddcmi_last_error says which stage, peer rank and direction failed;
 * after a timeout the RCCL communicator has been aborted (start a fresh process for another transport).  The all-gather also carries a
 * hash of what every rank must have been given alike (box, cut-offs, neighbour settings, LJ table, species, molecule tables, term counts,
 * groups, barostat, process grid: set them BEFORE the preflight): a rank set up from another deck ends the launch with DDCMI_EINVAL on
 * every rank, named ([4]; [5] = -1).
 * report (may be NULL): [0] distinct peer ranks, [1] directions exchanged, [2] bytes per direction message, [3] 1 if a peer was
 * named, [4] that peer, [5] its direction code, [6] stages verified (3 = all), [7] elapsed microseconds, [8..15] the peer ranks. [sync] */
int ddcmi_comm_preflight(ddcmi_ctx *ctx, double timeout_s, int64_t report[16]);
/* ---- process rendezvous without MPI (host/rdzv.c) ----------------------------
 * ddcMD takes rank, size, MPI_Bcast, MPI_Barrier and MPI_Allreduce from its MPI launcher
 * (ddcMD.c:93-139; energyInfo.c:9-63).  A one-process-per-GPU launch without MPI hands each
 * process RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT only; these calls turn that into a
 * full mesh of TCP streams.  Rank 0 listens on (addr, port); with port <= 0 (the launcher
 * itself occupies MASTER_PORT, as torch.distributed.run does) rank 0 binds an ephemeral port
 * and publishes it in port_file, which the other ranks poll.  All calls are collective,
 * blocking, and fail with DDCMI_ECOMM after timeout_s (<= 0: 300 s) instead of hanging. */
typedef struct ddcmi_rdzv ddcmi_rdzv;
int ddcmi_rdzv_create(ddcmi_rdzv **out, int rank, int world, const char *addr, int port, const char *port_file, double timeout_s);
void ddcmi_rdzv_destroy(ddcmi_rdzv *h);
/* leave the job at once (a rank that failed where its peers already wait for it): every stream is shut down, the peers'
 * transfers fail with "peer closed" instead of waiting out their timeout.  The handle stays valid for ddcmi_rdzv_destroy. */
void ddcmi_rdzv_abort(ddcmi_rdzv *h);
const char *ddcmi_rdzv_last_error(const ddcmi_rdzv *h);      /* h may be NULL: last create error */
int ddcmi_rdzv_rank(const ddcmi_rdzv *h);
int ddcmi_rdzv_world(const ddcmi_rdzv *h);
int ddcmi_rdzv_bcast(ddcmi_rdzv *h, void *buf, size_t nbytes, int root);                 /* MPI_Bcast: the 128-byte RCCL id */
int ddcmi_rdzv_barrier(ddcmi_rdzv *h);                                                   /* MPI_Barrier */
int ddcmi_rdzv_allreduce_f64(ddcmi_rdzv *h, double *v, int n, int op);                   /* op 0 sum (rank order), 1 max */
int ddcmi_rdzv_allgather(ddcmi_rdzv *h, const void *send, void *recv, size_t nbytes);    /* nbytes per rank */
/* grouped point-to-point exchange, matched like ncclSend/ncclRecv inside one group: the k-th message
 * sent to peer p is the k-th message p receives from this rank */
int ddcmi_rdzv_exchange(ddcmi_rdzv *h, int nsend, const int *send_peer, const void *const *send_buf, const size_t *send_bytes,
                        int nrecv, const int *recv_peer, void *const *recv_buf, const size_t *recv_bytes);
/* Decomposition over the HOST transport: the same migration / halo / all-reduce protocol as
 * ddcmi_comm_init, with every message staged through pinned host memory and carried by the
 * rendezvous' TCP streams instead of RCCL.  For ranks that share one GPU (RCCL refuses two ranks
 * on a device: tests on a single-GPU box) and for nodes without working GPU peer access; rank and
 * size come from the rendezvous, which must outlive the context. */
int ddcmi_comm_init_host(ddcmi_ctx *ctx, ddcmi_rdzv *rdzv, int px, int py, int pz);
/* Call order with decomposition: ddcmi_set_box -> ddcmi_comm_init -> set_* ->
 * ddcmi_upload_state with THIS rank's local beads (any beads inside the box are
 * accepted; the first rebuild migrates them to their owners, ddcAssignment.c) */
int ddcmi_domain_bounds(const ddcmi_ctx *ctx, double lo[3], double hi[3]);
/* current local beads in device order, identified by gid (beads migrate between
 * ranks; ddcMD identifies them by label).  Pointers may be NULL. [sync] */
int ddcmi_download_particles(ddcmi_ctx *ctx, int cap, int *nout, uint64_t *gid, int *species,
                             double *rx, double *ry, double *rz, double *vx, double *vy, double *vz,
                             double *fx, double *fy, double *fz);

#ifdef __cplusplus
}
#endif
#endif

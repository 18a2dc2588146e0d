/*
 * deck.h -- load a ddcMD input deck (object.data + restart + parmfile + atoms
 * file) into one flat, plain-C description of the Martini hot path.
 *
 * Replaces, for this path only, what simulate_init / system_init /
 * martini_parms / mmff_init / collection_read build as pointer graphs
 * (simulate.c:104-297, system.c:79-214, bioMartini.c:1210-1353, bioMMFF.c,
 * collection_read.c:86-200).  Every key and default follows those call sites.
 */
#ifndef DDCMI_DECK_H
#define DDCMI_DECK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the numbers of include/ddcmi.h's group kinds; OTHER: any other GROUP type, refused by ddcmi_set_groups */
enum { DDCMI_GROUP_FREE = 0, DDCMI_GROUP_BERENDSEN = 1, DDCMI_GROUP_LANGEVIN = 2, DDCMI_GROUP_OTHER = 3,
       DDCMI_GROUP_FROZEN = 4, DDCMI_GROUP_FIXEDVELOCITY = 5, DDCMI_GROUP_QUENCH = 6,
       DDCMI_GROUP_EXTFORCE = 7 /* read by the loader (Fzeq); no kind of include/ddcmi.h yet: refused by name where a deck is to run */ };

/* one ANALYSIS object (analysis_init, analysis.c:120-160).  type: the row of host/analysis.c's table that evaluates it; DDCMI_AN_NONE is any
 * other type (not supported: the driver names it once on stderr) */
enum ddcmi_analysis_kind { DDCMI_AN_NONE = 0, DDCMI_AN_PAIRCORRELATION, DDCMI_AN_VAF, DDCMI_AN_VCMWRITE, DDCMI_AN_ZDENSITY, DDCMI_AN_KDIST, DDCMI_AN_DSF, DDCMI_AN_SUBSETWRITE, DDCMI_AN_COARSEGRAIN, DDCMI_AN_CHOL, DDCMI_AN_FORCEAVERAGE };
/* one BIN object of a KINETICENERGYDISTN analysis (kineticEnergyDistn.c:58-83): the histogram of one species' kinetic energies */
typedef struct ddcmi_kdist_group { char *name, *species; double emin, emax; int nbins; } ddcmi_kdist_group;      /* internal energy units; nbins >= 1, emax > emin */
typedef struct ddcmi_analysis
{
   char *name, *type_name;
   enum ddcmi_analysis_kind type;
   int eval_rate, outputrate;
   char *filename;
   int length;                  /* PAIRCORRELATION (paircorrelation.c:68-135): bins; VELOCITYAUTOCORRELATION (velocityAutocorrelation.c:59-60): samples per window behind the origin (>= 1) */
   int rscale_log, method;      /* from here on PAIRCORRELATION only, zero otherwise.  method: 0 geom, 1 grid, 2 neighborList (all evaluated the same way: exactly) */
   double rmin, delta_r;        /* internal length units */
   int nz, smear_method;        /* from here on zdensity only (zdensity.c:36-50), zero otherwise.  nz: bins along z (>= 1); smear_method: 0 impulse, 1 hat */
   double smear_radius;         /* internal length units; <= 0: no smearing */
   int ndist;                   /* from here on KINETICENERGYDISTN only (kineticEnergyDistn.c:45-93), zero otherwise: the BIN objects of distGroups, in list order */
   ddcmi_kdist_group *dist;
   int nm;                      /* from here on DSF only (dsf.c:33-96), zero / NULL otherwise: the list of the `m` key as written (an entry <= 0 adds no wave vector) */
   int *m;
   char *dsf_species;           /* the one species that takes part, or NULL: every bead */
   /* from here on subsetWrite with format = binaryCharmm only (subsetWrite.c:72-139), zero / NULL otherwise.  Internal units; a bound
    * the deck leaves out is the reference's default: -+ the longest box edge (through its "%e") for x, y, z, -+ DBL_MAX for the velocities */
   char *sw_length_unit;        /* lengthUnit, default Ang: the unit of the records' coordinates */
   int sw_modulus, sw_odd, sw_nfiles;      /* nfiles is read and ignored: one file */
   uint64_t sw_idmin, sw_idmax;
   int sw_nid;                  /* idList, sorted ascending; sw_idlist NULL: no such key */
   uint64_t *sw_idlist;
   int sw_nspecies;             /* the names of the species key; 0: every species */
   char **sw_species;
   double sw_rmin[3], sw_rmax[3], sw_vmin[3], sw_vmax[3];
   int sw_given;                /* bit 2 a + q of x, y, z and 6 + 2 a + q of vx, vy, vz: the deck has the key (q = 0 min, 1 max) */
   /* from here on COARSEGRAIN only (coarsegrain.c:80-119), zero otherwise; its smearRadius / smearMethod are smear_radius / smear_method above */
   int cg_n[3];                 /* nx, ny, nz: each >= 1 */
   int cg_output_mode;          /* outputMode 1 (13 fields) or 2 (19 fields, the default); an object with 3 stays unsupported */
   int cg_nfiles;               /* nfiles is read and ignored: one file */
   char *cg_smear_string;       /* smearMethod as the deck spells it (the file's misc_info echoes it) */
   /* from here on cholAnalysis only (cholAnalysis.c:41-71), zero / NULL otherwise.  Internal length units; nbins = lrint((rmax - rmin) / delta) >= 1
    * and delta formed anew as (rmax - rmin) / nbins; chol_gid[7 chol_nmol]: the first seven gids of every CHOL residue of the particle set, in gid order */
   char *chol_potential, *chol_data_filename;
   double chol_rmin, chol_rmax, chol_delta;
   int chol_nbins, chol_nmol;
   uint64_t *chol_gid;
   /* from here on FORCE_AVERAGE only (forceAverage.c:28-73), zero / NULL otherwise.  fa_gid[fa_nid]: idParticle as written, duplicates kept;
    * fa_what: data_type 0 force, 1 velocity, 2 position (any case).  eval_rate and outputrate above default to 1 for this type */
   int fa_nid, fa_what;
   uint64_t *fa_gid;
} ddcmi_analysis;

/* one TRANSFORM object of SIMULATE transform = name ... (transform_init, transform.c:30-60).  type DDCMI_TR_THERMALIZE: thermalizeTransform_parms
 * (thermalizeTransform.c:51-91) as checkInput (:111-175) lets it through; DDCMI_TR_NONE is any other type (not supported: the driver names
 * it once on stderr and never runs it) */
enum ddcmi_transform_kind { DDCMI_TR_NONE = 0, DDCMI_TR_THERMALIZE };
typedef struct ddcmi_transform
{
   char *name, *type_name;
   enum ddcmi_transform_kind type;
   int64_t rate;                /* an integer, atCheckpoint (the checkpoint rate) or atMaxLoop (maxloop); 0: no rate key -- the transform never runs at rate */
   int method;                  /* 0 BOLTZMANN, 1 RESCALE (method matched by its head, or rescale != 0) */
   int select;                  /* 0 global, 1 by species, 2 by group */
   int keep_vcm;
   uint64_t seed;
   int ntemp;                   /* select 0: 1; 1: the system's species; 2: its groups */
   double *temperature;         /* internal energy units (kB = 1); -1 for a class the object does not name (thermalize_init, thermalize.c:44-46) */
} ddcmi_transform;

typedef struct ddcmi_setup
{
   /* SIMULATE (simulate.c:141-169,239-244) */
   int64_t loop, maxloop, deltaloop;
   double time, dt;
   int printrate, snapshotrate, checkpointrate;
   /* BOX (box.c:56-67) */
   double h[9];
   int pbc;
   /* NEIGHBOR (neighbor.c:49-54), DDC (ddc.c:49-107) */
   double deltaR;
   int updateRate;
   int lx, ly, lz;
   /* POTENTIAL type=MARTINI (bioMartini.c:1210-1245, :876-879) */
   double rmax, rcoulomb, epsilon_r, epsilon_rf, krf, crf, keR;
   int excludePotentialTerm;
   int potentialShift;
   /* LJ atom types (mmff->nAtomType) */
   int nlj;
   double *sigma, *eps, *shift;     /* [nlj*nlj]; unset pairs are NaN */
   /* SPECIES in ddcMD index order (molecule order, species.c:30) */
   int nspecies;
   char **species_name;
   double *mass, *charge;
   int *ljtype;       /* getCGLJindexbySpecie (bioMartini.c:952-987) */
   int *moltype;      /* speciesIndexToMoleculeIndex (molecule.c:56) */
   int *resitype;     /* index of the RESIPARMS the species belongs to */
   int *atomoffset;   /* position of the atom inside its residue's atomList */
   /* MOLECULE types + reOrgPairs exclusion lists (bioMartini.c:135-282,1416-1423) */
   int nmoltype;
   int *mol_nspecies, *bpair_off, *bpairI, *bpairJ;
   /* RESIDUE types: bonded terms (genMartiniConn bioMartini.c:571-838) */
   int nresi;
   int *resi_natoms;
   int *bond_off, *bondI, *bondJ;
   double *bond_kb, *bond_b0;
   int *angle_off, *angleI, *angleJ, *angleK, *angle_func;
   double *angle_k, *angle_t0;
   int *tors_off, *torsI, *torsJ, *torsK, *torsL, *tors_func, *tors_n;
   double *tors_k, *tors_delta;
   /* GROUPs (group.c:48-90, berendsen.c:91-113) */
   int ngroup;
   char **group_name;
   int *group_type;
   double *group_Teq, *group_tau;
   int *group_interval;
   /* atoms (collection_read.c:86-200), internal units */
   int natoms;
   double *rx, *ry, *rz, *vx, *vy, *vz;
   uint64_t *gid;
   int *species, *group;
   int nConstraints;
   /* INTEGRATOR / ACCELERATOR */
   char *integrator_type;
   int has_accelerator;
   char *accelerator_type;
   /* PRINTINFO unit strings (printinfo.c:51-64) */
   char *u_pressure, *u_volume, *u_temperature, *u_energy, *u_time, *u_length;
   /* RANDOM seed (random.c:44-60): seeds the Langevin noise */
   uint64_t rng_seed;
   /* POTENTIAL type=RESTRAINT (restraint.c:28-49): restraints by gid, r0 as box fractions */
   int nrest, rest_origin;
   int printMolecularPressure;        /* PRINTINFO printMolecularPressure (printinfo.c:56) */
   int nresicons;                     /* constraint pairs in the residues of the molecules in use (nglfconstraint needs 0 here) */
   /* INTEGRATOR type=NGLFCONSTRAINT (nglfconstraint.c:86-95): T, P0, beta, tauBarostat; beta = 0: no barostat */
   double npt_T, npt_P0, npt_beta, npt_tau;
   uint64_t *rest_gid;
   int *rest_fc;
   double *rest_r0, *rest_kb;
   /* RESIDUE types: distance constraints (CONSLISTPARMS/CONSPARMS, bioMMFF.c:64-104): pairs of residue r are
    * [cons_off[r], cons_off[r+1]); cons_grp = the constraint list (group) of the pair inside its residue */
   int *cons_off, *consI, *consJ, *cons_grp;
   double *cons_r0;
   /* INTEGRATOR type=NGLFGPULANGEVIN (nglfGPU.cu:422-507): isotropic barostat, every bead under group 0's Langevin thermostat */
   int npt_isotropic;
   /* PRINTINFO printStress / printHmatrix (printinfo.c:52-53): stress.data (stress tensor + thermal flux) and hmatrix.data */
   int printStress, printHmatrix;
   char *u_energyflux;                /* PRINTINFO ENERGYFLUX (printinfo.c:35-36), default ueV/Ang^2/fs */
   /* RANDOM type=LCG64 (random.c:44-71, lcg64.c): the particles' own streams, LCG64_PARM {state, multID, prime} per atom in file
    * order -- read from the random field of the atoms records (collection_read.c:160-166) or, when a record carries none,
    * lcg64_default's values for every atom (collection.c:95-109).  random_lcg64 = 0: no such object, the arrays are NULL */
   char *random_name;
   int random_lcg64, lcg_from_file;
   uint64_t *lcg_state;
   uint32_t *lcg_multID, *lcg_prime;
   double *group_vcm;      /* [3 ngroup] LANGEVIN groups: `vcm` (langevin.c:167), internal units; zero otherwise */
   /* SIMULATE analysis = name ... (analysis.c:120-160): every ANALYSIS object in the list, in list order */
   int nanalysis;
   ddcmi_analysis *analysis;
   /* GROUP type FIXEDVELOCITY (fixedVelocity.c): group_vset[g] = 1 where the object has a `v` key, group_v[3 g ..] its value; type EXTFORCE
    * (extforce.c): group_Fz[g] = the constant of `Fzeq`.  Internal units; zero for every other group */
   int *group_vset;
   double *group_v, *group_Fz;
   /* SIMULATE transform = name ... (simulate.c): every TRANSFORM object in the list, in list order */
   int ntransform;
   ddcmi_transform *transform;
   /* the INTEGRATOR type's group override (its row of ddcmi_integrator_types): DDCMI_GROUPS_ASIS, _FREE, _LANGEVIN0 or _LANGEVIN0_OWN_VCM.  group_type and the
    * groups' parameters above stay as the deck wrote them; ddcmi_integrator_groups gives the groups as the integrator runs them */
   int group_override;
} ddcmi_setup;

/* The INTEGRATOR types of this path (integrator.c:37-167), one row each.  The loader, integrator_init and the refusal of any other type
 * read this table and nothing else. */
enum ddcmi_barostat_form { DDCMI_BARO_SEMI = 0,      /* changeVolume / changeVolumeGPU: x and y together, z alone */
                           DDCMI_BARO_ISOTROPIC,     /* changeVolumeGPUisotropic (molecularPressureGPU.cu:204-239) */
                           DDCMI_BARO_BY_KEY };      /* the `isotropic` key (INT, default 0) chooses between the two */
enum ddcmi_group_override { DDCMI_GROUPS_ASIS = 0,   /* every GROUP object's own thermostat */
                            DDCMI_GROUPS_FREE,       /* every bead gets the free kick (freeVelocityUpdateInterleavedGPU over all beads) */
                            DDCMI_GROUPS_LANGEVIN0,  /* every bead under group 0's tau, kBT and vcm; group 0 must be LANGEVIN */
                            DDCMI_GROUPS_LANGEVIN0_OWN_VCM };      /* the same with every group's own vcm: NGLFGPULANGEVIN as this path has always run it */
enum ddcmi_integrator_class { DDCMI_ICLASS_NGLF = 0, DDCMI_ICLASS_NVTGLF, DDCMI_ICLASS_NGLFCONSTRAINT };      /* the itype integrator_init sets */
typedef struct ddcmi_integrator_type
{
   const char *name;
   int barostat_keys;                        /* T, P0, beta, tauBarostat are read (nglfconstraint_parms); the constraint lists and the barostat are set up */
   enum ddcmi_barostat_form barostat_form;
   enum ddcmi_group_override group_override;
   int host_eligible;                        /* DDCMI_CPU_INTEGRATOR=1 may run it as nglf() on the host */
   enum ddcmi_integrator_class iclass;
} ddcmi_integrator_type;
extern const ddcmi_integrator_type ddcmi_integrator_types[];
int ddcmi_integrator_ntypes(void);
const ddcmi_integrator_type *ddcmi_integrator_type_find(const char *name);      /* NULL: not on this path */
/* "A, B, ... , Z": the names of the table in its order, for the refusal */
void ddcmi_integrator_type_names(char *buf, int len);
/* The groups as the INTEGRATOR type of `s` runs them: type[g] one of DDCMI_GROUP_*, Teq, tau, interval and vcm[3 g ..] per group (each array
 * ngroup long, vcm 3 ngroup; vcm may be NULL).  Returns 0, or -1 with the refusal in err (an unknown type; an override to group 0's Langevin
 * thermostat on a deck whose first GROUP is not LANGEVIN) */
int ddcmi_integrator_groups(const ddcmi_setup *s, int *type, double *Teq, double *tau, int *interval, double *vcm, char *err, int errlen);

/* lcg64_default over n particles in order (lcg64.c:98-110, primes.c:35-63 with prime_init(30000, task, ntasks), ddcMD.c:70) */
void ddcmi_lcg64_default(int n, const uint64_t *label, unsigned task, unsigned ntasks, uint64_t *state, uint32_t *multID, uint32_t *prime);

/* Load a deck.  object_file is required; restart_file may be NULL (then
 * "restart" next to object_file is tried, as run_ddcMD_CPU.sh does).  Relative
 * file names inside the deck (parmfile, atoms files) resolve against the
 * directory of object_file.  Returns NULL and fills err on failure. */
ddcmi_setup *ddcmi_deck_load(const char *object_file, const char *restart_file, char *err, int errlen);
/* Same, but additional object text (e.g. overriding the integrator/group
 * objects as SURVEY 8c prescribes) is compiled after the files. */
ddcmi_setup *ddcmi_deck_load_with(const char *object_file, const char *restart_file, const char *extra_objects, char *err, int errlen);
void ddcmi_setup_free(ddcmi_setup *s);
int ddcmi_setup_sizeof(void);

/* CRC-32 of the record checksums (crc32.c:46-84 of the reference: standard IEEE CRC-32) */
uint32_t ddcmi_crc32(const unsigned char *p, size_t n);

#ifdef __cplusplus
}
#endif
#endif

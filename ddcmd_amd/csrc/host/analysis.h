/* analysis.h -- the ANALYSIS objects of a deck (analysis.h:49-63, analysis.c:130-160 of the reference): one table of the supported
 * types in analysis.c, read by the deck loader (the type's keys) and by the driver (its state and its hooks). */
#ifndef DDCMI_ANALYSIS_H
#define DDCMI_ANALYSIS_H
#include "plugin.h"
#include "object.h"

/* a row of the table.  `prefix` is matched against the head of the type name, in any case (analysis.c:178), and so is every entry of
 * `heads` (analysis.c:231-233: DSF | DynamicStructureFactor | Dynamic_Structure_Factor) -- or, with `full_name` set, `prefix` is
 * matched against the whole type name and against `alias` (analysis.c:240,317: vcmWrite | vcm_write, zdensity) */
typedef struct analysis_type_st
{
   const char *prefix;
   enum ddcmi_analysis_kind type;
   const char *filename;                                   /* default of the `filename` key */
   /* the type's own keys, and the check of all of them: a refusal is written to msg, which holds the list's latest refusal so far */
   void (*parms)(const OBJECT *obj, ddcmi_analysis *an, char *msg, int msglen);
   void *(*init)(SIMULATE *simulate, const ddcmi_analysis *an);      /* the run-time state, handed to the hooks below */
   void (*eval)(SIMULATE *simulate, const ddcmi_analysis *an, void *state);
   void (*output)(SIMULATE *simulate, const ddcmi_analysis *an, void *state);
   void (*clear)(SIMULATE *simulate, const ddcmi_analysis *an, void *state);      /* NULL: analysis_NULL of the reference */
   void (*free)(void *state);
   int full_name;                                          /* the whole type name must match, not its head */
   const char *alias;                                      /* a second spelling (full_name rows), or NULL */
   const char *const *heads;                               /* further heads (rows matched by the head), NULL-terminated, or NULL */
} ANALYSIS_TYPE;
const ANALYSIS_TYPE *analysis_type_find(const char *type_name);      /* NULL: not supported */
/* pinfoMaxIndex (pinfo.c:148-151) of that many distinct group, species and type names fits the 4-byte field of a binaryCharmm record */
int ddcmi_pinfo_fits(int ngroups, int nspecies, int ntypes);

/* the driver's walks over the supported analyses of simulate->setup, in the order of the deck's list */
void analysis_init_all(SIMULATE *simulate);                           /* names every other analysis once on stderr */
void analysis_startup_all(SIMULATE *simulate);                        /* analysis_startup, analysis.c:133-138: eval if due, then clear */
int64_t analysis_next_stop(const SIMULATE *simulate, int64_t endLoop); /* findEndLoop, masters.c:277-282: the eval and output rates */
void analysis_do_all(SIMULATE *simulate);                             /* doAnalysis, masters.c:503-505: eval if due, then output if due */
void analysis_free_all(void);

/* what the analyses take from the driver (plugin.c; not exported from the library) */
typedef struct { int rank, world, local_rank, grid[3], host_transport; ddcmi_rdzv *rdzv; } PARENV;
extern PARENV par __attribute__((visibility("hidden")));
void die(const char *where, const char *msg) __attribute__((visibility("hidden")));
#endif

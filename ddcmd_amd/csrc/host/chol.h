/* chol.h -- ANALYSIS cholAnalysis on the host side of ddcmi_chol_offsets: completing the molecules that are split over ranks. */
#ifndef DDCMI_HOST_CHOL_H
#define DDCMI_HOST_CHOL_H
#include <stddef.h>
#include <stdint.h>
#include "ddcmi.h"

/* frag[nfrag]: the ranks' fragments, rank after rank; gid[7 nmol]: the list the device pass was given; L, pbc: the orthorhombic
 * box; rmin, delta, nbins as given to the device pass.  counts[2 nbins], *ndone and stats[6] hold the ranks' merged result (counts
 * and ndone added, sums added in rank order, minimum of the minima, maximum of the maxima) and receive the completed molecules in
 * ascending molecule order, each with the device lane's operations: the same dR1, dR5 and bins as whole on one device.
 * Returns 0; or -1 with a message in err and nothing changed: a molecule with fewer than seven fragments after the merge (the
 * message names the molecule and the first missing gid), a (molecule, role) given twice, a fragment outside the list. */
int ddcmi_chol_complete(int64_t nfrag, const ddcmi_chol_fragment *frag, int64_t nmol, const uint64_t *gid, const double L[3], int pbc, double rmin,
                        double delta, int nbins, int64_t *counts, int64_t *ndone, double *stats, char *err, size_t errlen);
/* r[7][3] of one molecule: d = {dR1, dR5} and, with bin, their bins */
void ddcmi_chol_molecule(const double r[21], const double L[3], int pbc, double rmin, double delta, int nbins, double d[2], int bin[2]);
#endif

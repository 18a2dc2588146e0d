#!/usr/bin/env python3
"""One ANALYSIS PAIRCORRELATION evaluation (ddcmi_pair_correlation: records, cell sort, histogram, copy out) timed on the host clock
around the [sync] call, on a state after a few steps:
   python3 tools/time_pair_correlation.py [water:<lattice> | lipid:<x,y,z>] ...   (default: water:64 water:102 lipid:12,12,6)
rmax 15 A, 150 bins; prints ms per evaluation (median of 10 after 2 warm-up calls)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ddcmd_amd
from ddcmd_amd.martini import MartiniHIP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def system(spec):
    kind, arg = spec.split(":")
    if kind == "water":
        return ddcmd_amd.make_water_setup(int(arg)), "water"
    from ddcmd_amd.deck import load_deck
    from ddcmd_amd.synth import replicate_setup
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    s = load_deck(os.path.join(deck, "object_nvt.data"), restart_file=os.path.join(deck, "relaxed", "restart"))
    return replicate_setup(s, tuple(int(x) for x in arg.split(","))), "bilayer"


for spec in (sys.argv[1:] or ["water:64", "water:102", "lipid:12,12,6"]):
    s, name = system(spec)
    m = MartiniHIP(s)
    m.eval_forces()
    m.step(10)
    nbins = 150
    dr = ddcmd_amd.units_convert(15.0, "Angstrom", None) / nbins
    for _ in range(2):
        c, nb = m.pair_correlation(0.0, dr, nbins)
    t = []
    for _ in range(10):
        t0 = time.perf_counter()
        c, nb = m.pair_correlation(0.0, dr, nbins)
        t.append(time.perf_counter() - t0)
    pairs = int(c.sum())
    ncombo = c.shape[0]
    print("%-8s %9d beads %3d species %5d combos: %8.3f ms per evaluation (min %.3f), %.3g counted pairs (%.1f per bead)"
          % (name, s.natoms, s.nspecies, ncombo, 1e3 * np.median(t), 1e3 * min(t), pairs, pairs / s.natoms), flush=True)
    m.close()

"""A deck with CHOL residues for the cholAnalysis loader and driver tests (helper module, no tests in here): the golden lipid deck with
one residue renamed to CHOL in every text file -- residue, species and atoms records alike.  DPPC (12 beads: the first seven are the
roles) gives 120 CHOL molecules among water; TSTM (5 beads) gives a CHOL residue that is too short."""
import os
import shutil

HERE = os.path.dirname(os.path.abspath(__file__))
LIPID = os.path.join(HERE, "golden", "lipid_deck")
SIM = "simulate SIMULATE { %sdeltaloop = 20; maxloop = 20; printrate = 5; snapshotrate = 10; checkpointrate = 100000; }\n"
CHOL = "chol ANALYSIS { type = cholAnalysis; eval_rate = 10; outputrate = 20; rmin = -6 Angstrom; rmax = 6 Angstrom; delta = 0.25 Angstrom; }\n"


def chol_deck(tmp_path, name="deck", residue="DPPC"):
    """a copy of the lipid deck under tmp_path/name with `residue` renamed to CHOL; returns the directory"""
    d = tmp_path / name
    shutil.copytree(LIPID, str(d))
    for top, _, files in os.walk(str(d)):
        for f in files:
            p = os.path.join(top, f)
            raw = open(p, "rb").read()
            if residue.encode() in raw:
                open(p, "wb").write(raw.replace(residue.encode(), b"CHOL"))
    return d

"""GPU tests (-m gpu) of the ANALYSIS type subsetWrite with format = binaryCharmm in the ddcmi_md driver on the golden water deck:
the files snapshot.<loop>/subset#000000 at the output loops, read back by analysis.read_subset and held against the restart
snapshot of the same loop; the run itself unchanged; a filter's count; two ranks against one; the reference's shipped waterbox deck.

The positions' bound: a record holds (float)((r - corner) * cL) of the device's double r; the restart file prints the same r with 14
significant digits, so the float of (r_restart - corner) * cL is the record's or its neighbour: at most one ulp of float32 at the box
length."""
import glob
import os

import numpy as np
import pytest

from ddcmd_amd.analysis import read_subset
from ddcmd_amd.deck import load_deck
from ranks import copy_deck, run_driver

pytestmark = pytest.mark.gpu
SIM = "simulate SIMULATE { %sdeltaloop = 20; maxloop = 20; printrate = 5; snapshotrate = 10; checkpointrate = 100000; }\n"
ALL = "w ANALYSIS { type = subsetWrite; format = binaryCharmm; outputrate = 10; }\n"


def _frames(d, name="subset"):
    return {int(os.path.basename(os.path.dirname(f)).split(".")[1]): f for f in glob.glob(str(d / "snapshot.*" / (name + "#000000")))}


def _restart_atoms(path):
    """{gid: (species name, group name, r[3] in Angstrom)} of a FIXRECORDASCII atoms file"""
    raw = open(path, "rb").read()
    head = raw[:raw.index(b"\n}\n") + 3].decode()
    lrec = int(head.split("lrec=")[1].split(";")[0])
    nrec = int(head.split("nrecord=")[1].split(";")[0])
    body = raw[len(raw) - lrec * nrec:]
    out = {}
    for k in range(nrec):
        w = body[k * lrec:(k + 1) * lrec].decode().split()
        out[int(w[1])] = (w[3], w[4], [float(w[5]), float(w[6]), float(w[7])])
    return out


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    t = tmp_path_factory.mktemp("subset")
    plain, with_an = copy_deck(t, "water_deck", "plain"), copy_deck(t, "water_deck", "frames")
    return plain, run_driver(plain, SIM % ""), with_an, run_driver(with_an, SIM % "analysis = w; " + ALL)


def test_frames_at_the_output_loops_hold_the_restart_snapshots_positions(runs):
    plain, _, d, outs = runs
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    s = load_deck(str(d / "object.data"))
    frames = _frames(d)
    assert sorted(frames) == [10, 20]      # nothing at start-up
    assert not glob.glob(str(d / "snapshot.*" / "*.tmp"))
    ng = max(1, s.ngroup)
    for loop, f in sorted(frames.items()):
        hdr, rec = read_subset(f)
        assert hdr["nrecord"] == len(rec) == s.natoms and hdr["loop"] == loop and hdr["nfiles"] == 1 and hdr["lrec"] == 24
        assert hdr["species"] == s.species_name and hdr["groups"] == (s.group_name or ["group"]) and hdr["types"] == ["ATOM"]
        assert hdr["field_units"] == ["1", "1", "Ang", "Ang", "Ang"]
        box = open(os.path.join(os.path.dirname(f), "restart")).read().split("h  =")[1].split(";")[0].split()      # (the deck's barostat moves the box)
        assert hdr["h"] == pytest.approx([float(x) for x in box], rel=1e-13, abs=1e-13)
        L = np.array(hdr["h"])[[0, 4, 8]]
        ulp = float(np.spacing(np.float32(L.max())))
        atoms = _restart_atoms(os.path.join(os.path.dirname(f), "atoms#000000"))
        assert sorted(atoms) == sorted(rec["id"].tolist()) == sorted(s.gid.tolist())
        want = np.array([atoms[int(g)][2] for g in rec["id"]]) + 0.5 * L
        err = np.abs(rec["r"].astype(np.float64) - want.astype(np.float32).astype(np.float64))
        print(loop, "largest difference / ulp", err.max() / ulp)
        assert err.max() <= ulp
        pinfo = np.array([(s.group_name.index(atoms[int(g)][1]) if s.group_name else 0) + ng * s.species_name.index(atoms[int(g)][0]) for g in rec["id"]])
        assert np.array_equal(rec["pinfo"], pinfo)
    a, b = read_subset(frames[10])[1], read_subset(frames[20])[1]
    assert np.array_equal(a["id"], b["id"]) and not np.array_equal(a["r"], b["r"])      # the beads moved


def test_the_run_is_bit_identical_with_and_without_the_analysis(runs):
    plain, _, d, _ = runs
    assert open(str(plain / "data"), "rb").read() == open(str(d / "data"), "rb").read()
    assert os.path.getsize(str(d / "data")) > 0 and not _frames(plain)
    for loop in (10, 20):
        f = "snapshot.%012d/atoms#000000" % loop
        strip = lambda raw: raw[raw.index(b"\n}\n"):]      # (the headers carry their creation times)
        assert strip(open(str(plain / f), "rb").read()) == strip(open(str(d / f), "rb").read())


def test_a_filter_selects_its_count(runs, tmp_path):
    d = copy_deck(tmp_path, "water_deck", "filtered")
    s = load_deck(str(d / "object.data"))
    name = s.species_name[-1]
    outs = run_driver(d, SIM % "analysis = w; " + "w ANALYSIS { type = subset_write; format = binaryCharmm; outputrate = 10; modulus = 3; species = %s; filename = third; }\n" % name)
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    want = np.sort(s.gid[(s.gid % np.uint64(3) == 0) & (s.species == s.nspecies - 1)])
    frames = _frames(d, "third")
    assert sorted(frames) == [10, 20] and 0 < len(want) < s.natoms and not _frames(d)
    for f in frames.values():
        hdr, rec = read_subset(f)
        assert hdr["nrecord"] == len(want) and np.array_equal(np.sort(rec["id"]), want) and hdr["modulus"] == "3"
    assert open(str(runs[0] / "data"), "rb").read() == open(str(d / "data"), "rb").read()


def test_two_ranks_write_the_record_set_of_one(runs, tmp_path):
    _, _, d1, _ = runs
    d2 = copy_deck(tmp_path, "water_deck", "two")
    outs = run_driver(d2, SIM % "analysis = w; " + ALL, world=2)
    assert not [l for o in outs for l in o[1].splitlines() if "not supported" in l]
    s = load_deck(str(d2 / "object.data"))
    f1, f2 = _frames(d1), _frames(d2)
    assert sorted(f1) == sorted(f2) == [10, 20]
    for loop in (10, 20):
        (h1, a), (h2, b) = read_subset(f1[loop]), read_subset(f2[loop])
        assert h1["nrecord"] == h2["nrecord"] == s.natoms and len(np.unique(b["id"])) == len(b)
        ulp = float(np.spacing(np.float32(max(h1["h"]))))
        a, b = np.sort(a, order="id"), np.sort(b, order="id")
        assert np.array_equal(a["id"], b["id"]) and np.array_equal(a["pinfo"], b["pinfo"])
        # the ranks add the forces in another order: after 20 steps a coordinate may round to the neighbouring float
        assert np.abs(a["r"].astype(np.float64) - b["r"].astype(np.float64)).max() <= ulp


def test_the_shipped_waterbox_deck_runs_and_writes_nothing_in_ten_steps(tmp_path):
    d = copy_deck(tmp_path, "ref_waterbox", "ref")
    outs = run_driver(d, "simulate SIMULATE { analysis = writeCharmm; }\n")
    assert not [l for l in outs[0][1].splitlines() if "not supported" in l]
    assert not _frames(d) and os.path.getsize(str(d / "data")) > 0      # outputrate = 10000 is never reached
    d0 = copy_deck(tmp_path, "ref_waterbox", "ref_as_shipped")
    run_driver(d0, "")
    assert open(str(d0 / "data"), "rb").read() == open(str(d / "data"), "rb").read()

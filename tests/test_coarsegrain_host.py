"""CPU tests of the COARSEGRAIN analysis's host side: the longdouble reference of coarsegrain_eval (tests/coarsegrain_systems.py) on
hand-placed beads, one per corner case; analysis.CoarseGrain's file and analysis.read_cgrid, its inverse -- lrec for grids whose label
needs 1, 2 and 3 bytes, every record's checksum, the byte order of the `b` fields (most significant byte first), the f4 rounding
(float)(sum * convert * (1 / nsteps)) -- and the merge of ranks with duplicate keys."""
import zlib

import numpy as np
import pytest

import coarsegrain_systems as cgs
from ddcmd_amd.analysis import CG_RECORD, CoarseGrain, b_field_size, merge_cg_records, read_cgrid
from ddcmd_amd.deck import units_convert

L = np.array([48.0, 56.0, 64.0])
MASS = np.array([72.0, 36.0])


def beads(r, v=None, species=None):
    r = np.asarray(r, float).reshape(-1, 3)
    n = len(r)
    v = np.zeros((n, 3)) if v is None else np.asarray(v, float).reshape(-1, 3)
    return {"r": [r[:, a].copy() for a in range(3)], "v": [v[:, a].copy() for a in range(3)], "species": np.zeros(n, np.int32) if species is None else np.asarray(species, np.int32),
            "gid": np.arange(n, dtype=np.uint64)}


def ref(p, grid=(3, 2, 5), pbc=7, sr=0.0, method="impulse", ns=2):
    return cgs.reference(p, MASS, L, pbc, grid[0], grid[1], grid[2], ns, sr, method)


def test_label_has_x_slowest_and_sums_are_the_beads():
    # cells of 16 x 28 x 12.8: the bead sits in (igx, igy, igz) = (2, 0, 3)
    p = beads([[10.0, -5.0, 8.0]], v=[[0.5, -0.25, 2.0]], species=[1])
    (key, e), = ref(p).items()
    assert key == (3 + 5 * (0 + 2 * 2), 1) and e.n_terms == 1
    assert [float(x) for x in e.sums] == [1.0, 36.0, 0.5 * 36.0 * 0.25, 0.5 * 36.0 * 0.0625, 0.5 * 36.0 * 4.0, 18.0, -9.0, 72.0]


def test_faces_of_the_box_and_the_wrap():
    # lower face: cell 0; upper face (not wrapped: it is not beyond L / 2): r = n, clamped to n - 1; beyond: wrapped to the other side
    p = beads([[-24.0, 0.0, 0.0], [24.0, 0.0, 0.0], [24.5, 0.0, 0.0], [-24.5, 0.0, 0.0]])
    igx = sorted(k[0] // 10 for k in ref(p))
    assert igx == [0, 2] and ref(p)[(0 * 10 + 1 * 5 + 2, 0)].n_terms == 2 and ref(p)[(2 * 10 + 1 * 5 + 2, 0)].n_terms == 2
    # an open axis does not wrap: the bead beyond the face is clamped into the last layer
    assert sorted(k[0] // 10 for k in ref(beads([[30.0, 0.0, 0.0], [-30.0, 0.0, 0.0]]), pbc=6)) == [0, 2]
    # NaN: cell 0 on that axis
    assert [k[0] for k in ref(beads([[np.nan, 27.0, 31.0]]))] == [0 * 10 + 1 * 5 + 4]


def test_a_bead_on_a_cell_face_belongs_to_the_upper_cell():
    (k,), = [list(ref(beads([[-24.0 + 16.0, -28.0 + 28.0, -32.0 + 2 * 12.8]])))]
    igz = k[0] % 5
    assert k[0] // 10 == 1 and (k[0] // 5) % 2 == 1 and igz in (1, 2)      # (2 x 12.8 is not exact: either side of the face, as the doubles say)


def test_smearing_impulse_and_hat_weights():
    # lSmear = min(2 x 3, cell) = 6 length units; the bead 0.25 cells above the wall between x cells 0 and 1: delta = -0.25 (grid units)
    p = beads([[-24.0 + 16.0 + 4.0, 1.0, 1.0]])
    for method, w0 in (("impulse", 0.5 + (-0.25) * (1.0 / 6.0)), ("hat", 0.5 + ((2 * -0.25) * (1.0 / 6.0)) * (1.0 - 0.25 * (1.0 / 6.0)))):
        r = ref(p, sr=3.0, method=method)
        assert len(r) == 8 and all(e.n_terms == 1 for e in r.values())
        wx = {0: 0.0, 1: 0.0}
        for (label, _), e in r.items():
            wx[label // 10] += float(e.sums[0])
        assert wx[0] == pytest.approx(w0, rel=1e-15) and wx[1] == pytest.approx(1.0 - w0, rel=1e-15)
        assert float(sum(e.sums[0] for e in r.values())) == pytest.approx(1.0, abs=4e-16)


def test_the_clamp_of_delta_gives_weights_zero_and_one_and_the_skip():
    # lSmear = 0.25: lSmearHalf = 0.125 (compared with delta in grid units, as the reference does), lSmearInv = 4: |delta| >= 0.125 gives
    # exactly 0 and 1.  x: delta = -0.25 -> w0 = 0, the lower cell is skipped; y, z: at the middle of a cell (delta = +-0.5)
    p = beads([[-24.0 + 16.0 + 4.0, -14.0, 6.4 - 32.0 + 12.8]])
    r = ref(p, sr=0.125)
    assert len(r) == 1 and list(r.values())[0].sums[0] == 1.0
    # delta = -0.125 exactly (2 of 16 length units above the wall): still 0 and 1; just inside: both cells
    assert len(ref(beads([[-24.0 + 16.0 + 2.0, -14.0, -12.8]]), sr=0.125)) == 1
    inside = ref(beads([[-24.0 + 16.0 + 1.0, -14.0, -12.8]]), sr=0.125)
    assert sorted(float(e.sums[0]) for e in inside.values()) == [0.25, 0.75]


def test_smeared_cells_wrap_on_open_axes_too():
    # 0.1 cells above the lower z face, z open: iWall = 0, the lower cell -1 becomes nz - 1 as on a periodic axis
    r = ref(beads([[1.0, 1.0, -32.0 + 1.28]]), pbc=3, sr=20.0)
    assert {k[0] % 5 for k in r} == {0, 4}
    r = ref(beads([[1.0, 1.0, 32.0 - 1.28]]), pbc=3, sr=20.0)      # iWall = nz: the upper cell becomes 0
    assert {k[0] % 5 for k in r} == {0, 4}


def table(entries):
    t = np.zeros(len(entries), CG_RECORD)
    for j, (label, sp, n, mass, K, p) in enumerate(entries):
        t[j] = (label, sp, 0, n, mass, K, p)
    return t


def test_merge_of_ranks_with_duplicate_keys():
    a = table([(1, 0, 1.0, 72.0, (1, 2, 3), (4, 5, 6)), (1, 1, 2.0, 72.0, (0, 0, 0), (1, 1, 1)), (9, 0, 1.0, 1.0, (1, 1, 1), (1, 1, 1))])
    b = table([(0, 1, 1.0, 36.0, (7, 7, 7), (7, 7, 7)), (1, 1, 0.5, 18.0, (1, 2, 3), (-1, -1, -1)), (9, 0, 2.0, 3.0, (1, 0, 0), (0, 1, 0)), (10, 0, 1.0, 1.0, (0, 0, 0), (0, 0, 0))])
    m = merge_cg_records([a, np.zeros(0, CG_RECORD), b])
    assert [(int(l), int(s)) for l, s in zip(m["label"], m["species"])] == [(0, 1), (1, 0), (1, 1), (9, 0), (10, 0)]
    assert m["n"].tolist() == [1.0, 1.0, 2.5, 3.0, 1.0] and m["mass"].tolist() == [36.0, 72.0, 90.0, 4.0, 1.0]
    assert m["K"][2].tolist() == [1.0, 2.0, 3.0] and m["p"][2].tolist() == [0.0, 0.0, 0.0] and m["K"][3].tolist() == [2.0, 1.0, 1.0] and m["p"][3].tolist() == [1.0, 2.0, 1.0]
    # rank order is the order of the additions
    x = table([(0, 0, 1e16, 0.0, (0, 0, 0), (0, 0, 0))])
    y = table([(0, 0, 1.0, 0.0, (0, 0, 0), (0, 0, 0))])
    z = table([(0, 0, -1e16, 0.0, (0, 0, 0), (0, 0, 0))])
    assert merge_cg_records([x, y, z])["n"][0] == (1e16 + 1.0) - 1e16 and merge_cg_records([x, z, y])["n"][0] == 1.0
    an = CoarseGrain(2, 2, 3, ["A", "B"])
    an.add(a)
    an.add([b, a])
    assert an.nsteps == 2 and an.table["n"].tolist() == [1.0, 2.0, 4.5, 4.0, 1.0]
    an.clear()
    assert an.nsteps == 0 and len(an.table) == 0


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("grid,lb", [((3, 2, 5), 1), ((16, 4, 4), 1), ((16, 4, 5), 2), ((41, 41, 38), 2), ((41, 41, 41), 3)])
def test_file_round_trip(tmp_path, mode, grid, lb):
    nx, ny, nz = grid
    top = nx * ny * nz - 1
    assert b_field_size(top) == lb and b_field_size(0) == 1 and b_field_size(255) == 1 and b_field_size(256) == 2 and b_field_size(65536) == 3
    names = ["S%d" % k for k in range(300)]      # 300 species: a species_index of two bytes
    an = CoarseGrain(nx, ny, nz, names, output_mode=mode, smear_radius=units_convert(3.0, "Angstrom"), smear_method="HAT", eval_rate=2, outputrate=6)
    assert an.smear_method == "hat" and an.species_bytes == 2 and an.lrec == 4 * (11 if mode == 1 else 17) + lb + 2
    rng = np.random.RandomState(7)
    labels = np.unique(np.concatenate([[0, top, min(top, 258)], rng.randint(0, top + 1, 40)]))
    t = np.zeros(len(labels), CG_RECORD)
    t["label"], t["species"] = labels, rng.randint(0, 300, len(labels))
    t["species"][0], t["species"][-1] = 299, 258
    t["n"], t["mass"] = rng.uniform(0, 9, len(t)), rng.uniform(1e4, 1e6, len(t))
    t["K"], t["p"] = rng.uniform(0, 1e-2, (len(t), 3)), rng.normal(0, 10, (len(t), 3))
    for _ in range(3):
        an.add(t)
    assert an.nsteps == 3
    h = np.diag(L) * units_convert(1.0, "Angstrom")
    path = an.write(str(tmp_path), 12, 240.0, h, version="v")
    assert path.endswith("cgrid#000000") and an.nsteps == 0 and len(an.table) == 0      # written, then cleared
    hdr, rec = read_cgrid(path)
    nf = 13 if mode == 1 else 19
    assert hdr["name"] == "cgrid" and hdr["datatype"] == "FIXRECORDBINARY" and hdr["checksum"] == "CRC32" and hdr["nfiles"] == 1
    assert hdr["nrecord"] == len(t) and hdr["lrec"] == 4 * (nf - 2) + lb + 2 and hdr["nfields"] == nf and hdr["loop"] == 12
    assert hdr["field_types"] == ["u4", "b%d" % lb, "b2"] + ["f4"] * (nf - 3)
    assert " ".join(hdr["field_names"]) == "checksum label species_index number_particles mass Kx Ky Kz U virial px py pz" + (" vir_xx vir_yy vir_zz vir_xy vir_xz vir_yz" if mode == 2 else "")
    assert " ".join(hdr["field_units"]) == "1 1 1 1 amu eV eV eV eV eV amu*Angstrom/fs amu*Angstrom/fs amu*Angstrom/fs" + (" eV" * 6 if mode == 2 else "")
    assert (hdr["nx"], hdr["ny"], hdr["nz"], hdr["nSamples"]) == (nx, ny, nz, 3) and hdr["species"] == names
    assert hdr["smearMethod"] == "HAT" and float(hdr["smearRadius"]) == pytest.approx(3.0) and hdr["ouputrate"] == "6" and hdr["eval_rate"] == "2"
    assert hdr["h"] == pytest.approx(list(np.diag(L).ravel()))
    assert rec["label"].tolist() == t["label"].tolist() and rec["species_index"].tolist() == t["species"].tolist()
    # the f4 rounding: three equal evaluations added, times convert, times (1.0 / 3), left to right in double, then one rounding
    inv = 1.0 / 3.0
    mc, ec, pc = units_convert(1.0, None, "amu"), units_convert(1.0, None, "eV"), units_convert(1.0, None, "amu*Angstrom/fs")
    three = lambda x: (x + x) + x
    assert np.array_equal(rec["number_particles"], (three(t["n"]) * inv).astype(np.float32))
    assert np.array_equal(rec["mass"], (three(t["mass"]) * mc * inv).astype(np.float32))
    for a, c in enumerate("xyz"):
        assert np.array_equal(rec["K" + c], (three(t["K"][:, a]) * ec * inv).astype(np.float32))
        assert np.array_equal(rec["p" + c], (three(t["p"][:, a]) * pc * inv).astype(np.float32))
    zeros = ["U", "virial"] + (["vir_xx", "vir_yy", "vir_zz", "vir_xy", "vir_xz", "vir_yz"] if mode == 2 else [])
    assert all(not rec[f].any() for f in zeros)
    # the bytes: checksum in native order over the rest of the record; the b fields most significant byte first
    raw = open(path, "rb").read()
    body = raw[len(raw) - hdr["nrecord"] * hdr["lrec"]:]
    for k in range(len(t)):
        line = body[k * hdr["lrec"]:(k + 1) * hdr["lrec"]]
        assert int(np.frombuffer(line[:4], np.uint32)[0]) == zlib.crc32(line[4:]) & 0xffffffff == int(rec["checksum"][k])
        assert line[4:4 + lb] == int(t["label"][k]).to_bytes(lb, "big") and line[4 + lb:6 + lb] == int(t["species"][k]).to_bytes(2, "big")
    assert body[4 + lb:6 + lb] == b"\x01\x2b"      # species 299 = 0x012b
    # a flipped bit is found
    bad = bytearray(raw)
    bad[-1] ^= 1
    open(path, "wb").write(bytes(bad))
    with pytest.raises(ValueError, match="checksum"):
        read_cgrid(path)


def test_refused_constructions():
    with pytest.raises(ValueError, match="at least 1"):
        CoarseGrain(0, 1, 1, ["A"])
    with pytest.raises(ValueError, match="outputMode = 3"):
        CoarseGrain(1, 1, 1, ["A"], output_mode=3)
    with pytest.raises(ValueError, match="nSamples"):
        CoarseGrain(1, 1, 1, ["A"]).file_bytes(0, 0.0, np.eye(3))

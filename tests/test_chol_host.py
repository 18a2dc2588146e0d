"""cholAnalysis without a GPU: the longdouble reference against closed forms, analysis.CholAnalysis' file texts against literal
strings, the host completion of split molecules (ddcmi_chol_complete) against the reference and -- as a stand-alone program under
AddressSanitizer and UBSan -- against hand-computed values, the list helper, and the conditions the GPU tests rely on (the share of
molecules on a bin edge, the sums' bound)."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import chol_systems as C
from chol_systems import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ddcmd_amd", "csrc", "host")


@pytest.fixture(scope="module")
def lib(built):
    from ddcmd_amd import _lib, martini
    h = _lib.load_library()
    martini._declare(h)
    return h


def _right_triangle(h, flip=False):
    """beads 0, 2, 3 a right-angled triangle in the xy-plane, bead 1 at height h; beads 4, 3, 6 one in the xz-plane, bead 5 at y = g"""
    r = np.zeros((7, 3))
    r[2], r[3] = (3.0, 0.0, 0.0), (0.0, 4.0, 0.0)
    if flip:
        r[2], r[3] = r[3].copy(), r[2].copy()
    r[1] = (0.7, -1.1, h)
    r[4] = r[3] + (0.0, 0.0, 2.0)
    r[6] = r[4] + (5.0, 0.0, 0.0)
    r[5] = r[4] + (0.3, 2.0 * h, 0.9)
    return r


@pytest.mark.parametrize("h", [0.0, 0.375, -2.5, 7.0])
def test_reference_closed_forms(h):
    box = np.array([100.0, 100.0, 100.0])
    d1, d5 = C.reference(_right_triangle(h)[None], box, 7)
    assert d1[0] == LD(h)                      # B x C = (0, 0, 12): dR1 = 12 h / 12
    # E = (0, 0, -2), F = (5, 0, 0): E x F = (0, -10, 0), D = (0.3, 2 h, 0.9): dR5 = -(-20 h) / 10
    assert d5[0] == LD(2.0 * h)
    e1, _ = C.reference(_right_triangle(h, flip=True)[None], box, 7)
    assert e1[0] == LD(-h)                     # the triangle walked the other way round: the normal turns over
    # a molecule across the periodic +x face is the same molecule
    r = _right_triangle(h) + (48.0, 0.0, 0.0)
    r[:, 0] -= 100.0 * np.rint(r[:, 0] / 100.0)
    w1, w5 = C.reference(r[None], box, 7)
    assert w1[0] == d1[0] and w5[0] == d5[0]
    o1, _ = C.reference(r[None], box, 6)       # x open: the images are taken as they are
    assert o1[0] == -d1[0]                     # B = (-97, 0, 0) unwrapped: the normal turns over


def test_reference_collinear_is_nan_and_goes_to_bin_0():
    r = _right_triangle(1.0)
    r[3] = (6.0, 0.0, 0.0)
    d1, d5 = C.reference(r[None], np.array([100.0] * 3), 7)
    assert np.isnan(d1[0])
    b, _ = C.bins_of(d1)
    assert b[0] == 0
    assert C.expected_edge_bins()[3] == (0, 20)


def test_chol_analysis_texts():
    from ddcmd_amd.analysis import CholAnalysis
    a = CholAnalysis(-1.0, 1.0, 0.5)
    assert (a.nbins, a.delta) == (4, 0.5)
    a.add([1, 2, 0, 1, 0, 2, 2, 0], [0.5, -0.9, 0.8, 1.0, -0.2, 0.3])
    a.add([0, 0, 3, 3, 0, 3, 3, 0], [0.5, -0.5, 0.75, 1.0, -0.25, 0.25])
    # lc = 0.52917721067 A per internal length unit; cnt1 = cnt3 = 10; ave = 1.0 / 10 and 2.0 / 10
    assert a.data_line(10, 2.5) == "10 2.500000 -0.476259 0.423342 0.052918 -0.132294 0.158753 0.105835\n"
    assert a.distn_text() == (" -3.968829e-01 3.779452e-01 0.000000e+00\n"
                              " -1.322943e-01 7.558905e-01 1.889726e+00\n"
                              " 1.322943e-01 1.133836e+00 1.889726e+00\n"
                              " 3.968829e-01 1.511781e+00 0.000000e+00\n")
    a.clear()
    # no molecule: 0/0 as C prints it, the extremes as they were set
    line = a.data_line(3, 0.0).split()
    assert line[0] == "3" and line[4] == "-nan" and line[7] == "-nan" and line[2].startswith("529177210") and line[3].startswith("-529177210")
    assert a.distn_text().splitlines()[0] == " -3.968829e-01 -nan -nan"


@pytest.mark.parametrize("args", [(0.0, 0.0, 0.1), (1.0, 0.0, 0.1), (0.0, 1.0, 3.0), (0.0, 1.0, 0.0)])
def test_chol_analysis_refuses_no_bins(args):
    from ddcmd_amd.analysis import CholAnalysis
    with pytest.raises(ValueError, match="bins"):
        CholAnalysis(*args)


def test_nbins_is_lrint_and_delta_is_recomputed():
    from ddcmd_amd.analysis import CholAnalysis
    a = CholAnalysis(0.0, 1.0, 0.4)            # 2.5 -> 2 (ties to even)
    assert a.nbins == 2 and a.delta == 0.5
    assert CholAnalysis(0.0, 1.0, 0.3).nbins == 3


@pytest.mark.parametrize("nmol", C.SIZES)
@pytest.mark.parametrize("pbc", [7, 3])
def test_conditions_of_the_gpu_tests(lib, nmol, pbc):
    """what tests/test_gpu_chol.py relies on, held by the reference alone: at most 1 % of the molecules within the rounding bound of
    a bin edge; the planted shapes within the limits d_bound assumes; the host lane within d_bound of the reference and its bins
    equal to the reference's away from the edges; its sums within the sums' bound"""
    from ddcmd_amd import martini
    s = C.made("system", nmol, pbc)
    L = C.box_of(s)
    d1, d5 = C.reference(s.mol_r, L, pbc)
    qb = C.q_bound(L.max())
    b1, q1 = C.bins_of(d1)
    b5, q5 = C.bins_of(d5)
    with np.errstate(invalid="ignore"):
        near = (np.abs(q1 - np.rint(q1)) <= qb) | (np.abs(q5 - np.rint(q5)) <= qb)
    assert near.sum() <= 0.01 * nmol, (int(near.sum()), nmol)
    assert near.sum() == (C.NEAR_EDGE_CASES if s.nedge else 0)
    h = np.array([martini.chol_molecule(lib, m, L, pbc, C.RMIN, C.DELTA, C.NBINS) for m in s.mol_r])
    ok = ~np.isnan(d1.astype(float))
    assert np.abs(h[ok, 0] - d1[ok]).max() <= C.d_bound(L.max()) and np.abs(h[:, 1] - d5).max() <= C.d_bound(L.max())
    far = ~near
    assert (h[far, 2] == b1[far]).all() and (h[far, 3] == b5[far]).all()
    if s.nedge:
        assert [tuple(int(x) for x in row) for row in h[:s.nedge, 2:]] == C.expected_edge_bins()
        assert np.isnan(h[3, 0]) and (h[[0, 1, 2, 4], 0] == [0.5, C.RMIN, C.RMIN - 1.0, 3.9375]).all()
    dmax = max(np.nanmax(np.abs(d1)), np.nanmax(np.abs(d5)))
    for k, d in ((0, d1), (1, d5)):
        fin = ~np.isnan(d.astype(float))
        assert abs(np.sum(h[fin, k].astype(LD)) - np.sum(d[fin])) <= nmol * C.EPS * dmax


def _as_fragments(s, owner):
    """the beads of s's molecules as `nrank` ranks would return them: owner[mol, role] the rank"""
    from ddcmd_amd.martini import CHOL_FRAGMENT
    out = []
    for r in range(int(owner.max()) + 1):
        mol, role = np.nonzero(owner == r)
        f = np.zeros(len(mol), CHOL_FRAGMENT)
        f["mol"], f["role"], f["r"] = mol, role, s.mol_r[mol, role]
        out.append(f)
    return out


def test_completion_against_the_reference(lib):
    from ddcmd_amd import martini
    s = C.made("system", 65, 7)
    L = C.box_of(s)
    rng = np.random.RandomState(5)
    owner = rng.randint(0, 3, (65, 7))
    owner[0] = (0, 1, 1, 1, 1, 1, 1)
    owner[1] = (2, 2, 2, 2, 2, 2, 0)
    frags = _as_fragments(s, owner)
    zero = (np.zeros((3, 2 * C.NBINS), np.int64), np.zeros(3, np.int64), np.tile([0.0, 1e300, -1e300], (3, 2)))
    counts, stats, n = martini.chol_merge(lib, s, s.gid7, C.RMIN, C.DELTA, C.NBINS, *zero, frags)
    d1, d5 = C.reference(s.mol_r, L, 7)
    b1, _ = C.bins_of(d1)
    b5, _ = C.bins_of(d5)
    assert n == 65
    assert (counts[:C.NBINS] == np.bincount(b1, minlength=C.NBINS)).all() and (counts[C.NBINS:] == np.bincount(b5, minlength=C.NBINS)).all()
    h = np.array([martini.chol_molecule(lib, m, L, 7, C.RMIN, C.DELTA, C.NBINS) for m in s.mol_r])
    for k in range(2):      # ascending molecule order: the very additions
        acc = 0.0
        for v in h[:, k]:
            acc += v
        assert stats[3 * k] == acc and stats[3 * k + 1] == h[:, k].min() and stats[3 * k + 2] == h[:, k].max()
    assert abs(stats[0] - float(d1.sum())) <= 65 * C.EPS * float(np.abs(d1).max())


def test_completion_names_the_missing_gid(lib):
    from ddcmd_amd import martini
    s = C.made("system", 65, 7)
    owner = np.zeros((65, 7), int)
    frags = _as_fragments(s, owner)
    keep = ~((frags[0]["mol"] == 40) & (frags[0]["role"] == 5))
    zero = (np.zeros((1, 2 * C.NBINS), np.int64), np.zeros(1, np.int64), np.array([[0.0, 1e300, -1e300] * 2]))
    with pytest.raises(martini.DdcmiError, match=r"molecule 40: gid %d \(role 5\) is owned by no rank" % int(s.gid7[40, 5])):
        martini.chol_merge(lib, s, s.gid7, C.RMIN, C.DELTA, C.NBINS, *zero, [frags[0][keep]])


def test_list_helper_follows_residue_runs_in_gid_order():
    from ddcmd_amd.martini import DdcmiError, chol_molecules
    names = ["POPCxNC3", "CHOLxROH", "CHOLxR1", "WxW"]
    gid, species = [], []
    for res, (sp, n) in enumerate([(0, 3), (1, 8), (3, 1), (1, 8), (3, 1)]):
        for k in range(n):
            gid.append((res << 16) | k)
            species.append(sp if sp != 1 or k == 0 else 2)
    perm = np.random.RandomState(1).permutation(len(gid))
    s = types.SimpleNamespace(gid=np.array(gid, np.uint64)[perm], species=np.array(species, np.int32)[perm], species_name=names)
    g7 = chol_molecules(s)
    assert g7.tolist() == [[(1 << 16) | k for k in range(7)], [(3 << 16) | k for k in range(7)]]
    short = types.SimpleNamespace(gid=np.array([(9 << 16) | k for k in range(6)], np.uint64), species=np.full(6, 1, np.int32), species_name=names)
    with pytest.raises(DdcmiError, match="6 beads"):
        chol_molecules(short)
    none = types.SimpleNamespace(gid=np.arange(4, dtype=np.uint64) << np.uint64(16), species=np.zeros(4, np.int32), species_name=names)
    assert chol_molecules(none).shape == (0, 7)


def test_completion_as_a_stand_alone_program_under_sanitizers(tmp_path):
    """chol.c with a main of its own, -fsanitize=address,undefined, run as its own process: nothing is loaded into Python"""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler"
    exe = str(tmp_path / "chol_standalone")
    subprocess.check_call([cc, "-O1", "-g", "-std=gnu99", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), "-I" + HOST, os.path.join(ROOT, "tests", "chol_standalone_main.c"),
                           os.path.join(HOST, "chol.c"), "-o", exe, "-lm"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    out = p.stdout.splitlines()
    assert out[0] == "rc 0 nfrag 14 ndone 7"
    assert [ln for ln in out if ln.startswith("count")] == ["count 10 1", "count 18 1", "count 47 1", "count 60 1"]
    assert [float(x) for x in out[5].split()[1:]] == [0.0, -3.0, 3.5, 4.75, -3.5, 3.0]
    assert "molecule 1: gid 2006 (role 6) is owned by no rank" in p.stdout
    assert "molecule 0: gid 1000 (role 0) came from two ranks" in p.stdout
    assert "names molecule 3" in p.stdout
    assert "empty: rc 0" in p.stdout
    assert "ERROR" not in p.stderr and "runtime error" not in p.stderr

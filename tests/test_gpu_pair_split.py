"""GPU tests (-m gpu) of the pair kernel's lane splits and row parts on the boxes of tests/pair_split_systems.py: 23 tiles that own exactly
1 ... 600 beads, every one of them cut into k = 1, 2, 3, 4, 6, 8 row parts by the test hook DDCMI_DEBUG_HOOKS=1 DDCMI_DEBUG_TAIL=k.  The
census ddcmi_debug_tile_items (include/ddcmi_test.h) shows that the hook took effect and which (rows per chunk, lanes per bead) the launch
walked; forces, energies and virial are held against the all-pairs longdouble reference of that module.

The bounds.  With u = 2^-53, A_i = sum_j |f_ij|, and the reference's sums of absolute pair terms:
    |f_dev - f_ref| <= C u A_i + Z_i                    per bead and component
    |e_dev - e_ref| <= C u sum |e_ij| + Z_e             lj and ele (ele: + the |self term|)
    |W_dev - W_ref| <= C u sum |f_ij,a d_ij,b| + Z_W    per virial component ab
Z is the price of the tags that bare list entries keep in the lowest nine mantissa bits of a staged z (k_nonbond's comment: z moves by
less than 2^-43 of itself): both beads of a pair move by at most 2^-43 zmax, zmax = Lz / 2 + list radius, so Z_i = 2^-42 zmax sum_j G_ij
with G_ij the largest singular value of d f_ij / d r, Z_e = 2^-42 zmax sum |f_ij|, Z_W = 2^-42 zmax sum (G_ij r_ij + |f_ij|).  It applies
where the entries are bare: types20, and charged_mol as well -- decks of 9 to 16 classes, whose entries once kept the class and only the
shifted-copy flag rode in z, take bare entries since ddcmi_rebuild.inl dropped that middle form.  one_type (packed entries) has Z = 0.
The geometry keeps every pair force above 6e-5 A_i (tests/test_pair_split_systems_host.py asks for 1e-6): a dropped or doubled pair stands
nine orders of magnitude above either term.

C was measured, not derived (v_rcp_f64 / v_rsq_f64 seeds plus one Newton step have no published error bound): the default schedule, no
hook, of the commit before this file, on an MI355X, largest ratio (error - Z) / (u x scale) over beads / components:
                  forces   lj     ele    virial (largest component)      without Z: forces   lj     virial
    one_type      56.0     0.10   -      1.99                                       56.0     0.10   1.99
    charged_mol   < 0      < 0    < 0    < 0     (Z covers the whole error)         40028    506    1009
    types20       < 0      < 0    -      < 0     (Z covers the whole error)         38255    481    994
The largest is 56.0; times 4 for the other summation orders of the splits, 224, rounded up to a power of two: C = 2^8, below the 2^12 at
which this test was to be given up.  The columns without Z show why the bare variants need it: the tags move their forces by 4e4 u A_i."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pair_split_systems as P
from pair_split_worker import context, tile_items, run_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
C = 2.0 ** 8          # (module docstring)
ZTAG = 2.0 ** -42     # two beads of a pair, each moved by less than 2^-43 of its staged |z|
BARE = ("charged_mol", "types20")
FUSED_K = (1, 3, 8)


def ratios(variant, f, e, vir):
    """(error - Z) / (u x scale) of the forces (largest over beads and components), lj, ele and the six virial components against the
    reference; f [3, n] as MartiniHIP.download() returns it"""
    s, ref = P.system(variant), P.system_reference(variant)
    ld = np.longdouble
    z = ld(ZTAG * (0.5 * s.h[8] + s.rmax + s.deltaR)) if variant in BARE else ld(0)
    df = np.abs(np.stack([np.asarray(c, ld) for c in f], 1) - ref["f"])
    out = {"force": float(((df - z * ref["G"][:, None]) / (U * ref["A"][:, None])).max()),
           "lj": float((abs(ld(e["lj"]) - ref["lj"]) - z * ref["G_e"]) / (U * ref["lj_abs"]))}
    if ref["ele_abs"] > 0:
        out["ele"] = float((abs(ld(e["ele"]) - ref["ele"]) - z * ref["G_e"]) / (U * ref["ele_abs"]))
    else:
        assert e["ele"] == 0.0
    dv = (np.abs(np.asarray(vir, ld) - ref["vir"]) - z * ref["G_vir"]) / (U * ref["vir_abs"])
    out.update({"vir_" + name: float(dv[c]) for c, name in enumerate(("xx", "yy", "zz", "xy", "xz", "yz"))})
    return out


def assert_bounds(variant, m, e, vir, tag):
    ref = P.system_reference(variant)
    f = m.download()["f"]
    got = ratios(variant, f, e, vir)
    print("%s %s: (error - Z) / (u x scale): %s" % (variant, tag, "  ".join("%s %.1f" % kv for kv in got.items())))
    assert float(ref["A"].min()) > 0
    for name, x in got.items():
        assert x <= C, (variant, tag, name, x, C)


def census(m):
    rc, n, item, nown = tile_items(m)
    assert rc == 0 and n == len(item)
    return [P.decode_item(int(x)) for x in item], nown


def walked(items, nown):
    out = set()
    for (t, part, nparts), c in zip(items, nown):
        out |= P.split_plan(int(c), part, nparts)
    return out


def assert_tiles(s, items, nown):
    """every tile of the plan among the items with its intended count, nobody else"""
    want = {P.device_tile(s, ijk): c for ijk, (c, _) in s.plan.items()}
    got = {}
    for (t, _, _), c in zip(items, nown):
        assert got.setdefault(t, int(c)) == int(c)
    assert got == want, (got, want)


@pytest.mark.parametrize("variant,k", [(v, k) for v in P.VARIANTS for k in P.NPARTS])
def test_forced_tail(variant, k):
    """DDCMI_DEBUG_TAIL=k: every live tile is cut into parts 0 .. k-1, each once, all carrying nparts == k; the tiles own the intended
    counts; the (R, parts, kb) the items walk are the ones tests/test_pair_split_systems_host.py promised for k; forces, energies and
    virial within the bounds of the module docstring"""
    s = P.system(variant)
    m = context(s, k)
    e, vir = m.eval_forces()
    items, nown = census(m)
    assert_tiles(s, items, nown)
    by_tile = {}
    for t, part, nparts in items:
        assert nparts == k, (t, part, nparts)
        by_tile.setdefault(t, []).append(part)
    assert all(sorted(p) == list(range(k)) for p in by_tile.values()), by_tile
    assert len(items) == k * len(P.COUNTS)
    assert walked(items, nown) == P.plan_union(P.COUNTS, (k,))
    assert_bounds(variant, m, e, vir, "k = %d" % k)
    m.close()


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_fused_steps_equal_split_steps(variant, tmp_path):
    """two steps of ddcmi_step_nglf under k = 1, 3, 8 (the pair kernel with the integrator's pass as its epilogue) against the split step,
    DDCMI_NO_FUSED_STEP=1 -- read once per process: one child process for the three k, under a time limit: positions and velocities
    bit for bit, the same work items"""
    s = P.system(variant)
    fused = {k: run_steps(s, k) for k in FUSED_K}
    env = dict(os.environ)
    env["DDCMI_NO_FUSED_STEP"] = "1"
    out = str(tmp_path / "split.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pair_split_worker.py"), variant, out, ",".join(map(str, FUSED_K))], cwd=ROOT,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0 and "pair_split_worker ok" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    split = dict(np.load(out))
    r0 = np.stack([s.rx, s.ry, s.rz])
    for k in FUSED_K:
        assert np.array_equal(fused[k]["item"], split["item%d" % k]), k
        assert len(fused[k]["item"]) == k * len(P.COUNTS)
        for q in ("r", "v"):
            a, b = fused[k][q], split["%s%d" % (q, k)]
            assert np.array_equal(a, b), (variant, k, q, int((a != b).any(axis=0).sum()), "beads differ")
        assert (fused[k]["r"] != r0).any(axis=0).all(), "a bead did not move"


@pytest.mark.parametrize("variant", P.VARIANTS)
def test_unforced_schedule(variant):
    """without the hook: the same tiles, the same bounds.  Which parts the makespan search chose is printed (shown on failure only)"""
    s = P.system(variant)
    m = context(s, None, hooks=False)
    e, vir = m.eval_forces()
    items, nown = census(m)
    assert_tiles(s, items, nown)
    chosen = {}
    for t, part, nparts in items:
        chosen[nparts] = chosen.get(nparts, 0) + 1
    print(variant, "the search chose {nparts: items}", chosen, "walked", sorted(walked(items, nown)))
    assert_bounds(variant, m, e, vir, "unforced")
    m.close()


def test_hook_needs_debug_hooks_and_refuses_other_values():
    """DDCMI_DEBUG_TAIL without DDCMI_DEBUG_HOOKS is ignored, whatever it holds: the schedule of a context without it.  With
    DDCMI_DEBUG_HOOKS a value outside {1, 2, 3, 4, 6, 8} is refused at ddcmi_create with a message.  A census with too little room
    returns DDCMI_EINVAL and the number of items, and touches neither array"""
    from ddcmd_amd.martini import DdcmiError
    s = P.system("one_type")
    plain = context(s, None, hooks=False)
    plain.eval_forces()
    want = tile_items(plain)[2]
    plain.close()
    for val in (8, 5, "x"):
        m = context(s, val, hooks=False)
        m.eval_forces()
        rc, n, item, nown = tile_items(m)
        assert rc == 0 and np.array_equal(item, want), val
        if val == 8:
            rc, n2, item2, nown2 = tile_items(m, cap=n - 1)
            assert rc != 0 and n2 == n and (item2 == -7).all() and (nown2 == -7).all()
            assert b"work items" in m.lib.ddcmi_last_error(m.ctx)
        m.close()
    for val in (0, 5, 7, 9, 16, -2, "x", "3x", ""):
        with pytest.raises(DdcmiError, match="DDCMI_DEBUG_TAIL"):
            context(s, val)
    m = context(s, 2)      # (and a refusal leaves the next context alone)
    m.eval_forces()
    assert all(nparts == 2 for _, _, nparts in census(m)[0])
    m.close()

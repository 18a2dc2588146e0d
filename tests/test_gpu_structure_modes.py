"""GPU tests (-m gpu) of ddcmi_structure_modes and the in-process group's twin: the density modes rho(k) = sum_j w_j exp(i 2 pi n . t_j),
t_j = (x_j / L_x, y_j / L_y, z_j / L_z), on lists of signed integer wave vectors n, on small synthetic states uploaded directly (internal
units; no list is built).

The yardstick is the same sum in numpy longdouble from the positions a download returns: the quotients, the phase n . t in turns less its
nearest integer, pi, cos and sin all in longdouble.  Its own error, about (|n|_1 / 2) 2^-64 turns of phase, is below 2^-10 of the bound.

The bound per wave vector, u = 2^-53, |n|_1 = |n_x| + |n_y| + |n_z|, to first order:
      B = u (|n|_1 (2 pi T + 3 pi) + C0 + DEPTH(n)) sum |w_j|,      T = max |r_a / L_a| over the selected beads and the axes.
Where it comes from, per bead and vector (k_structure_modes):
  t_a = r_a / L_a, one correctly rounded division: |dt_a| <= u |t_a| <= u T, which moves the phase by 2 pi |n_a| u T: 2 pi T |n|_1 u over the
     axes.  t - rint(t) is exact and leaves |t| <= 1/2;
  phi = fma(n_z, t_z, fma(n_y, t_y, n_x t_x)): three roundings of partial sums of at most |n_x| / 2, (|n_x| + |n_y|) / 2, |n|_1 / 2 turns,
     together at most 1.5 u |n|_1 turns = 3 pi |n|_1 u of phase.  phi - rint(phi) and the doubling are exact;
  sincospi is taken at 4 ulp per component (the OpenCL limit for sinpi / cospi in double; ROCm's table says 2): a component below 1 has
     ulp <= u, so the pair {cos, sin} is off by at most 4 sqrt(2) u;
  w cos and w sin round once each: sqrt(2) u |w|.   C0 = 5 sqrt(2) = 7.08.
DEPTH(n): the additions a term passes through.  A lane adds the selected beads of its workgroup's range one after the other into its
private sum -- at most per_wg additions, per_wg = 256 ceil(ceil(n / 1024) / 256) (one staging trip up to 262144 beads) -- and the second
launch adds the NWG(n) = ceil(n / per_wg) workgroups one after the other: DEPTH = per_wg + NWG - 1, each addition with a relative error
of at most u on a partial sum of at most sum |w| (Higham, Accuracy and Stability of Numerical Algorithms, ch. 4.2).  There is no
reduction across lanes.  Adding r domains on the host adds r.
Largest err / B seen on the device: 0.196 (one bead; 0.03 and less from 63 beads on)."""
import ctypes

import numpy as np
import pytest

from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield, splitmix64

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
C0 = 7.08
MAXN = 1024          # DDCMI_SM_MAX_N
MAXK = 4096          # DDCMI_SM_MAX_K
TILE = 256           # wave vectors per workgroup (CENSUS_THREADS)
EINVAL, EUNSUPPORTED = -2, -4
PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)      # pi to longdouble precision: the double and its residual
BOX = (64.0, 72.0, 96.0)
CHARGE = np.array([1.0, -1.0, 0.0, 0.5, 0.25, 0.0, 0.3, -0.7, 2.0])      # nine species: both signs, two neutral; species 4 has no members
WEIGHTS = ("unit", "charge")
WORST = [0.0]
dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)


def cdiv(a, b):
    return (a + b - 1) // b


def split(n):
    per_wg = cdiv(cdiv(n, 1024), 256) * 256
    return per_wg, cdiv(n, per_wg)


def depth(n):
    per_wg, nwg = split(n)
    return per_wg + nwg - 1


def _rand(n, stream):
    bits = splitmix64(np.arange(n, dtype=np.uint64) + np.uint64(1000003 * (stream + 1))) >> np.uint64(11)
    return bits.astype(np.float64) / 9007199254740992.0


def synthetic(n, box=BOX, charge=CHARGE, empty_species=4, pbc=7):
    """n beads in an orthorhombic box: the species changes from bead to bead (i * 7 % ns: any 64 consecutive beads hold every species
    that has members), one species without members, charges by species"""
    ns = len(charge)
    s = water_forcefield(Setup())
    s.h = np.diag(box).ravel().astype(np.float64)
    s.pbc = pbc
    s.nspecies = ns
    s.species_name = ["S%d" % k for k in range(ns)]
    s.mass = units_convert(72.0, "M_p") * np.ones(ns)
    s.charge = np.asarray(charge, np.float64).copy()
    s.ljtype = (np.arange(ns) % 2).astype(np.int32)
    s.moltype = (np.arange(ns) % 2).astype(np.int32)
    s.resitype = (np.arange(ns) % 2).astype(np.int32)
    s.atomoffset = np.zeros(ns, np.int32)
    s.ngroup = 1
    s.group_name = ["G0"]
    s.group_type = np.zeros(1, np.int32)
    s.group_Teq = np.zeros(1)
    s.group_tau = np.zeros(1)
    s.group_interval = np.ones(1, np.int32)
    s.natoms = n
    i = np.arange(n)
    sp = (i * 7) % ns
    if empty_species is not None:
        sp[sp == empty_species] = (empty_species + 1) % ns
    s.species, s.group = sp.astype(np.int32), np.zeros(n, np.int32)
    s.gid = (i.astype(np.uint64) << np.uint64(32))
    s.rx, s.ry, s.rz = ((_rand(n, k) - 0.5) * box[k] for k in range(3))
    s.vx, s.vy, s.vz = ((_rand(n, 3 + k) - 0.5) * 2e-3 for k in range(3))
    return s


def _ctx(s, **kw):
    from ddcmd_amd.martini import MartiniHIP
    return MartiniHIP(s, **kw)


def vectors(nk, stream=0):
    """nk wave vectors with components from {0, +-1, +-7, +-MAXN}: the first six fixed (mixed signs at the cap, (0,0,0), a duplicate of
    entry 0, all three at -MAXN), the others drawn"""
    fixed = [(MAXN, -MAXN, 7), (0, 0, 0), (1, -7, 0), (MAXN, -MAXN, 7), (-MAXN, -MAXN, -MAXN), (0, 0, -1)]
    pool = np.array([0, 1, -1, 7, -7, MAXN, -MAXN], np.int32)
    draw = pool[(splitmix64(np.arange(3 * nk, dtype=np.uint64) + np.uint64(7919 * (stream + 1))) % np.uint64(7)).astype(np.int64)].reshape(nk, 3)
    kv = np.concatenate([np.array(fixed, np.int32), draw])[:nk]
    return np.ascontiguousarray(kv, np.int32)


# ---- the yardstick ----------------------------------------------------------
def yardstick(s, r, kvec, weight, select=None, index=None):
    """(rho longdouble [nk, 2], count, T, sum |w|) over the selected beads at the positions r (as downloaded)"""
    assert np.finfo(LD).eps <= 2.0 ** -63
    sp = np.asarray(s.species)
    r = [np.asarray(a, np.float64) for a in r]
    if index is not None:
        sp, r = sp[index], [a[index] for a in r]
    keep = np.ones(len(sp), bool) if select is None else (np.asarray(select)[sp] != 0)
    w = (np.asarray(s.charge, np.float64)[sp[keep]] if weight == "charge" else np.ones(int(keep.sum()))).astype(LD)
    t = [r[a][keep].astype(LD) / LD(s.h[4 * a]) for a in range(3)]
    T = max([float(np.abs(x).max()) for x in t]) if len(w) else 0.0
    kvec = np.asarray(kvec).reshape(-1, 3)
    rho = np.zeros((len(kvec), 2), LD)
    for l0 in range(0, len(kvec), 32):      # (blocks of vectors: [32, n] longdoubles at a time)
        kv = kvec[l0:l0 + 32].astype(LD)
        turns = kv[:, 0:1] * t[0][None, :] + kv[:, 1:2] * t[1][None, :] + kv[:, 2:3] * t[2][None, :]
        ph = (2 * PI_LD) * (turns - np.rint(turns))
        rho[l0:l0 + 32, 0], rho[l0:l0 + 32, 1] = (w[None, :] * np.cos(ph)).sum(axis=1), (w[None, :] * np.sin(ph)).sum(axis=1)
    return rho, int(keep.sum()), T, float(np.abs(w).sum())


def bounds(n, kvec, T, sumabs, extra=0):
    """B[nk]"""
    n1 = np.abs(np.asarray(kvec, np.int64).reshape(-1, 3)).sum(axis=1)
    return U * (n1 * (2 * np.pi * T + 3 * np.pi) + C0 + depth(max(n, 1)) + extra) * sumabs * (1 + 2.0 ** -10)


def errors(rho, want):
    dr, di = rho.real.astype(LD) - want[:, 0], rho.imag.astype(LD) - want[:, 1]
    return np.sqrt(dr * dr + di * di)


def assert_modes(got, ref, n, kvec, what="", extra=0, B=None):
    rho, count = got
    want, wcount, T, sumabs = ref
    nk = len(want)
    assert rho.shape == (nk,) and rho.dtype == np.complex128 and count == wcount, (what, rho.shape, count, wcount)
    B = bounds(n, kvec, T, sumabs, extra) if B is None else B
    if sumabs > 0:
        assert np.all(B / sumabs < 1e-9), (what, float((B / sumabs).max()))      # the bound is not vacuous
    err = errors(rho, want)
    ratio = float((err / np.maximum(B, 1e-300)).max()) if sumabs > 0 else 0.0
    WORST[0] = max(WORST[0], ratio)
    print("%s n=%d nk=%d depth=%d: largest err/B %.4f (so far %.4f)" % (what, n, nk, depth(max(n, 1)) + extra, ratio, WORST[0]))
    assert np.all(err <= B), (what, np.argwhere(err > B)[:5], float(err.max()), float(B.min()))
    return B


# ---- exact structure --------------------------------------------------------
@pytest.mark.parametrize("weight", WEIGHTS)
def test_planes_give_peaks_where_their_numbers_divide_the_vector(weight):
    P, L, q = (8, 4, 16), (64.0, 32.0, 128.0), -0.75
    j = np.stack(np.meshgrid(np.arange(P[0]), np.arange(P[1]), np.arange(P[2]), indexing="ij"), -1).reshape(-1, 3)
    n = len(j)
    s = synthetic(n, box=L, charge=np.full(3, q), empty_species=None)
    s.rx, s.ry, s.rz = (L[a] * j[:, a] / P[a] for a in range(3))      # exact in binary
    kvec = np.concatenate([vectors(65), np.array([(8, 4, 16), (-8, 4, -16), (16, -8, 32), (8, 0, 0), (0, 4, -16), (8, 4, 15), (8, 2, 16), (4, 4, 16),
                                                  (MAXN, 0, -MAXN), (MAXN, 7, MAXN), (24, 1, 0), (0, -12, 48)], np.int32)])
    wabs = abs(q) if weight == "charge" else 1.0
    m = _ctx(s)
    r = m.download()["r"]
    rho, count = got = m.structure_modes(kvec, weight=weight)
    B = assert_modes(got, yardstick(s, r, kvec, weight), n, kvec, "planes " + weight)
    assert count == n == 512
    peaks = 0
    for l, v in enumerate(kvec.tolist()):
        if all(v[a] % P[a] == 0 for a in range(3)):
            peaks += 1
            assert abs(abs(rho[l]) - n * wabs) <= B[l] and B[l] / (n * wabs) < 1e-9, (v, rho[l])
        else:
            assert abs(rho[l]) <= B[l], (v, rho[l])
    assert 9 <= peaks <= len(kvec) - 9      # (the two fixed and seven of the listed vectors are peaks for certain)
    m.close()


def test_one_bead_at_the_origin_gives_its_weight_in_every_mode():
    s = synthetic(1, charge=np.full(2, -0.3), empty_species=None)
    s.rx, s.ry, s.rz = np.zeros(1), np.zeros(1), np.zeros(1)
    m = _ctx(s)
    kvec = vectors(TILE + 1)
    for weight, w in (("unit", 1.0), ("charge", -0.3)):
        rho, count = m.structure_modes(kvec, weight=weight)
        assert count == 1 and np.all(rho.real == w) and np.all(rho.imag == 0.0)
    m.close()


# ---- against the yardstick --------------------------------------------------
# n: the wave and block edges; 257: two workgroups; 70001: 274 workgroups; 262147: per_wg = 512, two staging trips per workgroup.
# nk: the wave edges and one full tile of wave vectors +- 1
@pytest.mark.parametrize("n,nk", [(1, 65), (63, 65), (64, 65), (65, 65), (255, 65), (256, 65), (257, 65), (1000, 65), (70001, 9), (262147, 5),
                                  (1000, 1), (1000, 63), (1000, 64), (1000, TILE - 1), (1000, TILE), (1000, TILE + 1)])
def test_random_beads_in_a_non_cubic_box(n, nk):
    s = synthetic(n)
    if n >= 63:
        assert len(np.unique(s.species[:63])) == 8      # every wave holds charges of both signs and neutral beads
    if n == 257:
        assert split(n) == (256, 2)
    if n > 262144:
        assert split(n) == (512, cdiv(n, 512)) and depth(n) == 512 + cdiv(n, 512) - 1      # two trips per workgroup
    kvec = vectors(nk, stream=n)
    if nk >= 6:
        assert (0, 0, 0) in [tuple(v) for v in kvec.tolist()] and np.array_equal(kvec[0], kvec[3]) and np.abs(kvec).max() == MAXN and (kvec < 0).any()
    m = _ctx(s)
    r = m.download()["r"]
    assert all(np.array_equal(a, b) for a, b in zip(r, (s.rx, s.ry, s.rz)))      # inside the box: as uploaded
    for weight in WEIGHTS:
        got = m.structure_modes(kvec, weight=weight)
        assert_modes(got, yardstick(s, r, kvec, weight), n, kvec, "random " + weight)
        again = m.structure_modes(kvec, weight=weight)
        assert got[0].tobytes() == again[0].tobytes() and got[1] == again[1] == n      # bit for bit
        if nk >= 6:
            assert got[0][0].tobytes() == got[0][3].tobytes()      # the duplicate
            sumw = float(np.asarray(s.charge)[s.species].sum()) if weight == "charge" else float(n)
            assert got[0][1].imag == 0.0 and abs(got[0][1].real - sumw) <= U * depth(n) * float(np.abs(np.asarray(s.charge)[s.species]).sum() if weight == "charge" else n)
    m.close()


# ---- invariant 1 ------------------------------------------------------------
@pytest.mark.parametrize("weight", WEIGHTS)
def test_a_vectors_value_does_not_depend_on_the_list(weight):
    n = 1000
    s = synthetic(n)
    m = _ctx(s)
    for v in ((7, -MAXN, 1), (0, 0, 0), (-1, 7, -7)):
        alone = m.structure_modes(np.array([v], np.int32), weight=weight)[0]
        assert alone.shape == (1,)
        seen = [alone[0].tobytes()]
        for nk, places in ((257, (0, 63, 64, 256)), (TILE + 1, (TILE - 1, TILE)), (3 * TILE + 7, (2 * TILE + 65,))):
            for at in places:
                kvec = vectors(nk, stream=at + 1)
                kvec[at] = v
                rho = m.structure_modes(kvec, weight=weight)[0]
                seen.append(rho[at].tobytes())
        assert len(set(seen)) == 1, (v, weight)
    m.close()


# ---- agreement with DSF -----------------------------------------------------
def test_axis_vectors_with_charge_weight_agree_with_the_dsf_modes():
    n, mmax = 1000, 17
    s = synthetic(n)
    m = _ctx(s)
    r = m.download()["r"]
    kvec = np.array([[(mm, 0, 0), (0, mm, 0), (0, 0, mm)] for mm in range(1, mmax + 1)], np.int32)      # [m - 1, axis, 3]
    rho, count = m.structure_modes(kvec.reshape(-1, 3), weight="charge")
    dsf, dcount = m.charge_density_modes(mmax)
    assert count == dcount == n
    ref = yardstick(s, r, kvec.reshape(-1, 3), "charge")
    B_sm = assert_modes((rho, count), ref, n, kvec.reshape(-1, 3), "axes").reshape(mmax, 3)
    # test_gpu_dsf.py's bound: u (m (thmax + 16) + DEPTH) sum |q|, DEPTH = trips + 6 (the wave) + 3 (its four rows) + NWG - 1 under the same split
    per_wg, nwg = split(n)
    thmax = np.array([2 * np.pi * np.abs(r[a] / BOX[a]).max() for a in range(3)])
    B_dsf = U * (np.arange(1, mmax + 1)[:, None] * (thmax[None, :] + 16.0) + (per_wg // 256 + 6 + 3 + nwg - 1)) * ref[3] * (1 + 2.0 ** -10)
    diff = np.abs(rho.reshape(mmax, 3) - dsf.T)
    print("against DSF: largest difference / (B_sm + B_dsf) %.4f" % float((diff / (B_sm + B_dsf)).max()))
    assert np.all(diff <= B_sm + B_dsf)
    m.close()


# ---- selection --------------------------------------------------------------
def test_selection_by_species():
    n = 1000
    kvec = vectors(70, stream=3)
    s = synthetic(n)
    m = _ctx(s)
    r = m.download()["r"]
    for weight in WEIGHTS:
        everything = m.structure_modes(kvec, weight=weight)
        ones = m.structure_modes(kvec, select=np.ones(9, np.int32), weight=weight)
        assert everything[0].tobytes() == ones[0].tobytes() and everything[1] == ones[1] == n      # NULL equals all ones, bit for bit
        for sel in ([0, 1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 0, 0, 0, 7], [0, 0, 1, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0, 0], [0] * 9):
            got = m.structure_modes(kvec, select=sel, weight=weight)
            ref = yardstick(s, r, kvec, weight, select=sel)
            assert_modes(got, ref, n, kvec, "select %s %s" % (sel, weight))
            assert got[1] == int(np.isin(s.species, np.flatnonzero(sel)).sum())
            if ref[3] == 0.0:      # neutral species under the charge weight, the species without members, no species: exact zeros
                assert not got[0].real.any() and not got[0].imag.any()
        assert m.structure_modes(kvec, select=[0, 0, 1, 0, 0, 1, 0, 0, 0], weight=weight)[1] > 0
        assert m.structure_modes(kvec, select=[0, 0, 0, 0, 1, 0, 0, 0, 0], weight=weight)[1] == 0 and m.structure_modes(kvec, select=[0] * 9, weight=weight)[1] == 0
    with pytest.raises(ValueError, match="8 entries of select for 9 species"):
        m.structure_modes(kvec, select=[1] * 8)
    with pytest.raises(ValueError, match="weight"):
        m.structure_modes(kvec, weight="mass")
    m.close()


@pytest.mark.parametrize("pbc", [7, 0])
def test_beads_outside_the_box(pbc):
    """a bead at 1.5 L and one at -0.75 L on every axis: the download moves them by one box side where the box is periodic and leaves
    them where it is open; the phase is that of the downloaded position either way"""
    n = 257
    kvec = vectors(70, stream=pbc)
    s = synthetic(n, pbc=pbc)
    for a, x in enumerate((s.rx, s.ry, s.rz)):
        x[5], x[72] = 1.5 * BOX[a], -0.75 * BOX[a]
    assert s.charge[s.species[5]] != 0 and s.charge[s.species[72]] != 0
    m = _ctx(s)
    r = m.download()["r"]
    for weight in WEIGHTS:
        ref = yardstick(s, r, kvec, weight)
        if pbc == 0:
            assert r[0][5] == 1.5 * BOX[0] and r[2][72] == -0.75 * BOX[2] and ref[2] == 1.5
        else:
            assert r[0][5] == 0.5 * BOX[0] and r[2][72] == 0.25 * BOX[2] and ref[2] <= 0.5
        assert_modes(m.structure_modes(kvec, weight=weight), ref, n, kvec, "outside, pbc %d %s" % (pbc, weight))
    m.close()


# ---- no effect on the run ---------------------------------------------------
def test_the_call_reads_only():
    s = synthetic(1021)
    kvec = vectors(300)
    m = _ctx(s)
    d0 = m.download()
    a = m.structure_modes(kvec, select=[1, 1, 0, 0, 0, 0, 0, 1, 1], weight="charge")
    b = m.structure_modes(kvec, select=[1, 1, 0, 0, 0, 0, 0, 1, 1], weight="charge")
    d1 = m.download()
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert np.concatenate(d0["r"] + d0["v"] + d0["f"]).tobytes() == np.concatenate(d1["r"] + d1["v"] + d1["f"]).tobytes()
    m.close()


# ---- decomposed -------------------------------------------------------------
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_in_process_groups_add_up_to_the_one_domain_result(grid):
    from ddcmd_amd.martini import MartiniGroup, domain_of
    n = 1021
    kvec = vectors(70, stream=11)
    sel = [1, 1, 1, 0, 1, 1, 1, 0, 1]
    s = synthetic(n)
    owner = domain_of(s, grid)
    last = grid[0] * grid[1] * grid[2] - 1
    s.rx = np.where(owner == last, -np.abs(s.rx), s.rx)      # the last domain is left empty
    one = _ctx(s)
    g = MartiniGroup(s, grid)
    nloc = [int(g.lib.ddcmi_nlocal(r.ctx)) for r in g.ranks]
    assert nloc[last] == 0 and sum(nloc) == n
    # the single-context form refuses a context of a group and says where to go
    rho, cnt = np.full((len(kvec), 2), 7.0), np.full(1, 7, np.int64)
    rc = g.lib.ddcmi_structure_modes(g.ranks[0].ctx, 9, None, 0, len(kvec), kvec.ctypes.data_as(ip), rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp))
    msg = g.lib.ddcmi_last_error(g.ranks[0].ctx)
    assert rc == EINVAL and msg.startswith(b"ddcmi_structure_modes") and b"ddcmi_group_structure_modes" in msg and np.all(rho == 7.0) and cnt[0] == 7
    for weight in WEIGHTS:
        want = one.structure_modes(kvec, select=sel, weight=weight)
        ref = yardstick(s, (s.rx, s.ry, s.rz), kvec, weight, select=sel)
        B_one = assert_modes(want, ref, n, kvec, "one domain " + weight)
        pz, pc = g.structure_modes(kvec, select=sel, weight=weight, per_rank=True)
        assert pz.shape == (len(nloc), len(kvec)) and pc.shape == (len(nloc),) and pc.dtype == np.int64
        assert pc[last] == 0 and not pz[last].real.any() and not pz[last].imag.any()      # the empty domain: zeros
        assert pc.sum() == want[1] == ref[1]
        B_ranks = np.zeros(len(kvec))
        for r, rk in enumerate(g.ranks):      # every rank against the yardstick over its own beads
            if nloc[r]:
                rr = yardstick(s, (s.rx, s.ry, s.rz), kvec, weight, select=sel, index=rk.index)
                B_ranks += assert_modes((pz[r], int(pc[r])), rr, nloc[r], kvec, "rank %d %s" % (r, weight))
        tot, count = g.structure_modes(kvec, select=sel, weight=weight)
        assert count == want[1]
        host = len(nloc) * U * ref[3]
        assert np.all(np.abs(tot - want[0]) <= B_one + B_ranks + host)
        assert_modes((tot, count), ref, n, kvec, "group total " + weight, B=B_ranks + host)
    g.close()
    one.close()


# ---- refusals ---------------------------------------------------------------
def test_refused_arguments_leave_a_message_and_a_usable_context():
    from ddcmd_amd.martini import MartiniHIP, DdcmiError
    s = synthetic(100)
    m = _ctx(s, test_api=True)
    lib, ctx = m.lib, m.ctx
    fn = lib.ddcmi_structure_modes
    good = vectors(4)
    big = np.zeros((MAXK + 1, 3), np.int32)
    rho, cnt, sel = np.full((MAXK + 1, 2), 7.0), np.full(1, 7, np.int64), np.ones(9, np.int32)

    def call(nspecies=9, weight=0, nk=4, kvec=good, outs=(True, True)):
        return fn(ctx, nspecies, sel.ctypes.data_as(ip), weight, nk, kvec.ctypes.data_as(ip) if kvec is not None else None,
                  rho.ctypes.data_as(dp) if outs[0] else None, cnt.ctypes.data_as(lp) if outs[1] else None)

    def with_component(at, value):
        kv = good.copy()
        kv.reshape(-1)[at] = value
        return kv

    cases = [(lambda: call(nk=0), EINVAL, b"nk = 0"), (lambda: call(nk=-3), EINVAL, b"nk = -3"),
             (lambda: call(kvec=None), EINVAL, b"NULL argument"), (lambda: call(outs=(False, True)), EINVAL, b"NULL argument"),
             (lambda: call(outs=(True, False)), EINVAL, b"NULL argument"),
             (lambda: call(nspecies=8), EINVAL, b"nspecies = 8, the context has 9"), (lambda: call(nspecies=10), EINVAL, b"nspecies = 10"),
             (lambda: call(weight=2), EINVAL, b"weight = 2"), (lambda: call(weight=-1), EINVAL, b"weight = -1"),
             (lambda: call(nk=MAXK + 1, kvec=big), EUNSUPPORTED, b"nk = 4097, at most 4096"),
             (lambda: call(kvec=with_component(5, MAXN + 1)), EUNSUPPORTED, b"kvec[1][2] = 1025, at most 1024"),
             (lambda: call(kvec=with_component(9, -MAXN - 1)), EUNSUPPORTED, b"kvec[3][0] = -1025, at most 1024")]
    want = m.structure_modes(good)
    for k, (c, code, word) in enumerate(cases):
        rc = c()
        msg = lib.ddcmi_last_error(ctx)
        assert rc == code and word in msg and msg.startswith(b"ddcmi_structure_modes"), (k, rc, msg)
        assert np.all(rho == 7.0) and cnt[0] == 7      # nothing written
        got = m.structure_modes(good)      # the context goes on working
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] == 100
    assert call(nk=MAXK, kvec=big) == 0 and cnt[0] == 100 and np.all(rho[:MAXK] == [100.0, 0.0]) and np.all(rho[MAXK] == 7.0)      # the cap itself
    rho[:] = 7.0
    cnt[0] = 7
    assert call(kvec=with_component(5, MAXN)) == 0 and call(kvec=with_component(5, -MAXN)) == 0
    rho[:] = 7.0
    cnt[0] = 7
    assert fn(None, 9, None, 0, 4, good.ctypes.data_as(ip), rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp)) == EINVAL
    # the group form on a context that belongs to no group
    from ddcmd_amd.martini import _declare_domains
    _declare_domains(lib)
    arr = (ctypes.c_void_p * 1)(ctx)
    assert lib.ddcmi_group_structure_modes(arr, 1, 9, None, 0, 4, good.ctypes.data_as(ip), rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp)) == EINVAL
    msg = lib.ddcmi_last_error(ctx)
    assert msg.startswith(b"ddcmi_group_structure_modes") and b"not the contexts of an in-process group: use ddcmi_structure_modes" in msg
    assert np.all(rho == 7.0) and cnt[0] == 7
    got = m.structure_modes(good)
    assert got[0].tobytes() == want[0].tobytes()
    m.close()
    # no uploaded state
    e = MartiniHIP(s, upload=False)
    assert e.lib.ddcmi_structure_modes(e.ctx, 9, None, 0, 4, good.ctypes.data_as(ip), rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp)) == EINVAL
    msg = e.lib.ddcmi_last_error(e.ctx)
    assert msg.startswith(b"ddcmi_structure_modes") and b"needs an uploaded state" in msg and np.all(rho == 7.0) and cnt[0] == 7
    e.upload(s.rx, s.ry, s.rz, s.vx, s.vy, s.vz)
    got = e.structure_modes(good)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    e.close()
    # a triclinic box
    t = synthetic(100)
    t.h[1] = 0.5
    try:
        tri = MartiniHIP(t)
    except DdcmiError:
        return      # (a context that takes no triclinic box has nothing to refuse)
    with pytest.raises(DdcmiError, match="ddcmi_structure_modes: only orthorhombic"):
        tri.structure_modes(good)
    tri.close()

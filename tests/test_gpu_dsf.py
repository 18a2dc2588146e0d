"""GPU tests (-m gpu) of the ANALYSIS type DSF on the device: ddcmi_charge_density_modes and the in-process group's twin, on small
synthetic states uploaded directly (internal units; no list is built).

The yardstick is rho_a(m) = sum_j q_j exp(i m theta_j), theta_j = 2 pi r_j / L_a, evaluated in numpy longdouble from the positions a
download returns (pi, the quotient, the product m theta, cos and sin all in longdouble; its own error is below 2^-10 of the bound).

The bound per (axis, m), u = 2^-53, to first order:   B = u (m (thmax + C1) + DEPTH(n)) sum |q_j|,   thmax = max |theta_j| on that axis
over the selected beads.  Where it comes from, per bead (k_census_dsf, C = 8 modes per chunk, m = m0 + k, 0 <= k < C):
  t = r / L, one correctly rounded division: |dt| <= u |t|, a phase error of c^m of 2 pi m u |t| = m u theta.  t - rint(t) is exact
     and leaves |t| <= 1/2;
  the chunk's first power (m0 > 1) is sincospi(2 (m0 t)): the product m0 t rounds once, at most u m0 / 2 turns = pi u m0 of phase;
  sincospi is taken at 4 ulp per component (the OpenCL limit for sinpi / cospi in double; ROCm's table says 2): a component below 1
     has ulp <= u, so the pair {cos, sin} is off by at most S = 4 sqrt(2) u = 5.66 u;
  a step c^m -> c^(m + 1) is a complex product: per component two products and a sum, |ac| + |bd| <= 1, so at most 2 u with or
     without fused multiply-adds, M = 2 sqrt(2) u = 2.83 u for the pair; it also carries c's own S: S + M per step, k <= C - 1 steps;
  q c^m rounds once per component (or not at all when fused): Q = sqrt(2) u |q|.
  In units of u |q|:   m theta + pi m0 + S + k (S + M) + Q  <=  m theta + m max(pi, S + M) + S + Q  <=  m (theta + 15.57):  C1 = 16.
DEPTH(n): the additions a term passes through -- a lane's private sum, one per trip over the workgroup's range (TRIPS(n) = per_wg / 256
with per_wg = 256 ceil(ceil(n / 1024) / 256): one trip up to 262144 beads), 6 levels inside a wave (wave_sum_dpp), 3 for the four waves'
rows, and the workgroups one after the other, NWG(n) - 1 = ceil(n / per_wg) - 1 -- each with a relative error of at most u on a partial
sum of at most sum |q| (Higham, Accuracy and Stability of Numerical Algorithms, ch. 4.2).  Adding r domains on the host adds r.
Largest err / B seen on the device: 0.095 (one bead, mmax 17)."""
import ctypes

import numpy as np
import pytest

from ddcmd_amd.deck import Setup, units_convert
from ddcmd_amd.synth import water_forcefield, splitmix64

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53
C1 = 16.0
CHUNK = 8            # DSF_CHUNK
CAP = 256            # DDCMI_DSF_MAX_M
EINVAL, EUNSUPPORTED = -2, -4
PI_LD = LD(np.pi) + LD(1.2246467991473532e-16)      # pi to longdouble precision: the double and its residual
BOX = (64.0, 72.0, 96.0)
CHARGE = np.array([1.0, -1.0, 0.0, 0.5, 0.25, 0.0, 0.3, -0.7, 2.0])      # nine species: both signs, two neutral; species 4 has no members
WORST = [0.0]


def cdiv(a, b):
    return (a + b - 1) // b


def depth(n):
    per_wg = cdiv(cdiv(n, 1024), 256) * 256
    return per_wg // 256 + 6 + 3 + cdiv(n, per_wg) - 1


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


# ---- the yardstick ----------------------------------------------------------
def yardstick(s, r, mmax, select=None, index=None):
    """(rho longdouble [3, mmax, 2], count, thmax[3], sum |q|) over the selected beads at the positions r (as downloaded)"""
    sp = np.asarray(s.species)
    r = [np.asarray(a, np.float64) for a in r]
    if index is not None:
        sp, r = sp[index], [a[index] for a in r]
    keep = np.ones(len(sp), bool) if select is None else (np.asarray(select)[sp] != 0)
    q = np.asarray(s.charge, np.float64)[sp[keep]].astype(LD)
    rho, thmax = np.zeros((3, mmax, 2), LD), np.zeros(3)
    m = np.arange(1, mmax + 1).astype(LD)[:, None]
    for a in range(3):
        th = (2 * PI_LD) * r[a][keep].astype(LD) / LD(s.h[4 * a])
        if len(th):
            thmax[a] = float(np.abs(th).max())
            ph = m * th[None, :]
            rho[a, :, 0], rho[a, :, 1] = (q[None, :] * np.cos(ph)).sum(axis=1), (q[None, :] * np.sin(ph)).sum(axis=1)
    return rho, int(keep.sum()), thmax, float(np.abs(q).sum())


def bounds(n, mmax, thmax, sumabs, extra=0):
    """B[3, mmax]"""
    m = np.arange(1, mmax + 1)[None, :]
    return U * (m * (np.asarray(thmax)[:, None] + C1) + depth(max(n, 1)) + extra) * sumabs * (1 + 2.0 ** -10)


def errors(rho, want):
    """|rho - want| [3, mmax] in longdouble"""
    dr, di = rho.real.astype(LD) - want[:, :, 0], rho.imag.astype(LD) - want[:, :, 1]
    return np.sqrt(dr * dr + di * di)


def assert_modes(got, ref, n, what="", extra=0, B=None):
    rho, count = got
    want, wcount, thmax, sumabs = ref
    mmax = want.shape[1]
    assert rho.shape == (3, mmax) and rho.dtype == np.complex128 and count == wcount, (what, rho.shape, count, wcount)
    B = bounds(n, mmax, thmax, sumabs, extra) if B is None else B
    err = errors(rho, want)
    ratio = float((err / np.maximum(B, 1e-300)).max()) if sumabs > 0 else 0.0
    WORST[0] = max(WORST[0], ratio)
    print("%s n=%d mmax=%d depth=%d: largest err/B %.4f (so far %.4f)" % (what, n, mmax, depth(max(n, 1)) + extra, ratio, WORST[0]))
    assert np.all(err <= B), (what, np.argwhere(err > B)[:5], float(err.max()), float(B.min()))
    return B


# ---- exact structure --------------------------------------------------------
def test_planes_give_peaks_where_their_number_divides_m():
    P, L, q, mmax = (8, 4, 16), (64.0, 32.0, 128.0), -0.75, 24
    j = np.stack(np.meshgrid(np.arange(P[0]), np.arange(P[1]), np.arange(P[2]), indexing="ij"), -1).reshape(-1, 3)
    n = len(j)
    s = synthetic(n, box=L, charge=np.full(3, q), empty_species=None)
    s.rx, s.ry, s.rz = (L[a] * j[:, a] / P[a] for a in range(3))      # exact in binary
    m = _ctx(s)
    r = m.download()["r"]
    rho, count = got = m.charge_density_modes(mmax)
    B = assert_modes(got, yardstick(s, r, mmax), n, "planes")
    assert count == n == 512
    for a in range(3):
        for mm in range(1, mmax + 1):
            if mm % P[a] == 0:
                assert abs(abs(rho[a, mm - 1]) - n * abs(q)) <= B[a, mm - 1] and B[a, mm - 1] / (n * abs(q)) < 1e-9, (a, mm, rho[a, mm - 1])
            else:
                assert abs(rho[a, mm - 1]) <= B[a, mm - 1], (a, mm, rho[a, mm - 1])
    assert [sum(mm % P[a] == 0 for mm in range(1, mmax + 1)) for a in range(3)] == [3, 6, 1]
    m.close()


def test_one_bead_at_the_origin_gives_its_charge_in_every_mode():
    s = synthetic(1, charge=np.full(2, -0.3), empty_species=None)
    s.rx, s.ry, s.rz = np.zeros(1), np.zeros(1), np.zeros(1)
    m = _ctx(s)
    rho, count = m.charge_density_modes(CAP)
    assert count == 1 and np.all(rho.real == -0.3) and np.all(rho.imag == 0.0)
    m.close()


# ---- against the yardstick --------------------------------------------------
@pytest.mark.parametrize("n,mmax", [(1, 17), (63, 17), (64, 17), (65, 17), (255, 17), (256, 17), (257, 17), (1000, 17), (70001, CHUNK + 1), (262147, 3),
                                    (1000, 1), (1000, CHUNK - 1), (1000, CHUNK), (1000, CHUNK + 1), (1000, CAP)])
def test_random_beads_in_a_non_cubic_box(n, mmax):
    s = synthetic(n)
    if n >= 63:
        assert len(np.unique(s.species[:63])) == 8      # every wave holds charges of both signs and neutral beads
    if n > 262144:
        assert depth(n) == 2 + 9 + cdiv(n, 512) - 1      # two trips per lane
    m = _ctx(s)
    r = m.download()["r"]
    assert all(np.array_equal(a, b) for a, b in zip(r, (s.rx, s.ry, s.rz)))      # inside the box: as uploaded
    got = m.charge_density_modes(mmax)
    assert_modes(got, yardstick(s, r, mmax), n, "random")
    again = m.charge_density_modes(mmax)
    assert got[0].tobytes() == again[0].tobytes() and got[1] == again[1] == n      # bit for bit
    m.close()


def test_selection_by_species():
    n, mmax = 1000, 2 * CHUNK + 1
    s = synthetic(n)
    m = _ctx(s)
    r = m.download()["r"]
    everything = m.charge_density_modes(mmax)
    ones = m.charge_density_modes(mmax, select=np.ones(9, np.int32))
    assert everything[0].tobytes() == ones[0].tobytes() and everything[1] == ones[1] == n      # NULL equals all ones, bit for bit
    for sel in ([0, 1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 1, 0, 0, 0, 7], [0, 0, 1, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0, 0], [0] * 9):
        got = m.charge_density_modes(mmax, select=sel)
        ref = yardstick(s, r, mmax, select=sel)
        assert_modes(got, ref, n, "select %s" % sel)
        assert got[1] == int(np.isin(s.species, np.flatnonzero(sel)).sum())
        if ref[3] == 0.0:      # neutral species, the species without members, no species: exact zeros
            assert not got[0].real.any() and not got[0].imag.any()
    assert m.charge_density_modes(mmax, select=[0, 0, 1, 0, 0, 1, 0, 0, 0])[1] > 0 and m.charge_density_modes(mmax, select=[0, 0, 0, 0, 1, 0, 0, 0, 0])[1] == 0
    assert m.charge_density_modes(mmax, select=[0] * 9)[1] == 0
    with pytest.raises(ValueError, match="8 entries of select for 9 species"):
        m.charge_density_modes(mmax, select=[1] * 8)
    m.close()


@pytest.mark.parametrize("pbc", [7, 0])
def test_beads_outside_the_box(pbc):
    """a bead at 1.5 L and one at -0.75 L on every axis: the download moves them by one box side where the box is periodic and leaves
    them where it is open; the phase is that of the downloaded position either way"""
    n, mmax = 257, 2 * CHUNK + 1
    s = synthetic(n, pbc=pbc)
    for a, x in enumerate((s.rx, s.ry, s.rz)):
        x[5], x[72] = 1.5 * BOX[a], -0.75 * BOX[a]
    assert s.charge[s.species[5]] != 0 and s.charge[s.species[72]] != 0
    m = _ctx(s)
    r = m.download()["r"]
    ref = yardstick(s, r, mmax)
    if pbc == 0:
        assert r[0][5] == 1.5 * BOX[0] and r[2][72] == -0.75 * BOX[2] and np.all(ref[2] > 9.42)      # thmax = 3 pi
    else:
        assert r[0][5] == 0.5 * BOX[0] and r[2][72] == 0.25 * BOX[2] and np.all(ref[2] <= 3.1416)
    assert_modes(m.charge_density_modes(mmax), ref, n, "outside, pbc %d" % pbc)
    m.close()


# ---- no effect on the run ---------------------------------------------------
def test_the_call_reads_only():
    s = synthetic(1021)
    m = _ctx(s)
    d0 = m.download()
    a = m.charge_density_modes(40, select=[1, 1, 0, 0, 0, 0, 0, 1, 1])
    b = m.charge_density_modes(40, select=[1, 1, 0, 0, 0, 0, 0, 1, 1])
    d1 = m.download()
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert np.concatenate(d0["r"] + d0["v"] + d0["f"]).tobytes() == np.concatenate(d1["r"] + d1["v"] + d1["f"]).tobytes()
    m.close()


# ---- decomposed -------------------------------------------------------------
@pytest.mark.parametrize("grid", [(2, 1, 1), (2, 2, 2)])
def test_in_process_groups_add_up_to_the_one_domain_result(grid):
    from ddcmd_amd.martini import MartiniGroup, domain_of
    n, mmax = 1021, 2 * CHUNK + 1
    sel = [1, 1, 1, 0, 1, 1, 1, 0, 1]
    s = synthetic(n)
    owner = domain_of(s, grid)
    last = grid[0] * grid[1] * grid[2] - 1
    s.rx = np.where(owner == last, -np.abs(s.rx), s.rx)      # the last domain is left empty
    one = _ctx(s)
    want = one.charge_density_modes(mmax, select=sel)
    ref = yardstick(s, (s.rx, s.ry, s.rz), mmax, select=sel)
    B_one = assert_modes(want, ref, n, "one domain")
    g = MartiniGroup(s, grid)
    nloc = [int(g.lib.ddcmi_nlocal(r.ctx)) for r in g.ranks]
    assert nloc[last] == 0 and sum(nloc) == n
    # the single-context form refuses a context of a group and says where to go
    rho, cnt = np.zeros((3, mmax, 2)), np.zeros(1, np.int64)
    rc = g.lib.ddcmi_charge_density_modes(g.ranks[0].ctx, 9, None, mmax, rho.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    assert rc == EINVAL and b"ddcmi_group_charge_density_modes" in g.lib.ddcmi_last_error(g.ranks[0].ctx)
    pz, pc = g.charge_density_modes(mmax, select=sel, per_rank=True)
    assert pz.shape == (len(nloc), 3, mmax) and pc.shape == (len(nloc),) and pc.dtype == np.int64
    assert pc[last] == 0 and not pz[last].real.any() and not pz[last].imag.any()      # the empty domain: zeros
    assert pc.sum() == want[1] == ref[1]
    B_ranks = np.zeros((3, mmax))
    for r, rk in enumerate(g.ranks):      # every rank against the yardstick over its own beads
        if nloc[r]:
            rr = yardstick(s, (s.rx, s.ry, s.rz), mmax, select=sel, index=rk.index)
            B_ranks += assert_modes((pz[r], int(pc[r])), rr, nloc[r], "rank %d" % r)
    tot, count = g.charge_density_modes(mmax, select=sel)
    assert count == want[1]
    host = len(nloc) * U * ref[3]
    assert np.all(np.abs(tot - want[0]) <= B_one + B_ranks + host)
    assert_modes((tot, count), ref, n, "group total", B=B_ranks + host)
    g.close()
    one.close()


# ---- refusals ---------------------------------------------------------------
def test_refused_arguments_leave_a_message_and_a_usable_context():
    from ddcmd_amd.martini import MartiniHIP
    dp, ip, lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)
    s = synthetic(100)
    m = _ctx(s, test_api=True)
    lib, ctx = m.lib, m.ctx
    fn = lib.ddcmi_charge_density_modes
    rho, cnt, sel = np.full((3, 4, 2), 7.0), np.full(1, 7, np.int64), np.ones(9, np.int32)

    def call(nspecies=9, mmax=4, outs=(True, True)):
        return fn(ctx, nspecies, sel.ctypes.data_as(ip), mmax, rho.ctypes.data_as(dp) if outs[0] else None, cnt.ctypes.data_as(lp) if outs[1] else None)

    cases = [(lambda: call(mmax=0), EINVAL, b"mmax = 0"), (lambda: call(mmax=-3), EINVAL, b"mmax = -3"),
             (lambda: call(mmax=CAP + 1), EUNSUPPORTED, b"mmax = 257, at most 256"),
             (lambda: call(outs=(False, True)), EINVAL, b"NULL output"), (lambda: call(outs=(True, False)), EINVAL, b"NULL output"),
             (lambda: call(nspecies=8), EINVAL, b"nspecies = 8, the context has 9"), (lambda: call(nspecies=10), EINVAL, b"nspecies = 10")]
    want = m.charge_density_modes(4)
    for k, (c, code, word) in enumerate(cases):
        rc = c()
        msg = lib.ddcmi_last_error(ctx)
        assert rc == code and word in msg and msg.startswith(b"ddcmi_charge_density_modes"), (k, rc, msg)
        assert np.all(rho == 7.0) and cnt[0] == 7      # nothing written
        got = m.charge_density_modes(4)      # the context goes on working
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1] == 100
    assert fn(None, 9, None, 4, rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp)) == EINVAL
    # the group form on a context that belongs to no group
    from ddcmd_amd.martini import _declare_domains
    _declare_domains(lib)
    arr = (ctypes.c_void_p * 1)(ctx)
    assert lib.ddcmi_group_charge_density_modes(arr, 1, 9, None, 4, rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp)) == EINVAL
    assert b"not the contexts of an in-process group: use ddcmi_charge_density_modes" in lib.ddcmi_last_error(ctx)
    assert np.all(rho == 7.0) and cnt[0] == 7
    m.close()
    # no uploaded state
    e = MartiniHIP(s, upload=False)
    assert e.lib.ddcmi_charge_density_modes(e.ctx, 9, None, 4, rho.ctypes.data_as(dp), cnt.ctypes.data_as(lp)) == EINVAL
    assert b"needs an uploaded state" in e.lib.ddcmi_last_error(e.ctx)
    e.upload(s.rx, s.ry, s.rz, s.vx, s.vy, s.vz)
    got = e.charge_density_modes(4)
    assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    e.close()

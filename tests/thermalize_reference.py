"""Reference of the THERMALIZE transform for the tests, written here in Python + numpy: prand48_init and erand48's 48-bit LCG in Python
integers (exact), gasdev0's values in numpy.longdouble, RESCALE in longdouble -- and the error bounds the GPU tests hold the device to.

BOLTZMANN.  A bead's stream: X0 = prand48_init((loop % 10000000 + 1) * gid mod 2^64, seed, 0x1234512345ab), X <- 0x5DEECE66D X + 0xB mod 2^48,
u = X 2^-48.  gasdev0: v1 = 2 u - 1, v2 = 2 u' - 1 (exact), rsq = v1 v1 + v2 v2, rejected while rsq >= 1 or rsq == 0; returns
v2 sqrt(-2 ln rsq / rsq).  The DECISION is taken on rsq as the reference's C forms it in doubles -- each product rounded, then the sum
(Python floats do exactly that) -- the VALUE is formed in longdouble from the exact v1, v2.

Bound of a BOLTZMANN component, in ulps of the result (boltzmann_bound_ulps), u = 2^-53 the unit roundoff, 1 ulp >= u |result|:
  rsq in doubles carries two roundings, relative 2 u; ln(rsq (1 + d)) = ln rsq + d, relative 2 u / |ln rsq| -- the one term that grows, as rsq -> 1;
  log: 1 ulp = 2 u (the HIP math API's table: log, double precision, 1 ULP); times -2: exact; the quotient by rsq: its own u and rsq's 2 u;
  the square root halves all that -- (2 u / |ln rsq| + 2 u + 2 u + u) / 2 = u / |ln rsq| + 2.5 u -- and adds its own rounding, taken as 1 ulp = 2 u;
  v2 fac: u.  sigma = sqrt(T / m): u / 2 + 2 u; sigma g: u.
  Sum: (9 + 1 / |ln rsq|) u relative, hence at most 9 + 1 / |ln rsq| ulps; one more for rounding the longdouble reference to the grid: 10 + 1 / |ln rsq|.

RESCALE (rescale_bound), per class of N beads, u as above, A_a = sum m |v_a|, M = sum m, d = v - vcm, S = sum m |d|^2:
  sum m v_a: every term rounded, the sum in any order: (N + 16) u A_a; M likewise (N + 16) u M.
  vcm_a = (sum m v_a) / M: dv_a = 2 (N + 17) u A_a / M.
  S: its terms (a difference, three squares, two sums, a product: 7 u) and their sum: (N + 23) u S; the vcm it is formed with is off by dv:
     2 sum_a (sum m |d_a|) dv_a.  dS = (N + 23) u S + 2 sum_a (sum m |d_a|) dv_a.
  vScale = sqrt(T / (S / (3 (N - 1)))): ds = (dS / S + 3 u) / 2 + 2 u relative.
  v'_a = d_a vScale + vcmNew_a:  vScale (2 dv_a + |d_a| (ds + 3 u)) + |vcm_a| vScale (ds + u) + dv_a + 2 u |v'_a|.
The temperature after the call (temperature_bound): T' / T = S_true / S_device up to the roundings of v': dS / S + 4 u + 2 sum m |d'_a| e_a / S',
e_a = 4 u (|v'_a| + 2 |vcmNew_a|)."""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
A48, C48, M48 = 0x5DEECE66D, 0xB, (1 << 48) - 1
M64 = (1 << 64) - 1
CALLSITE = 0x1234512345AB
DEFAULT_SEED = 385212586


def lcg48(x):
    """one step of erand48's generator"""
    return (A48 * x + C48) & M48


def prand48_init(gid, seed, callsite=CALLSITE):
    """random.c:370-386: the three 16-bit words as one 48-bit state, word 0 lowest"""
    seed = (seed ^ callsite) & M64
    gid = (gid ^ seed) & M64
    sv = [0, 0, 0]
    for mask in (0x000F, 0x00F0, 0x0F00, 0xF000):
        sv[0] = (sv[0] + (gid & mask)) & 0xFFFF
        gid >>= 4
        sv[1] = (sv[1] + (gid & mask)) & 0xFFFF
        gid >>= 4
        sv[2] = (sv[2] + (gid & mask)) & 0xFFFF
    return sv[0] | sv[1] << 16 | sv[2] << 32


def modlabel(loop, gid):
    """thermalize.c:118-119: C's remainder (the sign of the dividend), the product modulo 2^64"""
    r = int(math.fmod(loop, 10000000))
    return (((r + 1) & M64) * int(gid)) & M64


def uniform(x):
    """erand48's double of the state x: exact"""
    return x / 281474976710656.0


def gasdev0(x):
    """(deviate longdouble, new state, rejected draws, rsq longdouble, the uniforms of the accepted draw)"""
    nrej = 0
    while True:
        x = lcg48(x); u1 = uniform(x)
        x = lcg48(x); u2 = uniform(x)
        v1, v2 = 2.0 * u1 - 1.0, 2.0 * u2 - 1.0
        rsq = v1 * v1 + v2 * v2          # doubles, every operation rounded once: the reference's C
        if not (rsq >= 1.0 or rsq == 0.0):
            break
        nrej += 1
    l1, l2 = LD(v1), LD(v2)
    rl = l1 * l1 + l2 * l2
    return l2 * np.sqrt(LD(-2.0) * np.log(rl) / rl), x, nrej, rl, (u1, u2)


def boltzmann(gid, mass, T, seed=DEFAULT_SEED, loop=0):
    """per bead (mass and T of its class; T < 0: not written): v[n, 3] longdouble (NaN where not written), rejected draws[n] (-1 where not
    written), rsq[n, 3] longdouble of the accepted draws"""
    n = len(gid)
    v = np.full((n, 3), np.nan, LD)
    rsq = np.full((n, 3), np.nan, LD)
    nrej = np.full(n, -1, np.int64)
    for i in range(n):
        if T[i] < 0.0:
            continue
        x = prand48_init(modlabel(loop, int(gid[i])), int(seed))
        sigma = np.sqrt(LD(T[i]) / LD(mass[i]))
        tot = 0
        for k in range(3):
            g, x, r, rl, _ = gasdev0(x)
            v[i, k], rsq[i, k] = sigma * g, rl
            tot += r
        nrej[i] = tot
    return v, nrej, rsq


def boltzmann_bound_ulps(rsq):
    return 10.0 + 1.0 / np.abs(np.log(rsq)).astype(np.float64)


def rescale(v, mass, cls, T, keep_vcm):
    """thermalize_rescale in longdouble.  v[n, 3] float64, mass[n], cls[n] the class of every bead, T[nclass].  Returns (v' longdouble, info):
    info[c] = dict(N, vcm, S, scale, vcm_new, applied) -- applied False where N <= 1 or S == 0 (the class keeps its bits)"""
    v = np.asarray(v, LD)
    m = np.asarray(mass, LD)
    out = v.copy()
    info = []
    for c in range(len(T)):
        k = np.flatnonzero(cls == c)
        N = len(k)
        d = dict(N=N, applied=False, idx=k)
        if N > 0:
            M = m[k].sum()
            vcm = (m[k, None] * v[k]).sum(axis=0) / M
            dv = v[k] - vcm
            S = (m[k] * (dv * dv).sum(axis=1)).sum()
            d.update(M=M, vcm=vcm, S=S)
            if N > 1 and S != 0:
                scale = np.sqrt(LD(T[c]) / (S / (LD(3) * (N - 1)))) if T[c] > 0.0 else LD(1)
                vnew = vcm if keep_vcm else vcm * scale
                out[k] = dv * scale + vnew
                d.update(scale=scale, vcm_new=vnew, applied=True)
        info.append(d)
    return out, info


def rescale_bound(v, mass, info):
    """(bound[n, 3] on |v' - reference|, relative bound on the class temperature per class) -- module docstring"""
    v = np.asarray(v, LD)
    m = np.asarray(mass, LD)
    bound = np.zeros(v.shape, LD)
    tb = []
    for d in info:
        if not d["applied"]:
            tb.append(0.0)
            continue
        k, N = d["idx"], d["N"]
        A = (m[k, None] * np.abs(v[k])).sum(axis=0)
        dvcm = 2 * (N + 17) * U * A / d["M"]
        dd = np.abs(v[k] - d["vcm"])
        dS = (N + 23) * U * d["S"] + 2 * ((m[k, None] * dd).sum(axis=0) * dvcm).sum()
        ds = (dS / d["S"] + 3 * U) / 2 + 2 * U
        sc = d["scale"]
        vp = dd * sc + np.abs(d["vcm_new"])
        bound[k] = sc * (2 * dvcm + dd * (ds + 3 * U)) + np.abs(d["vcm"]) * sc * (ds + U) + dvcm + 2 * U * vp
        e = 4 * U * (vp + 2 * np.abs(d["vcm_new"]))
        Sp = sc * sc * d["S"]
        tb.append(float(dS / d["S"] + 4 * U + 2 * (m[k, None] * dd * sc * e).sum() / Sp))
    return bound, tb


def class_temperature(v, mass, cls, c):
    """(T, vcm) of class c in longdouble: sum m |v - vcm|^2 / (3 (N - 1))"""
    k = np.flatnonzero(cls == c)
    v = np.asarray(v, LD)[k]
    m = np.asarray(mass, LD)[k]
    vcm = (m[:, None] * v).sum(axis=0) / m.sum()
    dv = v - vcm
    return (m * (dv * dv).sum(axis=1)).sum() / (LD(3) * (len(k) - 1)), vcm


def maxwell_cdf(x):
    """P(K < x T) of K = m v^2 / 2 at temperature T (chi-square with 3 degrees of freedom in 2 K / T)"""
    x = np.asarray(x, float)
    return np.array([math.erf(math.sqrt(t)) - 2.0 * math.sqrt(t / math.pi) * math.exp(-t) for t in x])


CHI2_CRIT_20_1E4 = 52.386      # the 1 - 1e-4 quantile of chi-square with 20 degrees of freedom (tables: 52.39)


def chi2_maxwell(K_over_T_counts, n, edges):
    """chi-square of a histogram of K / T over the bins edges[0] < ... < edges[-1] plus the overflow beyond (K >= 0, edges[0] = 0)"""
    cdf = maxwell_cdf(edges)
    p = np.concatenate([np.diff(cdf), [1.0 - cdf[-1]]])
    obs = np.asarray(K_over_T_counts, float)
    assert len(obs) == len(p) and abs(obs.sum() - n) < 0.5
    return float(((obs - n * p) ** 2 / (n * p)).sum())

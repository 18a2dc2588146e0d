"""analysis.StaticStructureFactor (ssf.c on the host side): the wave-vector list against a brute-force statement of ssf_kvector's three
rules, the four sign combinations, fact by the number of zero components, S_k from hand-made rho, and the reference's line format."""
import math

import numpy as np
import pytest

from ddcmd_amd.analysis import StaticStructureFactor, expand_signs, in_plane

BOXES = [(64.0, 72.0, 96.0), (50.0, 50.0, 120.0)]
# none of kmax L / 2 pi is within 1e-3 of an integer on any axis of either box (asserted below); 0.09: (int)(0.09 * 64 / 2 pi) = 0
KMAXES = [0.09, 0.12, 0.35, 0.5, 0.8]


def brute(box, kmax):
    """rule 1: n_a in [0, (int)(kmax L_a / 2 pi)); rule 2: along n_z, everything from the first k^2 >= kmax^2 on is dropped; rule 3: kept
    if k^2 < kmax^2 / 2 and not (0,0,0).  Order: n_x slowest."""
    top = [int(kmax * L / (2 * math.pi)) for L in box]
    k2 = lambda n: sum((2 * math.pi * n[a] / box[a]) ** 2 for a in range(3))
    out = []
    for nx in range(top[0]):
        for ny in range(top[1]):
            ended = False
            for nz in range(top[2]):
                ended = ended or k2((nx, ny, nz)) >= kmax * kmax
                if not ended and (nx, ny, nz) != (0, 0, 0) and k2((nx, ny, nz)) < 0.5 * kmax * kmax:
                    out.append((nx, ny, nz))
    return top, out


@pytest.mark.parametrize("box", BOXES)
@pytest.mark.parametrize("kmax", KMAXES)
def test_the_list_is_ssf_kvectors(box, kmax):
    for L in box:
        x = kmax * L / (2 * math.pi)
        assert abs(x - round(x)) > 1e-3      # the (int) is not decided by a rounding
    top, want = brute(box, kmax)
    ssf = StaticStructureFactor(np.diag(box).ravel(), kmax)
    assert ssf.n.dtype == np.int32 and ssf.n.shape == (len(want), 3)
    assert [tuple(v) for v in ssf.n.tolist()] == want
    assert ssf.kvec.shape == (4 * len(want), 3) and len(ssf.fact) == len(want)
    if min(top) == 0:
        assert want == []
    if kmax >= 0.35:
        assert len(want) > 10
    assert all(v[a] < top[a] for v in want for a in range(3))


def test_an_axis_with_no_room_gives_an_empty_list():
    assert int(0.09 * 64.0 / (2 * math.pi)) == 0 and int(0.09 * 72.0 / (2 * math.pi)) == 1
    ssf = StaticStructureFactor(np.diag(BOXES[0]).ravel(), 0.09)
    assert ssf.n.shape == (0, 3) and ssf.kvec.shape == (0, 3) and ssf.lines(np.zeros(0, np.complex128)) == ""
    assert ssf.Sk([]).shape == (0,)


def test_the_list_is_not_trivial_and_the_break_matters():
    """in the (50, 50, 120) box at kmax 0.8 vectors with k^2 >= kmax^2 exist inside the loop bounds, and the half-kmax^2 rule drops more"""
    box, kmax = BOXES[1], 0.8
    top, want = brute(box, kmax)
    assert top == [6, 6, 15]
    k2 = lambda n: sum((2 * math.pi * n[a] / box[a]) ** 2 for a in range(3))
    assert any(k2((nx, ny, nz)) >= kmax * kmax for nx in range(top[0]) for ny in range(top[1]) for nz in range(top[2]))
    assert 0 < len(want) < top[0] * top[1] * top[2] - 1
    assert (0, 0, 1) == want[0] and (0, 0, 0) not in want


def test_sign_expansion():
    n = [(1, 2, 3), (0, 5, 0), (4, 0, 7)]
    kv = expand_signs(n)
    assert kv.dtype == np.int32 and kv.tolist() == [[1, 2, 3], [1, 2, -3], [1, -2, 3], [1, -2, -3],
                                                    [0, 5, 0], [0, 5, 0], [0, -5, 0], [0, -5, 0],
                                                    [4, 0, 7], [4, 0, -7], [4, 0, 7], [4, 0, -7]]
    ssf = StaticStructureFactor(np.diag(BOXES[0]).ravel(), 0.35)
    assert np.array_equal(ssf.kvec, expand_signs(ssf.n)) and np.array_equal(ssf.kvec[0::4], ssf.n)
    assert np.array_equal(ssf.kvec[3::4], ssf.n * np.array([1, -1, -1]))


def test_fact_by_the_number_of_zero_components():
    ssf = StaticStructureFactor(np.diag(BOXES[0]).ravel(), 0.5)
    zeros = (ssf.n == 0).sum(axis=1)
    assert set(zeros.tolist()) == {0, 1, 2}
    assert np.array_equal(ssf.fact, np.where(zeros == 0, 1.0, np.where(zeros == 1, 0.5, 0.25)))
    assert ssf.fact[ssf.n.tolist().index([0, 0, 1])] == 0.25 and ssf.fact[ssf.n.tolist().index([1, 0, 1])] == 0.5 and ssf.fact[ssf.n.tolist().index([1, 1, 1])] == 1.0


def test_sk_from_hand_made_rho():
    ssf = StaticStructureFactor(np.diag(BOXES[0]).ravel(), 0.35)
    nv = len(ssf.n)
    assert nv >= 3
    rho = np.zeros((nv, 4), np.complex128)
    rho[0] = [3 + 4j, 1j, -2, 0.5 - 0.5j]      # 25 + 1 + 4 + 0.5
    rho[1] = [1, 1, 1, 1]
    rho[2] = [2j, 0, 0, 0]
    sk = ssf.Sk(rho.ravel())
    assert sk.shape == (nv,) and np.array_equal(sk[:3], ssf.fact[:3] * np.array([30.5, 4.0, 4.0])) and not sk[3:].any()
    with pytest.raises(ValueError, match="four sign combinations"):
        ssf.Sk(rho.ravel()[:-1])


def test_line_format():
    box = BOXES[0]
    ssf = StaticStructureFactor(np.diag(box).ravel(), 0.35)
    rho = (np.arange(4 * len(ssf.n)) + 1.0) * (1 - 2j)
    text = ssf.lines(rho)
    rows = text.splitlines()
    assert text.endswith("\n") and len(rows) == len(ssf.n)
    sk = ssf.Sk(rho)
    for v, s, row in zip(ssf.n.tolist(), sk, rows):
        k = [2 * math.pi * v[a] / box[a] for a in range(3)]
        assert row == "%f %f %f %f %e" % (k[0] ** 2 + k[1] ** 2 + k[2] ** 2, k[0], k[1], k[2], s)
    first = rows[0].split()
    assert len(first) == 5 and ssf.n[0].tolist() == [0, 0, 1] and first[1] == first[2] == "0.000000" and first[3] == "%f" % (2 * math.pi / 96.0)
    assert "e+" in first[4] or "e-" in first[4]


def test_species_selection_and_in_plane():
    ssf = StaticStructureFactor(np.diag(BOXES[0]).ravel(), 0.35, species="PO4")
    assert ssf.select(["W", "PO4", "NC3"]).tolist() == [0, 1, 0] and StaticStructureFactor(np.diag(BOXES[0]).ravel(), 0.35).select(["W"]) is None
    with pytest.raises(ValueError, match="not a species"):
        ssf.select(["W"])
    with pytest.raises(ValueError, match="orthorhombic"):
        StaticStructureFactor([64, 1, 0, 0, 72, 0, 0, 0, 96], 0.35)
    p = in_plane(2)
    assert p.dtype == np.int32 and p.tolist() == [[0, 1, 0], [0, 2, 0], [1, 0, 0], [1, 1, 0], [1, 2, 0], [2, 0, 0], [2, 1, 0], [2, 2, 0]]
    assert len(in_plane(16)) == 288 and np.array_equal(StaticStructureFactor.in_plane(3), in_plane(3))
    with pytest.raises(ValueError):
        in_plane(0)

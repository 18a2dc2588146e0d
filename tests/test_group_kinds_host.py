"""CPU tests of the GROUP kinds FROZEN, FIXEDVELOCITY and QUENCH: the deck loader reads the three types (FIXEDVELOCITY with and without
`v`) and EXTFORCE (`Fzeq` as a constant with an optional unit of force; the device has no such kind yet, MartiniHIP and the driver
refuse it by the group's name), refuses what it cannot represent, the Setup carries them, every other type stays "other", and the
longdouble reference of tests/group_kind_reference.py is held against closed forms."""
import os
import shutil

import numpy as np
import pytest

import group_kind_systems as G
import restraint_systems as R
from group_kind_reference import KindReference, LD
from ddcmd_amd import deck
from ddcmd_amd.deck import load_deck, units_convert

HERE = os.path.dirname(os.path.abspath(__file__))
WATER = os.path.join(HERE, "golden", "water_deck")
GROUPS = "system SYSTEM { groups = group free wall pull coast bath push; }\n"


def _deck(tmp_path):
    d = tmp_path / "deck"
    shutil.copytree(WATER, str(d))
    return str(d / "object.data")


def test_kind_numbers():
    """the numbers of include/ddcmi.h; 3 stays the loader's "any other type" """
    assert (deck.GROUP_FREE, deck.GROUP_BERENDSEN, deck.GROUP_LANGEVIN, deck.GROUP_OTHER) == (0, 1, 2, 3)
    assert (deck.GROUP_FROZEN, deck.GROUP_FIXEDVELOCITY, deck.GROUP_QUENCH, deck.GROUP_EXTFORCE) == (4, 5, 6, 7)
    text = open(os.path.join(HERE, "..", "include", "ddcmi.h")).read()
    assert "DDCMI_FROZEN = 4, DDCMI_FIXEDVELOCITY = 5, DDCMI_QUENCH = 6 }" in text


def test_loader_reads_the_types(tmp_path):
    extra = (GROUPS + "wall GROUP { type = FROZEN; }\n"
             "pull GROUP { type = FIXEDVELOCITY; v = 0.001 -0.002 0.0005 Angstrom/fs; }\n"
             "coast GROUP { type = FIXEDVELOCITY; }\n"
             "bath GROUP { type = QUENCH; }\n"
             "push GROUP { type = EXTFORCE; Fzeq = -2.5 kJ/mol/nm; }\n")
    s = load_deck(_deck(tmp_path), extra_objects=extra)
    assert s.group_name == ["group", "free", "wall", "pull", "coast", "bath", "push"]
    assert s.group_type.tolist() == [2, 2, 4, 5, 5, 6, 7]
    assert s.group_vset.tolist() == [0, 0, 0, 1, 0, 0, 0]
    v = s.group_v.reshape(7, 3)
    want = np.array([units_convert(x, "Angstrom/fs", None) for x in (0.001, -0.002, 0.0005)])
    assert np.array_equal(v[3], want) and not v[[0, 1, 2, 4, 5, 6]].any()
    assert s.group_Fz[6] == units_convert(-2.5, "kJ/mol/nm", None) and s.group_Fz[6] < 0 and not s.group_Fz[:6].any()
    # the Setup keeps them through its dict form (fixtures), and a dict written before these fields existed still loads
    d = deck.setup_to_dict(s)
    t = deck.setup_from_dict(d)
    assert np.array_equal(t.group_vset, s.group_vset) and np.array_equal(t.group_v, s.group_v) and np.array_equal(t.group_Fz, s.group_Fz)
    for k in ("setup_group_vset", "setup_group_v", "setup_group_Fz"):
        del d[k]
    assert deck.setup_from_dict(d).group_vset is None


def test_loader_fzeq_without_unit(tmp_path):
    """a bare number is in the deck's default units of m l / t^2, as object_get's WITH_UNITS reads it"""
    s = load_deck(_deck(tmp_path), extra_objects=GROUPS + "wall GROUP { type = FROZEN; } pull GROUP { type = QUENCH; } coast GROUP { type = QUENCH; } "
                  "bath GROUP { type = QUENCH; } push GROUP { type = EXTFORCE; Fzeq = 0.125; }\n")
    assert s.group_Fz[6] == units_convert(0.125, "m*l/t^2", None) and s.group_Fz[6] > 0


@pytest.mark.parametrize("body, word", [
    ("type = EXTFORCE; Fzeq = 3*t;", "Fzeq"),
    ("type = EXTFORCE; Fzeq = 3 * t;", "Fzeq"),
    ("type = EXTFORCE; Fzeq = 2.0 fs;", "Fzeq"),
    ("type = EXTFORCE; Fzeq = sin(t);", "Fzeq"),
    ("type = EXTFORCE; Fzeq = nan;", "Fzeq"),
    ("type = EXTFORCE;", "Fzeq"),
    ("type = FIXEDVELOCITY; v = 0.001 nan 0.0 Angstrom/fs;", "v needs"),
    ("type = FIXEDVELOCITY; v = 0.001 inf 0.0;", "v needs"),
    ("type = FIXEDVELOCITY; v = 0.001 0.002;", "v needs"),
])
def test_loader_refusals(tmp_path, body, word):
    extra = (GROUPS + "wall GROUP { type = FROZEN; } pull GROUP { type = QUENCH; } coast GROUP { type = QUENCH; } bath GROUP { type = QUENCH; }\n"
             "push GROUP { %s }\n" % body)
    with pytest.raises(Exception) as ei:
        load_deck(_deck(tmp_path), extra_objects=extra)
    assert "push" in str(ei.value) and word in str(ei.value), str(ei.value)


def test_unknown_type_stays_other(tmp_path):
    s = load_deck(_deck(tmp_path), extra_objects=GROUPS + "wall GROUP { type = PISTON; } pull GROUP { type = QUENCH; } coast GROUP { type = QUENCH; } "
                  "bath GROUP { type = QUENCH; } push GROUP { type = QUENCH; }\n")
    assert s.group_type[2] == deck.GROUP_OTHER


# ---- the reference against closed forms ------------------------------------------------------------------------------------
def test_reference_frozen_bead():
    """a frozen bead: position and velocity after 25 steps are the start's, bit for bit, whatever force acts on it"""
    s = G.system("gas", 65, "frozen-fast")
    ref = KindReference(s)
    r0, v0 = ref.r.copy(), ref.v.copy()
    ref.step(25)
    fr = ref.frozen
    assert fr.sum() >= 20 and np.abs(ref.f[:, fr]).min() > 0
    assert np.array_equal(ref.r[:, fr], r0[:, fr]) and np.array_equal(ref.v[:, fr], v0[:, fr])
    assert not np.array_equal(ref.r[:, ~fr], r0[:, ~fr])
    # the stored velocities are in the kinetic energy
    K = 0.5 * (ref.m * (ref.v ** 2).sum(axis=0))
    assert abs(ref.rk - float(K.sum())) <= 1e-15 * float(K.sum()) and K[fr].sum() > 100 * K[~fr].sum()


def test_reference_dragged_bead():
    """FIXEDVELOCITY with a vector: r = r0 + k dt v after k steps and v the vector, whatever it started with and whatever pulls; without
    one: r = r0 + k dt v(0), the force has no say either"""
    s = G.system("gas", 64, "all")
    ref = KindReference(s)
    r0, v0 = ref.r.copy(), ref.v.copy()
    k = 12
    ref.step(k)
    pulled, coast = ref.group == 4, ref.group == 7
    vec = np.asarray(s.group_v, LD).reshape(-1, 3)[4]
    assert pulled.sum() == 8 and coast.sum() == 8
    assert np.array_equal(ref.v[:, pulled], np.repeat(vec[:, None], 8, 1))
    tol = 4 * k * np.finfo(LD).eps * np.abs(r0).max()
    assert np.abs(ref.r[:, pulled] - (r0[:, pulled] + k * ref.dt * vec[:, None])).max() <= tol
    assert np.array_equal(ref.v[:, coast], v0[:, coast])
    assert np.abs(ref.r[:, coast] - (r0[:, coast] + k * ref.dt * v0[:, coast])).max() <= tol


def test_reference_quenched_oscillator_never_gains_energy():
    """a quenched oscillator: E = K + kb |d|^2 never rises above its start (the zeroing removes kinetic energy, the kicks and the drift
    are the leapfrog of a harmonic well, whose energy oscillates by O((w dt)^2) only), and falls far below it within 4 of the slowest periods"""
    for s in (G.system("gas", 63, "last:%d" % G.QUENCH), G.system("gas", 63, "frozen-fast")):
        ref = KindReference(s)
        q = ref.quench
        assert q.any()

        def energy():
            res = R.reference(s, ref.r.T, ref.box, s.pbc)
            e = np.zeros(ref.n, LD)
            np.add.at(e, res["bead"], res["e"])
            return (e + 0.5 * ref.m * (ref.v ** 2).sum(axis=0))[q]
        e0 = energy()
        wdt2 = (2 * np.pi / 40.0) ** 2
        for _ in range(960):
            ref.step(1)
            e = energy()
            assert (e <= e0 * (1 + wdt2)).all()
        assert (energy() < 0.05 * e0).all()


def test_quench_cases_cover_every_decision():
    """the hand-placed beads: on the first FRONT kick the reference zeroes exactly the v f < 0 components, and the products of the
    underflow bead are exact zeros in float64 although neither factor is"""
    s = G.system("quench_cases")
    ref = KindReference(s)
    v0, f0 = ref.v.astype(np.float64), ref.f.astype(np.float64)
    ref.front()
    dec = ref.decisions[0]
    qidx = np.flatnonzero(ref.quench)
    seen = set()
    for b, comp, case in s.case:
        col = int(np.flatnonzero(qidx == b)[0])
        p = v0[comp, b] * f0[comp, b]
        seen.add(case)
        assert dec[comp, col] == (case == "vf<0"), (b, comp, case)
        if case == "vf<0":
            assert p < 0
        elif case == "vf>0":
            assert p > 0
        elif case == "f=0":
            assert f0[comp, b] == 0.0 and v0[comp, b] != 0.0
        elif case in ("v=+0", "v=-0"):
            assert v0[comp, b] == 0.0 and np.signbit(v0[comp, b]) == (case == "v=-0") and f0[comp, b] != 0.0
        else:
            assert p == 0.0 and v0[comp, b] != 0.0 and f0[comp, b] != 0.0
    assert seen == set(G.CASES)

"""The table of INTEGRATOR types (deck.c) as the loader and ddcmd_amd.martini.integrator_plan read it -- no device needed.  The three names
of the NGLFCONSTRAINTGPU family (integrator.c:103-129: NGLFCONSTRAINTGPU, NGLFCONSTRAINTGPULANGEVIN, NGLFCONSTRAINTGPULANGEVINLCG64) load
with nglfconstraint_parms' keys (nglfconstraint.c:86-95), the override of the GROUP objects' thermostats is reported, and a type that is
not in the table is refused with every name of it."""
import os

import numpy as np
import pytest

from ddcmd_amd import deck as D
from ddcmd_amd.deck import load_deck, units_convert
from ddcmd_amd.martini import DdcmiError, integrator_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WATER = os.path.join(ROOT, "tests", "golden", "water_deck", "object.data")      # two LANGEVIN groups, 310 K, tau 1 ps
REF_WATERBOX = os.path.join(ROOT, "tests", "golden", "ref_waterbox", "object.data")
NEW = ("NGLFCONSTRAINTGPU", "NGLFCONSTRAINTGPULANGEVIN", "NGLFCONSTRAINTGPULANGEVINLCG64")
ALL = ("NGLF", "NVTGLF", "NGLFGPU", "NGLFHIP", "NGLFGPULANGEVIN", "NGLFCONSTRAINT") + NEW
KEYS = "T = 300 K; P0 = 2 bar; beta = 4.5e-4 1/bar; tauBarostat = 2 ps;"


def integrator(name, keys=""):
    return "nglf INTEGRATOR { type = %s; %s }" % (name, keys)


def test_the_table_has_the_nine_types_in_order():
    rows = D.integrator_types()
    assert tuple(r["name"] for r in rows) == ALL
    by = {r["name"]: r for r in rows}
    assert [n for n in ALL if by[n]["barostat_keys"]] == ["NGLFGPULANGEVIN", "NGLFCONSTRAINT"] + list(NEW)
    assert [n for n in ALL if by[n]["host_eligible"]] == ["NGLF", "NVTGLF"]
    assert by["NGLFCONSTRAINTGPU"]["group_override"] == D.GROUPS_FREE
    assert by["NGLFCONSTRAINTGPULANGEVIN"]["group_override"] == by["NGLFCONSTRAINTGPULANGEVINLCG64"]["group_override"] == D.GROUPS_LANGEVIN0
    assert by["NGLFGPULANGEVIN"]["group_override"] == D.GROUPS_LANGEVIN0_OWN_VCM and by["NGLFGPULANGEVIN"]["barostat_form"] == D.BARO_ISOTROPIC
    assert by["NGLFCONSTRAINT"]["group_override"] == D.GROUPS_ASIS and by["NGLFCONSTRAINT"]["barostat_form"] == D.BARO_SEMI
    assert all(by[n]["barostat_form"] == D.BARO_BY_KEY for n in NEW)


@pytest.mark.parametrize("name", NEW)
def test_the_loader_reads_the_barostat_keys_and_isotropic(name):
    s = load_deck(WATER, extra_objects=integrator(name, KEYS))
    assert s.integrator_type == name
    assert s.npt_T == units_convert(300.0, "K") and s.npt_P0 == units_convert(2.0, "bar")
    assert s.npt_beta == units_convert(4.5e-4, "1/bar") and s.npt_tau == units_convert(2.0, "ps")
    assert s.npt_isotropic == 0                                       # the key's default
    assert load_deck(WATER, extra_objects=integrator(name, KEYS + " isotropic = 1;")).npt_isotropic == 1
    assert load_deck(WATER, extra_objects=integrator(name, KEYS + " isotropic = 0;")).npt_isotropic == 0
    # nglfconstraint_parms' defaults: T = 310 (kelvin), the rest zero -- no barostat.  (-x text adds to an object of the same name, so the
    # deck to ask is one whose INTEGRATOR object has no such keys: the lipid deck's `nglf INTEGRATOR {type = NGLF; }`)
    d = load_deck(os.path.join(ROOT, "tests", "golden", "lipid_deck", "object.data"), extra_objects=integrator(name))
    assert d.integrator_type == name
    assert d.npt_T == units_convert(310.0, "K") and d.npt_P0 == 0.0 and d.npt_beta == 0.0 and d.npt_tau == 0.0 and d.npt_isotropic == 0


def test_the_references_deck_line_loads():
    """tests/golden/ref_waterbox/object.data:69, the alternative the shipped deck carries as a comment"""
    line = "nglf INTEGRATOR { type=NGLFCONSTRAINTGPULANGEVIN; T=310K; P0 = 1.0 bar; beta = 3.0e-4 /bar; tauBarostat = 1.0 ps; isotropic=1; }"
    assert line in open(REF_WATERBOX).read()
    s = load_deck(REF_WATERBOX, extra_objects=line)
    assert s.integrator_type == "NGLFCONSTRAINTGPULANGEVIN" and s.npt_isotropic == 1 and s.group_override == D.GROUPS_LANGEVIN0
    assert abs(s.npt_beta - units_convert(3.0e-4, "1/bar")) <= 1e-15 * s.npt_beta and s.npt_tau == units_convert(1.0, "ps")
    assert integrator_plan(s)["overridden"] == []                    # its two LANGEVIN groups carry the same Teq and tau


def test_the_loader_reports_the_override():
    assert load_deck(WATER).group_override == D.GROUPS_ASIS           # NGLFCONSTRAINT
    assert load_deck(WATER, extra_objects=integrator("NGLF")).group_override == D.GROUPS_ASIS
    assert load_deck(WATER, extra_objects=integrator("NGLFCONSTRAINTGPU", KEYS)).group_override == D.GROUPS_FREE
    assert load_deck(WATER, extra_objects=integrator("NGLFCONSTRAINTGPULANGEVIN", KEYS)).group_override == D.GROUPS_LANGEVIN0
    assert load_deck(WATER, extra_objects=integrator("NGLFCONSTRAINTGPULANGEVINLCG64", KEYS)).group_override == D.GROUPS_LANGEVIN0
    assert load_deck(WATER, extra_objects=integrator("NGLFGPULANGEVIN", KEYS)).group_override == D.GROUPS_LANGEVIN0_OWN_VCM


def test_the_plan_overrides_the_groups():
    """the deck's groups stay in the Setup as written; the plan carries what runs"""
    groups = ("group GROUP { type = LANGEVIN; Teq = 290 K; tau = 0.5 ps; vcm = 1e-4 0 0; } "
              "free GROUP { type = BERENDSEN; Teq = 320 K; tau = 200 fs; interval = 3; } ")
    s = load_deck(WATER, extra_objects=groups + integrator("NGLFCONSTRAINTGPU", KEYS))
    assert list(s.group_type) == [D.GROUP_LANGEVIN, D.GROUP_BERENDSEN] and s.group_interval[1] == 3
    p = integrator_plan(s)
    assert list(p["group_type"]) == [D.GROUP_FREE, D.GROUP_FREE] and p["overridden"] == [0, 1] and list(p["group_interval"]) == [1, 1]
    for name in NEW[1:]:
        s = load_deck(WATER, extra_objects=groups + integrator(name, KEYS))
        p = integrator_plan(s)
        assert list(p["group_type"]) == [D.GROUP_LANGEVIN, D.GROUP_LANGEVIN] and p["overridden"] == [1]
        assert p["group_Teq"][1] == s.group_Teq[0] == units_convert(290.0, "K") and p["group_tau"][1] == s.group_tau[0] == units_convert(0.5, "ps")
        assert np.array_equal(p["group_vcm"], np.tile(np.asarray(s.group_vcm)[:3], 2)) and p["group_vcm"][0] != 0.0
        assert s.group_Teq[1] == units_convert(320.0, "K")           # untouched
    # a type without an override: the groups as written, interval included
    p = integrator_plan(load_deck(WATER, extra_objects=groups + integrator("NGLFCONSTRAINT", KEYS)))
    assert list(p["group_type"]) == [D.GROUP_LANGEVIN, D.GROUP_BERENDSEN] and p["overridden"] == [] and list(p["group_interval"]) == [1, 3]
    assert p["group_Teq"][1] == units_convert(320.0, "K")


def test_nglfconstraint_ignores_isotropic_and_nglfgpulangevin_stays_isotropic():
    assert load_deck(WATER, extra_objects=integrator("NGLFCONSTRAINT", KEYS + " isotropic = 1;")).npt_isotropic == 0
    assert load_deck(WATER, extra_objects=integrator("NGLFGPULANGEVIN", KEYS + " isotropic = 0;")).npt_isotropic == 1
    assert load_deck(WATER, extra_objects=integrator("NGLFGPULANGEVIN", KEYS)).npt_isotropic == 1


def test_an_unknown_type_is_refused_with_all_nine_names():
    s = load_deck(WATER, extra_objects=integrator("NGLFRATTLE"))     # the loader takes it; what would run it refuses it
    assert s.integrator_type == "NGLFRATTLE" and s.npt_beta == 0.0
    with pytest.raises(DdcmiError) as e:
        integrator_plan(s)
    msg = str(e.value)
    assert msg.startswith("INTEGRATOR type NGLFRATTLE is not on this path (") and msg.endswith(" are)")
    assert msg[msg.index("(") + 1:-len(" are)")].split(", ") == list(ALL)


@pytest.mark.parametrize("name", NEW[1:])
def test_group_zero_must_be_langevin(name):
    groups = "group GROUP { type = FREE; } free GROUP { type = LANGEVIN; Teq = 310 K; tau = 1 ps; } "
    s = load_deck(WATER, extra_objects=groups + integrator(name, KEYS))
    with pytest.raises(DdcmiError, match="^%s needs the first GROUP to be of type LANGEVIN$" % name):
        integrator_plan(s)
    # NGLFCONSTRAINTGPU consults no group
    assert integrator_plan(load_deck(WATER, extra_objects=groups + integrator("NGLFCONSTRAINTGPU", KEYS)))["overridden"] == [1]


def test_the_plan_sets_up_constraints_like_the_driver():
    """the types that read the barostat keys set up the residues' constraint lists where the deck has some (nglfconstraintHIP_parms)"""
    from test_oracle import CONSTRAINT_X
    lipid = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    load = lambda x: load_deck(os.path.join(lipid, "object_nvt.data"), restart_file=os.path.join(lipid, "relaxed", "restart"), extra_objects=x)
    lang = "group GROUP { type = LANGEVIN; Teq = 310 K; tau = 1 ps; } "      # (the deck's one group is BERENDSEN)
    for name in ("NGLFCONSTRAINT",) + NEW:
        s = load(CONSTRAINT_X + lang + integrator(name, KEYS))
        assert s.nresicons == 5 and integrator_plan(s)["constraints"] is True
        assert integrator_plan(load(lang + integrator(name, KEYS)))["constraints"] is False
    assert integrator_plan(load(CONSTRAINT_X))["constraints"] is False          # the deck's NGLF

"""CPU tests: the deck loader reads ANALYSIS objects of the type cholAnalysis (cholAnalysis.c:41-71) -- keys, defaults, units, the
full-name match in any case, the list of CHOL molecules -- and refuses at load what the reference leaves to an assert or a division
by zero."""
import numpy as np
import pytest

from chol_deck import chol_deck
from ddcmd_amd.deck import load_deck, units_convert
from ddcmd_amd.martini import chol_molecules

ANG = units_convert(1.0, "Angstrom", None)
HEAD = "simulate SIMULATE { analysis = chol; }\n"


@pytest.fixture(scope="module")
def deck(tmp_path_factory):
    return chol_deck(tmp_path_factory.mktemp("chol"))


def _load(d, extra):
    return load_deck(str(d / "object.data"), extra_objects=extra)


def test_keys_defaults_and_the_molecule_list(deck):
    s = _load(deck, HEAD + "chol ANALYSIS { type = cholAnalysis; eval_rate = 10; outputrate = 20; rmin = -6 Angstrom; rmax = 6 Angstrom; delta = 0.25 Angstrom; }\n")
    (a,) = s.analysis
    assert a["supported"] and a["type"] == "cholAnalysis" and (a["eval_rate"], a["outputrate"]) == (10, 20)
    assert (a["filename"], a["data_filename"], a["potential_name"]) == ("cholAnalysis.distn", "cholAnalysis.data", "martini")
    assert a["nbins"] == 48 and a["delta"] == (a["rmax"] - a["rmin"]) / 48 and abs(a["rmin"] + 6 * ANG) <= 1e-14 * ANG
    g7 = a["gid7"]
    assert g7.shape == (120, 7) and np.array_equal(g7, chol_molecules(s))
    assert np.all(np.diff(g7.reshape(-1).astype(np.int64)) > 0)      # gid order, roles ascending


def test_other_keys_lrint_and_the_recomputed_delta(deck):
    s = _load(deck, HEAD + "chol ANALYSIS { type = CHOLANALYSIS; filename = d.distn; dataFilename = d.data; rmin = 0; rmax = 1; delta = 0.4; }\n")
    (a,) = s.analysis
    assert a["supported"] and (a["filename"], a["data_filename"]) == ("d.distn", "d.data")
    # lrint(2.5) = 2 (ties to even), and delta formed anew; a bare number is a length in Angstrom
    assert a["nbins"] == 2 and a["delta"] == (a["rmax"] - a["rmin"]) / 2 and a["rmin"] == 0.0 and abs(a["rmax"] - ANG) <= 1e-15 * ANG


def test_the_name_is_matched_in_full(deck):
    s = _load(deck, HEAD + "chol ANALYSIS { type = cholAnalysisX; rmin = 0; rmax = 1; }\n")
    assert not s.analysis[0]["supported"]


def test_a_deck_without_chol_is_legal(tmp_path):
    from chol_deck import LIPID
    import os
    s = load_deck(os.path.join(LIPID, "object.data"), extra_objects=HEAD + "chol ANALYSIS { type = cholAnalysis; rmin = 0; rmax = 1; }\n")
    assert s.analysis[0]["supported"] and s.analysis[0]["gid7"].shape == (0, 7)


@pytest.mark.parametrize("keys, message", [
    ("", "chol: rmin = 0, rmax = 0, delta = .* give 0 bins"),                                    # the defaults: the reference divides by zero
    ("rmin = 1; rmax = 0;", "chol: .* give -10 bins"),
    ("rmin = 0; rmax = 1; delta = 0;", "chol: .* bins"),
    ("rmin = 0; rmax = 1; potentialName = nothing;", "chol: potentialName = nothing, and there is no POTENTIAL object"),
    ("rmin = 0; rmax = 1; potentialName = other;", "chol: potentialName = other is a POTENTIAL of type RESTRAINT, not MARTINI"),
    ("rmin = 0; rmax = 8168; delta = 1;", "chol: 8168 bins need 65544 bytes of the device's LDS, at most 65536"),
])
def test_refusals(deck, keys, message):
    with pytest.raises(RuntimeError, match="ANALYSIS " + message):
        _load(deck, HEAD + "chol ANALYSIS { type = cholAnalysis; %s }\nother POTENTIAL { type = RESTRAINT; }\n" % keys)


def test_the_cap_itself_loads(deck):
    s = _load(deck, HEAD + "chol ANALYSIS { type = cholAnalysis; rmin = 0; rmax = 8167; delta = 1; }\n")
    assert s.analysis[0]["nbins"] == 8167


def test_a_short_chol_residue_is_refused(tmp_path):
    d = chol_deck(tmp_path, "short", residue="TSTM")
    with pytest.raises(RuntimeError, match="ANALYSIS chol: the CHOL residue has 5 atoms, cholAnalysis needs seven"):
        _load(d, HEAD + "chol ANALYSIS { type = cholAnalysis; rmin = 0; rmax = 1; }\n")
    assert load_deck(str(d / "object.data")).natoms > 0      # without the analysis the deck loads

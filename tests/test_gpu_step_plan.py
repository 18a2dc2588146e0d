"""GPU test (-m gpu): WHICH path every force evaluation of a configuration takes -- halo mode, fused, lean, the reduction launch behind a
fused launch, the LDS layout -- as ddcmi_debug_step_plan reports it, against a table written out by hand (tests/step_plan_cases.py).
The rest of the suite holds every path bit for bit against its other side; a configuration that silently stopped running lean, or fell
back to the update launch, would pass all of it and only get slower."""
import json
import os
import sys

import pytest

import step_plan_cases as C
from ranks import run_ranks

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _plans(name, monkeypatch):
    case = C.CASES[name]
    if case.get("fresh_process"):
        res = run_ranks([[sys.executable, os.path.join(HERE, "step_plan_worker.py"), name]], [dict(os.environ)], timeout=300, check=True)
        return [[None if p is None else tuple(p) for p in r] for r in json.loads(res[0].stdout.strip().splitlines()[-1])[name]]
    for k in C.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    return C.run_case(name)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_step_plan(name, monkeypatch):
    case = C.CASES[name]
    want = case["want"]
    for rank, got in enumerate(_plans(name, monkeypatch)):
        print(name, rank, got)
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            if w is None:
                continue
            assert g is not None and g[:4] == w, (name, rank, k, g, w)
            halo, fused, lean, red, level, fixed, hdisp, direct = g
            pair_kernel = name != "lipid_bit_128"
            assert fixed == (1 if pair_kernel else 0), (name, k, g)      # every Martini neighbourhood fits the fixed layout
            if name.startswith("water") or name.startswith("no_"):
                assert level == 0, (name, k, g)      # one or two classes: the direct table costs no workgroup
            if name == "force_level_table":
                assert level == 1, (name, k, g)
            # received beads are read from the receive buffer exactly where the exchange is staged directly, fresh or not
            assert direct == (1 if name == "loopback" else 0), (name, k, g)

"""One case (or several, one after the other) of tests/step_plan_cases.py in a process of its own, with the case's switches in its
environment: prints {case: plans} as one JSON line.  `--no-plans` only runs the cases (a library without ddcmi_debug_step_plan)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, HERE)
import step_plan_cases as C

if __name__ == "__main__":
    names = [a for a in sys.argv[1:] if not a.startswith("--")]
    out = {}
    for name in names:
        for k in C.SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(C.CASES[name]["env"])
        out[name] = C.run_case(name, plans="--no-plans" not in sys.argv)
    print(json.dumps(out))

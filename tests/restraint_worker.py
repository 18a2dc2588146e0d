"""A run of the oscillators of tests/restraint_systems.py in a fresh child process, for the switch the library reads once per process
(DDCMI_NO_FUSED_STEP): started by tests/test_gpu_restraints.py with the switch in the environment.  Writes what it computed to
<out>.npz; never imports the oracle or the reference -- the parent process is the checker.

   python tests/restraint_worker.py <out.npz>"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_blocks(s, blocks=6, per=10, single_steps=False):
    """step 0, then `blocks` times `per` steps (in one call each, or step by step): the state and the sums after every block"""
    from ddcmd_amd.martini import MartiniHIP
    m = MartiniHIP(s)
    m.eval_forces()
    out = {}
    for b in range(blocks):
        if single_steps:
            for _ in range(per):
                m.step(1)
        else:
            m.step(per)
        e, vir, rk, tion = m.energies()
        d = m.download()
        out.update({"r%d" % b: np.stack(d["r"], 1), "v%d" % b: np.stack(d["v"], 1), "f%d" % b: np.stack(d["f"], 1),
                    "e%d" % b: np.array([e["restraint"], e["total"]]), "vir%d" % b: vir, "rk%d" % b: np.array([rk]), "tion%d" % b: tion})
    out["rebuilds"] = np.array([m.list_stats()["rebuilds"]])
    out["box"] = m.box()
    m.close()
    return out


if __name__ == "__main__":
    from restraint_systems import oscillators
    np.savez(sys.argv[1], **run_blocks(oscillators()))
    print("restraint_worker ok")

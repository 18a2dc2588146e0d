"""Six interacting steps of the systems of tests/integrator_reference.py by one of the step's paths: what
tests/test_gpu_integrator_groups.py::test_the_step_paths_agree_bit_for_bit holds against each other.  As a program, every case in
one call of six steps, in a fresh child process for the switch the library reads once per process (DDCMI_NO_FUSED_STEP): started by
that test with the switch in the environment, writes what it computed to <out>.npz; the parent process is the checker.

   python tests/integrator_paths_worker.py <out.npz>"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import integrator_reference as ir

CASES = [(t, n, False) for t in ("mixed", "free", "free+equal-berendsen") for n in ir.TABLE_SIZES] + [("mixed", 65, True)]
IDS = ["%s-%d%s" % (t, n, "-lcg64" if lcg else "") for t, n, lcg in CASES]


def six_steps(s, calls):
    """{sums: per call {rk, tion[6]}; behind the last call: r, v, the group temperatures T, the LCG64 states lcg (if any)}"""
    from ddcmd_amd import martini
    m = martini.MartiniHIP(s)
    try:
        m.eval_forces()
        m.group_temperatures()
        sums = []
        for k in calls:
            m.step(k)
            _, _, rk, tion = m.energies()
            sums.append(np.concatenate(([rk], tion)))
        d = m.download(martini.POS | martini.VEL)
        # (read once, behind the last step, in every run: a read publishes the temperatures to Berendsen's next lambda)
        out = {"sums": np.array(sums), "r": np.stack(d["r"]), "v": np.stack(d["v"]), "T": m.group_temperatures()}
        if s.lcg64 is not None:
            out["lcg"] = m.get_random_lcg64()["state"]
        return out
    finally:
        m.close()


if __name__ == "__main__":
    out = {}
    for name, (table, n, lcg) in zip(IDS, CASES):
        out.update({"%s %s" % (name, k): v for k, v in six_steps(ir.make_system(n, table, True, lcg=lcg), [6]).items()})
    np.savez(sys.argv[1], **out)
    print("integrator_paths_worker ok")

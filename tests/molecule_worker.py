"""A run of the adversarial molecular system (tests/molecule_systems.py) in a fresh child process, for the switches the library
reads once per process (DDCMI_NO_FUSED_STEP, DDCMI_DEBUG_GUARD): started by tests/test_gpu_molecules.py with the switch in
the environment.  Writes what it computed to <out>.npz; never imports the oracle -- the parent process is the checker.

   python tests/molecule_worker.py <wide|narrow> <single|group222> <out.npz>"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_single(s):
    """step 0, then 45 steps in two calls (two rebuilds at updateRate 20): the arrays the parent compares"""
    from ddcmd_amd.martini import MartiniHIP
    m = MartiniHIP(s)
    e0, vir0 = m.eval_forces()
    f0 = np.stack(m.download()["f"])
    st0 = m.list_stats()
    m.step(20)
    m.step(25)
    e, vir, rk, tion = m.energies()
    d = m.download()
    st = m.list_stats()
    m.close()
    return dict(e0=np.array([e0[k] for k in ("lj", "ele", "total")]), vir0=vir0, f0=f0, e=np.array([e[k] for k in ("lj", "ele", "total")]), vir=vir, rk=rk, tion=tion,
                r=np.stack(d["r"]), v=np.stack(d["v"]), f=np.stack(d["f"]),
                stats0=np.array([st0["entries"], st0["excluded"], st0["rebuilds"]]), stats=np.array([st["entries"], st["excluded"], st["rebuilds"]]))


def run_group(s, grid):
    from ddcmd_amd.martini import MartiniGroup
    g = MartiniGroup(s, grid)
    e0, vir0 = g.eval_forces()
    st0 = g.gather()
    g.step(45)
    e, vir, rk, tion = g.energies()
    st = g.gather()
    g.close()
    return dict(e0=np.array([e0[k] for k in ("lj", "ele", "total")]), vir0=vir0, f0=np.stack(st0["f"]), gid=st["gid"],
                e=np.array([e[k] for k in ("lj", "ele", "total")]), vir=vir, rk=rk, tion=tion, r=np.stack(st["r"]), v=np.stack(st["v"]), f=np.stack(st["f"]))


def main():
    variant, mode, out = sys.argv[1], sys.argv[2], sys.argv[3]
    from molecule_systems import make_molecule_setup
    s = make_molecule_setup(variant)
    res = run_single(s) if mode == "single" else run_group(s, (2, 2, 2))
    np.savez(out, **res)
    print("molecule_worker ok")


if __name__ == "__main__":
    main()

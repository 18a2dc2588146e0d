"""Runs of the bonded-layout systems (tests/bonded_systems.py) that tests/test_gpu_bonded_layout.py shares with a fresh child process, for
the switches the library reads once per process (DDCMI_NO_FUSED_STEP, DDCMI_DEBUG_GUARD): the parent starts this file with the switch in
the environment and checks what it wrote to <out>.npz.

   python tests/bonded_worker.py <variant> <0|1: pair kernel on> <single|group222> <out.npz>"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
E_KEYS = ("lj", "ele", "bond", "angle", "tors", "impr", "total")


def with_terms(terms, make):
    """make() with the term lists handed to the device in place of the residue tables' expansion"""
    import ddcmd_amd.martini as martini
    orig = martini.expand_bonded_terms
    martini.expand_bonded_terms = lambda _s: terms
    try:
        return make()
    finally:
        martini.expand_bonded_terms = orig


def census(m):
    """ddcmi_debug_bonded_layout of a context of libddcmi_test.so: [2][12]"""
    import ctypes
    out = ((ctypes.c_int * 12) * 2)()
    m.lib.ddcmi_debug_bonded_layout.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert m.lib.ddcmi_debug_bonded_layout(m.ctx, ctypes.byref(out)) == 0
    return np.array([list(out[0]), list(out[1])])


def run_single(s, terms, by_gid=False):
    """step 0, then 45 steps in two calls (rebuilds at 16 and 32): the arrays the parent compares"""
    from ddcmd_amd.martini import MartiniHIP
    m = with_terms(terms, lambda: MartiniHIP(s, bonded_by_gid=by_gid, test_api=True))
    e0, vir0 = m.eval_forces()
    f0 = np.stack(m.download()["f"])
    cen = census(m)
    m.step(20)
    m.step(25)
    e, vir, rk, tion = m.energies()
    d = m.download()
    st = m.list_stats()
    m.close()
    return dict(e0=np.array([e0[k] for k in E_KEYS]), vir0=vir0, f0=f0, census=cen, e=np.array([e[k] for k in E_KEYS]), vir=vir, rk=rk, tion=tion,
                r=np.stack(d["r"]), v=np.stack(d["v"]), f=np.stack(d["f"]), rebuilds=st["rebuilds"])


def run_group(s, terms, grid):
    """a decomposed run, everything by gid order: step 0, then 45 steps"""
    from ddcmd_amd.martini import MartiniGroup
    g = with_terms(terms, lambda: MartiniGroup(s, grid))
    e0, vir0 = g.eval_forces()
    st0 = g.gather()
    g.step(45)
    e, vir, rk, tion = g.energies()
    st = g.gather()
    g.close()
    return dict(e0=np.array([e0[k] for k in E_KEYS]), vir0=vir0, f0=np.stack(st0["f"]), gid=st["gid"], nlocal0=np.array(st0["nlocal"]), nlocal=np.array(st["nlocal"]),
                e=np.array([e[k] for k in E_KEYS]), vir=vir, rk=rk, tion=tion, r=np.stack(st["r"]), v=np.stack(st["v"]), f=np.stack(st["f"]))


def main():
    variant, nonbonded, mode, out = sys.argv[1], sys.argv[2] == "1", sys.argv[3], sys.argv[4]
    from bonded_systems import make_bonded_setup
    s, terms, _ = make_bonded_setup(variant, nonbonded)
    res = run_single(s, terms) if mode == "single" else run_group(s, terms, (2, 2, 2))
    np.savez(out, **res)
    print("bonded_worker ok")


if __name__ == "__main__":
    main()

"""Runs of the split-occupancy boxes (tests/pair_split_systems.py) that tests/test_gpu_pair_split.py shares with a fresh child process: the
split step is a switch the library reads once per process (DDCMI_NO_FUSED_STEP), so the parent starts this file with it in the environment.
Writes what it computed to <out>.npz; imports neither the oracle nor the reference -- the parent process is the checker.

   python tests/pair_split_worker.py <one_type|charged_mol|types20> <out.npz> <k,k,...>"""
import ctypes
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def context(s, k=None, hooks=True):
    """a context of libddcmi_test.so created under DDCMI_DEBUG_TAIL=k (k None: the variable unset) with or without DDCMI_DEBUG_HOOKS=1;
    the environment is put back before returning (ddcmi_create reads both)"""
    from ddcmd_amd.martini import MartiniHIP
    keep = {v: os.environ.get(v) for v in ("DDCMI_DEBUG_HOOKS", "DDCMI_DEBUG_TAIL")}
    try:
        for v, val in (("DDCMI_DEBUG_HOOKS", "1" if hooks else None), ("DDCMI_DEBUG_TAIL", None if k is None else str(k))):
            if val is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = val
        return MartiniHIP(s, test_api=True)
    finally:
        for v, val in keep.items():
            if val is None:
                os.environ.pop(v, None)
            else:
                os.environ[v] = val


def tile_items(m, cap=None):
    """ddcmi_debug_tile_items (include/ddcmi_test.h): (return code, nitems, item[], nown[])"""
    fn = m.lib.ddcmi_debug_tile_items
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    n = ctypes.c_int(-1)
    if cap is None:
        fn(m.ctx, 0, ctypes.byref(n), None, None)
        cap = n.value
    item, nown = np.full(max(cap, 1), -7, np.int32), np.full(max(cap, 1), -7, np.int32)
    rc = fn(m.ctx, int(cap), ctypes.byref(n), item.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), nown.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return rc, n.value, item[:cap], nown[:cap]


def run_steps(s, k, nsteps=2):
    """step 0 and nsteps steps under DDCMI_DEBUG_TAIL=k: positions and velocities [3, n], the work items"""
    m = context(s, k)
    m.eval_forces()
    m.step(nsteps)
    d = m.download()
    rc, n, item, nown = tile_items(m)
    m.close()
    assert rc == 0
    return dict(r=np.stack(d["r"]), v=np.stack(d["v"]), item=item)


def main():
    variant, out, ks = sys.argv[1], sys.argv[2], [int(x) for x in sys.argv[3].split(",")]
    from pair_split_systems import make_split_setup
    s = make_split_setup(variant)
    rec = {}
    for k in ks:
        rec.update({"%s%d" % (name, k): a for name, a in run_steps(s, k).items()})
    np.savez(out, **rec)
    print("pair_split_worker ok")


if __name__ == "__main__":
    main()

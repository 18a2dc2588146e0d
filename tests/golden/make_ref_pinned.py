"""Record the reference's answers that tests/test_ref_pinned.py and tests/test_gpu_ref_solve.py are pinned to:
tests/golden/ref_pinned.npz.  Runs where oracle/_ref is built (make -C oracle ref: the reference's crc32.c, primes.c,
format.c and solve.c compiled where they lie); every answer comes from that library through tests/ref_probe.py.

    crc               [table, bitwise] checksum of each record of ref_probe.records()
    primes_T_N        700 x nextPrime() after prime_init(30000, T, N)
    formats           loopFormat(), gidFormat()
    solve_<tape>_*    solve() over the linear systems one run of res_move_cons meets, in order: a digest of each
                      system (size, sum |M|, sum |rhs|) and the solutions, concatenated

    python tests/golden/make_ref_pinned.py
"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ref_pinned as T  # noqa: E402

DT = 20.0


def main():
    assert os.path.exists(T.REF), "%s is not built (make -C oracle ref)" % T.REF
    out = {"crc": np.array(T._live("crc"), dtype=np.uint64), "formats": np.array(T._live("formats"))}
    for task, ntasks in ((0, 1), (3, 8), (7, 8), (1, 2)):
        out["primes_%d_%d" % (task, ntasks)] = np.array(T._live("primes", task, ntasks), dtype=np.uint64)
    T.RECORD = {}
    for seed in (1, 2):          # test_constraint_solve_against_the_references_linear_solver
        sysd = T.make_constraint_system(seed)
        for location in (0, 1):
            T.res_move_cons(location, T.groups_of(sysd, sysd["r"], sysd["v"]), DT, "cpu%d_%d" % (seed, location))
    for seed in (3, 4):          # test_device_constraint_step_against_the_references_linear_solver: its FRONT, drift, BACK
        sysd = T.make_constraint_system(seed, box=120.0, copies=4)
        g0 = T.groups_of(sysd, sysd["r"], sysd["v"])
        T.res_move_cons(0, g0, DT, "gpu%d_0" % seed)
        v1 = sysd["v"].copy()
        for g in g0:
            v1[g["idx"]] = g["V"]
        T.res_move_cons(1, T.groups_of(sysd, sysd["r"] + DT * v1, v1), DT, "gpu%d_1" % seed)
    for name, (digests, xs) in sorted(T.RECORD.items()):
        out["solve_%s_digest" % name] = np.array(digests)
        out["solve_%s_x" % name] = np.concatenate(xs)
    np.savez_compressed(T.RECORDED, **out)
    print("wrote %s (%d bytes)" % (T.RECORDED, os.path.getsize(T.RECORDED)))


if __name__ == "__main__":
    main()

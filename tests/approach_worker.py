"""A run of the collider (tests/approach_systems.py) in a fresh child process, for the switch the library reads once per process
(DDCMI_NO_FUSED_STEP): started by tests/test_gpu_shell_walk.py with the switch in the environment.  Writes what it computed to
<out>.npz; never imports the oracle -- the parent process is the checker.

   python tests/approach_worker.py <one_type|types20|charged> <out.npz>
   python tests/approach_worker.py rank <outdir> <calls, e.g. 3,4,4>      one rank of the two-rank run of one_sided() over the host transport
                                                                         (RANK / WORLD_SIZE / MASTER_ADDR / DDCMI_RDZV_FILE as for tests/mp_worker.py)"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def run_one_call(s):
    """step 0, then updateRate + 5 steps in ONE call: the arrays the parent compares"""
    from ddcmd_amd.martini import MartiniHIP
    m = MartiniHIP(s)
    m.eval_forces()
    m.step(int(s.updateRate) + 5)
    e, vir, rk, tion = m.energies()
    d = m.download()
    st = m.list_stats()
    m.close()
    return dict(e=np.array([e[k] for k in ("lj", "ele", "total")]), vir=vir, rk=rk, tion=tion, r=np.stack(d["r"]), v=np.stack(d["v"]), f=np.stack(d["f"]),
                rebuilds=st["rebuilds"])


def run_rank(outdir, pattern):
    """this rank's beads (by gid) after the force evaluation of step 0 and after every call: rank<r>.npz"""
    from approach_systems import one_sided
    from ddcmd_amd.martini import MartiniRank, Rendezvous, domain_of, _declare_domains
    rdzv = Rendezvous.from_env(timeout=60.0)
    s = one_sided()
    m = MartiniRank(s, np.flatnonzero(domain_of(s, s.grid) == rdzv.rank), device=0)
    _declare_domains(m.lib)
    m.comm_init_host(rdzv, s.grid)
    m.upload_local()
    m.eval_forces()
    rec = {}
    for c, k in enumerate((0,) + tuple(pattern)):
        if k:
            m.step(k)
        p = m.download_particles()
        rec.update({"gid%d" % c: p["gid"], "r%d" % c: np.stack(p["r"], 1), "v%d" % c: np.stack(p["v"], 1), "f%d" % c: np.stack(p["f"], 1)})
    rec["transport"] = np.array([m.comm_stats()["transport"]])
    np.savez(os.path.join(outdir, "rank%d.npz" % rdzv.rank), **rec)
    m.close()
    rdzv.barrier()
    rdzv.close()


def main():
    if sys.argv[1] == "rank":
        run_rank(sys.argv[2], [int(x) for x in sys.argv[3].split(",")])
        print("approach_worker ok")
        return
    variant, out = sys.argv[1], sys.argv[2]
    from approach_systems import collider
    np.savez(out, **run_one_call(collider(variant)))
    print("approach_worker ok")


if __name__ == "__main__":
    main()

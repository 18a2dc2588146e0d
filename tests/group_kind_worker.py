"""One rank of a decomposed run of a gas of tests/group_kind_systems.py over the host transport (started by
tests/test_gpu_group_kinds.py as a fresh child process): rendezvous from RANK / WORLD_SIZE / MASTER_ADDR, the table's groups from the
Setup, then -- as a host would between steps -- a new vector for the FIXEDVELOCITY groups through MartiniRank.set_group_velocity on
every rank, `nsteps` NGLF steps, and every rank writes its own beads (by gid) to <outdir>/rank<r>.npz.  The parent is the checker.

   python tests/group_kind_worker.py <table> <n> <px>x<py>x<pz> <outdir> <nsteps> <factor>"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def new_vectors(s, factor):
    """the vectors the run sets after the contexts exist: the Setup's, scaled"""
    return np.asarray(s.group_vset, np.int32), np.asarray(s.group_v, float) * factor


def main():
    table, n, gridtxt, outdir, nsteps, factor = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4], int(sys.argv[5]), float(sys.argv[6])
    grid = tuple(int(x) for x in gridtxt.split("x"))
    from ddcmd_amd.martini import MartiniRank, Rendezvous, domain_of, _declare_domains
    import group_kind_systems as G
    rdzv = Rendezvous.from_env(timeout=120.0)
    s = G.system("gas", n, table)
    owner = domain_of(s, grid)
    m = MartiniRank(s, np.flatnonzero(owner == rdzv.rank), device=0)
    _declare_domains(m.lib)
    m.comm_init_host(rdzv, grid)
    m.upload_local()
    m.set_group_velocity(*new_vectors(s, factor))
    m.eval_forces()
    m.step(nsteps)
    p = m.download_particles()
    np.savez(os.path.join(outdir, "rank%d.npz" % rdzv.rank), gid=p["gid"], r=np.stack(p["r"]), v=np.stack(p["v"]), f=np.stack(p["f"]))
    m.close()
    rdzv.barrier()
    rdzv.close()


if __name__ == "__main__":
    main()

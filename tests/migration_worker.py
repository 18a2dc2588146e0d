"""One rank of crossers((2, 1, 1)) with passengers between real processes over the host transport (started by
tests/test_gpu_migration.py through tests/ranks.py): step 0 and two rebuild periods, the rank's own beads by gid after each, written to
<outdir>/rank<r>.npz.  The parent process is the checker.

   python tests/migration_worker.py <outdir>"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    outdir = sys.argv[1]
    import migration_systems as M
    from ddcmd_amd.martini import MartiniRank, Rendezvous, domain_of, _declare_domains
    rdzv = Rendezvous.from_env(timeout=float(os.environ.get("DDCMI_TEST_RDZV_TIMEOUT", "120")))
    grid = (2, 1, 1)
    s = M.system("crossers", grid, 7, passengers=True)
    m = MartiniRank(s, np.flatnonzero(domain_of(s, grid) == rdzv.rank), device=0)
    _declare_domains(m.lib)
    m.comm_init_host(rdzv, grid)
    m.upload_local()
    m.eval_forces()
    rec = {}
    for k in range(3):
        if k:
            m.step(M.UPDATE)
        p = m.download_particles()
        rec.update({"gid%d" % k: p["gid"], "species%d" % k: p["species"], "r%d" % k: np.stack(p["r"], 1), "v%d" % k: np.stack(p["v"], 1),
                    "f%d" % k: np.stack(p["f"], 1), "state%d" % k: p["lcg64"]["state"], "prime%d" % k: p["lcg64"]["prime"],
                    "multID%d" % k: p["lcg64"]["multID"]})
    np.savez(os.path.join(outdir, "rank%d.npz" % rdzv.rank), **rec)
    m.close()
    rdzv.barrier()
    rdzv.close()


if __name__ == "__main__":
    main()

"""One rank of a multi-process decomposed run with ANALYSIS VELOCITYAUTOCORRELATION tracking (started by tests/test_gpu_vaf.py as a
fresh child process, after the pattern of tests/mp_worker.py): rendezvous from RANK / WORLD_SIZE / MASTER_ADDR, decomposition over
the host transport, an origin, then a sample every <every> steps with a new origin after <length> samples.  At every sample the
rank writes its own beads (by gid) and its own sums to <outdir>/rank<r>.npz; the parent process is the checker."""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    gridtxt, outdir, nsamples, every, length = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    grid = tuple(int(x) for x in gridtxt.split("x"))
    import ddcmd_amd
    from ddcmd_amd.martini import MartiniRank, Rendezvous, domain_of, _declare_domains
    rdzv = Rendezvous.from_env(timeout=float(os.environ.get("DDCMI_TEST_RDZV_TIMEOUT", "120")))
    rank = rdzv.rank
    s = ddcmd_amd.make_water_setup(12)
    owner = domain_of(s, grid)
    m = MartiniRank(s, np.flatnonzero(owner == rank), device=0)
    _declare_domains(m.lib)
    m.comm_init_host(rdzv, grid)
    m.upload_local()
    m.eval_forces()
    rec = {}

    def take(tag):
        p = m.download_particles()
        vaf, msd = m.vaf_sample()
        rec.update({"gid_" + tag: p["gid"], "r_" + tag: np.stack(p["r"]), "v_" + tag: np.stack(p["v"]), "vaf_" + tag: vaf, "msd_" + tag: msd})

    m.vaf_origin()
    take("o0")
    k = 0
    for it in range(nsamples):
        m.step(every)
        k += 1
        take("s%d" % it)
        if k == length:
            m.vaf_origin()      # every rank, at the same point of the run
            take("o%d" % (it + 1))
            k = 0
    rec["rebuilds"] = np.array([m.list_stats()["rebuilds"]])
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), **rec)
    m.close()
    rdzv.barrier()
    rdzv.close()


if __name__ == "__main__":
    main()

"""Child processes of tests/test_gpu_track.py (no tests in here).
   python tests/track_worker.py paths <out.npz>            the twin runs of track_systems.twin_run on the small water box, with and without
                                                           tracking, in a fresh process for the switches the library reads once
                                                           (DDCMI_NO_FUSED_STEP in the environment)
   python tests/track_worker.py rank <PxQxR> <outdir>      one rank of a decomposed run over the host transport (RANK / WORLD_SIZE /
                                                           MASTER_ADDR from the environment, as tests/mp_vaf_worker.py): the crossers of
                                                           tests/migration_systems.py, tracked over a window of samples; writes the rank's
                                                           sums and hits and, on rank 0, the sum over the ranks in rank order"""
import os
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
RANK_SCHEDULE = (0, 4, 6, 10, 3, 7)      # steps in front of each sample: 30 in all, rebuilds every 10


def paths(out):
    import ddcmd_amd
    import track_systems as T
    s = ddcmd_amd.make_water_setup(6)
    gids = T.tracked_list(s, 65)[0]
    a, b = T.twin_run(s, True, gids), T.twin_run(s, False)
    np.savez(out, **dict([("a_" + k, v) for k, v in a.items()] + [("b_" + k, v) for k, v in b.items()]))


def rank(gridtxt, outdir):
    import migration_systems as M
    import track_systems as T
    from ddcmd_amd.martini import MartiniRank, Rendezvous, domain_of, _declare_domains
    grid = tuple(int(x) for x in gridtxt.split("x"))
    rdzv = Rendezvous.from_env(timeout=float(os.environ.get("DDCMI_TEST_RDZV_TIMEOUT", "120")))
    s = M.crossers(grid)
    gids = planted_list(s)
    m = MartiniRank(s, np.flatnonzero(domain_of(s, grid) == rdzv.rank), device=0)
    _declare_domains(m.lib)
    m.comm_init_host(rdzv, grid)
    m.upload_local()
    m.eval_forces()
    m.track_set(gids)
    owned = []
    for k in RANK_SCHEDULE:
        if k:
            m.step(k)
        m.track_accumulate("position")
        owned.append(int(m.lib.ddcmi_nlocal(m.ctx)))
    tot, hits = m.track_read()
    both = rdzv.allreduce(np.concatenate([tot.ravel(), hits.astype(np.float64)]))      # op 0: the sum in rank order
    np.savez(os.path.join(outdir, "rank%d.npz" % rdzv.rank), tot=tot, hits=hits, both=both, owned=np.array(owned))
    m.close()
    rdzv.barrier()
    rdzv.close()


def planted_list(s):
    """every planted mover and as many beads of the background, shuffled, with two gids no bead carries"""
    rng = np.random.RandomState(5)
    gid = np.asarray(s.gid, np.uint64)
    pl = np.asarray(s.planted_all)
    bg = np.setdiff1d(np.arange(len(gid)), pl)[:len(pl)]
    out = np.concatenate([gid[pl], gid[bg], np.array([gid.max() + np.uint64(1), np.uint64(1)], np.uint64)])
    return out[rng.permutation(len(out))]


if __name__ == "__main__":
    if sys.argv[1] == "paths":
        paths(sys.argv[2])
    else:
        rank(sys.argv[2], sys.argv[3])
    print("track_worker ok")

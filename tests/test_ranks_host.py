"""CPU: the rank launcher of the tests themselves (tests/ranks.py) -- one time limit for the group, nobody killed before it, nobody
left after it, no pipe to fill, and the environment the ranks have always been given."""
import os
import subprocess
import sys
import time

import pytest

import ranks
from ranks import rank_env, run_ranks


def py(code):
    return [sys.executable, "-c", code]


@pytest.fixture
def spawned(monkeypatch):
    """every Popen object run_ranks makes"""
    made, real = [], subprocess.Popen

    def popen(*args, **kw):
        made.append(real(*args, **kw))
        return made[-1]
    monkeypatch.setattr(ranks.subprocess, "Popen", popen)
    return made


def assert_gone(procs):
    for p in procs:
        assert p.returncode is not None
        with pytest.raises(ProcessLookupError):
            os.kill(p.pid, 0)


def test_timeout_reaps_the_group(spawned):
    t0 = time.time()
    with pytest.raises(TimeoutError) as ei:
        run_ranks([py("import sys; sys.stderr.write('QUICK-MARK'); sys.exit(5)"), py("import sys, time; sys.stderr.write('SLOW-MARK'); sys.stderr.flush(); time.sleep(60)")],
                  [None, None], timeout=2)
    assert time.time() - t0 < 5
    msg = str(ei.value)
    assert "ranks [1] were still running" in msg and "rank 1: still running" in msg and "rank 0: ended with code 5" in msg
    assert "QUICK-MARK" in msg and "SLOW-MARK" in msg
    assert len(spawned) == 2 and spawned[1].returncode == -9
    assert_gone(spawned)


def test_a_failing_ranks_peers_are_not_killed_early():
    res = run_ranks([py("import sys; sys.exit(3)"), py("import sys, time; time.sleep(1); sys.exit(3)")], [None, None], timeout=30)
    assert [r.returncode for r in res] == [3, 3]


def test_check_reaps_before_it_raises(spawned):
    with pytest.raises(AssertionError) as ei:
        run_ranks([py("import sys; sys.stderr.write('BAD-MARK'); sys.exit(3)"), py("import sys, time; time.sleep(0.3); sys.stderr.write('GOOD-MARK')")],
                  [None, None], timeout=30, check=True)
    msg = str(ei.value)
    assert "BAD-MARK" in msg and "GOOD-MARK" in msg and "rank 0: ended with code 3" in msg and "rank 1: ended with code 0" in msg
    assert len(spawned) == 2
    assert_gone(spawned)


def test_a_megabyte_of_output_blocks_nobody(tmp_path):
    """rank 0 ends only after rank 1 has written everything: with the ranks' pipes drained one after another, rank 1 would fill its
    pipe while the parent reads rank 0's, and neither would end"""
    flag = str(tmp_path / "written")
    waits = "import os, time\nwhile not os.path.exists(%r): time.sleep(0.01)\n" % flag
    writes = "import sys\nsys.stderr.write('e' * (1 << 20)); sys.stdout.write('o' * (1 << 20)); sys.stderr.flush(); sys.stdout.flush(); open(%r, 'w').close()\n" % flag
    t0 = time.time()
    res = run_ranks([py(waits), py(writes)], [None, None], timeout=30, check=True)
    assert time.time() - t0 < 10
    assert res[1].stdout == "o" * (1 << 20) and res[1].stderr == "e" * (1 << 20) and res[0].stdout == res[0].stderr == ""


def test_rank_env_is_what_the_ranks_were_always_given(monkeypatch):
    monkeypatch.setenv("DDCMI_RCCL_LOOPBACK", "1")
    monkeypatch.setenv("MASTER_PORT", "29500")
    rank, world, d = 1, 4, "/some/dir"
    # a worker script's rank, as tests/test_gpu_multiproc.py wrote it out before this module existed
    env = dict(os.environ)
    env.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": "1",
                "DDCMI_RDZV_FILE": os.path.join(d, "port"), "DDCMI_TRANSPORT": "host"})
    env.pop("DDCMI_RCCL_LOOPBACK", None)
    assert rank_env(rank, world, d) == env and "DDCMI_SINGLE_DEVICE" not in env
    env.update({"DDCMI_DEBUG_HOOKS": "1"})
    assert rank_env(rank, world, d, {"DDCMI_DEBUG_HOOKS": "1"}) == env
    # a rank of the ddcmi_md driver, as the driver tests wrote it out
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", DDCMI_TRANSPORT="host", DDCMI_SINGLE_DEVICE="1",
               DDCMI_RDZV_FILE=os.path.join(d, "rdzv_port"))
    env = dict(env, RANK=str(rank), LOCAL_RANK=str(rank))
    assert rank_env(rank, world, d, single_device=True) == env and env["MASTER_PORT"] == "29500" and env["DDCMI_RCCL_LOOPBACK"] == "1"

"""The one place where the tests start a group of real processes -- ranks of ddcmi_md, of the worker scripts, of the rendezvous --
and the one place that ends them: whatever happens to a test, no rank it started outlives run_ranks()."""
import collections
import os
import shutil
import subprocess
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ddcmd_amd", "bin", "ddcmi_md")
GOLDEN = os.path.join(ROOT, "tests", "golden")
Result = collections.namedtuple("Result", "returncode stdout stderr")
Out = collections.namedtuple("Out", "stdout stderr")


def rank_env(rank, world, rdzv_dir, extra=None, single_device=False):
    """the environment a launcher hands rank `rank` of `world`: the host transport, the port published in a file under rdzv_dir.
    single_device: the ddcmi_md driver's ranks, all on the one device of a test box; otherwise the worker scripts' ranks, which
    publish an ephemeral port (MASTER_PORT = 1) and must not inherit the loopback transport"""
    env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", DDCMI_TRANSPORT="host")
    if single_device:
        env.update(DDCMI_SINGLE_DEVICE="1", DDCMI_RDZV_FILE=os.path.join(rdzv_dir, "rdzv_port"))
    else:
        env.update(MASTER_PORT="1", DDCMI_RDZV_FILE=os.path.join(rdzv_dir, "port"))
        env.pop("DDCMI_RCCL_LOOPBACK", None)
    env.update(extra or {})
    return env


def _report(procs, late, results):
    lines = []
    for r, (p, res) in enumerate(zip(procs, results)):
        lines.append("rank %d: %s" % (r, "still running at the time limit, killed" if r in late else "ended with code %d" % p.returncode))
        lines.append("  stdout: ..." + res.stdout[-1500:])
        lines.append("  stderr: ..." + res.stderr[-3000:])
    return "\n".join(lines)


def run_ranks(cmds, envs, cwd=None, timeout=600, check=False):
    """start every command (envs[k] = None inherits the environment), wait for ALL of them under one time limit, return [Result].
    The output goes to files, so no rank waits on a pipe nobody reads.  A rank that fails does not end its peers: how they end by
    themselves is what some tests are about.  At the limit the ranks still running are killed and TimeoutError says who had
    ended how; check = True asserts afterwards that every rank returned 0.  No process is left when this returns or raises."""
    with tempfile.TemporaryDirectory() as logs:
        paths = [(os.path.join(logs, "rank%d.out" % r), os.path.join(logs, "rank%d.err" % r)) for r in range(len(cmds))]
        procs, late = [], []
        try:
            for cmd, env, (po, pe) in zip(cmds, envs, paths):
                with open(po, "w") as fo, open(pe, "w") as fe:
                    procs.append(subprocess.Popen(cmd, cwd=cwd, env=env, stdout=fo, stderr=fe))
            deadline = time.monotonic() + timeout
            try:
                for p in procs:
                    p.wait(timeout=max(0.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                late = [r for r, p in enumerate(procs) if p.poll() is None]
        finally:
            for p in procs:
                if p.poll() is None:
                    p.kill()
                p.wait()
        results = [Result(p.returncode, open(po, errors="replace").read(), open(pe, errors="replace").read()) for p, (po, pe) in zip(procs, paths)]
    if late:
        raise TimeoutError("ranks %s were still running after %g s\n%s" % (late, timeout, _report(procs, late, results)))
    if check:
        assert all(res.returncode == 0 for res in results), "\n" + _report(procs, late, results)
    return results


def driver_ranks(world, args, cwd, timeout=600, check=False):
    """`world` ddcmi_md processes as a launcher that only sets RANK / WORLD_SIZE / LOCAL_RANK starts them: [Result]"""
    return run_ranks([[EXE] + args] * world, [rank_env(r, world, str(cwd), single_device=True) for r in range(world)], cwd=str(cwd),
                     timeout=timeout, check=check)


def run_driver(cwd, extra, world=1, timeout=600):
    """ddcmi_md on the deck in cwd with the objects of `extra` added, on one rank or several: [Out] by rank, every rank returned 0"""
    args = ["-o", "object.data", "-d", "data"] + (["-x", extra] if extra else [])
    if world == 1:
        res = run_ranks([[EXE] + args], [None], cwd=str(cwd), timeout=timeout, check=True)
    else:
        res = driver_ranks(world, args, cwd, timeout=timeout, check=True)
    return [Out(r.stdout, r.stderr) for r in res]


def copy_deck(tmp_path, which, name):
    d = tmp_path / name
    shutil.copytree(os.path.join(GOLDEN, which), str(d))
    return d


def tree_files(d):
    """every file under d, as sorted paths relative to it"""
    return sorted(os.path.relpath(os.path.join(p, f), str(d)) for p, _, fs in os.walk(str(d)) for f in fs)

#!/usr/bin/env python3
"""ANALYSIS VELOCITYAUTOCORRELATION on the headline water box: what one sample costs and what tracking costs the run.
   python3 tools/time_vaf.py [lattice]   (default 102: 4.24 M beads)
Prints (1) one ddcmi_vaf_sample by HIP events recorded on the context's stream around the call (both kernels and the copy of the
result; median of 20 after 3 warm-up calls) beside the bytes it reads -- position 32 B, velocity 24 B, record 48 B, group and
species words 8 B per bead -- and the share of the 8 TB/s HBM roof that is, with the host clock around the [sync] call next to it;
(2) ms per step of three runs of 400 steps (100 warm-up, rebuilds included) without tracking -- the code path of a build without
the feature -- and three with an origin set and no sample; (3) the list rebuild (ddcmi_build_list, host clock, median of 10)
without and with the record riding through k_gather_state."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ddcmd_amd
from ddcmd_amd.martini import MartiniHIP

n = int(sys.argv[1]) if len(sys.argv) > 1 else 102
s = ddcmd_amd.make_water_setup(n)
hip = ctypes.CDLL("libamdhip64.so")
vp = ctypes.c_void_p
hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
hip.hipEventRecord.argtypes = [vp, vp]
hip.hipEventSynchronize.argtypes = [vp]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]


def run(track, steps=400, warm=100):
    m = MartiniHIP(s)
    m.eval_forces()
    if track:
        m.vaf_origin()
    m.step(warm)
    m.sync()
    t0 = time.perf_counter()
    m.step(steps)
    m.sync()
    dt = (time.perf_counter() - t0) / steps
    m.close()
    return 1e3 * dt


def rebuild(track, reps=10):
    m = MartiniHIP(s)
    m.eval_forces()
    if track:
        m.vaf_origin()
    m.step(5)
    t = []
    for _ in range(reps + 2):
        m.sync()
        t0 = time.perf_counter()
        m.build_list()
        m.sync()
        t.append(time.perf_counter() - t0)
    m.close()
    return 1e3 * float(np.median(t[2:]))


m = MartiniHIP(s)
m.eval_forces()
m.vaf_origin()
m.step(10)
stream = m.lib.ddcmi_stream(m.ctx)
e0, e1 = vp(), vp()
assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
for _ in range(3):
    m.vaf_sample()
host, dev = [], []
for _ in range(20):
    hip.hipEventRecord(e0, stream)
    t0 = time.perf_counter()
    m.vaf_sample()
    host.append(time.perf_counter() - t0)
    hip.hipEventRecord(e1, stream)
    hip.hipEventSynchronize(e1)
    ms = ctypes.c_float(0)
    hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1)
    dev.append(ms.value * 1e-3)
m.close()
nbytes = s.natoms * (32 + 24 + 48 + 8)
med = float(np.median(dev))
print("sample: %d beads, %.3f ms by events (min %.3f; host clock %.3f ms), %.3f GB read, %.2f TB/s = %.0f %% of 8 TB/s"
      % (s.natoms, 1e3 * med, 1e3 * min(dev), 1e3 * float(np.median(host)), nbytes / 1e9, nbytes / med / 1e12, 100 * nbytes / med / 8e12), flush=True)
off = [run(False) for _ in range(3)]
on = [run(True) for _ in range(3)]
print("ms/step without tracking:   %s" % " ".join("%.4f" % x for x in off), flush=True)
print("ms/step with an origin set: %s" % " ".join("%.4f" % x for x in on), flush=True)
print("rebuild without / with the record: %.3f / %.3f ms" % (rebuild(False), rebuild(True)), flush=True)

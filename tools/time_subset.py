"""One subsetWrite frame of the 4.24 M-bead water box (run from the repository root on a GPU): ddcmi_subset_records for every bead and
for modulus = 10, next to ddcmi_download_particles of gid and positions followed by packing in numpy.  Medians of 15 synchronous
calls after two warm-up calls; the output is profiles/subset_time.txt."""
import ctypes, sys, time
import numpy as np
sys.path.insert(0, ".")
import ddcmd_amd
from ddcmd_amd.martini import MartiniHIP, SUBSET_RECORD, _up, _d
s = ddcmd_amd.make_water_setup(102)
m = MartiniHIP(s)
n = s.natoms
cL = ddcmd_amd.deck.units_convert(1.0, None, "Ang")
corner = -0.5 * np.array([s.h[0], s.h[4], s.h[8]])
gid = np.zeros(n + 16, np.uint64); r = [np.zeros(n + 16) for _ in range(3)]
def parent(modulus):
    k = ctypes.c_int(0)
    rc = m.lib.ddcmi_download_particles(m.ctx, n + 16, ctypes.byref(k), gid.ctypes.data_as(_up), None, _d(r[0]), _d(r[1]), _d(r[2]), None, None, None, None, None, None)
    assert rc == 0
    keep = slice(None) if modulus == 1 else np.flatnonzero(gid[:n] % np.uint64(modulus) == 0)
    out = np.zeros(n if modulus == 1 else len(keep), SUBSET_RECORD)
    out["id"] = gid[:n][keep]
    for a in range(3):
        out["r"][:, a] = ((r[a][:n][keep] - corner[a]) * cL).astype(np.float32)
    return out
def med(f, reps=15):
    f(); f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append(time.perf_counter() - t0)
    t = np.array(t) * 1e3
    return "median %.2f ms (min %.2f, max %.2f, %d runs)" % (np.median(t), t.min(), t.max(), reps)
for modulus in (1, 10):
    a = m.subset_records(modulus=modulus, cL=cL); b = parent(modulus)
    assert a["id"].tobytes() == b["id"].tobytes() and a["r"].tobytes() == b["r"].tobytes()
    print("n = %d modulus = %d: %d records" % (n, modulus, len(a)))
    print("  ddcmi_subset_records (count call + records call): " + med(lambda: m.subset_records(modulus=modulus, cL=cL)))
    print("  count only:                                       " + med(lambda: m.subset_records(count_only=True, modulus=modulus, cL=cL)))
    print("  download_particles(gid, r) + numpy packing:       " + med(lambda: parent(modulus)))
    k = ctypes.c_int(0)
    print("  download_particles(gid, r) alone:                 " + med(lambda: m.lib.ddcmi_download_particles(m.ctx, n + 16, ctypes.byref(k), gid.ctypes.data_as(_up), None, _d(r[0]), _d(r[1]), _d(r[2]), None, None, None, None, None, None)))
m.close()

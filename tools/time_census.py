#!/usr/bin/env python3
"""ANALYSIS vcmWrite, zdensity, KINETICENERGYDISTN, DSF, subsetWrite, COARSEGRAIN, (chol:<lattice>, default 63: 1.0 M beads, 10^5 molecules) cholAnalysis and (track:<lattice>, 64: 1.05 M beads) FORCE_AVERAGE on the headline boxes: what one call of each entry point costs, beside one ddcmi_vaf_sample and
one plain step of the same box in the same process.
   python3 tools/time_census.py [water:<lattice> | lipid:<x,y,z>] ...   (default: water:102 lipid:12,12,6 -- 4.24 M and 2.04 M beads)
Every call is timed by HIP events recorded on the context's stream around it (the kernels and the copy of the result; median of
20 after 3 warm-up calls), with the host clock around the [sync] call next to it; the step is the mean of 200 steps after 50
(rebuilds included), host clock.  Bytes read per bead: momentum 24 (velocity) + 8 (group, species words); zdensity 32 (the position
record); the VAF sample 32 + 24 + 48 + 8; the kinetic-energy histogram 24 (velocity) + 4 (species word).  The rows of
ddcmi_structure_modes give sincospi evaluations per second against the FP64 vector issue rate instead: its work is arithmetic."""
import ctypes, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import ddcmd_amd
from ddcmd_amd.martini import MartiniHIP
from ddcmd_amd.analysis import expand_signs, in_plane

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
hip = ctypes.CDLL("libamdhip64.so")
vp = ctypes.c_void_p
hip.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
hip.hipEventRecord.argtypes = [vp, vp]
hip.hipEventSynchronize.argtypes = [vp]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]


def system(spec):
    kind, arg = spec.split(":")
    if kind == "water":
        return ddcmd_amd.make_water_setup(int(arg)), "water"
    from ddcmd_amd.deck import load_deck
    from ddcmd_amd.synth import replicate_setup
    deck = os.path.join(ROOT, "tests", "golden", "lipid_deck")
    s = load_deck(os.path.join(deck, "object_nvt.data"), restart_file=os.path.join(deck, "relaxed", "restart"))
    return replicate_setup(s, tuple(int(x) for x in arg.split(","))), "bilayer"


def timed(m, call, e0, e1, reps=20, warm=3):
    """(median ms by events, min, median ms on the host clock)"""
    stream = m.lib.ddcmi_stream(m.ctx)
    for _ in range(warm):
        call()
    host, dev = [], []
    for _ in range(reps):
        hip.hipEventRecord(e0, stream)
        t0 = time.perf_counter()
        call()
        host.append(time.perf_counter() - t0)
        hip.hipEventRecord(e1, stream)
        hip.hipEventSynchronize(e1)
        ms = ctypes.c_float(0)
        hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1)
        dev.append(ms.value)
    return float(np.median(dev)), min(dev), 1e3 * float(np.median(host))


def chol_rows(lattice, nmol=100000):
    """ANALYSIS cholAnalysis (ddcmi_chol_offsets) on a synthetic box: the water lattice of about 10^6 beads with nmol molecules planted as
    lists of seven beads each (the pass costs the same whatever their geometry), beside what the same result cost before the pass
    existed: ddcmi_download_particles of the same state, without the host arithmetic.  The first call sorts and uploads the list; the
    later ones find it kept with the context."""
    s = ddcmd_amd.make_water_setup(int(lattice))
    m = MartiniHIP(s)
    m.eval_forces()
    m.step(20)
    m.sync()
    rng = np.random.RandomState(1)
    gid7 = np.asarray(s.gid, np.uint64)[rng.permutation(s.natoms)[:7 * nmol]].reshape(-1, 7)
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    L = float(s.h[0])
    t0 = time.perf_counter()
    m.chol_offsets(gid7, -0.5 * L, L / 100, 100)
    first = 1e3 * (time.perf_counter() - t0)
    print("cholAnalysis: %d beads, %d molecules listed; the first call (sorts and uploads the list) %.3f ms on the host clock" % (s.natoms, len(gid7), first), flush=True)
    cap, nout = s.natoms + 16, ctypes.c_int(0)
    dg, dr = np.zeros(cap, np.uint64), [np.zeros(cap) for _ in range(3)]

    def download():      # what the host arithmetic needs: the gids and the positions (no species, velocities or forces)
        m._chk(m.lib.ddcmi_download_particles(m.ctx, cap, ctypes.byref(nout), dg.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), None,
                                              *[a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for a in dr], None, None, None, None, None, None))
    rows = [("chol_offsets 100 bins", lambda: m.chol_offsets(gid7, -0.5 * L, L / 100, 100)),
            ("chol_offsets 8167 bins", lambda: m.chol_offsets(gid7, -0.5 * L, L / 8167, 8167)),
            ("chol_offsets other list", None),
            ("ddcmi_download_particles gid, r", download)]
    flip = [gid7, gid7[::-1].copy()]
    for label, call in rows:
        if call is None:      # the list changes every call: the sort and the upload every time
            state = [0]

            def call():
                state[0] ^= 1
                m.chol_offsets(flip[state[0]], -0.5 * L, L / 100, 100)
        med, lo, host = timed(m, call, e0, e1)
        print("  %-32s %8.4f ms by events (min %.4f; host clock %.4f ms)" % (label, med, lo, host), flush=True)
    m.close()


def track_rows(lattice):
    """ANALYSIS FORCE_AVERAGE: one ddcmi_track_accumulate on the water box with 64 and with 65536 tracked gids (picked at random, so
    the list's gid range covers the box and every bead searches), beside one ddcmi_momentum_by_class of the same state, the cheapest
    census pass.  The accumulation does not wait for the device: the events around the call time the launch alone, and the host clock
    the enqueue.  Under `rocprofv3 --kernel-trace --stats` the two list sizes are told apart by their instantiation: the 64 gids sum
    the velocity (k_track_accumulate<1>), the 65536 the force (<0>); both read three double arrays on a hit."""
    s = ddcmd_amd.make_water_setup(int(lattice))
    m = MartiniHIP(s)
    m.eval_forces()
    m.step(20)
    m.sync()
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    rng = np.random.RandomState(2)
    print("FORCE_AVERAGE: %d beads" % s.natoms, flush=True)
    med, lo, host = timed(m, m.momentum_by_class, e0, e1)
    print("  %-32s %8.4f ms by events (min %.4f; host clock %.4f ms)" % ("ddcmi_momentum_by_class", med, lo, host), flush=True)
    for nid, what in ((64, "velocity"), (65536, "force")):
        m.track_set(np.asarray(s.gid, np.uint64)[rng.permutation(s.natoms)[:nid]])
        med, lo, host = timed(m, lambda: m.track_accumulate(what), e0, e1)
        tot, hits = m.track_read(reset=True)
        assert hits.min() == hits.max() == 23      # 3 warm-up calls and 20 timed ones found every gid
        print("  %-32s %8.4f ms by events (min %.4f; host clock %.4f ms)  %.4f GB of gids read, %.2f TB/s"
              % ("track_accumulate %d gids %s" % (nid, what), med, lo, host, 8 * s.natoms / 1e9, 8 * s.natoms / (1e-3 * med) / 1e12), flush=True)
    m.close()


for spec in (sys.argv[1:] or ["water:102", "lipid:12,12,6", "chol:63", "track:64"]):
    if spec.startswith("track:"):
        track_rows(spec.split(":")[1])
        continue
    if spec.startswith("chol:"):
        chol_rows(spec.split(":")[1])
        continue
    s, name = system(spec)
    m = MartiniHIP(s)
    m.eval_forces()
    m.group_temperatures()
    m.step(50)
    m.sync()
    t0 = time.perf_counter()
    m.step(200)
    m.sync()
    step_ms = 1e3 * (time.perf_counter() - t0) / 200
    m.vaf_origin()
    m.step(10)
    e0, e1 = vp(), vp()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    smear = ddcmd_amd.units_convert(1.0, "Angstrom", None)
    # KINETICENERGYDISTN: 0 to 6 kT at 310 K (the bulk of a Maxwell-Boltzmann distribution); the most populous species alone in 100
    # bins and in the largest histogram one group may have, and every species in a group of its own with 100 bins each
    kd_lo, kd_hi = np.zeros(s.nspecies), np.full(s.nspecies, 6 * 310.0 * ddcmd_amd.units_convert(1.0, "K", None))
    kd_one = np.full(s.nspecies, -1, np.int32)
    kd_one[np.argmax(np.bincount(s.species, minlength=s.nspecies))] = 0
    rows = [("ddcmi_vaf_sample", 32 + 24 + 48 + 8, m.vaf_sample),
            ("ddcmi_momentum_by_class", 24 + 8, m.momentum_by_class),
            ("ddcmi_zdensity nz=300", 32, lambda: m.zdensity(300)),
            ("ddcmi_zdensity nz=300 hat 1 A", 32, lambda: m.zdensity(300, smear, "hat")),
            ("ddcmi_zdensity nz=2048", 32, lambda: m.zdensity(2048)),
            ("kinetic_energy_distn 100 bins", 24 + 4, lambda: m.kinetic_energy_distn(kd_lo[:1], kd_hi[:1], [100], kd_one)),
            ("kinetic_energy_distn all x 100", 24 + 4, lambda: m.kinetic_energy_distn(kd_lo, kd_hi, [100] * s.nspecies, np.arange(s.nspecies))),
            ("kinetic_energy_distn 16357 bins", 24 + 4, lambda: m.kinetic_energy_distn(kd_lo[:1], kd_hi[:1], [16357], kd_one)),
            ("charge_density_modes mmax=8", 32 + 4, lambda: m.charge_density_modes(8)),      # one chunk of modes: one pass over the positions
            ("charge_density_modes mmax=64", 8 * (32 + 4), lambda: m.charge_density_modes(64)),
            # the record-writing passes (count, scan, pack; two waits): every 16th gid's record; every bead's (the copy of 24 B each in the time);
            # a 32^3 grid one cell per bead, and smeared over eight (a sort of eight contributions per bead)
            ("subset_records modulus 16", 2 * (32 + 24 + 8 + 4), lambda: m.subset_records(modulus=16)),
            ("subset_records all", 2 * (32 + 24 + 8 + 4), lambda: m.subset_records()),
            ("coarsegrain 32^3", 32 + 24 + 4, lambda: m.coarsegrain(32, 32, 32)),
            ("coarsegrain 32^3 hat 1 A", 32 + 24 + 4, lambda: m.coarsegrain(32, 32, 32, smear, "hat"))]
    print("%s: %d beads, %d groups, %d species; one plain step %.4f ms" % (name, s.natoms, max(1, s.ngroup), s.nspecies, step_ms), flush=True)
    for label, bpb, call in rows:
        med, lo, host = timed(m, call, e0, e1)
        nbytes = s.natoms * bpb
        print("  %-32s %8.4f ms by events (min %.4f; host clock %.4f ms)  %.3f GB read, %.2f TB/s = %.0f %% of 8 TB/s"
              % (label, med, lo, host, nbytes / 1e9, nbytes / (1e-3 * med) / 1e12, 100 * nbytes / (1e-3 * med) / 8e12), flush=True)
    # structure_modes is bound by arithmetic, not by bytes: one sincospi per selected bead and wave vector.  The roof is the FP64 vector
    # issue rate, 256 CUs x 64 lanes x 2.4 GHz = 39.3e12 lane-instructions / s (78.6 TFLOP/s counts an FMA twice); one evaluation costs
    # SM_FP64 FP64 instructions in k_structure_modes' inner loop (counted in the gfx950 code: the phase 3, its reduction 3, sincospi 26,
    # the two sums 2) beside about as many 32-bit selects
    SM_FP64, ROOF = 34, 256 * 64 * 2.4e9
    quad = expand_signs(in_plane(16))      # 4 x 288 wave vectors: every in-plane vector up to n = 16 in its four sign combinations
    big = int(np.argmax(np.bincount(s.species, minlength=s.nspecies)))
    one = np.zeros(s.nspecies, np.int32)
    one[big] = 1
    sm_rows = [("structure_modes %s nk=%d" % (s.species_name[big], len(quad)), int((s.species == big).sum()), len(quad), lambda: m.structure_modes(quad, select=one)),
               ("structure_modes all nk=1024", s.natoms, 1024, lambda: m.structure_modes(quad[:1024])),
               ("structure_modes all nk=64", s.natoms, 64, lambda: m.structure_modes(quad[:64]))]
    for label, nsel, nk, call in sm_rows:
        med, lo, host = timed(m, call, e0, e1)
        rate = nsel * nk / (1e-3 * med)
        print("  %-32s %8.4f ms by events (min %.4f; host clock %.4f ms)  %d beads x %d vectors: %.3g sincospi/s = %.0f %% of the FP64 vector roof"
              % (label, med, lo, host, nsel, nk, rate, 100 * rate * SM_FP64 / ROOF), flush=True)
    m.close()

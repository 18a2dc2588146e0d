"""Python driver of the C-ABI (include/ddcmi.h) used by tests and bench.py.

Mirrors the call order of ddcMD's own plugin glue: accelerator_init ->
martini_parms (set_* calls) -> sendGPUState (upload) -> firstEnergyCall
(eval_forces) -> eval_integrator (step_nglf).  No computation happens in Python.
"""
import ctypes
import numpy as np
from . import _lib

E_NAMES = ("lj", "ele", "bond", "angle", "tors", "impr", "total", "restraint")
POS, VEL, FORCE = 1, 2, 4
_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_up = ctypes.POINTER(ctypes.c_uint64)
_lp = ctypes.POINTER(ctypes.c_int64)
_MOLRES = np.uint64(0xFFFFFFFFFFFF0000)


class DdcmiError(RuntimeError):
    pass


def _d(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _i(a):
    return a.ctypes.data_as(_ip) if a is not None else None


def _smear_method(m):
    """zdensity's smearMethod as ddcmi_zdensity takes it: an int as it is, "hat" in any case 1, every other word 0 (zdensity.c:45-48)"""
    return int(m) if isinstance(m, (int, np.integer)) else int(str(m).lower() == "hat")


def _kdist_args(nspecies, emin, emax, nbins, species_dist, nrank=1):
    """the arrays ddcmi_kinetic_energy_distn takes and fills: (emin, emax, nbins, species_dist, counts, tallies, stats), nrank blocks"""
    emin, emax = np.ascontiguousarray(emin, np.float64).reshape(-1), np.ascontiguousarray(emax, np.float64).reshape(-1)
    nbins, sd = np.ascontiguousarray(nbins, np.int32).reshape(-1), np.ascontiguousarray(species_dist, np.int32).reshape(-1)
    if not (len(emin) == len(emax) == len(nbins)) or len(sd) != int(nspecies):
        raise ValueError("kinetic_energy_distn: %d emin, %d emax, %d nbins; %d entries of species_dist for %d species"
                         % (len(emin), len(emax), len(nbins), len(sd), nspecies))
    nd, nbt = len(nbins), int(np.maximum(nbins, 0).astype(np.int64).sum())
    return (emin, emax, nbins, sd, np.zeros((nrank, nbt), np.int64), np.zeros((nrank, max(nd, 1), 3), np.int64)[:, :nd],
            np.zeros((nrank, max(nd, 1), 3))[:, :nd])


def _dsf_args(nspecies, mmax, select, nrank=1):
    """the arrays ddcmi_charge_density_modes takes and fills: (select or None, rho[nrank, 3, mmax, 2], count[nrank])"""
    sel = None
    if select is not None:
        sel = np.ascontiguousarray(np.asarray(select) != 0, np.int32).reshape(-1)
        if len(sel) != int(nspecies):
            raise ValueError("charge_density_modes: %d entries of select for %d species" % (len(sel), nspecies))
    return sel, np.zeros((nrank, 3, max(int(mmax), 1), 2)), np.zeros(nrank, np.int64)


SM_WEIGHTS = {"unit": 0, "charge": 1}


def _sm_args(nspecies, kvec, select, weight, nrank=1):
    """the arrays ddcmi_structure_modes takes and fills: (select or None, weight 0 / 1, kvec int32 [nk, 3], rho[nrank, nk, 2], count[nrank])"""
    sel = None
    if select is not None:
        sel = np.ascontiguousarray(np.asarray(select) != 0, np.int32).reshape(-1)
        if len(sel) != int(nspecies):
            raise ValueError("structure_modes: %d entries of select for %d species" % (len(sel), nspecies))
    if weight not in SM_WEIGHTS:
        raise ValueError("structure_modes: weight %r, one of %s" % (weight, sorted(SM_WEIGHTS)))
    kv = np.asarray(kvec)
    if kv.size % 3 or (kv.size and not np.issubdtype(kv.dtype, np.integer)) or (kv.size and np.abs(kv.astype(np.int64)).max() >= 2 ** 31):
        raise ValueError("structure_modes: kvec must be integer triples (shape %s, dtype %s)" % (kv.shape, kv.dtype))
    kv = np.ascontiguousarray(kv.reshape(-1, 3), np.int32)
    return sel, SM_WEIGHTS[weight], kv, np.zeros((nrank, max(len(kv), 1), 2)), np.zeros(nrank, np.int64)


SUBSET_RECORD = np.dtype([("id", "<u8"), ("pinfo", "<u4"), ("r", "<f4", (3,))])      # struct ddcmi_subset_record: 24 bytes, the file's record
CG_RECORD = np.dtype([("label", "<i8"), ("species", "<i4"), ("pad", "<i4"), ("n", "<f8"), ("mass", "<f8"), ("K", "<f8", (3,)), ("p", "<f8", (3,))])      # struct ddcmi_cg_record: 80 bytes
CHOL_FRAGMENT = np.dtype([("mol", "<i4"), ("role", "<i4"), ("r", "<f8", (3,))])      # struct ddcmi_chol_fragment: 32 bytes
GID_MAX = 2 ** 64 - 1


def _chol_args(gid7, nbins, nrank=1):
    """the arrays ddcmi_chol_offsets takes and fills: (gid[7 nmol], counts[nrank, 2 nbins], ndone[nrank], stats[nrank, 6], nfrag[nrank])"""
    gid = np.ascontiguousarray(gid7, np.uint64).reshape(-1)
    if gid.size % 7:
        raise ValueError("chol_offsets: %d gids, not seven per molecule" % gid.size)
    return (np.ascontiguousarray(np.concatenate([gid, np.zeros(1, np.uint64)])), np.zeros((nrank, 2 * max(int(nbins), 1)), np.int64), np.zeros(nrank, np.int64),
            np.zeros((nrank, 6)), np.zeros(nrank, np.int64))


def chol_merge(lib, setup, gid7, rmin, delta, nbins, counts, ndone, stats, frags):
    """the ranks' results of ddcmi_chol_offsets merged as its contract says -- counts and ndone added, the sums added in rank order,
    minimum of the minima, maximum of the maxima -- and the split molecules completed on the host from the fragments, concatenated in
    rank order, in ascending molecule order (ddcmi_chol_complete).  Returns (counts[2 nbins], stats[6], n)."""
    gid = np.ascontiguousarray(gid7, np.uint64).reshape(-1)
    nmol = gid.size // 7
    c = np.ascontiguousarray(np.asarray(counts, np.int64).reshape(-1, 2 * int(nbins)).sum(axis=0))
    st = np.asarray(stats, np.float64).reshape(-1, 6)
    tot = st[0].copy()
    for r in range(1, len(st)):
        tot[0::3] += st[r, 0::3]
        tot[1::3] = np.minimum(tot[1::3], st[r, 1::3])
        tot[2::3] = np.maximum(tot[2::3], st[r, 2::3])
    tot = np.ascontiguousarray(tot)
    n = np.array([int(np.sum(ndone))], np.int64)
    fr = np.ascontiguousarray(np.concatenate([np.asarray(f, CHOL_FRAGMENT).reshape(-1) for f in frags]) if len(frags) else np.zeros(0, CHOL_FRAGMENT))
    if len(fr):
        box = np.ascontiguousarray(np.asarray(setup.h, np.float64).reshape(-1)[[0, 4, 8]])
        err = ctypes.create_string_buffer(512)
        rc = lib.ddcmi_chol_complete(len(fr), fr.ctypes.data_as(ctypes.c_void_p), nmol, gid.ctypes.data_as(_up), _d(box), int(getattr(setup, "pbc", 7)),
                                     float(rmin), float(delta), int(nbins), c.ctypes.data_as(_lp), n.ctypes.data_as(_lp), _d(tot), err, 512)
        if rc != 0:
            raise DdcmiError(err.value.decode())
    return c, tot, int(n[0])


def chol_molecule(lib, r7, box, pbc, rmin, delta, nbins):
    """(dR1, dR5, bin1, bin5) of one molecule's seven positions r7[7, 3] with the device lane's operations on the host (ddcmi_chol_molecule)"""
    r = np.ascontiguousarray(r7, np.float64).reshape(21)
    L = np.ascontiguousarray(box, np.float64).reshape(3)
    d, b = np.zeros(2), np.zeros(2, np.int32)
    lib.ddcmi_chol_molecule(_d(r), _d(L), int(pbc), float(rmin), float(delta), int(nbins), _d(d), _i(b))
    return float(d[0]), float(d[1]), int(b[0]), int(b[1])


def chol_molecules(setup):
    """gid7[nmol, 7] of a Setup's CHOL molecules: the residue runs in gid order, cut where gid & molResMask changes as the bonded
    terms cut them (expand_bonded_terms); a run is a CHOL residue when its first bead's species has the residue name CHOL (the
    species name up to the first of 'c', 'n', 'x'); roles 0..6 are its first seven beads, an eighth is unused"""
    import re
    order = np.argsort(setup.gid, kind="stable")
    g = np.asarray(setup.gid, np.uint64)[order]
    key = g & _MOLRES
    first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1]))) if len(g) else np.zeros(0, np.int64)
    cnt = np.diff(np.concatenate((first, [len(g)])))
    is_chol = np.array([re.split("[cnx]", nm, 1)[0] == "CHOL" for nm in setup.species_name], bool)
    out = []
    for f, c in zip(first, cnt):
        if not is_chol[setup.species[order[f]]]:
            continue
        if c < 7:
            raise DdcmiError("CHOL residue at gid %d has %d beads, cholAnalysis needs seven" % (int(g[f]), int(c)))
        out.append(g[f:f + 7])
    return np.array(out, np.uint64).reshape(-1, 7)


class CSubsetFilter(ctypes.Structure):
    """Mirror of struct ddcmi_subset_filter (include/ddcmi.h)."""
    _fields_ = [("idmin", ctypes.c_uint64), ("idmax", ctypes.c_uint64), ("modulus", ctypes.c_int), ("odd", ctypes.c_int),
                ("rmin", ctypes.c_double * 3), ("rmax", ctypes.c_double * 3), ("vmin", ctypes.c_double * 3), ("vmax", ctypes.c_double * 3),
                ("nspecies", ctypes.c_int), ("ngroup", ctypes.c_int), ("include_species", _ip),
                ("group_term", ctypes.POINTER(ctypes.c_uint32)), ("species_term", ctypes.POINTER(ctypes.c_uint32)),
                ("nid", ctypes.c_int64), ("idlist", _up), ("corner", ctypes.c_double * 3), ("cL", ctypes.c_double)]


def _subset_filter(setup, idmin=0, idmax=GID_MAX, modulus=1, odd=False, rmin=None, rmax=None, vmin=None, vmax=None, species=None, id_list=None,
                   group_term=None, species_term=None, corner=None, cL=1.0):
    """(struct ddcmi_subset_filter, the arrays it points into) of ddcmi_subset_records.  Bounds in internal units, None: -+ inf; species:
    one flag per species, None: all; id_list: ascending gids, None: no list; the two pinfo tables default to {group index} and {species
    index * number of groups}; corner defaults to the box's (-L/2)."""
    ns, ng = int(setup.nspecies), max(1, int(setup.ngroup))
    inf = float("inf")
    keep = {"include": None if species is None else np.ascontiguousarray(np.asarray(species) != 0, np.int32).reshape(-1),
            "gterm": np.ascontiguousarray(np.arange(ng) if group_term is None else group_term, np.uint32).reshape(-1),
            "sterm": np.ascontiguousarray(np.arange(ns) * ng if species_term is None else species_term, np.uint32).reshape(-1),
            "ids": None if id_list is None else np.ascontiguousarray(np.concatenate([np.asarray(id_list, np.uint64).reshape(-1), np.zeros(1, np.uint64)]))}
    if keep["include"] is not None and len(keep["include"]) != ns:
        raise ValueError("subset_records: %d entries of species for %d species" % (len(keep["include"]), ns))
    f = CSubsetFilter()
    f.idmin, f.idmax, f.modulus, f.odd = int(idmin), int(idmax), int(modulus), int(bool(odd))
    for k, (lo, hi) in enumerate(((rmin, rmax), (vmin, vmax))):
        for a in range(3):
            (f.rmin, f.vmin)[k][a] = -inf if lo is None else float(lo[a])
            (f.rmax, f.vmax)[k][a] = inf if hi is None else float(hi[a])
    f.nspecies, f.ngroup = len(keep["sterm"]), len(keep["gterm"])
    f.include_species = _i(keep["include"])
    f.group_term = keep["gterm"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    f.species_term = keep["sterm"].ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    f.nid = 0 if keep["ids"] is None else len(keep["ids"]) - 1      # (one spare entry: a list without a member still has an address)
    f.idlist = None if keep["ids"] is None else keep["ids"].ctypes.data_as(_up)
    box = np.asarray(setup.h, np.float64).reshape(-1)[[0, 4, 8]]
    for a in range(3):
        f.corner[a] = -0.5 * box[a] if corner is None else float(corner[a])
    f.cL = float(cL)
    return f, keep


def _declare(lib):
    if getattr(lib, "_ddcmi_declared", False):
        return
    vp = ctypes.c_void_p
    lib.ddcmi_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.ddcmi_destroy.argtypes = [vp]
    lib.ddcmi_destroy.restype = None
    lib.ddcmi_last_error.argtypes = [vp]
    lib.ddcmi_last_error.restype = ctypes.c_char_p
    lib.ddcmi_version.restype = ctypes.c_char_p
    lib.ddcmi_set_box.argtypes = [vp, _dp, ctypes.c_int]
    lib.ddcmi_set_species.argtypes = [vp, ctypes.c_int, _dp, _dp, _ip, _ip]
    lib.ddcmi_set_nonbonded.argtypes = [vp, ctypes.c_int, _dp, _dp, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    lib.ddcmi_set_molecules.argtypes = [vp, ctypes.c_int, _ip, _ip, _ip, _ip]
    lib.ddcmi_set_bonded.argtypes = [vp, ctypes.c_int, _ip, _dp, _dp, ctypes.c_int, _ip, _ip, _dp, _dp,
                                     ctypes.c_int, _ip, _ip, _ip, _dp, _dp, ctypes.c_int]
    lib.ddcmi_set_bonded_gid.argtypes = [vp, ctypes.c_int, _up, _dp, _dp, ctypes.c_int, _up, _ip, _dp, _dp,
                                         ctypes.c_int, _up, _ip, _ip, _dp, _dp, ctypes.c_int]
    lib.ddcmi_set_neighbor.argtypes = [vp, ctypes.c_double, ctypes.c_int]
    lib.ddcmi_set_groups.argtypes = [vp, ctypes.c_int, _ip, _dp, _dp, _ip]
    lib.ddcmi_set_group_vcm.argtypes = [vp, ctypes.c_int, _dp]
    lib.ddcmi_set_group_velocity.argtypes = [vp, ctypes.c_int, _ip, _dp]
    lib.ddcmi_set_group_temperature.argtypes = [vp, ctypes.c_int, ctypes.c_double]
    lib.ddcmi_set_clock.argtypes = [vp, ctypes.c_int64, ctypes.c_double]
    lib.ddcmi_set_random.argtypes = [vp, ctypes.c_uint64]
    lib.ddcmi_set_barostat.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double]
    lib.ddcmi_get_box.argtypes = [vp, _dp]
    lib.ddcmi_get_barostat_pressure.argtypes = [vp, _dp]
    lib.ddcmi_set_barostat_isotropic.argtypes = [vp, ctypes.c_int]
    lib.ddcmi_set_molecule_lists.argtypes = [vp, ctypes.c_long, ctypes.c_int, _ip, _ip]
    lib.ddcmi_set_constraints.argtypes = [vp, ctypes.c_int, _ip, _ip, _ip, _dp]
    lib.ddcmi_set_constraints_gid.argtypes = [vp, ctypes.c_int, _ip, _up, _up, _dp]
    lib.ddcmi_set_molecule_lists_gid.argtypes = [vp, ctypes.c_long, ctypes.c_int, _ip, _up, _dp]
    lib.ddcmi_constraint_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.ddcmi_set_restraints.argtypes = [vp, ctypes.c_int, _up, _ip, _dp, _dp, ctypes.c_int]
    lib.ddcmi_get_clock.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), _dp]
    lib.ddcmi_upload_state.argtypes = [vp, ctypes.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _up, _ip, _ip]
    lib.ddcmi_download_state.argtypes = [vp, ctypes.c_int] + [_dp] * 9
    lib.ddcmi_nlocal.argtypes = [vp]
    lib.ddcmi_build_list.argtypes = [vp]
    lib.ddcmi_eval_forces.argtypes = [vp, _dp, _dp]
    lib.ddcmi_step_nglf.argtypes = [vp, ctypes.c_double, ctypes.c_int]
    lib.ddcmi_get_energies.argtypes = [vp, _dp, _dp, _dp, _dp]
    lib.ddcmi_kinetic.argtypes = [vp, _dp, _dp]
    lib.ddcmi_group_temperatures.argtypes = [vp, _dp]
    lib.ddcmi_sync.argtypes = [vp]
    lib.ddcmi_list_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64)]
    lib.ddcmi_get_list.argtypes = [vp, ctypes.c_int, _ip, _ip, ctypes.POINTER(ctypes.c_int64)]
    lib.ddcmi_timing_enable.argtypes = [vp, ctypes.c_int]
    lib.ddcmi_timing_read.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), _dp, ctypes.c_int]
    lib.ddcmi_stream.argtypes = [vp]
    lib.ddcmi_stream.restype = vp
    lib.ddcmi_comm_unique_id.argtypes = [ctypes.c_char_p]
    lib.ddcmi_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.ddcmi_comm_allreduce_sum.argtypes = [vp, _dp, ctypes.c_int]
    lib.ddcmi_comm_init_host.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    # process rendezvous (host/rdzv.c)
    szt = ctypes.c_size_t
    lib.ddcmi_rdzv_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double]
    lib.ddcmi_rdzv_destroy.argtypes = [vp]
    lib.ddcmi_rdzv_destroy.restype = None
    lib.ddcmi_rdzv_last_error.argtypes = [vp]
    lib.ddcmi_rdzv_last_error.restype = ctypes.c_char_p
    lib.ddcmi_rdzv_rank.argtypes = [vp]
    lib.ddcmi_rdzv_world.argtypes = [vp]
    lib.ddcmi_rdzv_bcast.argtypes = [vp, vp, szt, ctypes.c_int]
    lib.ddcmi_rdzv_barrier.argtypes = [vp]
    lib.ddcmi_rdzv_allreduce_f64.argtypes = [vp, _dp, ctypes.c_int, ctypes.c_int]
    lib.ddcmi_rdzv_allgather.argtypes = [vp, vp, vp, szt]
    lib.ddcmi_rdzv_exchange.argtypes = [vp, ctypes.c_int, _ip, ctypes.POINTER(vp), ctypes.POINTER(szt), ctypes.c_int, _ip, ctypes.POINTER(vp), ctypes.POINTER(szt)]
    lib.ddcmi_domain_bounds.argtypes = [vp, _dp, _dp]
    lib.ddcmi_download_particles.argtypes = [vp, ctypes.c_int, _ip, _up, _ip] + [_dp] * 9
    lib.ddcmi_pair_correlation.argtypes = [vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, _lp, _lp]
    lib.ddcmi_vaf_origin.argtypes = [vp]
    lib.ddcmi_vaf_sample.argtypes = [vp, ctypes.c_int, ctypes.c_int, _dp, _dp]
    lib.ddcmi_vaf_clear.argtypes = [vp]
    lib.ddcmi_momentum_by_class.argtypes = [vp, ctypes.c_int, ctypes.c_int, _dp, _dp]
    lib.ddcmi_zdensity.argtypes = [vp, ctypes.c_int, ctypes.c_double, ctypes.c_int, _dp]
    lib.ddcmi_kinetic_energy_distn.argtypes = [vp, ctypes.c_int, ctypes.c_int, _dp, _dp, _ip, _ip, _lp, _lp, _dp]
    lib.ddcmi_charge_density_modes.argtypes = [vp, ctypes.c_int, _ip, ctypes.c_int, _dp, _lp]
    lib.ddcmi_structure_modes.argtypes = [vp, ctypes.c_int, _ip, ctypes.c_int, ctypes.c_int, _ip, _dp, _lp]
    lib.ddcmi_subset_records.argtypes = [vp, ctypes.POINTER(CSubsetFilter), ctypes.c_int64, vp, _lp]
    lib.ddcmi_coarsegrain.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int64, vp, _lp]
    lib.ddcmi_thermalize.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int]
    lib.ddcmi_chol_offsets.argtypes = [vp, ctypes.c_int64, _up, ctypes.c_double, ctypes.c_double, ctypes.c_int, _lp, _lp, _dp, ctypes.c_int64, vp, _lp]
    lib.ddcmi_chol_fragments.argtypes = [vp, ctypes.c_int64, vp, _lp]
    lib.ddcmi_chol_complete.argtypes = [ctypes.c_int64, vp, ctypes.c_int64, _up, _dp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _lp, _lp, _dp,
                                        ctypes.c_char_p, ctypes.c_size_t]
    lib.ddcmi_chol_molecule.argtypes = [_dp, _dp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, _dp, _ip]
    lib.ddcmi_chol_molecule.restype = None
    lib.ddcmi_track_set.argtypes = [vp, ctypes.c_int64, _up]
    lib.ddcmi_track_accumulate.argtypes = [vp, ctypes.c_int]
    lib.ddcmi_track_read.argtypes = [vp, ctypes.c_int64, _dp, _lp, ctypes.c_int]
    lib._ddcmi_declared = True


TRACK_WHAT = {"force": 0, "velocity": 1, "position": 2}      # ddcmi_track_accumulate
THERMALIZE_METHODS = {"BOLTZMANN": 0, "RESCALE": 1, "JUTTNER": 2}
THERMALIZE_SELECTS = {"global": 0, "species": 1, "group": 2}


def _thermalize_args(setup, method, temperature, select):
    """(method, select, temperature array) of ddcmi_thermalize: names or the numbers themselves; the temperatures in internal energy units
    (kB = 1), one for "global", one per species / group otherwise (< 0: that class is left alone)"""
    m = THERMALIZE_METHODS[method.upper()] if isinstance(method, str) else int(method)
    sel = THERMALIZE_SELECTS[select.lower()] if isinstance(select, str) else int(select)
    t = np.ascontiguousarray(np.atleast_1d(temperature), dtype=np.float64)
    return m, sel, t


def default_port_file():
    """Where rank 0 publishes its port when the launcher keeps MASTER_PORT for itself
    (torch.distributed.run's store listens there): one name per launch -- all workers of a
    launch share the launcher as parent."""
    import os
    import tempfile
    key = "%s_%s_%s_%d" % (os.environ.get("MASTER_ADDR", "127.0.0.1"), os.environ.get("MASTER_PORT", "0"),
                           os.environ.get("TORCHELASTIC_RUN_ID", "none"), os.getppid())
    return os.environ.get("DDCMI_RDZV_FILE") or os.path.join(tempfile.gettempdir(), "ddcmi_rdzv_" + key.replace("/", "_"))


class Rendezvous(object):
    """Ranks of one launch meeting over TCP (host/rdzv.c): what ddcMD takes from MPI
    (rank/size, Bcast, Barrier, Allreduce) for launches that only provide
    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT.  No torch, no MPI."""

    def __init__(self, rank, world, addr="127.0.0.1", port=0, port_file=None, timeout=300.0):
        self.lib = _lib.load_library()
        _declare(self.lib)
        self.h = ctypes.c_void_p()
        pf = port_file.encode() if port_file else None
        rc = self.lib.ddcmi_rdzv_create(ctypes.byref(self.h), int(rank), int(world), addr.encode(), int(port), pf, float(timeout))
        if rc != 0:
            raise DdcmiError("ddcmi_rdzv_create failed (%d): %s" % (rc, self.lib.ddcmi_rdzv_last_error(None).decode()))
        self.rank, self.world = int(rank), int(world)

    @classmethod
    def from_env(cls, timeout=300.0):
        """RANK / WORLD_SIZE / MASTER_ADDR from the environment; the port through a file in the temporary
        directory (MASTER_PORT itself belongs to the launcher) unless DDCMI_RDZV_PORT names a free one"""
        import os
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        addr = os.environ.get("MASTER_ADDR", "127.0.0.1")
        port = int(os.environ.get("DDCMI_RDZV_PORT", "0"))
        return cls(rank, world, addr, port, None if port > 0 else default_port_file(), timeout)

    def _chk(self, rc):
        if rc != 0:
            raise DdcmiError("rendezvous error %d: %s" % (rc, self.lib.ddcmi_rdzv_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.lib.ddcmi_rdzv_destroy(self.h)
            self.h = ctypes.c_void_p()

    def bcast(self, data, root=0):
        """bytes in (significant on root), bytes out; the length must agree on all ranks"""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        self._chk(self.lib.ddcmi_rdzv_bcast(self.h, ctypes.cast(buf, ctypes.c_void_p), len(data), int(root)))
        return buf.raw

    def barrier(self):
        self._chk(self.lib.ddcmi_rdzv_barrier(self.h))

    def allreduce(self, values, op="sum"):
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        self._chk(self.lib.ddcmi_rdzv_allreduce_f64(self.h, _d(v), v.size, 0 if op == "sum" else 1))
        return v

    def allgather(self, arr):
        a = np.ascontiguousarray(arr)
        out = np.zeros((self.world,) + a.shape, a.dtype)
        self._chk(self.lib.ddcmi_rdzv_allgather(self.h, a.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), a.nbytes))
        return out

    def exchange(self, sends, recvs):
        """sends: [(peer, ndarray)], recvs: [(peer, ndarray to fill)]; matched per peer in order"""
        vp, szt = ctypes.c_void_p, ctypes.c_size_t
        sends = [(p, np.ascontiguousarray(a)) for p, a in sends]
        ns, nr = len(sends), len(recvs)
        sp = (ctypes.c_int * max(ns, 1))(*[p for p, _ in sends])
        sb = (vp * max(ns, 1))(*[a.ctypes.data for _, a in sends])
        sz = (szt * max(ns, 1))(*[a.nbytes for _, a in sends])
        rp = (ctypes.c_int * max(nr, 1))(*[p for p, _ in recvs])
        rb = (vp * max(nr, 1))(*[a.ctypes.data for _, a in recvs])
        rz = (szt * max(nr, 1))(*[a.nbytes for _, a in recvs])
        self._chk(self.lib.ddcmi_rdzv_exchange(self.h, ns, sp, sb, sz, nr, rp, rb, rz))


def plan_recv_counts(grid, rank, pbc, all_counts, loopback=False):
    """recv_cnt[27] from the all-gathered send counts [nranks, 27] (host logic of libddcmi; test API: libddcmi_test.so)"""
    lib = _lib.load_test_library()
    _declare(lib)
    _declare_domains(lib)
    ac = np.ascontiguousarray(all_counts, dtype=np.int32)
    out = np.zeros(27, np.int32)
    rc = lib.ddcmi_plan_recv_counts(grid[0], grid[1], grid[2], int(rank), int(pbc), int(loopback), _i(ac), _i(out))
    if rc != 0:
        raise DdcmiError("ddcmi_plan_recv_counts failed: %d" % rc)
    return out


def plan_halo_layout(grid, rank, pbc, send_cnt, recv_cnt, loopback=False):
    """(send_off[28], recv_off[28], send messages [(peer, off, cnt)], receive messages) of the per-step halo
    exchange: libddcmi's own peer-major layout (ddcmi_multigpu.inl plan_halo_layout; test API: libddcmi_test.so)"""
    lib = _lib.load_test_library()
    _declare(lib)
    _declare_domains(lib)
    sc, rcn = np.ascontiguousarray(send_cnt, dtype=np.int32), np.ascontiguousarray(recv_cnt, dtype=np.int32)
    so, ro = np.zeros(28, np.int32), np.zeros(28, np.int32)
    ms, mr = np.zeros(1 + 3 * 27, np.int32), np.zeros(1 + 3 * 27, np.int32)
    rc = lib.ddcmi_plan_halo_layout(grid[0], grid[1], grid[2], int(rank), int(pbc), int(loopback), _i(sc), _i(rcn), _i(so), _i(ro), _i(ms), _i(mr))
    if rc != 0:
        raise DdcmiError("ddcmi_plan_halo_layout failed: %d" % rc)
    unpack = lambda m: [tuple(int(x) for x in m[1 + 3 * k:4 + 3 * k]) for k in range(int(m[0]))]
    return so, ro, unpack(ms), unpack(mr)


def expand_bonded_terms(s):
    """Residue-relative bonded tables -> term lists over caller-order atom indices.

    Follows charmmResidues (bioCharmmCovalent.c:48-93): sort atoms by gid, cut
    residue runs at changes of gid & molResMask; term atoms are offsets into the run.
    """
    n = s.natoms
    empty_i = np.zeros(0, np.int32)
    out = {"bond_ij": empty_i, "bond_kb": np.zeros(0), "bond_b0": np.zeros(0),
           "angle_ijk": empty_i, "angle_func": empty_i, "angle_k": np.zeros(0), "angle_t0": np.zeros(0),
           "tors_ijkl": empty_i, "tors_func": empty_i, "tors_n": empty_i, "tors_k": np.zeros(0), "tors_delta": np.zeros(0)}
    if s.nresi == 0 or (s.bond_off[-1] == 0 and s.angle_off[-1] == 0 and s.tors_off[-1] == 0):
        return out
    order = np.argsort(s.gid, kind="stable")
    key = s.gid[order] & _MOLRES
    first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    cnt = np.diff(np.concatenate((first, [n])))
    rt = s.resitype[s.species[order[first]]]
    if np.any(cnt != s.resi_natoms[rt]):
        raise DdcmiError("incomplete residue in the particle set")
    bi, bk, b0 = [], [], []
    ai, af, ak, a0 = [], [], [], []
    ti, tf, tn, tk, td = [], [], [], [], []
    for r in range(s.nresi):
        starts = first[rt == r]
        if starts.size == 0:
            continue
        b = slice(s.bond_off[r], s.bond_off[r + 1])
        if b.stop > b.start:
            I = order[starts[:, None] + s.bondI[b][None, :]]
            J = order[starts[:, None] + s.bondJ[b][None, :]]
            bi.append(np.stack((I, J), axis=-1).reshape(-1, 2))
            bk.append(np.tile(s.bond_kb[b], starts.size))
            b0.append(np.tile(s.bond_b0[b], starts.size))
        a = slice(s.angle_off[r], s.angle_off[r + 1])
        if a.stop > a.start:
            idx = [order[starts[:, None] + getattr(s, k)[a][None, :]] for k in ("angleI", "angleJ", "angleK")]
            ai.append(np.stack(idx, axis=-1).reshape(-1, 3))
            af.append(np.tile(s.angle_func[a], starts.size))
            ak.append(np.tile(s.angle_k[a], starts.size))
            a0.append(np.tile(s.angle_t0[a], starts.size))
        t = slice(s.tors_off[r], s.tors_off[r + 1])
        if t.stop > t.start:
            idx = [order[starts[:, None] + getattr(s, k)[t][None, :]] for k in ("torsI", "torsJ", "torsK", "torsL")]
            ti.append(np.stack(idx, axis=-1).reshape(-1, 4))
            tf.append(np.tile(s.tors_func[t], starts.size))
            tn.append(np.tile(s.tors_n[t], starts.size))
            tk.append(np.tile(s.tors_k[t], starts.size))
            td.append(np.tile(s.tors_delta[t], starts.size))

    def cat(lst, dt):
        return np.ascontiguousarray(np.concatenate(lst), dtype=dt) if lst else np.zeros(0, dt)

    out.update(bond_ij=cat(bi, np.int32).ravel(), bond_kb=cat(bk, np.float64), bond_b0=cat(b0, np.float64),
               angle_ijk=cat(ai, np.int32).ravel(), angle_func=cat(af, np.int32), angle_k=cat(ak, np.float64), angle_t0=cat(a0, np.float64),
               tors_ijkl=cat(ti, np.int32).ravel(), tors_func=cat(tf, np.int32), tors_n=cat(tn, np.int32),
               tors_k=cat(tk, np.float64), tors_delta=cat(td, np.float64))
    return out


def expand_constraints(s):
    """Residue-relative constraint lists -> constraint groups over caller-order atom indices.

    One group per CONSLISTPARMS of every residue instance (genConstraint, bioMartini.c:300-445),
    pairs in deck order.  Returns (pair_off, pairI, pairJ, dist)."""
    n = s.natoms
    cons_off = np.asarray(getattr(s, "cons_off", np.zeros(1, np.int32)))
    if s.nresi == 0 or cons_off[-1] == 0:
        return np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0)
    order = np.argsort(s.gid, kind="stable")
    key = s.gid[order] & _MOLRES
    first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    cnt = np.diff(np.concatenate((first, [n])))
    rt = s.resitype[s.species[order[first]]]
    if np.any(cnt != s.resi_natoms[rt]):
        raise DdcmiError("incomplete residue in the particle set")
    counts, pi, pj, dd = [], [], [], []
    for r in range(s.nresi):
        starts = first[rt == r]
        if starts.size == 0 or cons_off[r + 1] == cons_off[r]:
            continue
        sl = np.arange(cons_off[r], cons_off[r + 1])
        grp = s.cons_grp[sl]
        for c in dict.fromkeys(grp.tolist()):
            k = sl[grp == c]
            I = order[starts[:, None] + s.consI[k][None, :]]
            J = order[starts[:, None] + s.consJ[k][None, :]]
            pi.append(I.ravel()); pj.append(J.ravel())
            dd.append(np.tile(s.cons_r0[k], starts.size))
            counts.append(np.full(starts.size, k.size, np.int64))
    counts = np.concatenate(counts)
    pair_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    return (pair_off, np.ascontiguousarray(np.concatenate(pi), dtype=np.int32), np.ascontiguousarray(np.concatenate(pj), dtype=np.int32),
            np.ascontiguousarray(np.concatenate(dd), dtype=np.float64))


def molecule_lists(s):
    """Molecules = runs of equal gid & molMask.  Returns (nmol_total, mol_off, mol_atoms) with only the
    molecules of two or more beads listed (caller-order atom indices)."""
    n = s.natoms
    order = np.argsort(s.gid, kind="stable")
    key = np.asarray(s.gid, dtype=np.uint64)[order] >> np.uint64(32)
    first = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    cnt = np.diff(np.concatenate((first, [n])))
    multi = cnt >= 2
    sel = np.repeat(multi, cnt)
    mol_off = np.concatenate(([0], np.cumsum(cnt[multi]))).astype(np.int32)
    return int(first.size), mol_off, np.ascontiguousarray(order[sel], dtype=np.int32)


def integrator_plan(s):
    """What the INTEGRATOR type of a Setup makes of its groups, constraints and barostat -- the driver's integrator_init, from the same
    table of types (deck.c).  Returns a dict: group_type / group_Teq / group_tau / group_interval / group_vcm as the integrator runs them
    (NGLFCONSTRAINTGPU: every group FREE; NGLFCONSTRAINTGPULANGEVIN[LCG64]: every group LANGEVIN with group 0's Teq, tau and vcm;
    NGLFGPULANGEVIN: the same with each group's own vcm), overridden (the groups whose deck type or parameters do not run as written),
    constraints (the type sets up the residues' constraint lists and the Setup has some), isotropic (the barostat's form).  A type that is
    not in the table, or group 0's thermostat asked for where group 0 is not LANGEVIN, raises DdcmiError by name."""
    from . import deck
    rows = {r["name"]: r for r in deck.integrator_types()}
    name = str(getattr(s, "integrator_type", "NGLF"))
    if name not in rows:
        raise DdcmiError("INTEGRATOR type %s is not on this path (%s are)" % (name, ", ".join(rows)))
    row = rows[name]
    ov, ng = row["group_override"], int(s.ngroup)
    gt = np.array(s.group_type, dtype=np.int32)
    Teq, tau = np.array(s.group_Teq, dtype=np.float64), np.array(s.group_tau, dtype=np.float64)
    iv = np.array(s.group_interval, dtype=np.int32)
    vcm = getattr(s, "group_vcm", None)
    vcm = np.zeros((ng, 3)) if vcm is None or np.size(vcm) != 3 * ng else np.array(vcm, dtype=np.float64).reshape(ng, 3)
    written = (gt.copy(), Teq.copy(), tau.copy(), vcm.copy())
    if ov in (deck.GROUPS_LANGEVIN0, deck.GROUPS_LANGEVIN0_OWN_VCM):
        if ng < 1 or int(gt[0]) != deck.GROUP_LANGEVIN:
            raise DdcmiError("%s needs the first GROUP to be of type LANGEVIN" % name)
        gt[:], Teq[:], tau[:], iv[:] = deck.GROUP_LANGEVIN, Teq[0], tau[0], 1
        if ov == deck.GROUPS_LANGEVIN0:
            vcm[:] = vcm[0]
    elif ov == deck.GROUPS_FREE:
        gt[:], iv[:] = deck.GROUP_FREE, 1
    if ov == deck.GROUPS_FREE:
        changed = written[0] != gt
    else:
        changed = (written[0] != gt) | (written[1] != Teq) | (written[2] != tau) | np.any(written[3] != vcm, axis=1)
    iso = bool(getattr(s, "npt_isotropic", 0))      # the loader has applied the row's barostat form (and the `isotropic` key where the row reads it)
    return {"type": name, "group_override": ov, "group_type": gt, "group_Teq": Teq, "group_tau": tau, "group_interval": iv, "group_vcm": vcm.ravel(),
            "overridden": [int(g) for g in np.flatnonzero(changed)],
            "constraints": bool(row["barostat_keys"]) and int(getattr(s, "nresicons", 0)) > 0, "isotropic": iso}


class MartiniHIP(object):
    """One device context running the Martini hot path for a Setup."""

    def __init__(self, setup, device=0, upload=True, bonded_by_gid=False, constraints=None, test_api=False, constraint_groups=None):
        # constraints: None -- as the driver does: the INTEGRATOR types that read the barostat keys set up the residues' constraint lists
        # constraint_groups: (pair_off, pairI, pairJ, dist) over caller-order atom indices, in place of expand_constraints(setup)
        # test_api: the context lives in libddcmi_test.so (same objects + the entry points of include/ddcmi_test.h)
        self.lib = _lib.load_test_library() if test_api else _lib.load_library()
        _declare(self.lib)
        self.s = setup
        self.ctx = ctypes.c_void_p()
        rc = self.lib.ddcmi_create(ctypes.byref(self.ctx), int(device))
        if rc != 0:
            raise DdcmiError("ddcmi_create failed (%d): %s" % (rc, self.lib.ddcmi_last_error(None).decode()))
        s = setup
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        self._chk(self.lib.ddcmi_set_box(self.ctx, _d(f64(s.h)), int(s.pbc)))
        self._chk(self.lib.ddcmi_set_species(self.ctx, s.nspecies, _d(f64(s.mass)), _d(f64(s.charge)), _i(i32(s.ljtype)), _i(i32(s.moltype))))
        self._chk(self.lib.ddcmi_set_nonbonded(self.ctx, s.nlj, _d(f64(s.sigma)), _d(f64(s.eps)), _d(f64(s.shift)),
                                               s.rmax, s.keR, s.krf, s.crf))
        if s.nmoltype > 0:
            bi, bj = i32(s.bpairI), i32(s.bpairJ)
            if bi.size == 0:
                bi = bj = np.zeros(1, np.int32)
            self._chk(self.lib.ddcmi_set_molecules(self.ctx, s.nmoltype, _i(i32(s.mol_nspecies)), _i(i32(s.bpair_off)), _i(bi), _i(bj)))
        else:
            self._chk(self.lib.ddcmi_set_molecules(self.ctx, 0, None, None, None, None))
        t = self.terms = expand_bonded_terms(s)
        nb, na, nt = t["bond_kb"].size, t["angle_k"].size, t["tors_k"].size
        if bonded_by_gid:
            # decomposed runs: every rank holds the global term list, atoms named by gid
            gids = np.asarray(s.gid, dtype=np.uint64)
            g = lambda idx: np.ascontiguousarray(gids[np.asarray(idx, dtype=np.int64)], dtype=np.uint64)
            self._term_gids = (g(t["bond_ij"]), g(t["angle_ijk"]), g(t["tors_ijkl"]))
            u = lambda a: a.ctypes.data_as(_up)
            self._chk(self.lib.ddcmi_set_bonded_gid(self.ctx, nb, u(self._term_gids[0]), _d(t["bond_kb"]), _d(t["bond_b0"]),
                                                    na, u(self._term_gids[1]), _i(t["angle_func"]), _d(t["angle_k"]), _d(t["angle_t0"]),
                                                    nt, u(self._term_gids[2]), _i(t["tors_func"]), _i(t["tors_n"]), _d(t["tors_k"]), _d(t["tors_delta"]),
                                                    int(s.excludePotentialTerm)))
        else:
            self._chk(self.lib.ddcmi_set_bonded(self.ctx, nb, _i(t["bond_ij"]), _d(t["bond_kb"]), _d(t["bond_b0"]),
                                                na, _i(t["angle_ijk"]), _i(t["angle_func"]), _d(t["angle_k"]), _d(t["angle_t0"]),
                                                nt, _i(t["tors_ijkl"]), _i(t["tors_func"]), _i(t["tors_n"]), _d(t["tors_k"]), _d(t["tors_delta"]),
                                                int(s.excludePotentialTerm)))
        self._chk(self.lib.ddcmi_set_neighbor(self.ctx, s.deltaR, int(s.updateRate)))
        plan = self.plan = integrator_plan(s)      # the INTEGRATOR type's row: NGLFCONSTRAINTGPU and the ...LANGEVIN types override the groups
        if constraints is None:
            constraints = plan["constraints"]
        gt = i32(plan["group_type"])      # FREE / BERENDSEN / LANGEVIN / FROZEN / FIXEDVELOCITY / QUENCH: as they are, unless the type overrides them
        if np.any((gt == 3) | (gt == 7)):         # EXTFORCE (7: read by the loader, not built on the device) and any other GROUP type of a deck: never run as FREE
            raise DdcmiError("GROUP %s: its type (EXTFORCE or another) is none of FREE, BERENDSEN, LANGEVIN, FROZEN, FIXEDVELOCITY, QUENCH"
                             % ", ".join(str(s.group_name[g]) if g < len(s.group_name) else str(g) for g in np.flatnonzero((gt == 3) | (gt == 7))))
        self._chk(self.lib.ddcmi_set_groups(self.ctx, s.ngroup, _i(gt), _d(f64(plan["group_Teq"])), _d(f64(plan["group_tau"])), _i(i32(plan["group_interval"]))))
        vcm = plan["group_vcm"] if getattr(s, "group_vcm", None) is not None else None
        if vcm is not None and np.any(np.asarray(vcm) != 0.0):      # LANGEVIN groups: the velocity the friction relaxes towards (langevin.c:167)
            self._vcm = f64(np.ravel(vcm))
            self._chk(self.lib.ddcmi_set_group_vcm(self.ctx, s.ngroup, _d(self._vcm)))
        if getattr(s, "group_vset", None) is not None and np.any(np.asarray(s.group_vset) != 0):      # FIXEDVELOCITY groups with a `v` key
            self.set_group_velocity(s.group_vset, s.group_v)
        self._chk(self.lib.ddcmi_set_random(self.ctx, int(getattr(s, "rng_seed", 0))))
        if float(getattr(s, "npt_beta", 0.0)) > 0.0:      # INTEGRATOR type=NGLFCONSTRAINT: barostat on the molecular pressure
            self.set_barostat(float(s.npt_T), float(s.npt_P0), float(s.npt_beta), float(s.npt_tau), isotropic=plan["isotropic"],
                              by_gid=bonded_by_gid)
        if constraints or constraint_groups is not None:  # INTEGRATOR type=NGLFCONSTRAINT: velocity constraints
            if constraint_groups is None:
                self._cons = expand_constraints(s)
            else:
                po, pi, pj, dd = constraint_groups
                self._cons = (i32(po), i32(pi), i32(pj), f64(dd))
            po, pi, pj, dd = self._cons
            if bonded_by_gid:                             # decomposed runs: the groups' atoms named by gid
                gids = np.asarray(s.gid, dtype=np.uint64)
                self._cons_gid = (np.ascontiguousarray(gids[pi]), np.ascontiguousarray(gids[pj]))
                self._chk(self.lib.ddcmi_set_constraints_gid(self.ctx, int(po.size - 1), _i(po), self._cons_gid[0].ctypes.data_as(_up),
                                                             self._cons_gid[1].ctypes.data_as(_up), _d(dd)))
            else:
                self._chk(self.lib.ddcmi_set_constraints(self.ctx, int(po.size - 1), _i(po), _i(pi), _i(pj), _d(dd)))
        nrest = int(getattr(s, "nrest", 0))
        if nrest > 0:     # RESTRAINT potential
            self._rest = (np.ascontiguousarray(s.rest_gid, dtype=np.uint64), i32(np.asarray(s.rest_fc).ravel()),
                          f64(np.asarray(s.rest_r0).ravel()), f64(s.rest_kb))
            self._chk(self.lib.ddcmi_set_restraints(self.ctx, nrest, self._rest[0].ctypes.data_as(_up), _i(self._rest[1]), _d(self._rest[2]),
                                                    _d(self._rest[3]), int(getattr(s, "rest_origin", 0))))
        self._chk(self.lib.ddcmi_set_clock(self.ctx, int(s.loop), float(s.time)))
        self.n = s.natoms
        if upload:
            self.upload(s.rx, s.ry, s.rz, s.vx, s.vy, s.vz)

    def _chk(self, rc):
        if rc != 0:
            raise DdcmiError("ddcmi error %d: %s" % (rc, self.lib.ddcmi_last_error(self.ctx).decode()))

    def set_group_velocity(self, vset, v):
        """ddcmi_set_group_velocity: FIXEDVELOCITY groups -- vset[g] != 0: the group's beads get v[g] (internal units) at every velocity
        update; 0: they coast.  One entry per group of the Setup."""
        vs = np.ascontiguousarray(np.ravel(vset), dtype=np.int32)
        vv = np.ascontiguousarray(np.ravel(v), dtype=np.float64)
        if vv.size != 3 * vs.size:
            raise DdcmiError("set_group_velocity: %d flags, %d components" % (vs.size, vv.size))
        self._chk(self.lib.ddcmi_set_group_velocity(self.ctx, int(vs.size), _i(vs), _d(vv)))

    def close(self):
        if self.ctx:
            self.lib.ddcmi_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, rx, rz_or_ry, rz=None, vx=None, vy=None, vz=None):
        s = self.s
        ry = rz_or_ry
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        a = [f64(x) for x in (rx, ry, rz)]
        v = [f64(x) for x in (vx, vy, vz)] if vx is not None else [None, None, None]
        gid = np.ascontiguousarray(s.gid, dtype=np.uint64)
        sp = np.ascontiguousarray(s.species, dtype=np.int32)
        gr = np.ascontiguousarray(s.group, dtype=np.int32)
        self._chk(self.lib.ddcmi_upload_state(self.ctx, self.n, _d(a[0]), _d(a[1]), _d(a[2]), _d(v[0]), _d(v[1]), _d(v[2]),
                                              gid.ctypes.data_as(_up), _i(sp), _i(gr)))
        lcg = getattr(s, "lcg64", None)
        if lcg is not None and type(self) is MartiniHIP and len(lcg) == self.n and np.any(np.asarray(self.plan["group_type"]) == 2):
            self.set_random_lcg64(lcg)      # RANDOM type=LCG64 in the deck: the Langevin groups of a one-domain run draw from the particles' own streams

    def build_list(self):
        self._chk(self.lib.ddcmi_build_list(self.ctx))

    def eval_forces(self):
        e = np.zeros(8)
        v = np.zeros(6)
        self._chk(self.lib.ddcmi_eval_forces(self.ctx, _d(e), _d(v)))
        return dict(zip(E_NAMES, e.tolist())), v

    def step(self, nsteps=1, dt=None):
        self._chk(self.lib.ddcmi_step_nglf(self.ctx, float(self.s.dt if dt is None else dt), int(nsteps)))

    def energies(self):
        e, v, t = np.zeros(8), np.zeros(6), np.zeros(6)
        rk = ctypes.c_double(0)
        self._chk(self.lib.ddcmi_get_energies(self.ctx, _d(e), _d(v), ctypes.byref(rk), _d(t)))
        return dict(zip(E_NAMES, e.tolist())), v, rk.value, t

    def lean_history(self):
        """(test_api) sums of the lean steps formed by the last batch launch: [nsteps, 32] = pair sums {lj, ele, vir6} as the full list counts
        them (twice), kinetic sums {rk, tion6}, 0, bonded sums {bond, angle, tors, impr, vir6}, zeros -- include/ddcmi_test.h"""
        out = np.zeros((32, 32))
        nst = ctypes.c_int(0)
        self.lib.ddcmi_debug_lean_history.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), _dp]
        self._chk(self.lib.ddcmi_debug_lean_history(self.ctx, ctypes.byref(nst), _d(out)))
        return out[:nst.value].copy()

    STEP_PLAN_FIELDS = ("halo", "fused", "lean", "level_table", "fixed_layout", "reduction", "halo_disp", "direct")

    def step_plan(self, back=0):
        """(test_api) the plan of the force evaluation `back` evaluations before the last one this context ran, as a dict of small
        integers -- include/ddcmi_test.h, ddcmi_debug_step_plan: halo 0 none, 1 images at their owners, 2 exchange + update launch, 3 direct
        from the receive buffer, 4 second stream, 5 update launch alone; reduction 0 none, 1 alone, 2 with the images, 3 with the next
        exchange's messages"""
        out = (ctypes.c_int * 8)(int(back))
        self.lib.ddcmi_debug_step_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        self._chk(self.lib.ddcmi_debug_step_plan(self.ctx, out))
        return dict(zip(self.STEP_PLAN_FIELDS, list(out)))

    def kinetic(self):
        t = np.zeros(6)
        rk = ctypes.c_double(0)
        self._chk(self.lib.ddcmi_kinetic(self.ctx, ctypes.byref(rk), _d(t)))
        return rk.value, t

    def set_random_lcg64(self, parms):
        """RANDOM type LCG64: the particles' own streams, records {state, multID, prime} (lcg64.h:8-12) in upload order; None clears them"""
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self.lib.ddcmi_set_random_lcg64.argtypes = [ctypes.c_void_p, ctypes.c_int, _up, u32p, u32p]
        if parms is None:
            self._lcg_set = False
            return self._chk(self.lib.ddcmi_set_random_lcg64(self.ctx, 0, None, None, None))
        st = np.ascontiguousarray(parms["state"], dtype=np.uint64)
        mu = np.ascontiguousarray(parms["multID"], dtype=np.uint32)
        pr = np.ascontiguousarray(parms["prime"], dtype=np.uint32)
        self._chk(self.lib.ddcmi_set_random_lcg64(self.ctx, int(st.size), st.ctypes.data_as(_up), mu.ctypes.data_as(u32p), pr.ctypes.data_as(u32p)))
        self._lcg_set = True

    def get_random_lcg64(self):
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self.lib.ddcmi_get_random_lcg64.argtypes = [ctypes.c_void_p, ctypes.c_int, _up, u32p, u32p]
        n = self.n
        out = np.zeros(n, dtype=[("state", "<u8"), ("multID", "<u4"), ("prime", "<u4")])
        st, mu, pr = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._chk(self.lib.ddcmi_get_random_lcg64(self.ctx, n, st.ctypes.data_as(_up), mu.ctypes.data_as(u32p), pr.ctypes.data_as(u32p)))
        out["state"], out["multID"], out["prime"] = st, mu, pr
        return out

    def kinetic_detail(self, by_species):
        """per-group / per-species {rk, tion[6], mass, number, J[3]} (energy.c:104-147) of this rank's beads"""
        ncl = int(self.s.nspecies if by_species else max(1, self.s.ngroup))
        out = np.zeros((ncl, 12))
        self.lib.ddcmi_kinetic_detail.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _dp]
        self._chk(self.lib.ddcmi_kinetic_detail(self.ctx, int(bool(by_species)), ncl, _d(out)))
        return out

    def set_barostat(self, T, P0, beta, tau, isotropic=False, by_gid=False):
        """nglfconstraint's Berendsen barostat (isotropic: NGLFGPULANGEVIN's); the molecule lists feed its molecular virial
        (by_gid: atoms named by gid + the molecules' masses, for decomposed runs)"""
        nmol, off, atoms = self._mols = molecule_lists(self.s)
        if by_gid:
            gids = np.ascontiguousarray(np.asarray(self.s.gid, dtype=np.uint64)[atoms]) if atoms.size else np.zeros(1, np.uint64)
            m_at = np.asarray(self.s.mass, dtype=np.float64)[np.asarray(self.s.species)[atoms]] if atoms.size else np.zeros(0)
            mtot = np.ascontiguousarray(np.add.reduceat(m_at, off[:-1])) if off.size > 1 else np.zeros(1)
            self._mol_gid = (gids, mtot)
            self._chk(self.lib.ddcmi_set_molecule_lists_gid(self.ctx, nmol, int(off.size - 1), _i(off), gids.ctypes.data_as(_up), _d(mtot)))
        else:
            self._chk(self.lib.ddcmi_set_molecule_lists(self.ctx, nmol, int(off.size - 1), _i(off), _i(atoms if atoms.size else np.zeros(1, np.int32))))
        self._chk(self.lib.ddcmi_set_barostat(self.ctx, float(T), float(P0), float(beta), float(tau)))
        self._chk(self.lib.ddcmi_set_barostat_isotropic(self.ctx, int(bool(isotropic))))

    def constraint_stats(self, reset=True):
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.lib.ddcmi_constraint_stats(self.ctx, ctypes.byref(a), ctypes.byref(b), int(reset)))
        return a.value, b.value

    def barostat_pressure(self):
        p = np.zeros(3)
        self._chk(self.lib.ddcmi_get_barostat_pressure(self.ctx, _d(p)))
        return p

    def box(self):
        h = np.zeros(9)
        self._chk(self.lib.ddcmi_get_box(self.ctx, _d(h)))
        return h[[0, 4, 8]]

    def group_temperatures(self):
        T = np.zeros(max(1, self.s.ngroup))
        self._chk(self.lib.ddcmi_group_temperatures(self.ctx, _d(T)))
        return T

    def pair_correlation(self, rmin, delta_r, nbins, log=False):
        """ANALYSIS PAIRCORRELATION, one evaluation (ddcmi_pair_correlation): (counts[ncombo, nbins], nbeads[nspecies]) of this
        rank -- ordered pairs (i owned here, species(i) <= species(j)) by comboIndex and bin, and the beads per species"""
        ns = int(self.s.nspecies)
        counts = np.zeros((ns * (ns + 1) // 2, int(nbins)), np.int64)
        nbeads = np.zeros(ns, np.int64)
        self._chk(self.lib.ddcmi_pair_correlation(self.ctx, float(rmin), float(delta_r), int(nbins), int(bool(log)), ns,
                                                  counts.ctypes.data_as(_lp), nbeads.ctypes.data_as(_lp)))
        return counts, nbeads

    def vaf_origin(self):
        """ANALYSIS VELOCITYAUTOCORRELATION: the current state becomes the time origin of every owned bead (ddcmi_vaf_origin)"""
        self._chk(self.lib.ddcmi_vaf_origin(self.ctx))

    def vaf_sample(self):
        """(vaf[nclass], msd[nclass]) of this rank: sum v0.v and sum d.d in internal units for the system, every group, every
        species -- class 0, 1 + g, 1 + ngroup + s (ddcmi_vaf_sample)"""
        ng, ns = max(1, int(self.s.ngroup)), int(self.s.nspecies)
        vaf, msd = np.zeros(1 + ng + ns), np.zeros(1 + ng + ns)
        self._chk(self.lib.ddcmi_vaf_sample(self.ctx, ng, ns, _d(vaf), _d(msd)))
        return vaf, msd

    def vaf_clear(self):
        """tracking off, the reference records released (ddcmi_vaf_clear)"""
        self._chk(self.lib.ddcmi_vaf_clear(self.ctx))

    def momentum_by_class(self):
        """ANALYSIS vcmWrite's sums of this rank (ddcmi_momentum_by_class): (mv[nclass, 3], m[nclass]) = sum m v and sum m in internal
        units for the system, every group, every species -- class 0, 1 + g, 1 + ngroup + s"""
        ng, ns = max(1, int(self.s.ngroup)), int(self.s.nspecies)
        mv, m = np.zeros((1 + ng + ns, 3)), np.zeros(1 + ng + ns)
        self._chk(self.lib.ddcmi_momentum_by_class(self.ctx, ng, ns, _d(mv), _d(m)))
        return mv, m

    def zdensity(self, nz, smear_radius=0.0, smear_method="impulse"):
        """ANALYSIS zdensity's histogram of this rank (ddcmi_zdensity): density[nz] weights along z; smear_radius in internal
        length units (<= 0: one bin per bead), smear_method "impulse" or "hat" (anything else is impulse)"""
        density = np.zeros(max(1, int(nz)))
        self._chk(self.lib.ddcmi_zdensity(self.ctx, int(nz), float(smear_radius), _smear_method(smear_method), _d(density)))
        return density

    def kinetic_energy_distn(self, emin, emax, nbins, species_dist):
        """ANALYSIS KINETICENERGYDISTN, one evaluation of this rank (ddcmi_kinetic_energy_distn): group g histograms the kinetic
        energies of the species s with species_dist[s] == g into nbins[g] bins from emin[g] to emax[g] (internal units).  Returns
        (counts[sum nbins] int64 in group order, tallies[ndist, 3] int64 = {cntTotal, subCnt, supCnt}, stats[ndist, 3] = {sum K,
        min K, max K})"""
        emin, emax, nbins, sd, counts, tallies, stats = _kdist_args(self.s.nspecies, emin, emax, nbins, species_dist)
        counts, tallies, stats = counts[0], np.ascontiguousarray(tallies[0]), np.ascontiguousarray(stats[0])
        self._chk(self.lib.ddcmi_kinetic_energy_distn(self.ctx, int(self.s.nspecies), len(nbins), _d(emin), _d(emax), _i(nbins), _i(sd),
                                                      counts.ctypes.data_as(_lp), tallies.ctypes.data_as(_lp), _d(stats)))
        return counts, tallies, stats

    def chol_offsets(self, gid7, rmin, delta, nbins, fragments=False):
        """ANALYSIS cholAnalysis, one evaluation of this rank (ddcmi_chol_offsets): gid7[nmol, 7] the molecules' beads of roles 0..6,
        rmin and delta in internal length units.  Returns (counts[2 nbins] int64 -- the histogram of dR1, then of dR5 --, stats[6] =
        {sum, min, max} of dR1, then of dR5, n the molecules counted); with fragments, a fourth value: the beads of the molecules this
        rank owns in part, a structured array of CHOL_FRAGMENT (mol, role, r) for chol_merge"""
        gid, counts, ndone, stats, nfrag = _chol_args(gid7, nbins)
        nmol = (gid.size - 1) // 7
        self._chk(self.lib.ddcmi_chol_offsets(self.ctx, nmol, gid.ctypes.data_as(_up), float(rmin), float(delta), int(nbins), counts.ctypes.data_as(_lp),
                                              ndone.ctypes.data_as(_lp), _d(stats), 0, None, nfrag.ctypes.data_as(_lp)))      # (frag NULL: the count)
        frag = np.zeros(int(nfrag[0]), CHOL_FRAGMENT)
        if fragments and len(frag):      # (they stay packed on the device: a copy, not a second pass)
            self._chk(self.lib.ddcmi_chol_fragments(self.ctx, len(frag), frag.ctypes.data_as(ctypes.c_void_p), nfrag.ctypes.data_as(_lp)))
        out = (counts[0], stats[0], int(ndone[0]))
        return out + (frag[:int(nfrag[0])].copy(),) if fragments else out

    def track_set(self, gids):
        """ANALYSIS FORCE_AVERAGE: the gids whose beads this context follows (ddcmi_track_set), in any order, duplicates allowed; a new
        list clears the sums, an empty one removes the list"""
        g = np.ascontiguousarray(np.asarray(gids, dtype=np.uint64).reshape(-1))
        self._chk(self.lib.ddcmi_track_set(self.ctx, g.size, g.ctypes.data_as(_up) if g.size else None))
        self._ntrack = int(g.size)

    def track_accumulate(self, what):
        """one sample (ddcmi_track_accumulate): the owned beads with tracked gids add their force ("force" or 0), velocity ("velocity", 1)
        or position ("position", 2) to the running sums on the device; asynchronous"""
        self._chk(self.lib.ddcmi_track_accumulate(self.ctx, TRACK_WHAT[what.lower()] if isinstance(what, str) else int(what)))

    def track_read(self, reset=False):
        """(sum[n, 3], hits[n]) of this rank in the order of track_set (ddcmi_track_read); reset: the sums are zeroed afterwards"""
        n = getattr(self, "_ntrack", 0)
        tot, hits = np.zeros((n, 3)), np.zeros(n, np.int64)
        self._chk(self.lib.ddcmi_track_read(self.ctx, n, _d(tot), hits.ctypes.data_as(_lp), int(bool(reset))))
        return tot, hits

    def charge_density_modes(self, mmax, select=None):
        """ANALYSIS DSF, one evaluation of this rank (ddcmi_charge_density_modes): (rho complex128 [3, mmax], count) -- rho[a, m - 1] the
        sum of q exp(i 2 pi m r_a / L_a) over the owned beads of the species select marks (None: all), count their number; the division
        by the global count is the caller's"""
        sel, rho, count = _dsf_args(self.s.nspecies, mmax, select)
        self._chk(self.lib.ddcmi_charge_density_modes(self.ctx, int(self.s.nspecies), _i(sel), int(mmax), _d(rho), count.ctypes.data_as(_lp)))
        return rho[0, :, :, 0] + 1j * rho[0, :, :, 1], int(count[0])

    def structure_modes(self, kvec, select=None, weight="unit"):
        """ANALYSIS SSF's sums on any list of integer wave vectors, one evaluation of this rank (ddcmi_structure_modes): (rho complex128
        [nk], count) -- rho[l] the sum of w exp(i 2 pi (n_x x / L_x + n_y y / L_y + n_z z / L_z)), (n_x, n_y, n_z) = kvec[l] (signed), over
        the owned beads of the species select marks (None: all), count their number; weight "unit": w = 1, "charge": the species' charge"""
        sel, w, kv, rho, count = _sm_args(self.s.nspecies, kvec, select, weight)
        self._chk(self.lib.ddcmi_structure_modes(self.ctx, int(self.s.nspecies), _i(sel), w, len(kv), _i(kv), _d(rho), count.ctypes.data_as(_lp)))
        return rho[0, :len(kv), 0] + 1j * rho[0, :len(kv), 1], int(count[0])

    def subset_records(self, count_only=False, cap=None, out=None, **filt):
        """ANALYSIS subsetWrite, format binaryCharmm: this rank's selected beads as the file's records (ddcmi_subset_records), a
        structured array of SUBSET_RECORD (id u8, pinfo u4, r 3 x f4) in the order of download_particles.  The filter's keywords are
        those of _subset_filter.  count_only: the count alone.  cap / out: the capacity handed down (default: the count) and the
        array the records land in -- for the refusal of a buffer that is too small."""
        f, keep = _subset_filter(self.s, **filt)
        n = np.zeros(1, np.int64)
        self._chk(self.lib.ddcmi_subset_records(self.ctx, ctypes.byref(f), 0, None, n.ctypes.data_as(_lp)))
        if count_only:
            return int(n[0])
        rec = np.zeros(int(n[0]), SUBSET_RECORD) if out is None else out
        self._chk(self.lib.ddcmi_subset_records(self.ctx, ctypes.byref(f), int(n[0]) if cap is None else int(cap), rec.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(_lp)))
        del keep
        return rec[:int(n[0])]

    def coarsegrain(self, nx, ny, nz, smear_radius=0.0, smear_method="impulse", count_only=False, cap=None, out=None):
        """ANALYSIS COARSEGRAIN, one evaluation of this rank (ddcmi_coarsegrain): the non-empty (label, species) entries in ascending
        order as a structured array of CG_RECORD (label, species, n, mass, K[3], p[3]; internal units), label = igz + nz (igy + ny igx);
        smear_radius in internal length units (<= 0: one cell per bead), smear_method "impulse" or "hat" (anything else is impulse).
        count_only: the count alone.  cap / out: the capacity handed down (default: the count) and the array the records land in."""
        a = (int(nx), int(ny), int(nz), int(self.s.nspecies), float(smear_radius), _smear_method(smear_method))
        n = np.zeros(1, np.int64)
        self._chk(self.lib.ddcmi_coarsegrain(self.ctx, *a, 0, None, n.ctypes.data_as(_lp)))
        if count_only:
            return int(n[0])
        rec = np.zeros(int(n[0]), CG_RECORD) if out is None else out
        self._chk(self.lib.ddcmi_coarsegrain(self.ctx, *a, int(n[0]) if cap is None else int(cap), rec.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(_lp)))
        return rec[:int(n[0])]

    def thermalize(self, method, temperature, select="global", seed=385212586, loop=0, keep_vcm=False):
        """TRANSFORM type THERMALIZE (ddcmi_thermalize): new velocities for this context's beads, nothing else changes.  method "BOLTZMANN":
        v = sqrt(T / m) g on the bead's own erand48 stream of (gid, seed, loop); "RESCALE": per class (v - vcm) sqrt(T / T_now) + vcm
        (keep_vcm) or + vcm sqrt(T / T_now).  select "global" (one temperature), "species" or "group" (one per class, < 0: left alone);
        internal energy units, kB = 1.  Collective on a decomposed run."""
        m, sel, t = _thermalize_args(self.s, method, temperature, select)
        self._chk(self.lib.ddcmi_thermalize(self.ctx, m, sel, int(t.size), _d(t), int(seed), int(loop), int(bool(keep_vcm))))

    def download(self, mask=POS | VEL | FORCE):
        n = self.n
        out = [np.zeros(n) for _ in range(9)]
        self._chk(self.lib.ddcmi_download_state(self.ctx, int(mask), *[_d(a) for a in out]))
        return {"r": out[0:3], "v": out[3:6], "f": out[6:9]}

    def upload_positions(self, r, v=None):
        """new positions (and velocities) of the same beads in caller order: sendGPUState of the host-integrator mode"""
        self.lib.ddcmi_upload_positions.argtypes = [ctypes.c_void_p] + [_dp] * 6
        vv = v if v is not None else (None, None, None)
        self._chk(self.lib.ddcmi_upload_positions(self.ctx, _d(r[0]), _d(r[1]), _d(r[2]), _d(vv[0]), _d(vv[1]), _d(vv[2])))

    def sync(self):
        self._chk(self.lib.ddcmi_sync(self.ctx))

    def clock(self):
        loop = ctypes.c_int64(0)
        t = ctypes.c_double(0)
        self._chk(self.lib.ddcmi_get_clock(self.ctx, ctypes.byref(loop), ctypes.byref(t)))
        return loop.value, t.value

    def list_stats(self):
        st = (ctypes.c_int64 * 8)()
        self._chk(self.lib.ddcmi_list_stats(self.ctx, st))
        return {"entries": st[0], "excluded": st[1], "ell_width": st[2], "images": st[3], "cells": st[4], "rebuilds": st[5], "npad": st[6]}

    def comm_stats(self):
        st = (ctypes.c_int64 * 8)()
        self.lib.ddcmi_comm_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
        self._chk(self.lib.ddcmi_comm_stats(self.ctx, st))
        v = int(st[4])
        return {"send_beads": int(st[0]), "recv_beads": int(st[1]), "send_msgs": int(st[2]), "recv_msgs": int(st[3]),
                "rccl_version": "%d.%d.%d" % (v // 10000, (v // 100) % 100, v % 100) if v else None,
                "transport": ("none", "rccl", "host", "rccl-loopback")[int(st[5])], "ranks": int(st[6]), "rank": int(st[7])}

    def comm_peers(self):
        """[(peer rank, beads sent per step, beads received per step)] of the per-step halo exchange as laid out at the last rebuild"""
        i64p = ctypes.POINTER(ctypes.c_int64)
        self.lib.ddcmi_comm_peer_stats.argtypes = [ctypes.c_void_p, ctypes.c_int, _ip, i64p, i64p]
        peer = np.zeros(27, np.int32)
        sb, rb = np.zeros(27, np.int64), np.zeros(27, np.int64)
        n = int(self.lib.ddcmi_comm_peer_stats(self.ctx, 27, _i(peer), sb.ctypes.data_as(i64p), rb.ctypes.data_as(i64p)))
        return [(int(peer[k]), int(sb[k]), int(rb[k])) for k in range(max(n, 0))]

    def get_list(self, which=0):
        n = self.n
        tot = ctypes.c_int64(0)
        start = np.zeros(n + 1, np.int32)
        self._chk(self.lib.ddcmi_get_list(self.ctx, which, _i(start), None, ctypes.byref(tot)))
        j = np.zeros(max(1, tot.value), np.int32)
        self._chk(self.lib.ddcmi_get_list(self.ctx, which, _i(start), _i(j), ctypes.byref(tot)))
        return start, j[:tot.value]

    def timing(self, on=True):
        self._chk(self.lib.ddcmi_timing_enable(self.ctx, 1 if on else 0))

    def timing_fused(self):
        """of the last timing_read: (launches, ms) of the pair kernel with the integrator's pass as its epilogue"""
        n, ms = ctypes.c_int64(0), ctypes.c_double(0.0)
        self.lib.ddcmi_timing_fused.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64), _dp]
        self._chk(self.lib.ddcmi_timing_fused(self.ctx, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    def timing_read(self, reset=True):
        n = ctypes.c_int64(0)
        ms = ctypes.c_double(0)
        self._chk(self.lib.ddcmi_timing_read(self.ctx, ctypes.byref(n), ctypes.byref(ms), 1 if reset else 0))
        return n.value, ms.value


def _declare_domains(lib):
    """the test-only entry points (include/ddcmi_test.h): lib is the handle of libddcmi_test.so"""
    if getattr(lib, "_ddcmi_dom_declared", False):
        return
    if not hasattr(lib, "ddcmi_group_create"):
        return      # (a handle of the product library: it has none of them -- nothing to declare)
    vp = ctypes.c_void_p
    lib.ddcmi_plan_directions.argtypes = [ctypes.c_int] * 5 + [_ip, _ip]
    lib.ddcmi_plan_recv_counts.argtypes = [ctypes.c_int] * 6 + [_ip, _ip]
    lib.ddcmi_plan_halo_layout.argtypes = [ctypes.c_int] * 6 + [_ip, _ip, _ip, _ip, _ip, _ip]
    lib.ddcmi_group_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.ddcmi_group_destroy.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.ddcmi_group_eval_forces.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.ddcmi_group_step_nglf.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_double, ctypes.c_int]
    lib.ddcmi_group_temperatures_all.argtypes = [ctypes.POINTER(vp), ctypes.c_int, _dp]
    lib.ddcmi_group_pair_correlation.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, _lp, _lp]
    lib.ddcmi_group_vaf_origin.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.ddcmi_group_vaf_clear.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.ddcmi_group_vaf_sample.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp]
    lib.ddcmi_group_momentum_by_class.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp]
    lib.ddcmi_group_zdensity.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, _dp]
    lib.ddcmi_group_kinetic_energy_distn.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, _dp, _ip, _ip, _lp, _lp, _dp]
    lib.ddcmi_group_charge_density_modes.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, _ip, ctypes.c_int, _dp, _lp]
    lib.ddcmi_group_structure_modes.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, _ip, ctypes.c_int, ctypes.c_int, _ip, _dp, _lp]
    lib.ddcmi_group_subset_records.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(CSubsetFilter), ctypes.c_int64, vp, _lp]
    lib.ddcmi_group_coarsegrain.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                            ctypes.c_int64, vp, _lp]
    lib.ddcmi_group_thermalize.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _dp, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int]
    lib.ddcmi_group_chol_offsets.argtypes = [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int64, _up, ctypes.c_double, ctypes.c_double, ctypes.c_int, _lp, _lp, _dp,
                                             ctypes.c_int64, vp, _lp]
    lib._ddcmi_dom_declared = True


def plan_directions(px, py, pz, rank, pbc=7):
    """(dest[27], shift[27,3]) of the 26 neighbour directions (host logic, no GPU needed; test API: libddcmi_test.so)."""
    lib = _lib.load_test_library()
    _declare(lib)
    _declare_domains(lib)
    dest = np.zeros(27, np.int32)
    shift = np.zeros(81, np.int32)
    rc = lib.ddcmi_plan_directions(px, py, pz, rank, pbc, _i(dest), _i(shift))
    if rc != 0:
        raise DdcmiError("ddcmi_plan_directions failed: %d" % rc)
    return dest, shift.reshape(27, 3)


def domain_of(setup, grid):
    """owner rank of every bead for a px*py*pz brick decomposition (box centred on the origin); a bead outside the box on an open
    axis belongs to the edge brick on its side, as k_mig_classify has it"""
    px, py, pz = grid
    L = setup.box
    out = np.zeros(setup.natoms, np.int64)
    mult = 1
    pbc = int(getattr(setup, "pbc", 7))
    for a, (r, P) in enumerate(zip((setup.rx, setup.ry, setup.rz), (px, py, pz))):
        x = np.asarray(r, float)
        if (pbc >> a) & 1:
            x = x - L[a] * np.rint(x / L[a])
        b = np.clip(np.floor((x + 0.5 * L[a]) / (L[a] / P)).astype(np.int64), 0, P - 1)
        out += mult * b
        mult *= P
    return out


def select_rank(setup, owner, rank):
    """(index array) of the beads rank owns"""
    return np.flatnonzero(owner == rank)


class DomainMixin(object):
    """gid-addressed download for decomposed runs"""

    def download_particles(self):
        cap = int(self.lib.ddcmi_nlocal(self.ctx)) + 16
        n = ctypes.c_int(0)
        gid = np.zeros(cap, np.uint64)
        sp = np.zeros(cap, np.int32)
        arr = [np.zeros(cap) for _ in range(9)]
        self._chk(self.lib.ddcmi_download_particles(self.ctx, cap, ctypes.byref(n), gid.ctypes.data_as(_up), _i(sp), *[_d(a) for a in arr]))
        k = n.value
        out = {"gid": gid[:k], "species": sp[:k], "r": [a[:k] for a in arr[0:3]], "v": [a[:k] for a in arr[3:6]], "f": [a[:k] for a in arr[6:9]]}
        if getattr(self, "_lcg_set", False) and k > 0:
            self.n = k
            out["lcg64"] = self.get_random_lcg64()      # same order: the beads this rank owns now
        return out


class MartiniRank(MartiniHIP, DomainMixin):
    """One rank of a decomposed run: uploads only the beads `index` selects."""

    def __init__(self, setup, index, device=0, constraints=None, test_api=False, constraint_groups=None):
        MartiniHIP.__init__(self, setup, device=device, upload=False, bonded_by_gid=True, constraints=constraints, test_api=test_api,
                            constraint_groups=constraint_groups)
        self.index = np.asarray(index)

    def upload_local(self):
        s, ix = self.s, self.index
        f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        gid = np.ascontiguousarray(s.gid[ix], dtype=np.uint64)
        sp = np.ascontiguousarray(s.species[ix], dtype=np.int32)
        gr = np.ascontiguousarray(s.group[ix], dtype=np.int32)
        a = [f64(x[ix]) for x in (s.rx, s.ry, s.rz, s.vx, s.vy, s.vz)]
        self.n = len(ix)
        self._chk(self.lib.ddcmi_upload_state(self.ctx, self.n, _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), _d(a[4]), _d(a[5]),
                                              gid.ctypes.data_as(_up), _i(sp), _i(gr)))
        lcg = getattr(s, "lcg64", None)
        if lcg is not None and self.n > 0 and np.any(np.asarray(self.plan["group_type"]) == 2):
            self.set_random_lcg64(lcg[ix])      # the records migrate with their beads from here on

    def comm_init(self, rank, nranks, uid, grid):
        self._chk(self.lib.ddcmi_comm_init(self.ctx, rank, nranks, uid, grid[0], grid[1], grid[2]))

    def comm_init_host(self, rdzv, grid):
        """decomposition over the host transport (TCP streams of the rendezvous) instead of RCCL"""
        self._rdzv = rdzv      # must outlive the context
        self._chk(self.lib.ddcmi_comm_init_host(self.ctx, rdzv.h, grid[0], grid[1], grid[2]))

    def preflight(self, timeout=60.0):
        """ddcmi_comm_preflight: one grouped exchange of a known pattern with every peer of the brick plan, one 24-double all-reduce,
        one int all-gather, verified; raises DdcmiError naming the stage / peer / direction.  Returns the report as a dict."""
        self.lib.ddcmi_comm_preflight.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.POINTER(ctypes.c_int64)]
        rep = (ctypes.c_int64 * 16)()
        rc = self.lib.ddcmi_comm_preflight(self.ctx, float(timeout), rep)
        out = {"peers": [int(rep[8 + k]) for k in range(min(int(rep[0]), 8))], "directions": int(rep[1]), "bytes_per_direction": int(rep[2]),
               "stages_verified": int(rep[6]), "elapsed_us": int(rep[7])}
        if rep[3]:
            out.update(failed_peer=int(rep[4]), failed_direction_code=int(rep[5]))
        self.preflight_report = out
        if rc != 0:
            raise DdcmiError("ddcmi error %d: %s" % (rc, self.lib.ddcmi_last_error(self.ctx).decode()))
        return out

    def allreduce(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._chk(self.lib.ddcmi_comm_allreduce_sum(self.ctx, _d(v), v.size))
        return v


class MartiniGroup(object):
    """px*py*pz domains emulated inside one process on one GPU (device copies
    instead of RCCL): exercises migration, halo tables and per-step halo refresh."""

    def __init__(self, setup, grid, device=0, constraints=None, constraint_groups=None):
        self.s = setup
        self.grid = tuple(grid)
        self.n = grid[0] * grid[1] * grid[2]
        owner = domain_of(setup, grid)
        self.ranks = [MartiniRank(setup, select_rank(setup, owner, r), device=device, constraints=constraints, test_api=True,
                                  constraint_groups=constraint_groups) for r in range(self.n)]
        self.lib = self.ranks[0].lib
        _declare_domains(self.lib)
        self.arr = (ctypes.c_void_p * self.n)(*[r.ctx for r in self.ranks])
        rc = self.lib.ddcmi_group_create(self.arr, self.n, grid[0], grid[1], grid[2])
        if rc != 0:
            msgs = [self.lib.ddcmi_last_error(r.ctx).decode() for r in self.ranks]
            raise DdcmiError("ddcmi_group_create failed: %d %s" % (rc, "; ".join(sorted(set(m for m in msgs if m)))))
        for r in self.ranks:
            r.upload_local()

    def _chk(self, rc):
        if rc != 0:
            msgs = [self.lib.ddcmi_last_error(r.ctx).decode() for r in self.ranks]
            raise DdcmiError("ddcmi group error %d: %s" % (rc, "; ".join(m for m in msgs if m)))

    def eval_forces(self):
        self._chk(self.lib.ddcmi_group_eval_forces(self.arr, self.n))
        return self.energies()[:2]

    def step(self, nsteps=1, dt=None):
        self._chk(self.lib.ddcmi_group_step_nglf(self.arr, self.n, float(self.s.dt if dt is None else dt), int(nsteps)))

    def set_group_velocity(self, vset, v):
        """MartiniHIP.set_group_velocity on every domain: the per-group tables belong to each context"""
        for r in self.ranks:
            r.set_group_velocity(vset, v)

    def group_temperatures(self):
        T = np.zeros(max(1, self.s.ngroup))
        self._chk(self.lib.ddcmi_group_temperatures_all(self.arr, self.n, _d(T)))
        return T

    def pair_correlation(self, rmin, delta_r, nbins, log=False, per_rank=False):
        """ddcmi_group_pair_correlation: the domains' (counts, nbeads) summed -- or, per_rank, stacked [rank, ...]"""
        ns = int(self.s.nspecies)
        counts = np.zeros((self.n, ns * (ns + 1) // 2, int(nbins)), np.int64)
        nbeads = np.zeros((self.n, ns), np.int64)
        self._chk(self.lib.ddcmi_group_pair_correlation(self.arr, self.n, float(rmin), float(delta_r), int(nbins), int(bool(log)), ns,
                                                        counts.ctypes.data_as(_lp), nbeads.ctypes.data_as(_lp)))
        if per_rank:
            return counts, nbeads
        return counts.sum(axis=0), nbeads.sum(axis=0)

    @staticmethod
    def _sum_in_rank_order(a):
        """a[0] + a[1] + ... from left to right (np.sum(axis=0) may add pairwise): the same bits every time"""
        tot = a[0].copy()
        for r in range(1, len(a)):
            tot += a[r]
        return tot

    def vaf_origin(self):
        """ddcmi_group_vaf_origin: the time origin of every domain's beads"""
        self._chk(self.lib.ddcmi_group_vaf_origin(self.arr, self.n))

    def vaf_clear(self):
        """ddcmi_group_vaf_clear: tracking off on every domain"""
        self._chk(self.lib.ddcmi_group_vaf_clear(self.arr, self.n))

    def vaf_sample(self, per_rank=False):
        """ddcmi_group_vaf_sample: the domains' (vaf, msd) summed in rank order -- or, per_rank, stacked [rank, class]"""
        ng, ns = max(1, int(self.s.ngroup)), int(self.s.nspecies)
        vaf, msd = np.zeros((self.n, 1 + ng + ns)), np.zeros((self.n, 1 + ng + ns))
        self._chk(self.lib.ddcmi_group_vaf_sample(self.arr, self.n, ng, ns, _d(vaf), _d(msd)))
        if per_rank:
            return vaf, msd
        return self._sum_in_rank_order(vaf), self._sum_in_rank_order(msd)

    def momentum_by_class(self, per_rank=False):
        """ddcmi_group_momentum_by_class: the domains' (mv, m) summed in rank order -- or, per_rank, stacked [rank, class, ...]"""
        ng, ns = max(1, int(self.s.ngroup)), int(self.s.nspecies)
        mv, m = np.zeros((self.n, 1 + ng + ns, 3)), np.zeros((self.n, 1 + ng + ns))
        self._chk(self.lib.ddcmi_group_momentum_by_class(self.arr, self.n, ng, ns, _d(mv), _d(m)))
        if per_rank:
            return mv, m
        return self._sum_in_rank_order(mv), self._sum_in_rank_order(m)

    def zdensity(self, nz, smear_radius=0.0, smear_method="impulse", per_rank=False):
        """ddcmi_group_zdensity: the domains' histograms summed in rank order -- or, per_rank, stacked [rank, bin]"""
        density = np.zeros((self.n, max(1, int(nz))))
        self._chk(self.lib.ddcmi_group_zdensity(self.arr, self.n, int(nz), float(smear_radius), _smear_method(smear_method), _d(density)))
        if per_rank:
            return density
        return self._sum_in_rank_order(density)

    def kinetic_energy_distn(self, emin, emax, nbins, species_dist, per_rank=False):
        """ddcmi_group_kinetic_energy_distn: the domains' (counts, tallies, stats) combined -- counts and sums added in rank order,
        minimum of the minima, maximum of the maxima -- or, per_rank, stacked [rank, ...]"""
        emin, emax, nbins, sd, counts, tallies, stats = _kdist_args(self.s.nspecies, emin, emax, nbins, species_dist, self.n)
        tallies, stats = np.ascontiguousarray(tallies), np.ascontiguousarray(stats)
        self._chk(self.lib.ddcmi_group_kinetic_energy_distn(self.arr, self.n, int(self.s.nspecies), len(nbins), _d(emin), _d(emax), _i(nbins), _i(sd),
                                                            counts.ctypes.data_as(_lp), tallies.ctypes.data_as(_lp), _d(stats)))
        if per_rank:
            return counts, tallies, stats
        tot = stats[0].copy()
        tot[:, 0] = self._sum_in_rank_order(stats[:, :, 0])
        for r in range(1, self.n):
            tot[:, 1] = np.minimum(tot[:, 1], stats[r, :, 1])
            tot[:, 2] = np.maximum(tot[:, 2], stats[r, :, 2])
        return counts.sum(axis=0), tallies.sum(axis=0), tot

    def chol_offsets(self, gid7, rmin, delta, nbins, per_rank=False, cap=None, out=None):
        """ddcmi_group_chol_offsets: the domains' results merged (chol_merge: counts and ndone added, sums in rank order, extremes
        combined) and the molecules split over domains completed on the host -- (counts[2 nbins], stats[6], n) -- or, per_rank,
        (counts[rank], ndone[rank], stats[rank], fragments in rank order, nfrag[rank]).  cap / out: the capacity handed down (default:
        what the fragments need) and the array they land in -- for the refusal of a buffer that is too small."""
        gid, counts, ndone, stats, nfrag = _chol_args(gid7, nbins, self.n)
        nmol = (gid.size - 1) // 7
        a = (self.arr, self.n, nmol, gid.ctypes.data_as(_up), float(rmin), float(delta), int(nbins), counts.ctypes.data_as(_lp), ndone.ctypes.data_as(_lp), _d(stats))
        if cap is None and out is None:      # the count first (frag NULL), then the ranks' packed fragments: copies, not a second pass
            self._chk(self.lib.ddcmi_group_chol_offsets(*a, 0, None, nfrag.ctypes.data_as(_lp)))
            frag = np.zeros(int(nfrag.sum()), CHOL_FRAGMENT)
            off, one = 0, np.zeros(1, np.int64)
            for r, k in zip(self.ranks, nfrag):
                if k:
                    part = np.zeros(int(k), CHOL_FRAGMENT)
                    r._chk(self.lib.ddcmi_chol_fragments(r.ctx, int(k), part.ctypes.data_as(ctypes.c_void_p), one.ctypes.data_as(_lp)))
                    frag[off:off + int(k)] = part
                off += int(k)
        else:
            frag = np.zeros(max(int(cap), 1), CHOL_FRAGMENT) if out is None else out
            self._chk(self.lib.ddcmi_group_chol_offsets(*a, len(frag) if cap is None else int(cap), frag.ctypes.data_as(ctypes.c_void_p), nfrag.ctypes.data_as(_lp)))
        frag = frag[:int(nfrag.sum())]
        if per_rank:
            return counts, ndone, stats, frag, nfrag
        return chol_merge(self.lib, self.s, gid[:-1], rmin, delta, nbins, counts, ndone, stats, [frag])

    def track_set(self, gids):
        """MartiniHIP.track_set on every domain: each keeps its own sums of the beads it owns at each sample"""
        for r in self.ranks:
            r.track_set(gids)

    def track_accumulate(self, what):
        """MartiniHIP.track_accumulate on every domain; no communication"""
        for r in self.ranks:
            r.track_accumulate(what)

    def track_read(self, reset=False, per_rank=False):
        """the domains' (sum[n, 3], hits[n]) added in rank order -- or, per_rank, stacked [rank, ...]"""
        parts = [r.track_read(reset) for r in self.ranks]
        tot, hits = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
        if per_rank:
            return tot, hits
        return self._sum_in_rank_order(tot), hits.sum(axis=0)

    def charge_density_modes(self, mmax, select=None, per_rank=False):
        """ddcmi_group_charge_density_modes: the domains' (rho, count) added in rank order -- or, per_rank, stacked [rank, ...]"""
        sel, rho, count = _dsf_args(self.s.nspecies, mmax, select, self.n)
        self._chk(self.lib.ddcmi_group_charge_density_modes(self.arr, self.n, int(self.s.nspecies), _i(sel), int(mmax), _d(rho), count.ctypes.data_as(_lp)))
        z = rho[..., 0] + 1j * rho[..., 1]
        if per_rank:
            return z, count
        return self._sum_in_rank_order(z), int(count.sum())

    def structure_modes(self, kvec, select=None, weight="unit", per_rank=False):
        """ddcmi_group_structure_modes: the domains' (rho, count) added in rank order -- or, per_rank, stacked [rank, ...]"""
        sel, w, kv, rho, count = _sm_args(self.s.nspecies, kvec, select, weight, self.n)
        self._chk(self.lib.ddcmi_group_structure_modes(self.arr, self.n, int(self.s.nspecies), _i(sel), w, len(kv), _i(kv), _d(rho), count.ctypes.data_as(_lp)))
        z = rho[:, :len(kv), 0] + 1j * rho[:, :len(kv), 1]
        if per_rank:
            return z, count
        return self._sum_in_rank_order(z), int(count.sum())

    def subset_records(self, per_rank=False, cap=None, out=None, **filt):
        """ddcmi_group_subset_records: the domains' records one block behind the other in rank order -- or, per_rank, (records, count[rank])"""
        f, keep = _subset_filter(self.s, **filt)
        n = np.zeros(self.n, np.int64)
        self._chk(self.lib.ddcmi_group_subset_records(self.arr, self.n, ctypes.byref(f), 0, None, n.ctypes.data_as(_lp)))
        tot = int(n.sum())
        rec = np.zeros(tot, SUBSET_RECORD) if out is None else out
        self._chk(self.lib.ddcmi_group_subset_records(self.arr, self.n, ctypes.byref(f), tot if cap is None else int(cap), rec.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(_lp)))
        del keep
        return (rec[:tot], n) if per_rank else rec[:tot]

    def coarsegrain(self, nx, ny, nz, smear_radius=0.0, smear_method="impulse", per_rank=False, cap=None, out=None):
        """ddcmi_group_coarsegrain: the domains' entries merged by (label, species) in rank order, duplicate keys added -- or, per_rank,
        (records one block behind the other in rank order, count[rank])"""
        a = (int(nx), int(ny), int(nz), int(self.s.nspecies), float(smear_radius), _smear_method(smear_method))
        n = np.zeros(self.n, np.int64)
        self._chk(self.lib.ddcmi_group_coarsegrain(self.arr, self.n, *a, 0, None, n.ctypes.data_as(_lp)))
        tot = int(n.sum())
        rec = np.zeros(tot, CG_RECORD) if out is None else out
        self._chk(self.lib.ddcmi_group_coarsegrain(self.arr, self.n, *a, tot if cap is None else int(cap), rec.ctypes.data_as(ctypes.c_void_p), n.ctypes.data_as(_lp)))
        if per_rank:
            return rec[:tot], n
        from .analysis import merge_cg_records
        off = np.concatenate([[0], np.cumsum(n)])
        return merge_cg_records([rec[off[r]:off[r + 1]] for r in range(self.n)])

    def thermalize(self, method, temperature, select="global", seed=385212586, loop=0, keep_vcm=False):
        """ddcmi_group_thermalize: MartiniHIP.thermalize on every domain; RESCALE adds the domains' sums in rank order"""
        m, sel, t = _thermalize_args(self.s, method, temperature, select)
        self._chk(self.lib.ddcmi_group_thermalize(self.arr, self.n, m, sel, int(t.size), _d(t), int(seed), int(loop), int(bool(keep_vcm))))

    def energies(self):
        """sum over ranks = energyInfo.c allreduce()"""
        tot_e, tot_v, tot_rk, tot_t = None, None, 0.0, None
        for r in self.ranks:
            e, v, rk, t = r.energies()
            if tot_e is None:
                tot_e, tot_v, tot_t = dict(e), v.copy(), t.copy()
            else:
                for k in e:
                    tot_e[k] += e[k]
                tot_v += v
                tot_t += t
            tot_rk += rk
        return tot_e, tot_v, tot_rk, tot_t

    def gather(self):
        """all beads ordered by gid"""
        parts = [r.download_particles() for r in self.ranks]
        gid = np.concatenate([p["gid"] for p in parts])
        order = np.argsort(gid, kind="stable")
        out = {"gid": gid[order], "nlocal": [len(p["gid"]) for p in parts]}
        for k in ("r", "v", "f"):
            out[k] = [np.concatenate([p[k][c] for p in parts])[order] for c in range(3)]
        if all("lcg64" in p or len(p["gid"]) == 0 for p in parts) and any("lcg64" in p for p in parts):
            out["lcg64"] = np.concatenate([p["lcg64"] for p in parts if "lcg64" in p])[order]
        return out

    def close(self):
        try:
            self.lib.ddcmi_group_destroy(self.arr, self.n)
        except Exception:
            pass
        for r in self.ranks:
            r.close()

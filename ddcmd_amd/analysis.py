"""ANALYSIS types PAIRCORRELATION, VELOCITYAUTOCORRELATION, vcmWrite, zdensity, KINETICENERGYDISTN, DSF, subsetWrite, COARSEGRAIN and cholAnalysis on the host side.
PairCorrelation: accumulation of the device's pair counts into g(r) and the output file, as paircorrelation_eval_geom /
paircorrelation_output (paircorrelation.c) do.  The counting itself is ddcmi_pair_correlation (Martini*.pair_correlation); nothing
here searches pairs.
VelocityAutocorrelation: the windows of velocityAutocorrelation_eval and the file of velocityAutocorrelation_output
(velocityAutocorrelation.c) over the device's sums (Martini*.vaf_origin / vaf_sample).
VcmWrite, ZDensity: the file text of vcmWrite.c / zdensity.c from the device's sums (Martini*.momentum_by_class / zdensity).
KineticEnergyDistn: the accumulation and the two files of kineticEnergyDistn.c from the device's histograms
(Martini*.kinetic_energy_distn).
DynamicStructureFactor: the wave vectors, the buffer and the file text of dsf.c from the device's charge-density modes
(Martini*.charge_density_modes).
StaticStructureFactor: the wave vectors of ssf_kvector, their four sign combinations, S(k) and the lines of ssf_eval (ssf.c) from the
device's density modes (Martini*.structure_modes); in_plane lists the (n_x, n_y, 0) of an undulation spectrum.
SubsetWrite: the pinfo tables of pinfo.c, the header of write_fileheader (io.c) and the file of subsetWriteBinaryCharmm
(subsetWrite.c) around the device's packed records (Martini*.subset_records); read_subset reads such a file back.
CoarseGrain: the table keyed by (label, species) that accumulates the device's evaluations (Martini*.coarsegrain) and the cgrid file
of coarsegrain_output (coarsegrain.c:449-573); read_cgrid reads such a file back and verifies every record's checksum."""
import zlib
import os
import time as _time

import numpy as np

from .deck import units_convert


def combo_index(i, j, nspecies):
    """comboIndex (paircorrelation.c): place of the species pair {i, j} in combo-major order"""
    a, b = min(i, j), max(i, j)
    return (b - a) + nspecies * a - (a * (a - 1)) // 2


def combo_pairs(nspecies):
    """(a, b) with a <= b of every combo, in combo order (comboReverseIndex)"""
    out = [None] * (nspecies * (nspecies + 1) // 2)
    for a in range(nspecies):
        for b in range(a, nspecies):
            out[combo_index(a, b, nspecies)] = (a, b)
    return out


def bin_edges(rmin, delta_r, nbins, log=False):
    """binLeft / binRight of paircorrelation_parms, internal length units"""
    rmax = rmin + nbins * delta_r
    if not log:
        left = rmin + np.arange(nbins) * delta_r
        right = rmin + (np.arange(nbins) + 1) * delta_r
    else:
        ld = (np.log10(rmax) - np.log10(rmin)) / nbins
        left = 10.0 ** (np.log10(rmin) + np.arange(nbins) * ld)
        right = np.append(left[1:], rmax)
    return left, right


class PairCorrelation(object):
    """one PAIRCORRELATION analysis: add() takes the counts of one evaluation summed over the ranks, output() scales the sum
    of the samples with the box volume and the shell volumes and clears it (paircorrelation_output)"""

    def __init__(self, nspecies, rmin, delta_r, nbins, log=False, eval_rate=0, outputrate=0, filename="paircorrelation.dat"):
        self.ns, self.rmin, self.delta_r, self.nbins, self.log = int(nspecies), float(rmin), float(delta_r), int(nbins), bool(log)
        self.eval_rate, self.outputrate, self.filename = int(eval_rate), int(outputrate), filename
        self.clear()

    def clear(self):
        self.g = np.zeros((self.ns * (self.ns + 1) // 2, self.nbins))
        self.nsample = 0

    def add(self, counts, nbeads):
        """one sample: nBonds *= 1/(N_a N_b), then g += nBonds (the reference's order)"""
        counts = np.asarray(counts, dtype=np.float64).reshape(self.g.shape)
        nb = np.asarray(nbeads, dtype=np.float64)
        nbonds = counts.copy()
        for l, (a, b) in enumerate(combo_pairs(self.ns)):
            nbonds[l] *= 1.0 / (nb[a] * nb[b])
        self.g += nbonds
        self.nsample += 1

    def normalised(self, volume):
        """g * (V / nsample) / dv of each bin (volume in internal units)"""
        left, right = bin_edges(self.rmin, self.delta_r, self.nbins, self.log)
        dv = 4.0 * np.pi / 3.0 * (right ** 3 - left ** 3)
        return self.g * (volume / self.nsample) / dv[None, :]

    def header(self):
        return "rmin = %f Ang; delta_r = %f Ang; length = %d; eval_rate = %d; outputrate = %d;" % (
            units_convert(self.rmin, None, "Angstrom"), units_convert(self.delta_r, None, "Angstrom"), self.nbins, self.eval_rate, self.outputrate)

    def output_text(self, volume, species_names):
        """the file paircorrelation_output writes; clears the accumulator"""
        if self.nsample == 0:
            self.clear()
            return None
        g = self.normalised(volume)
        left, right = bin_edges(self.rmin, self.delta_r, self.nbins, self.log)
        lines = ["# %s\n" % self.header(), "# nsample = %d;\n" % self.nsample,
                 "# r(Ang) " + "".join("%s-%s " % (species_names[a], species_names[b]) for a, b in combo_pairs(self.ns)) + "\n"]
        for k in range(self.nbins):
            row = "%f " % units_convert(0.5 * (left[k] + right[k]), None, "Angstrom")
            row += "".join("%e " % g[l, k] for l in range(g.shape[0]))
            lines.append(row + "\n")
        self.clear()
        return "".join(lines)


def parse_output(text):
    """(header fields, nsample, column names, r[nbins] in A, g[ncombo, nbins]) of a paircorrelation file"""
    lines = text.splitlines()
    fields = {}
    for item in lines[0].lstrip("# ").split(";"):
        if "=" in item:
            k, v = item.split("=", 1)
            fields[k.strip()] = v.strip()
    nsample = int(lines[1].split("=")[1].strip().rstrip(";"))
    names = lines[2].lstrip("#").split()[1:]
    rows = np.array([[float(x) for x in ln.split()] for ln in lines[3:] if ln.strip()])
    return fields, nsample, names, rows[:, 0], rows[:, 1:].T


class VelocityAutocorrelation(object):
    """one VELOCITYAUTOCORRELATION analysis (velocityAutocorrelation.c:117-327).  eval(sample, origin) is the reference's state
    machine: sample() returns (vaf, msd) of [1 + ngroup + nspecies] classes summed over the ranks, origin() sets the time origin;
    add(vaf, msd) stores one sample by hand.  Every class is kept; output_text leaves out the group block of a single group and the
    species block of a single species, as the reference does."""

    def __init__(self, ngroup, nspecies, length=1, eval_rate=0, outputrate=0, filename="vaf.dat"):
        if int(length) < 1:
            raise ValueError("length = %d" % length)
        self.ng, self.ns, self.length = max(1, int(ngroup)), int(nspecies), int(length)
        self.eval_rate, self.outputrate, self.filename = int(eval_rate), int(outputrate), filename
        self.ncl = 1 + self.ng + self.ns
        self.last = 0
        self.vaf0, self.msd0 = np.zeros((self.ncl, self.length + 1)), np.zeros((self.ncl, self.length + 1))
        self.clear()

    def clear(self):
        """the reset velocityAutocorrelation_output does after writing"""
        self.vaf_, self.msd_ = np.zeros((self.ncl, self.length + 1)), np.zeros((self.ncl, self.length + 1))
        self.nsample = 0

    def add(self, vaf, msd, k=None):
        """sample k (default: the current entry, last) of the current window"""
        k = self.last if k is None else int(k)
        self.vaf0[:, k] = np.asarray(vaf, dtype=np.float64)
        self.msd0[:, k] = np.asarray(msd, dtype=np.float64)

    def accumulate(self):
        """a full window joins the sums over the windows"""
        self.nsample += 1
        self.msd_ += self.msd0
        self.vaf_ += self.vaf0
        self.msd0[:] = 0.0
        self.vaf0[:] = 0.0
        self.last = 0

    def eval(self, sample, origin):
        k = self.last
        if k > 0:
            self.add(*sample(), k=k)
        if k == self.length:
            self.accumulate()
            k = 0
        if k == 0:
            origin()
            self.add(*sample(), k=0)
        self.last += 1

    def gate(self):
        """does output write (and reset)?  nsample * length * eval_rate == outputrate"""
        return self.nsample * self.length * self.eval_rate == self.outputrate

    def columns(self, group_names, species_names):
        """(label, class index) of the blocks the file holds"""
        cols = [("System", 0)]
        if self.ng > 1:
            cols += [("Group %s" % group_names[g], 1 + g) for g in range(self.ng)]
        if self.ns > 1:
            cols += [("Species %s" % species_names[t], 1 + self.ng + t) for t in range(self.ns)]
        return cols

    def output_text(self, dt, nglobal, group_counts, species_counts, group_names, species_names):
        """the file velocityAutocorrelation_output writes, or None when the gate is shut (then nothing is reset).  dt in internal
        units; the counts are those of the whole system"""
        if not self.gate():
            return None
        tc, v2c, r2c = units_convert(1.0, None, "t"), units_convert(1.0, None, "velocity^2"), units_convert(1.0, None, "l^2")
        cols = self.columns(group_names, species_names)
        count = {0: float(nglobal)}
        count.update({1 + g: float(group_counts[g]) for g in range(len(group_counts))})
        count.update({1 + self.ng + t: float(species_counts[t]) for t in range(len(species_counts))})
        head = "%-33s" % "#time (fs)  System vaf MSD"
        head += "".join("%-26s" % ("  %s vaf MSD" % lab) for lab, _ in cols[1:])
        lines = [head + " (vaf in Ang^2/fs^2; msd in Ang^2)\n"]
        for k in range(self.length + 1):
            row = "%f" % (tc * k * dt * self.eval_rate)
            for _, c in cols:
                row += " %e %e" % ((v2c * self.vaf_[c, k] / self.nsample) / count[c], (r2c * self.msd_[c, k] / self.nsample) / count[c])
            lines.append(row + "\n")
        self.clear()
        return "".join(lines)


def parse_vaf_output(text):
    """(block labels, time[length + 1] in fs, vaf[nblock, length + 1], msd[nblock, length + 1]) of a vaf file"""
    lines = text.splitlines()
    head = lines[0]
    body = head[1:head.index("(vaf in")]
    words = body.split()      # time (fs) System vaf MSD [Group NAME vaf MSD ...] [Species NAME vaf MSD ...]
    labels, i = [], 2
    while i < len(words):
        if words[i] == "System":
            labels.append("System")
            i += 3
        else:
            labels.append("%s %s" % (words[i], words[i + 1]))
            i += 4
    rows = np.array([[float(x) for x in ln.split()] for ln in lines[1:] if ln.strip()])
    assert rows.shape[1] == 1 + 2 * len(labels)
    return labels, rows[:, 0], rows[:, 1::2].T, rows[:, 2::2].T


LOOP_WIDTH = 12      # the driver's loop format: the width of the data file's loop column


class VcmWrite(object):
    """one vcmWrite analysis (vcmWrite.c): header() is the line written when the file is opened, line(loop, time, mv, m) one output
    line from the sums over the ranks (Martini*.momentum_by_class: mv[nclass, 3] = sum m v, m[nclass] = sum m, internal units).
    Every group and every species has a block, a single one too."""

    def __init__(self, group_names, species_names, outputrate=0, filename="vcm.data"):
        self.group_names, self.species_names = list(group_names) or ["group"], list(species_names)
        self.ncl = 1 + len(self.group_names) + len(self.species_names)
        self.outputrate, self.filename = int(outputrate), filename

    def header(self):
        head = "-%*s %14s" % (LOOP_WIDTH, "#loop", "time(fs)")      # (the reference's format as it stands)
        head += "%-51s" % "     System vx vy vz (Ang/fs)"
        head += "".join("%-51s" % ("     Group %s vx vy vz (Ang/fs)" % g) for g in self.group_names)
        head += "".join("%-51s" % ("     Species %s vx vy vz (Ang/fs)" % sp) for sp in self.species_names)
        return head + "\n"

    def velocities(self, mv, m):
        """vcm[nclass, 3] in Ang/fs: sum m v / sum m where the class has mass, the sum as it is otherwise"""
        mv, m = np.array(mv, dtype=np.float64).reshape(self.ncl, 3), np.asarray(m, dtype=np.float64).reshape(self.ncl)
        for c in range(self.ncl):
            if m[c] > 0.0:
                mv[c] *= 1 / m[c]
        return mv * units_convert(1.0, None, "Ang/fs")

    def line(self, loop, time, mv, m):
        """time in internal units"""
        row = "%*d" % (LOOP_WIDTH, int(loop)) + " %16.6f" % (units_convert(1.0, None, "fs") * time)
        row += "".join(" %16.6e %16.6e %16.6e" % tuple(v) for v in self.velocities(mv, m))
        return row + "\n"


def parse_vcm_output(text):
    """(loop[nline], time[nline] in fs, vcm[nline, nclass, 3] in Ang/fs) of a vcmWrite file (header lines skipped)"""
    rows = [ln.split() for ln in text.splitlines() if ln.strip() and not ln.startswith("-")]
    loop = np.array([int(r[0]) for r in rows], np.int64)
    val = np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64).reshape(len(rows), -1)
    return loop, val[:, 0], val[:, 1:].reshape(len(rows), -1, 3)


class ZDensity(object):
    """one zdensity analysis (zdensity.c): output_text(density, box) is the file from the histogram summed over the ranks
    (Martini*.zdensity); box = (Lx, Ly, Lz) in internal units"""

    def __init__(self, nz, smear_radius=0.0, smear_method="impulse", outputrate=0, filename="zden.dat"):
        if int(nz) < 1:
            raise ValueError("nz = %d" % nz)
        self.nz, self.smear_radius = int(nz), float(smear_radius)
        self.smear_method = "hat" if str(smear_method).lower() == "hat" else "impulse"
        self.outputrate, self.filename = int(outputrate), filename

    def output_text(self, density, box):
        density = np.asarray(density, dtype=np.float64).reshape(self.nz)
        lc = units_convert(1.0, None, "Angstrom")
        box_vol = (box[0] * box[1] * box[2]) * lc * lc * lc
        bz = float(box[2])
        lines = []
        for ii in range(self.nz):
            z = ((ii + 0.5) * (bz / self.nz)) / bz
            lines.append("%f %f %f\n" % (z, density[ii] * (self.nz / box_vol), density[ii]))
        return "".join(lines)


class KineticEnergyDistn(object):
    """one KINETICENERGYDISTN analysis (kineticEnergyDistn.c).  groups: one dict per BIN object of distGroups, {"name", "species",
    "emin", "emax", "nbins"} in internal units (load_deck's "dist_groups").  add() takes one evaluation combined over the ranks
    (Martini*.kinetic_energy_distn: counts and sums added, minimum of minima, maximum of maxima); evaluations accumulate until
    clear().  dist_text(i) is snapshot.<loop>/<name>_kDist.data of group i, line(loop, time) the line of kinetic.data, header() the
    line written when that file is opened; the reference clears after writing both."""

    def __init__(self, groups, eval_rate=0, outputrate=0):
        self.groups = [dict(g) for g in groups]
        for g in self.groups:
            if int(g["nbins"]) < 1 or not g["emax"] > g["emin"]:
                raise ValueError("BIN %s: nBins = %d, emin = %g, emax = %g" % (g.get("name", "?"), g["nbins"], g["emin"], g["emax"]))
        self.nd = len(self.groups)
        self.emin = np.array([g["emin"] for g in self.groups], np.float64)
        self.emax = np.array([g["emax"] for g in self.groups], np.float64)
        self.nbins = np.array([g["nbins"] for g in self.groups], np.int32)
        self.offset = np.concatenate([[0], np.cumsum(self.nbins, dtype=np.int64)])
        self.eval_rate, self.outputrate = int(eval_rate), int(outputrate)
        self.clear()

    def species_dist(self, species_names):
        """mapS2D: the group of each species, or -1; the reference asserts that no species is claimed twice"""
        out = -np.ones(len(species_names), np.int32)
        for j, g in enumerate(self.groups):
            if g["species"] in species_names:
                i = list(species_names).index(g["species"])
                if out[i] != -1:
                    raise ValueError("species %s is claimed by two BINs" % g["species"])
                out[i] = j
        return out

    def filename(self, i):
        return "%s_kDist.data" % self.groups[i]["name"]

    def clear(self):
        self.cnt = np.zeros(int(self.offset[-1]))
        self.tallies = np.zeros((self.nd, 3))      # cntTotal, subCnt, supCnt
        self.sum = np.zeros(self.nd)
        self.min, self.max = np.full(self.nd, 1e300), np.zeros(self.nd)

    def add(self, counts, tallies, stats):
        stats = np.asarray(stats, np.float64).reshape(self.nd, 3)
        self.cnt += np.asarray(counts, np.float64).reshape(-1)
        self.tallies += np.asarray(tallies, np.float64).reshape(self.nd, 3)
        self.sum += stats[:, 0]
        self.min = np.where(stats[:, 1] < self.min, stats[:, 1], self.min)
        self.max = np.where(stats[:, 2] > self.max, stats[:, 2], self.max)

    def header(self):
        return "# loop  time(fs)   \n"

    def dist_text(self, i):
        ec = units_convert(1.0, None, "eV")
        delta = (self.emax[i] - self.emin[i]) / self.nbins[i]
        cnt = self.cnt[self.offset[i]:self.offset[i + 1]]
        with np.errstate(all="ignore"):
            pdf = cnt / (self.tallies[i, 0] * delta) / ec      # (an empty group: 0/0, printed as C prints it)
        lines = ["%-14s %14s %14s\n" % ("# Energy (eV)", "pdf (1/eV)", "cnt")]
        for j in range(int(self.nbins[i])):
            lines.append("%e %e %e\n" % (((j + 0.5) * delta + self.emin[i]) * ec, pdf[j], cnt[j]))
        return "".join(lines)

    def line(self, loop, time):
        """time as simulate->time holds it (internal units: the reference converts nothing here)"""
        ec = units_convert(1.0, None, "eV")
        row = ""
        for i in range(self.nd):
            total = self.tallies[i, 0]
            ave = self.sum[i] / total if total else 0.0
            row += "%*d" % (LOOP_WIDTH, int(loop)) + " %16.6f " % time
            row += "%12.6f %12.8f %12.8f %4.0f %4.0f %8.0f " % (ave * ec, self.min[i] * ec, self.max[i] * ec, self.tallies[i, 1], self.tallies[i, 2], total)
        return row + "\n"


def _c_float(fmt, x):
    """fmt % x as C's printf prints it on x86-64: the NaN of an invalid operation (0/0, 0 * inf) carries the sign bit -- "-nan"""
    return "-nan" if x != x else fmt % x


class CholAnalysis(object):
    """one cholAnalysis analysis (cholAnalysis.c): the histograms of the cholesterol ring-plane offsets dR1 and dR5.  rmin, rmax and
    delta in internal length units; nbins = lrint((rmax - rmin) / delta) and delta is formed anew as (rmax - rmin) / nbins, as the
    reference's _parms has them (nbins < 1, where the reference divides by zero, is refused).  add() takes one evaluation combined
    over the ranks (Martini*.chol_offsets: counts, stats = {sum, min, max} of dR1, then of dR5); evaluations accumulate until
    clear().  data_line(loop, time) is the line appended to dataFilename, distn_text() the file snapshot.<loop>/<filename>; the
    reference clears after writing both.  Both averages divide by the total of the first histogram, as the reference does."""

    def __init__(self, rmin, rmax, delta=0.1, filename="cholAnalysis.distn", data_filename="cholAnalysis.data", eval_rate=0, outputrate=0):
        self.rmin, self.rmax = float(rmin), float(rmax)
        q = (self.rmax - self.rmin) / float(delta) if float(delta) != 0.0 else float("nan")
        self.nbins = int(round(q)) if q == q and abs(q) < 2.0 ** 31 else 0      # lrint: to nearest, ties to even
        if self.nbins < 1:
            raise ValueError("cholAnalysis: rmin = %g, rmax = %g, delta = %g give %d bins" % (self.rmin, self.rmax, float(delta), self.nbins))
        self.delta = (self.rmax - self.rmin) / self.nbins
        self.filename, self.data_filename = filename, data_filename
        self.eval_rate, self.outputrate = int(eval_rate), int(outputrate)
        self.clear()

    def clear(self):
        self.cnt = np.zeros(2 * self.nbins, np.int64)
        self.sum = np.zeros(2)
        self.min, self.max = np.full(2, 1e300), np.full(2, -1e300)

    def add(self, counts, stats):
        stats = np.asarray(stats, np.float64).reshape(2, 3)
        self.cnt += np.asarray(counts, np.int64).reshape(2 * self.nbins)
        self.sum += stats[:, 0]
        self.min = np.where(stats[:, 1] < self.min, stats[:, 1], self.min)
        self.max = np.where(stats[:, 2] > self.max, stats[:, 2], self.max)

    def data_line(self, loop, time):
        """time as simulate->time holds it (internal units: the reference converts nothing here)"""
        lc = units_convert(1.0, None, "Angstrom")
        cnt1 = float(self.cnt[:self.nbins].sum())
        with np.errstate(all="ignore"):
            ave = self.sum / np.float64(cnt1)      # (no molecule: 0/0, printed as C prints it)
        vals = [time, self.min[0] * lc, self.max[0] * lc, ave[0] * lc, self.min[1] * lc, self.max[1] * lc, ave[1] * lc]
        return "%d " % int(loop) + " ".join(_c_float("%f", float(v)) for v in vals) + "\n"

    def distn_text(self):
        lc = units_convert(1.0, None, "Angstrom")
        cnt1, cnt3 = float(self.cnt[:self.nbins].sum()), float(self.cnt[self.nbins:].sum())
        lines = []
        with np.errstate(all="ignore"):
            w1, w3 = np.float64(1.0) / np.float64(cnt1 * self.delta), np.float64(1.0) / np.float64(cnt3 * self.delta)
            for i in range(self.nbins):
                r = self.rmin + (i + 0.5) * self.delta
                v = (r * lc, np.float64(self.cnt[i]) / lc * w1, np.float64(self.cnt[i + self.nbins]) / lc * w3)
                lines.append("".join(" " + _c_float("%e", float(x)) for x in v) + "\n")
        return "".join(lines)


def parse_kdist_output(text):
    """(energy[nbins] in eV, pdf[nbins] in 1/eV, cnt[nbins]) of a <name>_kDist.data file"""
    rows = np.array([[float(x) for x in ln.split()] for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]).reshape(-1, 3)
    return rows[:, 0], rows[:, 1], rows[:, 2]


def parse_kinetic_output(text):
    """one (loop[ngroup], time[ngroup], values[ngroup, 6] = {ave, min, max in eV, subCnt, supCnt, cntTotal}) per output line of
    kinetic.data (header lines skipped; a line of an analysis without groups is empty)"""
    out = []
    for ln in text.splitlines():
        if ln.startswith("#"):
            continue
        w = ln.split()
        assert len(w) % 8 == 0, ln
        v = np.array([float(x) for x in w], np.float64).reshape(-1, 8)
        out.append((v[:, 0].astype(np.int64), v[:, 1], v[:, 2:]))
    return out


class DynamicStructureFactor(object):
    """one DSF analysis (dsf.c).  m: the list of the `m` key as written -- every entry > 0 adds the wave vectors (0,0,m), (0,m,0),
    (m,0,0), in that order and as often as it is listed (addKvectors); kvec is their list, mmax the largest m.  add(loop, time, rho,
    count) takes one evaluation added over the ranks (Martini*.charge_density_modes(mmax): rho[3, mmax], the selected beads' count),
    divides by the count where that is positive and buffers one row; it returns the text of the rows it had to flush first (the
    buffer holds outputrate // eval_rate + 1 rows), "" otherwise.  output() is the text of the buffered rows and empties the buffer;
    header() the line written when the file is opened.  The time is written as the driver holds it (internal units)."""

    def __init__(self, m, species=None, eval_rate=1, outputrate=1, filename=None):
        if int(eval_rate) < 1 or int(outputrate) < 1:
            raise ValueError("eval_rate = %d, outputrate = %d: both must be at least 1" % (eval_rate, outputrate))
        self.m = [int(x) for x in m]
        if not self.m:
            raise ValueError("no m")
        self.species = species
        self.eval_rate, self.outputrate = int(eval_rate), int(outputrate)
        self.filename = filename or ("rho_k_%s.data" % species if species else "rho_k.data")
        self.kvec = [v for x in self.m if x > 0 for v in ((0, 0, x), (0, x, 0), (x, 0, 0))]
        self.mmax = max([x for x in self.m if x > 0] or [0])
        self.nbufmax = self.outputrate // self.eval_rate + 1
        self.rows = []

    def select(self, species_names):
        """the select array of Martini*.charge_density_modes: None without a species"""
        if self.species is None:
            return None
        if self.species not in list(species_names):
            raise ValueError("species %s is not a species of the system" % self.species)
        return np.array([int(n == self.species) for n in species_names], np.int32)

    def pick(self, rho):
        """the kvec columns out of rho[3, mmax] (axis 0 x, 1 y, 2 z; column m - 1)"""
        rho = np.asarray(rho, np.complex128).reshape(3, -1)
        return np.array([rho[0 if kx else (1 if ky else 2), kx + ky + kz - 1] for kx, ky, kz in self.kvec], np.complex128)

    def header(self):
        return "%-8s %16s" % ("#loop", "time") + "".join("%-30s" % ("    (%d,%d,%d)" % k) for k in self.kvec) + "\n"

    def add(self, loop, time, rho, count):
        flushed = self.output() if len(self.rows) >= self.nbufmax else ""
        z = self.pick(rho)
        if count > 0:
            z = z / float(count)
        self.rows.append((int(loop), float(time), z))
        return flushed

    def output(self):
        text = "".join("%8.8d %16.6f" % (loop, time) + "".join("   %13.6e %13.6e" % (v.real, v.imag) for v in z) + "\n" for loop, time, z in self.rows)
        self.rows = []
        return text


def parse_dsf_output(text):
    """(loop[nrow], time[nrow], rho complex128 [nrow, nk]) of a rho_k file (header lines skipped)"""
    rows = [ln.split() for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]
    loop = np.array([int(r[0]) for r in rows], np.int64)
    val = np.array([[float(x) for x in r[1:]] for r in rows], np.float64).reshape(len(rows), -1)
    return loop, val[:, 0], val[:, 1::2] + 1j * val[:, 2::2]


SSF_SIGNS = ((1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1))      # ssf_eval's ppp, ppm, pmp, pmm
SSF_FACT = (1.0, 0.5, 0.25)                                        # by the number of zero components: how often the four coincide


def expand_signs(n):
    """the signed triples of the vectors n[nv, 3] in ssf_eval's four combinations: [4 nv, 3] int32, vector after vector, +++ ++- +-+ +-- each"""
    n = np.asarray(n, np.int32).reshape(-1, 3)
    return (n[:, None, :] * np.array(SSF_SIGNS, np.int32)[None, :, :]).reshape(-1, 3)


def in_plane(nmax):
    """the wave vectors (n_x, n_y, 0), 0 <= n_x, n_y <= nmax without (0, 0, 0), n_x slowest, of a bilayer's undulation spectrum: [(nmax + 1)^2 - 1, 3]
    int32.  expand_signs gives the signed list for Martini*.structure_modes (every vector four times: its two in-plane signs, each twice)."""
    nmax = int(nmax)
    if nmax < 1:
        raise ValueError("nmax = %d: at least 1" % nmax)
    return np.array([(nx, ny, 0) for nx in range(nmax + 1) for ny in range(nmax + 1) if nx or ny], np.int32)


class StaticStructureFactor(object):
    """one SSF analysis (ssf.c) in an orthorhombic box h (the nine entries, internal length) with kmax a bare number in internal inverse
    length, as the reference reads it.  n[nv, 3]: ssf_kvector's list in its order -- n_a runs over [0, (int)(kmax L_a / 2 pi)), n_x slowest; the
    first n_z with k^2 >= kmax^2 ends its n_z loop; a vector is kept if k^2 < kmax^2 / 2 and it is not (0,0,0).  kvec[4 nv, 3]: the signed
    triples Martini*.structure_modes takes (expand_signs).  Sk(rho) is fact[zeros] times the sum of |rho|^2 over a vector's four combinations,
    rho added over the ranks; lines(rho) the text ssf_eval prints.  (The reference's evaluation ends the program; the deck word SSF stays
    unsupported.)"""
    in_plane = staticmethod(in_plane)

    def __init__(self, h, kmax, species=None):
        h = np.asarray(h, np.float64).reshape(3, 3)
        if np.abs(h - np.diag(np.diag(h))).max() > 1e-10 or not np.all(np.diag(h) > 0.0):
            raise ValueError("only orthorhombic boxes are supported")
        self.kmax, self.species = float(kmax), species
        self.kbasis = 2.0 * np.pi / np.diag(h)      # RECIP_LATTICEVECTORS of an orthorhombic box: one component each
        # kDirectionMax: 1 / |b_a| where the basis is orthogonal
        nmax = [int(self.kmax * (1.0 / np.sqrt(b * b))) for b in self.kbasis]
        kmax2, keep = self.kmax * self.kmax, []
        for nx in range(nmax[0]):
            for ny in range(nmax[1]):
                for nz in range(nmax[2]):
                    if self._k2((nx, ny, nz)) >= kmax2:
                        break
                    if (nx or ny or nz) and self._k2((nx, ny, nz)) < 0.5 * kmax2:
                        keep.append((nx, ny, nz))
        self.n = np.array(keep, np.int32).reshape(-1, 3)
        self.kvec = expand_signs(self.n)
        self.fact = np.array([SSF_FACT[int((v == 0).sum())] for v in self.n], np.float64)

    def _k(self, n):
        return tuple(float(n[a]) * self.kbasis[a] for a in range(3))

    def _k2(self, n):
        kx, ky, kz = self._k(n)
        return kx * kx + ky * ky + kz * kz

    def select(self, species_names):
        """the select array of Martini*.structure_modes: None without a species"""
        if self.species is None:
            return None
        if self.species not in list(species_names):
            raise ValueError("species %s is not a species of the system" % self.species)
        return np.array([int(s == self.species) for s in species_names], np.int32)

    def Sk(self, rho):
        """S_k[nv] from rho[4 nv] (Martini*.structure_modes(self.kvec), added over the ranks)"""
        rho = np.asarray(rho, np.complex128).reshape(-1)
        if len(rho) != 4 * len(self.n):
            raise ValueError("%d values of rho for %d wave vectors in four sign combinations" % (len(rho), len(self.n)))
        p = rho.reshape(-1, 4)
        return self.fact * (p.real * p.real + p.imag * p.imag).sum(axis=1)

    def lines(self, rho):
        """ssf_eval's output: one line "k^2 k_x k_y k_z S_k" per wave vector"""
        return "".join("%f %f %f %f %e\n" % ((self._k2(v),) + self._k(v) + (sk,)) for v, sk in zip(self.n, self.Sk(rho)))


SUBSET_RECORD = np.dtype([("id", "<u8"), ("pinfo", "<u4"), ("r", "<f4", (3,))])      # a binaryCharmm record: 24 bytes


def pinfo_field_size(ngroups, nspecies, ntypes):
    """bytes of the pinfo field that holds pinfoMaxIndex = ngroups * nspecies * ntypes (pinfo.c:148-151); subsetWriteBinaryCharmm
    asserts that 4 are enough, and here more is a ValueError"""
    top, nbytes = int(ngroups) * int(nspecies) * int(ntypes), 1
    while top >= 256 ** nbytes:
        nbytes += 1
    if nbytes > 4:
        raise ValueError("%d groups, %d species and %d types need a pinfo field of %d bytes, more than 4" % (ngroups, nspecies, ntypes, nbytes))
    return nbytes


def _unique(names):
    """(the distinct names in order, every entry's index among them): a repeated name has its first occurrence's index"""
    uniq = []
    index = []
    for n in names:
        if n not in uniq:
            uniq.append(n)
        index.append(uniq.index(n))
    return uniq, index


class SubsetWrite(object):
    """one subsetWrite analysis with format = binaryCharmm (subsetWrite.c).  group_names / species_names: the system's, in index
    order (a system without groups has the one group "group"); species_types: the species' type names, ATOM for every Martini
    species.  group_term / species_term are pinfoEncode (pinfo.c:119-126) split in two: pinfo = group_term[group] +
    species_term[species].  The filter's bounds are in internal units; None is the reference's default, -+ the longest box edge
    through its "%e" for x, y, z and -+ DBL_MAX likewise for the velocities, which default() forms for a box.
    filter() is the keyword dict of Martini*.subset_records; header(...) the file's header, file_bytes(...) header and records."""

    def __init__(self, group_names, species_names, species_types=None, filename="subset", length_unit="Ang", modulus=1, odd=0, idmin=0, idmax=2 ** 64 - 1,
                 id_list=None, species=None, rmin=None, rmax=None, vmin=None, vmax=None, outputrate=0, h=None):
        if int(modulus) < 1:
            raise ValueError("modulus = %d, it must be at least 1" % modulus)
        self.group_names = list(group_names) or ["group"]
        self.species_names = list(species_names)
        self.species_types = list(species_types) if species_types is not None else ["ATOM"] * len(self.species_names)
        for n in species or []:
            if n not in self.species_names:
                raise ValueError("species %s is not a species of the system" % n)
        self.groups, gmap = _unique(self.group_names)
        self.species_list, smap = _unique(self.species_names)
        self.types, tmap = _unique(self.species_types)
        self.pinfo_bytes = pinfo_field_size(len(self.groups), len(self.species_list), len(self.types))
        ng, ns = len(self.groups), len(self.species_list)
        self.group_term = np.array(gmap, np.uint32)
        self.species_term = np.array([(smap[i] + tmap[i]) * ng + tmap[i] * ns for i in range(len(self.species_names))], np.uint32)
        self.filename, self.length_unit, self.outputrate = filename, length_unit, int(outputrate)
        self.modulus, self.odd, self.idmin, self.idmax = int(modulus), int(odd), int(idmin), int(idmax)
        self.id_list = None if id_list is None else np.sort(np.asarray(id_list, np.uint64).reshape(-1))
        self.species = None if not species else list(species)
        big, vbig = self.default(h) if h is not None else (float("inf"), float("inf"))
        self.rmin = [-big] * 3 if rmin is None else [float(x) for x in rmin]
        self.rmax = [big] * 3 if rmax is None else [float(x) for x in rmax]
        self.vmin = [-vbig] * 3 if vmin is None else [float(x) for x in vmin]
        self.vmax = [vbig] * 3 if vmax is None else [float(x) for x in vmax]
        self.cL = units_convert(1.0, None, length_unit)

    @staticmethod
    def default(h):
        """(the default |bound| of x, y, z, that of the velocities) in internal units for the box h[9] (subsetWrite.c:119-139)"""
        h = np.asarray(h, np.float64).reshape(-1)
        big = units_convert(float("%e" % units_convert(float(max(h[0], h[4], h[8])), None, "l")), "l", None)
        vbig = units_convert(float("%e" % np.finfo(np.float64).max), "l/t", None)
        return big, vbig

    def filter(self):
        sel = None if self.species is None else [int(n in self.species) for n in self.species_names]
        return dict(idmin=self.idmin, idmax=self.idmax, modulus=self.modulus, odd=self.odd, rmin=self.rmin, rmax=self.rmax, vmin=self.vmin, vmax=self.vmax,
                    species=sel, id_list=self.id_list, group_term=self.group_term, species_term=self.species_term, cL=self.cL)

    def parms_info(self):
        """_parms_info (subsetWrite.c:149-166): the echo of the filter"""
        lc, vc = units_convert(1.0, None, "Angstrom"), units_convert(1.0, None, "Angstrom/fs")
        t = "idmin = %d; idmax = %d; modulus = %d; odd = %d;\n" % (self.idmin, self.idmax, self.modulus, self.odd)
        for a, n in enumerate("xyz"):
            t += "%smin = %f Ang; %smax = %f Ang;\n" % (n, self.rmin[a] * lc, n, self.rmax[a] * lc)
        for a, n in enumerate("xyz"):
            t += "v%smin = %f Ang/fs; v%smax = %f Ang/fs;\n" % (n, self.vmin[a] * vc, n, self.vmax[a] * vc)
        return t

    def misc_info(self):
        """the pieces of subsetWriteBinaryCharmm's PioSet(file, "misc_info", ...) calls in their order (subsetWrite.c:465-481), joined by one blank"""
        pieces = ["random = NONE;\n", "nrandomFieldSize = 0;\n", "types ="] + self.types + [";\n", "groups ="] + self.groups + [";\n", "species ="]
        return " ".join(pieces + self.species_list + [";\n", self.parms_info()])

    def header(self, nrecord, loop, time, h, version="", create_time=None):
        """write_fileheader (io.c:352-404) for `nrecord` records: time and h in internal units"""
        h = np.asarray(h, np.float64).reshape(-1) * units_convert(1.0, None, "l")
        stamp = create_time or _time.strftime("%Y-%m-%d-%H:%M:%S", _time.localtime())
        key = int(np.frombuffer(b"1234", "<i4")[0])
        u = self.length_unit
        t = "subset FILEHEADER {type=MULTILINE; datatype=FIXRECORDBINARY; checksum=NONE; create_time=%s; run_id=0x%08x;\n" % (stamp, 0)
        t += "code_version=%s; srcpath=libddcmi;\n" % version
        t += "loop=%d; time=%f fs;\n" % (loop, units_convert(time, None, "t"))
        t += "nfiles=1; nrecord=%d; lrec=%d; nfields=5; endian_key=%d;\n" % (nrecord, SUBSET_RECORD.itemsize, key)
        t += "field_names=id pinfo rx ry  rz;\n"
        t += "field_types= u8 u4 f4 f4 f4;\n"
        t += "field_units=1 1 %s %s %s;\n" % (u, u, u)
        t += "reducedcorner=%21.14f %21.14f %21.14f;\n" % (-0.5, -0.5, -0.5)
        t += "h=%21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f Ang;\n" % tuple(h)
        t += self.misc_info() + "\n"
        return t + "}\n \n\n"

    def file_bytes(self, records, loop, time, h, version="", create_time=None):
        records = np.ascontiguousarray(records, SUBSET_RECORD)
        return self.header(len(records), loop, time, h, version, create_time).encode() + records.tobytes()

    def write(self, directory, records, loop, time, h, version=""):
        """<directory>/<filename>#000000, under a temporary name first; returns the path"""
        path = os.path.join(directory, self.filename + "#000000")
        with open(path + ".tmp", "wb") as f:
            f.write(self.file_bytes(records, loop, time, h, version))
        os.rename(path + ".tmp", path)
        return path


def read_subset(path):
    """(header dict, records) of a binaryCharmm subset file: every `key=value;` / `key = value;` of the FILEHEADER block as a string
    (nrecord, lrec, nfields, nfiles, loop as int; groups, species, types, field_names, field_types, field_units as lists; h as nine
    floats in Angstrom), and the structured array of SUBSET_RECORD behind it"""
    raw = open(path, "rb").read()
    end = raw.index(b"\n}\n")
    text = raw[:end].decode()
    off = end + 1 + len(b"}\n \n\n")      # write_fileheader closes the block and adds " \n\n"
    if raw[end + 1:off] != b"}\n \n\n":
        raise ValueError("%s: the header does not end as write_fileheader ends it" % path)
    name, rest = text.split(" FILEHEADER {", 1)
    hdr = {"name": name.strip()}
    for item in rest.split(";"):
        if "=" not in item:
            continue
        k, v = item.split("=", 1)
        hdr[k.strip()] = v.strip()
    for k in ("nrecord", "lrec", "nfields", "nfiles", "loop", "endian_key"):
        hdr[k] = int(hdr[k])
    for k in ("groups", "species", "types", "field_names", "field_types", "field_units"):
        hdr[k] = hdr.get(k, "").split()
    hdr["h"] = [float(x) for x in hdr["h"].split()[:9]]
    if hdr["lrec"] != SUBSET_RECORD.itemsize or hdr["datatype"] != "FIXRECORDBINARY":
        raise ValueError("%s: lrec = %d, datatype = %s: not a binaryCharmm subset file" % (path, hdr["lrec"], hdr["datatype"]))
    if len(raw) - off != hdr["nrecord"] * hdr["lrec"]:
        raise ValueError("%s: %d bytes behind the header, nrecord * lrec = %d" % (path, len(raw) - off, hdr["nrecord"] * hdr["lrec"]))
    return hdr, np.frombuffer(raw, SUBSET_RECORD, count=hdr["nrecord"], offset=off).copy()


CG_RECORD = np.dtype([("label", "<i8"), ("species", "<i4"), ("pad", "<i4"), ("n", "<f8"), ("mass", "<f8"), ("K", "<f8", (3,)), ("p", "<f8", (3,))])      # struct ddcmi_cg_record
_CG_SUMS = ("n", "mass", "K", "p")
_CG_NAMES = {1: "checksum label species_index number_particles mass  Kx Ky Kz U virial px py pz",
             2: "checksum label species_index number_particles mass  Kx Ky Kz U virial px py pz vir_xx vir_yy vir_zz vir_xy vir_xz vir_yz"}
_CG_UNITS = {1: "1 1 1 1 amu eV eV eV eV eV amu*Angstrom/fs amu*Angstrom/fs amu*Angstrom/fs",
             2: "1 1 1 1 amu eV eV eV eV eV amu*Angstrom/fs amu*Angstrom/fs amu*Angstrom/fs eV eV eV eV eV eV"}


def b_field_size(top):
    """bFieldSize: the fewest whole bytes that hold the unsigned integer `top` (at least one)"""
    nbytes = 1
    while int(top) >> (8 * nbytes):
        nbytes += 1
    return nbytes


def merge_cg_records(blocks):
    """the blocks of CG_RECORD (each ascending in (label, species)) merged in the order given: one entry per key in ascending order, an entry
    of several blocks the sum of theirs, added block after block"""
    out = np.zeros(0, CG_RECORD)
    for blk in blocks:
        blk = np.asarray(blk, CG_RECORD)
        if len(blk) == 0:
            continue
        if len(out) == 0:
            out = blk.copy()
            continue
        both = np.concatenate([out, blk])
        order = np.lexsort((np.concatenate([np.zeros(len(out), np.int8), np.ones(len(blk), np.int8)]), both["species"], both["label"]))      # stable: out's entry first
        both = both[order]
        first = np.ones(len(both), bool)
        first[1:] = (both["label"][1:] != both["label"][:-1]) | (both["species"][1:] != both["species"][:-1])
        merged = both[first].copy()
        dup = np.flatnonzero(~first)      # a key of both: its second entry (blk's) sits right behind its first (out's)
        at = np.cumsum(first)[dup] - 1
        for f in _CG_SUMS:
            merged[f][at] = both[f][dup - 1] + both[f][dup]
        out = merged
    return out


class CoarseGrain(object):
    """one COARSEGRAIN analysis (coarsegrain.c).  add(records) takes one evaluation -- the records of Martini.coarsegrain, or a list of
    the ranks' records, merged in rank order -- into the table keyed by (label, species) and counts nsteps; clear() empties both;
    file_bytes(...) is the cgrid file of the table: header(...) and one record per entry in ascending (label, species): a u4 CRC-32 of the
    bytes behind it (native byte order), label and species_index as unsigned integers of b_field_size(nx ny nz - 1) and
    b_field_size(nspecies - 1) bytes, most significant byte first, and the f4 fields (float)(sum * convert * (1.0 / nsteps)) multiplied
    left to right in double; U, virial and the virial tensor are 0.0f.  output_mode 1: 13 fields, 2: 19 fields."""

    def __init__(self, nx, ny, nz, species_names, filename="cgrid", output_mode=2, smear_radius=0.0, smear_method="impulse", eval_rate=0, outputrate=0):
        if min(int(nx), int(ny), int(nz)) < 1:
            raise ValueError("nx = %d, ny = %d, nz = %d: each must be at least 1" % (nx, ny, nz))
        if int(output_mode) not in (1, 2):
            raise ValueError("outputMode = %d: 1 or 2 (3 divides by the species' charge and is not supported)" % output_mode)
        self.nx, self.ny, self.nz = int(nx), int(ny), int(nz)
        self.species_names = list(species_names)
        self.filename, self.output_mode = filename, int(output_mode)
        self.smear_radius, self.smear_string = float(smear_radius), str(smear_method)
        self.smear_method = "hat" if self.smear_string.lower() == "hat" else "impulse"
        self.eval_rate, self.outputrate = int(eval_rate), int(outputrate)
        self.label_bytes = b_field_size(self.nx * self.ny * self.nz - 1)
        self.species_bytes = b_field_size(max(len(self.species_names), 1) - 1)
        self.nf4 = 10 if self.output_mode == 1 else 16      # the f4 fields behind checksum, label and species_index
        self.lrec = 4 + self.label_bytes + self.species_bytes + 4 * self.nf4
        self.clear()

    def args(self):
        """the arguments of Martini*.coarsegrain"""
        return dict(nx=self.nx, ny=self.ny, nz=self.nz, smear_radius=self.smear_radius, smear_method=self.smear_method)

    def clear(self):
        self.table, self.nsteps = np.zeros(0, CG_RECORD), 0

    def add(self, records):
        blocks = [records] if isinstance(records, np.ndarray) else list(records)
        self.table = merge_cg_records([self.table] + blocks)
        self.nsteps += 1

    def misc_info(self):
        t = "nx = %d; ny = %d; nz=%d; smearRadius=%f; smearMethod=%s;\n       ouputrate=%d; eval_rate=%d; species=" % (
            self.nx, self.ny, self.nz, units_convert(self.smear_radius, None, "l"), self.smear_string, self.outputrate, self.eval_rate)
        return t + "".join(" " + n for n in self.species_names) + ";" + "\n  nSamples = %d;" % self.nsteps

    def header(self, nrecord, loop, time, h, version="", create_time=None):
        """write_fileheader (io.c:352-404) for class cgrid: time and h in internal units"""
        h = np.asarray(h, np.float64).reshape(-1) * units_convert(1.0, None, "l")
        stamp = create_time or _time.strftime("%Y-%m-%d-%H:%M:%S", _time.localtime())
        key = int(np.frombuffer(b"1234", "<i4")[0])
        t = "cgrid FILEHEADER {type=MULTILINE; datatype=FIXRECORDBINARY; checksum=CRC32; create_time=%s; run_id=0x%08x;\n" % (stamp, 0)
        t += "code_version=%s; srcpath=libddcmi;\n" % version
        t += "loop=%d; time=%f fs;\n" % (loop, units_convert(time, None, "t"))
        t += "nfiles=1; nrecord=%d; lrec=%d; nfields=%d; endian_key=%d;\n" % (nrecord, self.lrec, self.nf4 + 3, key)
        t += "field_names=%s;\n" % _CG_NAMES[self.output_mode]
        t += "field_types=u4 b%d b%d%s;\n" % (self.label_bytes, self.species_bytes, " f4" * self.nf4)
        t += "field_units=%s;\n" % _CG_UNITS[self.output_mode]
        t += "reducedcorner=%21.14f %21.14f %21.14f;\n" % (-0.5, -0.5, -0.5)
        t += "h=%21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f\n  %21.14f %21.14f %21.14f Ang;\n" % tuple(h)
        t += self.misc_info() + "\n"
        return t + "}\n \n\n"

    def fields(self):
        """the table's f4 fields [entry, nf4], in the file's order"""
        tab, inv = self.table, 1.0 / (self.nsteps * 1.0)
        mc, ec, pc = units_convert(1.0, None, "amu"), units_convert(1.0, None, "eV"), units_convert(1.0, None, "amu*Angstrom/fs")
        v = np.zeros((len(tab), self.nf4), np.float32)
        v[:, 0] = (tab["n"] * inv).astype(np.float32)
        v[:, 1] = (tab["mass"] * mc * inv).astype(np.float32)
        v[:, 2:5] = (tab["K"] * ec * inv).astype(np.float32)
        v[:, 7:10] = (tab["p"] * pc * inv).astype(np.float32)      # [5], [6]: U, virial; [10:]: the virial tensor
        return v

    def record_bytes(self):
        tab, lb, sb = self.table, self.label_bytes, self.species_bytes
        rec = np.zeros((len(tab), self.lrec), np.uint8)
        for k in range(lb):
            rec[:, 4 + k] = (tab["label"].astype(np.uint64) >> np.uint64(8 * (lb - 1 - k))).astype(np.uint8)
        for k in range(sb):
            rec[:, 4 + lb + k] = (tab["species"].astype(np.uint64) >> np.uint64(8 * (sb - 1 - k))).astype(np.uint8)
        rec[:, 4 + lb + sb:] = np.ascontiguousarray(self.fields()).view(np.uint8).reshape(len(tab), 4 * self.nf4)
        crc = np.array([zlib.crc32(row[4:].tobytes()) & 0xffffffff for row in rec], np.uint32)
        rec[:, :4] = crc.view(np.uint8).reshape(len(tab), 4)
        return rec.tobytes()

    def file_bytes(self, loop, time, h, version="", create_time=None):
        if self.nsteps < 1:
            raise ValueError("no evaluation since the last clear: nSamples = 0")
        return self.header(len(self.table), loop, time, h, version, create_time).encode() + self.record_bytes()

    def write(self, directory, loop, time, h, version=""):
        """<directory>/<filename>#000000, under a temporary name first; clears; returns the path"""
        path = os.path.join(directory, self.filename + "#000000")
        with open(path + ".tmp", "wb") as f:
            f.write(self.file_bytes(loop, time, h, version))
        os.rename(path + ".tmp", path)
        self.clear()
        return path


def read_cgrid(path):
    """(header dict, records) of a cgrid file: the header's keys as read_subset gives them, with nSamples, nx, ny, nz as int, and a
    structured array {checksum u4, label u8, species_index u8, then the f4 fields by their names}; a record whose CRC-32 does not match its
    checksum field is a ValueError"""
    raw = open(path, "rb").read()
    end = raw.index(b"\n}\n")
    text = raw[:end].decode()
    off = end + 1 + len(b"}\n \n\n")
    if raw[end + 1:off] != b"}\n \n\n":
        raise ValueError("%s: the header does not end as write_fileheader ends it" % path)
    name, rest = text.split(" FILEHEADER {", 1)
    hdr = {"name": name.strip()}
    for item in rest.split(";"):
        if "=" not in item:
            continue
        k, v = item.split("=", 1)
        hdr[k.strip()] = v.strip()
    for k in ("nrecord", "lrec", "nfields", "nfiles", "loop", "endian_key", "nSamples", "nx", "ny", "nz"):
        hdr[k] = int(hdr[k])
    for k in ("species", "field_names", "field_types", "field_units"):
        hdr[k] = hdr.get(k, "").split()
    hdr["h"] = [float(x) for x in hdr["h"].split()[:9]]
    names, types = hdr["field_names"], hdr["field_types"]
    if hdr["name"] != "cgrid" or hdr["datatype"] != "FIXRECORDBINARY" or hdr["checksum"] != "CRC32" or len(names) != hdr["nfields"] or len(types) != hdr["nfields"]:
        raise ValueError("%s: not a cgrid file" % path)
    if types[0] != "u4" or types[1][0] != "b" or types[2][0] != "b" or any(t != "f4" for t in types[3:]):
        raise ValueError("%s: field_types = %s" % (path, " ".join(types)))
    lb, sb = int(types[1][1:]), int(types[2][1:])
    lrec, nrec = hdr["lrec"], hdr["nrecord"]
    if lrec != 4 + lb + sb + 4 * (len(types) - 3):
        raise ValueError("%s: lrec = %d does not fit field_types = %s" % (path, lrec, " ".join(types)))
    if len(raw) - off != nrec * lrec:
        raise ValueError("%s: %d bytes behind the header, nrecord * lrec = %d" % (path, len(raw) - off, nrec * lrec))
    body = np.frombuffer(raw, np.uint8, count=nrec * lrec, offset=off).reshape(nrec, lrec)
    out = np.zeros(nrec, np.dtype([("checksum", "<u4"), ("label", "<u8"), ("species_index", "<u8")] + [(n, "<f4") for n in names[3:]]))
    out["checksum"] = np.ascontiguousarray(body[:, :4]).view(np.uint32).reshape(nrec)
    for k in range(lb):
        out["label"] = (out["label"] << np.uint64(8)) | body[:, 4 + k].astype(np.uint64)
    for k in range(sb):
        out["species_index"] = (out["species_index"] << np.uint64(8)) | body[:, 4 + lb + k].astype(np.uint64)
    f4 = np.ascontiguousarray(body[:, 4 + lb + sb:]).view(np.float32).reshape(nrec, len(names) - 3)
    for q, n in enumerate(names[3:]):
        out[n] = f4[:, q]
    for k in range(nrec):
        crc = zlib.crc32(body[k, 4:].tobytes()) & 0xffffffff
        if crc != int(out["checksum"][k]):
            raise ValueError("%s: record %d: checksum %08x, CRC-32 of its bytes %08x" % (path, k, int(out["checksum"][k]), crc))
    return hdr, out


class ForceAverage(object):
    """ANALYSIS type FORCE_AVERAGE (forceAverage.c): the time average of the force, velocity or position of the beads with the listed
    gids over a window of samples, one text line per window.  The running sums stay on the device (Martini*.track_set / track_accumulate /
    track_read); this class counts the samples, applies the reference's gate and formats the file's texts.  Internal units: the
    reference's conversions are commented out."""

    def __init__(self, gids, data_type="force", eval_rate=1, outputrate=1):
        self.gids = [int(g) for g in np.asarray(gids, dtype=np.uint64).reshape(-1)]
        self.data_type = data_type.lower()
        if self.data_type not in ("force", "velocity", "position"):
            raise ValueError("data_type = %s is none of force, velocity, position" % data_type)      # the reference's exit(19)
        self.eval_rate, self.outputrate = int(eval_rate), int(outputrate)
        if self.eval_rate < 1:
            raise ValueError("eval_rate = %d, it must be at least 1" % self.eval_rate)
        self.nsnap = 0
        self.m = None

    def header(self):
        return "# loop  time  " + "".join("%d  " % g for g in self.gids) + "\n"

    def sample(self, m):
        """forceAverage_eval on a MartiniHIP, a MartiniRank or a MartiniGroup: the first sample of the object hands it the list"""
        if self.m is not m:
            m.track_set(self.gids)
            self.m = m
        m.track_accumulate(self.data_type)
        self.nsnap += 1

    def clear(self):
        """forceAverage_clear: the sums on the device and the sample count"""
        if self.m is not None:
            self.m.track_read(reset=True)
        self.nsnap = 0

    def text(self, loop, time, total, hits):
        """the line of a window of self.nsnap samples with the sums total[n, 3]; every gid must have been found once per sample"""
        for g, h in zip(self.gids, np.asarray(hits).reshape(-1)):
            if int(h) != self.nsnap:
                raise RuntimeError("gid %d was found %d times in %d evaluations" % (g, int(h), self.nsnap))
        t = np.asarray(total, dtype=np.float64).reshape(-1, 3)
        body = "".join(" %12.7f %12.7f %12.7f " % tuple(float(x) / float(self.nsnap) for x in row) for row in t)
        return "%012d" % int(loop) + " %10.6f " % float(time) + body + "\n"

    def line(self, loop, time):
        """forceAverage_output: None while nSnapSum * eval_rate < outputrate (nothing is cleared); otherwise the line, and the window is
        cleared"""
        if self.nsnap * self.eval_rate < self.outputrate:
            return None
        total, hits = self.m.track_read() if self.m is not None else (np.zeros((len(self.gids), 3)), np.zeros(len(self.gids), np.int64))
        out = self.text(loop, time, total, hits)
        self.clear()
        return out

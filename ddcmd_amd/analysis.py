"""ANALYSIS type PAIRCORRELATION on the host side: accumulation of the device's pair counts into g(r) and the output file, as
paircorrelation_eval_geom / paircorrelation_output (paircorrelation.c) do.  The counting itself is ddcmi_pair_correlation
(Martini*.pair_correlation); nothing here searches pairs."""
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

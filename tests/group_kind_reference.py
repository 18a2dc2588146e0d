"""The velocity updates of the GROUP kinds FROZEN, FIXEDVELOCITY and QUENCH on top of tests/integrator_reference.py's
NGLFReference (by import and subclass), the state carried in numpy.longdouble -- written from nglf.c:74-108 and the formulas of
frozen.c, fixedVelocity.c and quench.c, not from the device code.  With a = (dt/2)/m and f the force the call sees, at
FRONT and at BACK:

    FROZEN          the bead does not drift and its velocity never changes (saved and zeroed at FRONT, put back at BACK)
    FIXEDVELOCITY   v = the group's vector where it has one; else nothing: the bead coasts
    QUENCH          per component: if (v f < 0) v = 0; then v += a f          (a product, strict <)

KindReference(setup) drives itself with the restraint forces of tests/restraint_systems.reference at its own positions;
`decisions` records, for every QUENCH bead, component and half kick, whether the component was zeroed, and `margin` the smallest
min(|v| / vscale, |f| / fscale) over the decisions whose product is not exactly zero (the scales: the largest speed and force of the
QUENCH beads at the first decision): the systems are chosen so that it stays far above the roundings (1e-13 of the scales after 40
steps), so that the device decides as the reference does."""
import numpy as np

import restraint_systems as R
from integrator_reference import NGLFReference

LD = np.longdouble
FROZEN, FIXEDVELOCITY, QUENCH = 4, 5, 6


class KindReference(NGLFReference):
    def __init__(self, s, dtype=LD, forces=True):
        NGLFReference.__init__(self, s)
        self.s, self.dtype = s, dtype
        self.r, self.v, self.m = self.r.astype(dtype), self.v.astype(dtype), self.m.astype(dtype)
        self.dt = dtype(self.dt)
        k = self.kind[self.group]
        self.frozen, self.fixed, self.quench = k == FROZEN, k == FIXEDVELOCITY, k == QUENCH
        self.new = self.frozen | self.fixed | self.quench
        vset = getattr(s, "group_vset", None)
        self.vset = np.zeros(self.ngroup, int) if vset is None else np.asarray(vset).astype(int)
        self.gv = np.zeros((self.ngroup, 3), dtype) if getattr(s, "group_v", None) is None else np.asarray(s.group_v, dtype).reshape(self.ngroup, 3)
        self.decisions, self.margin, self.vscale, self.fscale = [], np.inf, None, None
        self.box = R.box_of(s)
        self.with_forces = forces and int(getattr(s, "nrest", 0)) > 0
        self.f = self.forces()

    def forces(self):
        if not self.with_forces:
            return np.zeros((3, self.n), self.dtype)
        return R.reference(self.s, self.r.T, self.box, self.s.pbc)["F"].T.astype(self.dtype)

    def _update(self, v, f, sel):
        """velocityUpdate of the beads sel (a boolean mask) from the velocities v [3, nsel]: the new velocities"""
        v = v.copy()
        a = (self.dt / 2 / self.m[sel])
        gr = self.group[sel]
        q, x = self.quench[sel], self.fixed[sel] & (self.vset[gr] != 0)
        if q.any():
            # the predicate is quench.c's: a product of two doubles (it may underflow to zero), strict <
            with np.errstate(under="ignore"):
                prod = v[:, q].astype(np.float64) * f[:, q].astype(np.float64)
            zero = prod < 0
            nz = prod != 0
            if nz.any():
                # the sign of a product is safe when neither factor is within its error of zero: both measured against the scales
                # set at the start (vscale, fscale: the largest speed and force of the QUENCH beads then)
                if self.vscale is None:
                    self.vscale, self.fscale = float(np.abs(v[:, q]).max()), float(np.abs(f[:, q]).max())
                m = np.minimum(np.abs(v[:, q][nz]) / self.vscale, np.abs(f[:, q][nz]) / self.fscale)
                self.margin = min(self.margin, float(m.min()))
            self.decisions.append(zero.copy())
            vq = np.where(zero, 0, v[:, q])
            v[:, q] = vq + a[q] * f[:, q]
        if x.any():
            v[:, x] = self.gv[gr[x]].T
        return v

    def front(self, f=None):
        f = self.f if f is None else np.asarray(f, self.dtype)
        sel = self.new
        v0, r0 = self.v[:, sel].copy(), self.r[:, sel].copy()
        NGLFReference.front(self, f.astype(np.float64))          # the other kinds; the beads of the three kinds are redone below
        v = self._update(v0, f[:, sel], sel)
        self.v[:, sel] = v
        self.r[:, sel] = r0 + self.dt * np.where(self.frozen[sel], 0, v)

    def back(self, f=None):
        f = self.f if f is None else np.asarray(f, self.dtype)
        sel = self.new
        v0 = self.v[:, sel].copy()
        self.v[:, sel] = 0                                       # (keeps the parent's kick of these beads out of its sums' way)
        NGLFReference.back(self, np.where(sel, 0, f).astype(np.float64))
        self.v[:, sel] = self._update(v0, f[:, sel], sel)
        from integrator_reference import class_sums
        tot = class_sums(np.zeros(self.n, int), 1, self.m, self.v)[0]
        self.rk, self.tion = float(tot[0]), tot[1:7].astype(np.float64)

    def step(self, nsteps=1):
        for _ in range(nsteps):
            self.front()
            self.f = self.forces()
            self.back()
        return self.r.T, self.v.T

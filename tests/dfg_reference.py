"""gamma_scheme full_staggered restated literally on the doubly fine grid (test infrastructure only).

The reference (F = src/fibergen.cpp) evaluates every material law of a full_staggered / half_staggered run on a grid of
2nx x 2ny x 2nz: the strain is prolonged with a shift per component (prolongate_to_dfg F:14216-14270), PK1 is evaluated
per fine cell with the fine phase fractions, and the result is restricted back as the mean of 8 cells shifted the other way
(restrict_from_dfg F:14273-14335); calcStress F:18134-18348, calcMeanStress / calcMeanEnergy F:17765-17811.  Everything
else (Green operator, reference medium, "phi") stays on the coarse grid.

`DfgMixin` overrides pk1, mean_stress and mean_energy of the oracles with exactly that chain; `staggered_fractions` and
`pk1_fractions` are the coarse form the library runs (each component group reads its own 8-cell mean of the fine fractions).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from oracle.ls_oracle import LSOracle, energy_voigt, pk1_voigt
from oracle.viscosity_oracle import ViscosityOracle

# per component 11, 22, 33, 23, 13, 12 (F:14231-14233; restriction: the negatives, F:14289-14291)
SHIFTS = [(0, 0, 0), (0, 0, 0), (0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]
GROUP_SHIFTS = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]   # normal, 23, 13, 12


def prolongate_component(c, shift):
    """dest[i, j, k] = src[((i + si) % fnx) // 2, ...]  F:14243-14266"""
    nx, ny, nz = c.shape
    idx = [((np.arange(2 * n) + s) % (2 * n)) // 2 for n, s in zip((nx, ny, nz), shift)]
    return c[np.ix_(*idx)]


def restrict_component(f, shift):
    """dest[i, j, k] = 0.125 * sum of the 8 cells (2i - si + a, ...)  F:14303-14331, in the reference's order"""
    fnx, fny, fnz = f.shape
    si, sj, sk = (-s for s in shift)
    i0 = (2 * np.arange(fnx // 2) + si) % fnx
    i1 = (2 * np.arange(fnx // 2) + 1 + si) % fnx
    j0 = (2 * np.arange(fny // 2) + sj) % fny
    j1 = (2 * np.arange(fny // 2) + 1 + sj) % fny
    k0 = (2 * np.arange(fnz // 2) + sk) % fnz
    k1 = (2 * np.arange(fnz // 2) + 1 + sk) % fnz
    g = lambda a, b, c: f[np.ix_(a, b, c)]  # noqa: E731
    return 0.125 * (g(i0, j0, k0) + g(i1, j0, k0) + g(i0, j1, k0) + g(i1, j1, k0) + g(i0, j0, k1) + g(i1, j0, k1)
                    + g(i0, j1, k1) + g(i1, j1, k1))


def prolongate_to_dfg(c):
    return np.stack([prolongate_component(c[g], SHIFTS[g]) for g in range(c.shape[0])])


def restrict_from_dfg(f):
    return np.stack([restrict_component(f[g], SHIFTS[g]) for g in range(f.shape[0])])


def replicate(phi):
    """a coarse field piecewise-constant on the fine grid (initFullStageredRawPhases F:17648-17710)"""
    return phi.repeat(2, axis=0).repeat(2, axis=1).repeat(2, axis=2)


def staggered_fractions(phi_fine):
    """[normal, 23, 13, 12] coarse fractions of one phase's fine image"""
    return [restrict_component(phi_fine, s) for s in GROUP_SHIFTS]


def pk1_fractions(eps, phis_fine, mats, alpha=1.0, pk1=pk1_voigt):
    """the coarse form: component group g evaluated point-wise with the group's staggered fractions"""
    fr = [staggered_fractions(p) for p in phis_fine]
    P = np.empty_like(eps)
    for g, comps in enumerate(((0, 1, 2), (3,), (4,), (5,))):
        Pg = pk1(eps, [f[g] for f in fr], mats, alpha)
        for c in comps:
            P[c] = Pg[c]
    return P


class DfgMixin:
    """Overrides of the oracle's material evaluations; self.phis stays the coarse field (F:17180-17228) for the reference
    medium and "phi", self.phis_fine is the fine image."""

    def _dfg_setup(self):
        if not self.phis_fine:
            self.phis_fine = [replicate(np.asarray(p, dtype=np.float64)) for p in self.phis]
        self.phis_fine = [np.asarray(p, dtype=np.float64) for p in self.phis_fine]
        self.phis = [restrict_component(p, (0, 0, 0)) for p in self.phis_fine]

    def _fine(self, fn):
        coarse = self.phis
        self.phis = self.phis_fine
        try:
            return fn()
        finally:
            self.phis = coarse

    def pk1(self, eps, alpha=1.0):
        ef = prolongate_to_dfg(eps)
        return restrict_from_dfg(self._fine(lambda: super(DfgMixin, self).pk1(ef, alpha)))

    def mean_stress(self, eps=None):
        """calcMeanStress under dfg: meanPK1 of the fine grid (F:17793-17811), alpha = 1 / (8 N)"""
        eps = self.eps if eps is None else eps
        ef = prolongate_to_dfg(eps)
        P = self._fine(lambda: super(DfgMixin, self).pk1(ef, 1.0 / (8 * self.N)))
        return P.reshape(6, -1).sum(axis=1)

    def mean_energy(self, eps=None):
        """calcMeanEnergy under dfg (F:17765-17790): meanW of the fine grid"""
        eps = self.eps if eps is None else eps
        ef = prolongate_to_dfg(eps)
        W = energy_voigt(ef, self.phis_fine, self.mats)
        return float(W.sum()) / (8 * self.N)


@dataclass
class DfgLSOracle(DfgMixin, LSOracle):
    phis_fine: list = field(default_factory=list)

    def __post_init__(self):
        super().__post_init__()
        self._dfg_setup()


@dataclass
class DfgViscosityOracle(DfgMixin, ViscosityOracle):
    phis_fine: list = field(default_factory=list)

    def __post_init__(self):
        super().__post_init__()
        self._dfg_setup()


# ---------------------------------------------------------------------------------------------------------------------
# Shared problem builders of the dfg test files (CPU only)

def tile_shape(grid):
    """Which instantiation of the five-moduli tiled sweeps (k_u_tile / k_eps_tile, NMOD = 5) a grid takes, restated from
    u_tile_supported and launch_u_tile / launch_eps_tile in fg_kernels_fast.hip: "<8,1>" (nz = 128, one wave per row),
    "<6,2>" (nz = 256, two waves per row), "<8,0>" with halo lanes for the rest -- "short" (40 <= nz/2 < 62: one tile whose
    surplus lanes hold wrapped copies), "exact" (nz/2 = 62) or "two" (nz/2 > 62: several z tiles, the last one clamped) --
    and "untiled" where the tiles do not fit (odd nz, nz/2 < 40, ny < 14, nx < 4)."""
    nx, ny, nz = grid
    nzh = nz // 2
    if nz % 2 or nzh < 40 or ny < 14 or nx < 4:
        return "untiled"
    if nzh == 64:
        return "<8,1>"
    if nzh == 128:
        return "<6,2>"
    return "<8,0> short" if nzh < 62 else ("<8,0> exact" if nzh == 62 else "<8,0> two")


def smooth_field(rng, shape):
    """test_gpu_fuzz.smooth_field: a smooth periodic field in [0, 1] with flat parts at both ends (on the fine shape: pure
    fine cells at 0 and 1 next to mixtures)"""
    from test_gpu_fuzz import smooth_field as f
    return f(rng, shape)


def fine_images(rng, grid, nph, sharp=False):
    """nph fine phase images (shape 2 grid) that sum to one: smooth fields with pure cells, or a sharp 0/1 image"""
    fshape = tuple(2 * n for n in grid)
    if nph == 1:
        return [np.ones(fshape)]
    cut = (lambda f: (f > 0.5).astype(np.float64)) if sharp else (lambda f: f)
    p1 = cut(smooth_field(rng, fshape))
    if nph == 2:
        return [1.0 - p1, p1]
    p2 = np.minimum(cut(smooth_field(rng, fshape)), 1.0 - p1)
    out = [1.0 - p1 - p2, p1, p2]
    for _ in range(nph - 3):
        out.append(np.zeros(fshape))
    return out


def split_input(images, kinds):
    """(fine, coarse, oracle_fine) for per-phase input kinds "fine" / "coarse": a coarse phase is handed over as the
    8-cell mean of its image and is, for the reference, the piecewise-constant replica of that mean
    (initFullStageredRawPhases F:17648-17710)."""
    fine, coarse, ofine = [], [], []
    for img, kind in zip(images, kinds):
        if kind == "fine":
            fine.append(img)
            coarse.append(None)
            ofine.append(img)
        else:
            c = restrict_component(img, (0, 0, 0))
            fine.append(None)
            coarse.append(c)
            ofine.append(replicate(c))
    return fine, coarse, ofine


def input_kinds(kind, nph):
    """"fine" / "coarse": all phases alike; "mixed": alternating, phase 0 coarse (needs two phases)"""
    if kind == "mixed":
        assert nph >= 2
        return ["coarse" if p % 2 == 0 else "fine" for p in range(nph)]
    return [kind] * nph


def calc_stress_fractions(eps, phis_fine, mats, mu_0, lambda_0, viscosity=False):
    """calcStress F:18134-18184 on the coarse form: pk1_fractions with C0 subtracted the way LSOracle.calc_stress does"""
    if viscosity:   # ScalarLinearIsotropic(6) with mu / 2 (F:15237): the Hooke law with (mu / 4, 0)
        mats = [(m / 4, 0.0) for m, _ in mats]
    P = pk1_fractions(eps, phis_fine, mats)
    if mu_0 != 0:
        P = P + (-2.0 * mu_0) * eps
    if lambda_0 != 0:
        tr = eps[0] + eps[1] + eps[2]
        for c in range(3):
            P[c] = P[c] + (-lambda_0) * tr
    return P

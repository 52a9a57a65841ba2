"""Pins of the doubly fine grid restatement (tests/dfg_reference.py): the literal prolong -> PK1 -> restrict chain of
gamma_scheme full_staggered against the staggered-fraction form the library evaluates.  CPU only."""
import numpy as np

from dfg_reference import (DfgLSOracle, DfgViscosityOracle, pk1_fractions, prolongate_to_dfg, replicate,
                           restrict_component, restrict_from_dfg, staggered_fractions)
from oracle.ls_oracle import LSOracle

GRID = (5, 4, 3)
MATS = [(0.38, 0.58), (4.2, 2.8)]


def _random_fine(rng, n=GRID):
    f = rng.random(tuple(2 * k for k in n))
    return [1.0 - f, f]


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def test_restrict_prolongate_identity():
    rng = np.random.default_rng(1)
    c = rng.standard_normal((6,) + GRID)
    assert _rel(restrict_from_dfg(prolongate_to_dfg(c)), c) <= 4.5e-16


def test_homogeneous_material_equals_staggered():
    """the reference's self-test F:24153-24182: one material everywhere gives the staggered result"""
    rng = np.random.default_rng(2)
    ones = np.ones(GRID)
    eps = rng.standard_normal((6,) + GRID)
    d = DfgLSOracle(*GRID, mats=MATS[:1], phis=[ones])
    s = LSOracle(*GRID, mats=MATS[:1], phis=[ones])
    assert _rel(d.pk1(eps), s.pk1(eps)) <= 1e-15
    assert _rel(d.mean_stress(eps), s.mean_stress(eps)) <= 1e-14
    assert abs(d.mean_energy(eps) - s.mean_energy(eps)) <= 1e-14 * abs(s.mean_energy(eps))


def test_literal_chain_equals_staggered_fractions():
    rng = np.random.default_rng(3)
    fine = _random_fine(rng)
    eps = rng.standard_normal((6,) + GRID)
    d = DfgLSOracle(*GRID, mats=MATS, phis=[np.zeros(GRID)] * 2, phis_fine=fine)
    ref = pk1_fractions(eps, fine, MATS)
    assert _rel(d.pk1(eps), ref) <= 1e-13
    N = float(np.prod(GRID))
    assert _rel(d.mean_stress(eps), ref.reshape(6, -1).sum(axis=1) / N) <= 1e-13
    w = 0.5 * (ref[0] * eps[0] + ref[1] * eps[1] + ref[2] * eps[2] + 2 * (ref[3] * eps[3] + ref[4] * eps[4] + ref[5] * eps[5]))
    assert abs(d.mean_energy(eps) - w.sum() / N) <= 1e-13 * abs(w.sum() / N)
    # the coarse field the reference reports (F:17180-17228) is the normal group's fraction
    assert _rel(d.phis[1], staggered_fractions(fine[1])[0]) == 0.0


def test_viscosity_literal_chain_equals_staggered_fractions():
    rng = np.random.default_rng(4)
    fine = _random_fine(rng)
    eps = rng.standard_normal((6,) + GRID)
    mats = [(1.0, 0.0), (0.01, 0.0)]
    d = DfgViscosityOracle(*GRID, mats=mats, phis=[np.zeros(GRID)] * 2, phis_fine=fine)
    # ScalarLinearIsotropic(6) with mu / 2 (F:15237): the Hooke law with (mu / 4, 0)
    ref = pk1_fractions(eps, fine, [(m / 4, 0.0) for m, _ in mats])
    assert _rel(d.pk1(eps), ref) <= 1e-13
    assert _rel(d.mean_stress(eps), ref.reshape(6, -1).sum(axis=1) / np.prod(GRID)) <= 1e-13


def test_replicated_input_gives_edge_means():
    rng = np.random.default_rng(5)
    phi = rng.random(GRID)
    fr = staggered_fractions(replicate(phi))
    r = lambda a, sj, sk, si=0: np.roll(np.roll(np.roll(a, si, 0), sj, 1), sk, 2)  # noqa: E731
    assert _rel(fr[0], phi) <= 1e-15
    assert _rel(fr[1], 0.25 * (phi + r(phi, 1, 0) + r(phi, 0, 1) + r(phi, 1, 1))) <= 1e-15
    assert _rel(fr[2], 0.25 * (phi + r(phi, 0, 0, 1) + r(phi, 0, 1) + r(phi, 0, 1, 1))) <= 1e-15
    assert _rel(fr[3], 0.25 * (phi + r(phi, 0, 0, 1) + r(phi, 1, 0) + r(phi, 1, 0, 1))) <= 1e-15
    # and the oracle built from a coarse field takes it as such a replica
    d = DfgLSOracle(*GRID, mats=MATS, phis=[1.0 - phi, phi])
    assert _rel(d.phis[1], phi) <= 1e-15 and _rel(restrict_component(d.phis_fine[1], (0, 1, 1)), fr[1]) <= 1e-15


def test_oracle_runs_full_staggered():
    """a short basic-scheme solve on the mixin converges and differs from the staggered one"""
    rng = np.random.default_rng(6)
    fine = _random_fine(rng, (6, 6, 6))
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    d = DfgLSOracle(6, 6, 6, mats=MATS, phis=[np.zeros((6, 6, 6))] * 2, phis_fine=fine, tol=1e-8)
    assert d.run(E) is False
    s = LSOracle(6, 6, 6, mats=MATS, phis=d.phis, tol=1e-8)
    assert s.run(E) is False
    assert _rel(d.mean_stress(), s.mean_stress()) > 1e-6

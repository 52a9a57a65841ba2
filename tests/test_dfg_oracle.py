"""Pins of the doubly fine grid restatement (tests/dfg_reference.py): the literal prolong -> PK1 -> restrict chain of
gamma_scheme full_staggered against the staggered-fraction form the library evaluates.  CPU only."""
import numpy as np
import pytest

from dfg_reference import (DfgLSOracle, DfgViscosityOracle, calc_stress_fractions, fine_images, input_kinds, pk1_fractions,
                           prolongate_to_dfg, replicate, restrict_component, restrict_from_dfg, split_input,
                           staggered_fractions, tile_shape)
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


# ---------------------------------------------------------------------------------------------------------------------
# The oracle side of the GPU files test_gpu_dfg_stages / _fuzz / _state / _project, pinned without a GPU

MATS3 = MATS + [(1.7, 0.4)]


def _pure_fraction(images):
    return [float(np.mean((p == 0.0) | (p == 1.0))) for p in images]


@pytest.mark.parametrize("grid", [GRID, (1, 1, 4), (10, 1, 1)], ids=["5x4x3", "1x1x4", "10x1x1"])
@pytest.mark.parametrize("kind", ["fine", "coarse", "mixed"])
def test_three_phases_with_pure_cells_chain_equals_fraction_form(grid, kind):
    """three phases whose fine images have pure cells (fractions exactly 0 and 1: the Voigt threshold decides), fine, coarse
    (replicated) and mixed input, also on degenerate grids where the shifted 8-cell block wraps onto itself: the literal
    chain equals the fraction form, for the stress, its mean and the mean energy"""
    rng = np.random.default_rng(7)
    images = fine_images(rng, grid, 3)
    if grid == GRID:
        assert min(_pure_fraction(images)) > 0.02
    fine, coarse, ofine = split_input(images, input_kinds(kind, 3))
    assert [f is None for f in fine] == [c is not None for c in coarse]
    eps = rng.standard_normal((6,) + grid)
    d = DfgLSOracle(*grid, mats=MATS3, phis=[np.zeros(grid)] * 3, phis_fine=ofine)
    for p in range(3):   # "phi" is the 8-cell mean; a coarse phase gets its own field back
        assert _rel(d.phis[p], restrict_component(images[p], (0, 0, 0))) <= 1e-15
    ref = pk1_fractions(eps, ofine, MATS3)
    assert _rel(d.pk1(eps), ref) <= 1e-13
    assert _rel(d.calc_stress(0.77, 0.31, eps), calc_stress_fractions(eps, ofine, MATS3, 0.77, 0.31)) <= 1e-13
    N = float(np.prod(grid))
    assert _rel(d.mean_stress(eps), ref.reshape(6, -1).sum(axis=1) / N) <= 1e-13
    w = 0.5 * (ref[0] * eps[0] + ref[1] * eps[1] + ref[2] * eps[2] + 2 * (ref[3] * eps[3] + ref[4] * eps[4] + ref[5] * eps[5]))
    assert abs(d.mean_energy(eps) - w.sum() / N) <= 1e-13 * abs(w.sum() / N)
    fl = [(1.0, 0.0), (0.05, 0.0), (3.0, 0.0)]
    v = DfgViscosityOracle(*grid, mats=fl, phis=[np.zeros(grid)] * 3, phis_fine=ofine)
    assert _rel(v.calc_stress(0.77, 0.31, eps), calc_stress_fractions(eps, ofine, fl, 0.77, 0.31, viscosity=True)) <= 1e-13


def test_all_coarse_input_is_the_replica_construction():
    """split_input with coarse phases builds what DfgLSOracle builds from phis alone"""
    rng = np.random.default_rng(8)
    images = fine_images(rng, GRID, 2)
    _fine, coarse, ofine = split_input(images, ["coarse", "coarse"])
    a = DfgLSOracle(*GRID, mats=MATS, phis=coarse)
    b = DfgLSOracle(*GRID, mats=MATS, phis=[np.zeros(GRID)] * 2, phis_fine=ofine)
    eps = rng.standard_normal((6,) + GRID)
    assert _rel(a.pk1(eps), b.pk1(eps)) == 0.0


def test_tile_shape_restates_the_launch_selection():
    assert [tile_shape(g) for g in [(16, 16, 128), (4, 14, 256), (4, 16, 80), (8, 14, 124), (4, 14, 200), (8, 16, 78),
                                    (8, 12, 128), (3, 14, 128), (9, 14, 125)]] == \
        ["<8,1>", "<6,2>", "<8,0> short", "<8,0> exact", "<8,0> two", "untiled", "untiled", "untiled", "untiled"]


@pytest.mark.parametrize("estimator", ["epsilon", "sigma", "energy"])
@pytest.mark.parametrize("method", ["basic", "cg"])
def test_oracle_load_steps_and_estimators_converge(method, estimator):
    """the fine-grid oracle under run_load_steps with every estimator the GPU files draw, three phases with pure cells"""
    grid = (6, 5, 4)
    rng = np.random.default_rng(9)
    images = fine_images(rng, grid, 3)
    d = DfgLSOracle(*grid, mats=MATS3, phis=[np.zeros(grid)] * 3, phis_fine=images, tol=1e-7, maxiter=400,
                    error_estimator=estimator)
    assert d.run_load_steps(np.array([1.0, 0, 0, 0, 0, 0.5]), params=[0.0, 0.4, 1.0], method=method) is False
    assert len(d.step_iterations) == 3 and 1 < d.iterations < 400


def test_oracle_cg_with_mixed_projector_and_viscosity_three_phases_converge():
    grid = (6, 5, 4)
    rng = np.random.default_rng(10)
    images = fine_images(rng, grid, 3)
    d = DfgLSOracle(*grid, mats=MATS3, phis=[np.zeros(grid)] * 3, phis_fine=images, tol=1e-7, maxiter=400)
    P = np.diag([1.0, 0, 0, 0, 0, 0.5])
    assert d.run_cg(np.array([1.0, 0, 0, 0, 0, 0.3]), np.zeros(6), P) is False and 1 < d.iterations < 400
    v = DfgViscosityOracle(*grid, mats=[(1.0, 0.0), (0.05, 0.0), (3.0, 0.0)], phis=[np.zeros(grid)] * 3, phis_fine=images,
                           tol=1e-7, maxiter=400)
    assert v.run(np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])) is False and 1 < v.iterations < 400

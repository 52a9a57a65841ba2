"""The NumPy restatement of law="aniso" (tests/aniso_reference.py) against what is known without it: the isotropic oracle for
K = mu I, the homogeneous body, and the laminate closed form, which the staggered discretisation reproduces exactly when every
field depends on one coordinate only."""
import numpy as np
import pytest

from aniso_reference import (AnisoScalarOracle, aniso3, check_laminate, k6, layer_problem, pk1_voigt_aniso, random_spd3,
                             voigt_tangent3)
from helpers import rel_err, sphere_phi
from oracle.scalar_oracle import ScalarOracle


def test_isotropic_equivalence():
    """K_p = mu_p I: number materials take ScalarOracle's own code (bit for bit); matrix materials differ from it by the
    operation order only -- alpha * (mu * g + 0 + 0) against g * (alpha * mu), two roundings each -- <= 1e-15 relative"""
    grid = (9, 7, 5)
    rng = np.random.default_rng(3)
    phi1 = sphere_phi(grid, 0.3)
    mus, phis = [1.0, 12.0], [1 - phi1, phi1]
    g = rng.standard_normal((3,) + grid)
    ref = ScalarOracle(*grid, mus=mus, phis=phis)
    same = AnisoScalarOracle(*grid, mus=mus, phis=phis)
    assert np.array_equal(same.pk1(g, 0.37), ref.pk1(g, 0.37))
    same.calc_ref_material()
    ref.calc_ref_material()
    assert same.mu_0 == ref.mu_0
    mat = AnisoScalarOracle(*grid, mus=[m * np.eye(3) for m in mus], phis=phis)
    for alpha in (1.0, 0.37, 1.0 / 315):
        a, b = mat.pk1(g, alpha), ref.pk1(g, alpha)
        assert np.abs(a - b).max() <= 1e-15 * np.abs(b).max()
    mat.calc_ref_material()
    assert abs(mat.mu_0 - ref.mu_0) <= 1e-15 * ref.mu_0
    # a whole run: same iteration count, fields to the rounding of the two orders
    E = np.array([1.0, -0.5, 0.25])
    mat.tol = ref.tol = 1e-9
    assert mat.run(E) is False and ref.run(E) is False
    assert mat.iterations == ref.iterations
    assert rel_err(mat.eps, ref.eps) < 1e-13
    # mixed laws: phase 0 a number, phase 1 a matrix
    mix = AnisoScalarOracle(*grid, mus=[mus[0], mus[1] * np.eye(3)], phis=phis)
    a, b = mix.pk1(g), ref.pk1(g)
    assert np.abs(a - b).max() <= 1e-15 * np.abs(b).max()


def test_operation_order_and_threshold():
    """PK1 F:11114-11128 literally on one voxel; phases at or below 10 eps do not count, the first that counts assigns"""
    K = random_spd3(np.random.default_rng(5), 4.0)
    E = np.array([0.3, -1.1, 0.7])
    alpha = 0.41
    S = aniso3(E, K, alpha)
    for c in range(3):
        assert S[c] == alpha * (K[c, 0] * E[0] + K[c, 1] * E[1] + K[c, 2] * E[2])
    assert list(k6(K)) == [K[0, 0], K[1, 1], K[2, 2], K[1, 2], K[0, 2], K[0, 1]]
    g = E.reshape(3, 1, 1, 1)
    tiny, one = np.full((1, 1, 1), 2e-15), np.ones((1, 1, 1))
    P = pk1_voigt_aniso(g, [tiny, one], [7.0, K], alpha)
    assert np.array_equal(P[:, 0, 0, 0], aniso3(E, K, 1.0 * alpha))
    A = voigt_tangent3([tiny, one * 0.25, one * 0.75], [7.0, 2.0, K])
    assert np.array_equal(A[0, 0, 0], 0.25 * 2.0 * np.eye(3) + 0.75 * K.T)


def test_homogeneous_body():
    grid = (6, 5, 4)
    K = random_spd3(np.random.default_rng(11), 3.0)
    E = np.array([1.0, -0.5, 0.25])
    o = AnisoScalarOracle(*grid, mus=[K], phis=[np.ones(grid)], tol=1e-13)
    assert o.run(E) is False
    w = np.linalg.eigvalsh(K)
    assert o.mu_0 == pytest.approx(0.25 * (w[0] + w[-1]), rel=1e-14)
    assert rel_err(o.mean_stress(), K @ E) <= 1e-13
    assert np.abs(o.eps - E[:, None, None, None]).max() <= 1e-13


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_three_layers_reproduce_the_laminate(axis):
    shape, fr, edges, phis, Ks = layer_problem(axis)
    E = np.array([1.0, -0.5, 0.25])
    o = AnisoScalarOracle(*shape, mus=Ks, phis=phis, tol=1e-13, maxiter=5000)
    assert o.run(E) is False
    assert o.iterations < 5000
    check_laminate(axis, o.eps, o.pk1(o.eps), fr, edges, Ks, E, 1e-10)

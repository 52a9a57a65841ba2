"""The NumPy restatement of the pressure accessor (tests/pressure_reference.py) against what it must satisfy by itself: the
Poisson solve inverts the 7-point periodic Laplacian with the scale the restatement derives (SCALE = 1), the pressure has zero
mean, and the closed forms the discretisation reproduces exactly -- a homogeneous fluid and a layered fluid sheared in the layer
plane carry no pressure.

Bounds.  L_h has eigenvalues between -4 sum_a n_a^2/d_a^2 and about -(2 pi / d_max)^2, so solving and applying it again loses at
most cond(L_h) ~ 12 n^2 / 40 < 100 units of the double rounding 1.1e-16 on these grids (n <= 12): 1e-12 relative to max |f|
leaves two decades.  The closed forms are zero up to the rounding of the converged strain field (1e-16 relative, amplified by the
two difference quotients n^2/d^2 <= 144 and divided again by the solve): 1e-12 of max |epsilon| likewise."""
import numpy as np
import pytest

import pressure_reference as pr
from test_oracle_pins import _layers_x

GRIDS = [((8, 8, 8), (1.0, 1.0, 1.0)), ((12, 10, 6), (2.0, 1.0, 0.5)), ((6, 5, 7), (1.0, 1.0, 1.0)), ((9, 1, 4), (1.0, 0.5, 3.0))]


@pytest.mark.parametrize("grid,dims", GRIDS)
def test_poisson_solve_inverts_the_seven_point_laplacian(grid, dims):
    """s = SCALE = 1: the unnormalised transform pair gives nxyz, c = 2 nxyz takes it back and leaves the 2 that turns
    n^2/d^2 (cos xi - 1) into the symbol of the second difference"""
    assert pr.SCALE == 1.0
    f = np.random.default_rng(5).standard_normal(grid)
    f -= f.mean()
    u = pr.poisson_solve(f, dims)
    assert np.isfinite(u).all()
    assert np.abs(pr.laplacian7(u, dims) - pr.SCALE * f).max() < 1e-12 * np.abs(f).max()
    assert abs(u.mean()) < 1e-14 * np.abs(u).max()
    # a mean in f is dropped with bin 0 (F:23496), not turned into a NaN
    v = pr.poisson_solve(f + 3.0, dims)
    assert np.abs(v - u).max() < 1e-12 * np.abs(u).max()


def test_div_vector_takes_the_forward_neighbour_with_a_minus_sign():
    """F:19996-19998 on a field that is linear in the voxel index away from the wrap: t[k] - t[k + 1] = -slope"""
    grid, dims = (6, 5, 7), (2.0, 1.0, 0.5)
    i, j, k = np.meshgrid(*[np.arange(n, dtype=float) for n in grid], indexing="ij")
    b = pr.div_vector(np.stack([2.0 * i, 3.0 * j, 5.0 * k]), dims, alpha=0.5)
    want = -0.5 * (2.0 * grid[0] / dims[0] + 3.0 * grid[1] / dims[1] + 5.0 * grid[2] / dims[2])
    assert np.allclose(b[:-1, :-1, :-1], want, rtol=1e-15)
    # the last plane along x wraps to plane 0: t[nx - 1] - t[0]
    assert b[-1, 0, 0] == pytest.approx(0.5 * (2.0 * (grid[0] - 1) * grid[0] / dims[0] - 3.0 * grid[1] / dims[1] - 5.0 * grid[2] / dims[2]))


def _sphere_oracle(grid, dims, cls=None, mats=((1.0, 0.0), (0.05, 0.0)), **kw):
    from helpers import sphere_phi
    from oracle.viscosity_oracle import ViscosityOracle
    phi1 = sphere_phi(grid, 0.3)
    return (cls or ViscosityOracle)(*grid, *dims, mats=list(mats), phis=[1 - phi1, phi1], **kw)


@pytest.mark.parametrize("mixing", ["voigt", "reuss"])
def test_pressure_has_zero_mean_and_solves_its_equation(mixing):
    from reuss_reference import ReussViscosityOracle
    grid, dims = (12, 10, 6), (2.0, 1.0, 0.5)
    o = _sphere_oracle(grid, dims, cls=ReussViscosityOracle if mixing == "reuss" else None, tol=1e-30, maxiter=3)
    o.run(np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0]))
    p, f = pr.pressure(o), pr.pressure_rhs(o)
    assert np.abs(p).max() > 1e-3                      # a sphere in shear does carry a pressure
    assert abs(p.mean()) < 1e-14 * np.abs(p).max()
    assert np.abs(pr.laplacian7(p, dims) - (f - f.mean())).max() < 1e-12 * np.abs(f).max()
    assert abs(f.mean()) < 1e-12 * np.abs(f).max()   # a divergence of periodic fields


def test_homogeneous_fluid_has_no_pressure():
    from oracle.viscosity_oracle import ViscosityOracle
    shape = (8, 6, 10)
    one = np.ones(shape)
    o = ViscosityOracle(*shape, mats=[(3.0, 0.0), (7.0, 0.0)], phis=[one, 0 * one])
    E = np.array([0.5, -0.2, -0.3, 0.1, 0.0, 0.7])
    assert o.run(E) is False
    assert np.abs(pr.pressure(o)).max() < 1e-12 * np.abs(o.eps).max()


def test_layered_fluid_sheared_in_the_layer_plane_has_no_pressure():
    """the layers of test_oracle_pins.py::test_viscosity_layered_fluid_and_incompressibility, stacked along x, under s23: the
    polarisation depends on x alone and has the single component 23, whose differences run along y and z"""
    from oracle.viscosity_oracle import ViscosityOracle
    shape, fr, mus = (12, 4, 6), [0.25, 0.25, 0.5], [1.0, 4.0, 0.5]
    o = ViscosityOracle(*shape, mats=[(m, 0.0) for m in mus], phis=_layers_x(shape, fr), tol=1e-12, maxiter=3000)
    assert o.run(np.array([0, 0, 0, 1.0, 0, 0])) is False
    assert np.abs(o.eps[3]).max() > 0.1 and np.ptp(o.eps[3]) > 0.1   # a field that does vary across the layers
    assert np.abs(pr.pressure(o)).max() < 1e-12 * np.abs(o.eps).max()

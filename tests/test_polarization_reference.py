"""The NumPy restatement of method "polarization" (polarization_reference.py) pinned without the product: its fixed point
against the oracle's basic scheme, the two per-voxel forms against each other, the inverse map, the iteration counts, and
the reference's staggered pass as written."""
import warnings

import numpy as np
import pytest

import general_reference as gr
import polarization_reference as pr

E_LOAD = np.array([1.0, 0.2, -0.3, 0.1, 0.25, 0.5])
GRIDS = [(8, 8, 8), (12, 10, 6)]
_cache = {}


def converged(grid, contrast, scheme, method, same_operator=False):
    """(oracle after its converged run at tol 1e-10) -- computed once per case and shared.  same_operator: the polarisation
    loop runs on the basic scheme's reference material (update_ref never) instead of its own sqrt(min max)"""
    key = (grid, contrast, scheme, method, same_operator)
    if key not in _cache:
        mats = [(1.0, 1.0), (contrast, contrast)]
        kw = {}
        if same_operator:
            kw = {"update_ref": "never", "mu_0": converged(grid, contrast, scheme, "basic")[0].mu_0}
        o = pr.make_polarization_oracle(grid, mats, scheme=scheme, tol=1e-10, maxiter=40000, **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            failed = o.run_polarization(E_LOAD) if method == "polarization" else o.run(E_LOAD)
        _cache[key] = (o, failed)
    return _cache[key]


@pytest.mark.parametrize("contrast", [10.0, 1000.0])
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("scheme", ["collocated", "willot", "staggered"])
def test_same_fixed_point_as_the_basic_scheme(scheme, grid, contrast):
    """(a) max |eps_pol - eps_basic| / max |eps_basic|, both converged at tol 1e-10 ON THE SAME OPERATOR: the Green operator
    of the same reference material (the basic scheme's mu_0, which the polarisation loop takes with update_ref never; the
    basic scheme does not converge on the polarisation loop's smaller mu_0).  The estimator watches increments of a norm, so
    the slowly converging loops stop about tol / (1 - rate) away from the solution.  Measured (collocated / willot / staggered):
    contrast 10: 1.5e-8 / 9.7e-9 / 2.3e-8 (8^3), 1.0e-8 / 9.9e-9 / 2.0e-8 (12 x 10 x 6); contrast 1000: 1.7e-6 / 6.7e-7 / 1.3e-6,
    9.3e-7 / 7.0e-7 / 1.2e-6.  The bounds were set from the willot and staggered figures (10 x the largest per contrast: 2.3e-7
    and 1.3e-5) and hold for collocated as well.

    The same mu_0 matters for collocated only: see test_collocated_solution_depends_on_the_reference_material."""
    pol, f1 = converged(grid, contrast, scheme, "polarization", same_operator=True)
    bas, f2 = converged(grid, contrast, scheme, "basic")
    assert f1 is False and f2 is False and pol.mu_0 == bas.mu_0
    d = np.abs(pol.eps - bas.eps).max() / np.abs(bas.eps).max()
    print("fixed point", scheme, grid, contrast, d, pol.iterations, bas.iterations)
    assert d <= (2.3e-7 if contrast == 10.0 else 1.3e-5)


@pytest.mark.parametrize("scheme", ["collocated", "willot", "staggered"])
def test_collocated_solution_depends_on_the_reference_material(scheme):
    """Each method on its OWN reference material (8^3, contrast 10: mu_0 = 5 for polarisation, 13 for basic), both fully
    converged (the polarisation iterates stand still to 1e-14).  willot and staggered reach the same strain field (measured
    9.7e-9, 2.3e-8: their discrete solution does not depend on mu_0).  collocated does not (measured 7.5e-3; 6.6e-2 at contrast
    1000): on an even axis the signed frequency of index n / 2 is -n / 2 on both conjugate partners, the operator's Nyquist
    planes are not Hermitian, the inverse transform projects them, and the projected operator no longer satisfies
    Gamma0 : C0 : Gamma0 = Gamma0 there -- the discrete problem itself depends on mu_0.  On odd grids it does not
    (test_collocated_agrees_on_an_odd_grid).  A property of the reference's collocated operator with freq_hack off, whatever the
    method; it is why the comparison above fixes mu_0."""
    pol, _ = converged((8, 8, 8), 10.0, scheme, "polarization")
    bas, _ = converged((8, 8, 8), 10.0, scheme, "basic")
    assert pol.mu_0 != bas.mu_0
    d = np.abs(pol.eps - bas.eps).max() / np.abs(bas.eps).max()
    print("own reference material", scheme, d)
    if scheme == "collocated":
        assert d > 1e-3
    else:
        assert d <= 2.3e-7


def test_collocated_agrees_on_an_odd_grid():
    """the collocated scheme without Nyquist planes: measured 3.9e-10 at tol 1e-12, asserted at 10 x"""
    mats = [(1.0, 1.0), (10.0, 10.0)]
    pol = pr.make_polarization_oracle((9, 7, 5), mats, scheme="collocated", tol=1e-12, maxiter=5000)
    bas = pr.make_polarization_oracle((9, 7, 5), mats, scheme="collocated", tol=1e-12, maxiter=20000)
    assert pol.run_polarization(E_LOAD) is False and bas.run(E_LOAD) is False
    assert np.abs(pol.eps - bas.eps).max() / np.abs(bas.eps).max() <= 3.9e-9


def test_iso_form_equals_generic_form():
    """(b) on a pure isotropic voxel, <= 1e-13 relative"""
    rng = np.random.default_rng(3)
    for _ in range(200):
        mu, lam, mu_0 = rng.uniform(0.1, 50.0), rng.uniform(0.0, 50.0), 10.0 ** rng.uniform(-2, 2)
        F = rng.standard_normal((6, 1, 1, 1))
        C = pr.dpk1_matrix((mu, lam))[None, None, None]
        for inv in (False, True):
            a, b = pr.polarize_iso(F, mu, lam, mu_0, inv), pr.polarize_generic(F, C, mu_0, inv)
            assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


def test_inverse_undoes_the_forward_map():
    """(c) P = (C + C0) eps, inv -> eps; mixed voxels, iso and general phases"""
    grid = (6, 5, 4)
    phis = pr.sphere_phi(grid)
    for mats in ([(1.0, 2.0), (30.0, 10.0)], [(1.0, 2.0), gr.distinct_stiffness(5.0)]):
        o = pr.make_polarization_oracle(grid, mats, phis)
        o.mu_0 = 3.7
        eps = np.random.default_rng(4).standard_normal((6,) + grid)
        C = pr.tangent_full(phis, mats)
        P = np.moveaxis((C + 2 * o.mu_0 * np.eye(6)) @ np.moveaxis(eps, 0, -1)[..., None], -2, 0)[..., 0]
        assert np.abs(o.calc_polarization(P, inv=True) - eps).max() <= 1e-12 * np.abs(eps).max()
        Q = np.moveaxis((C - 2 * o.mu_0 * np.eye(6)) @ np.moveaxis(eps, 0, -1)[..., None], -2, 0)[..., 0]
        assert np.abs(o.calc_polarization(P) - Q).max() <= 1e-12 * np.abs(Q).max()


@pytest.mark.parametrize("scheme", ["willot", "staggered"])
def test_fewer_iterations_at_contrast_1000(scheme):
    """(d) 12 x 10 x 6, contrast 1000, tol 1e-10: the polarisation loop took 533 passes, the basic scheme 12625 (willot) /
    12444 (staggered).  The estimators watch different fields (P and eps), so the counts are a record, not a like-for-like
    comparison (that is test_accuracy_at_equal_pass_counts); asserted here is only that the polarisation loop needs fewer than a
    tenth."""
    pol, _ = converged((12, 10, 6), 1000.0, scheme, "polarization")
    bas, _ = converged((12, 10, 6), 1000.0, scheme, "basic")
    print("iterations", scheme, pol.iterations, bas.iterations)
    assert 10 * pol.iterations < bas.iterations


@pytest.mark.parametrize("scheme", ["willot", "staggered"])
def test_accuracy_at_equal_pass_counts(scheme):
    """(d), second half: 12 x 10 x 6, contrast 1000, both loops stopped after the same number of passes N (no tolerance), each
    on its own reference material, error max |eps - eps_ref| / max |eps_ref| against a tight CG solution of the same operator
    (tol 1e-13, 266 / 265 iterations).  Measured, polarisation / basic:
      willot     N = 50: 2.3e-2 / 1.4e-1   N = 200: 5.8e-5 / 9.5e-2   N = 533: 8.6e-8 / 5.9e-2
      staggered  N = 50: 2.4e-2 / 1.6e-1   N = 200: 6.9e-5 / 8.5e-2   N = 533: 3.5e-7 / 4.5e-2
    So the smaller iteration count of the polarisation loop is backed by accuracy: after 533 passes, where its own stop rule
    ends it at tol 1e-10, it is within 1e-6 of the solution while the basic scheme is still 5 % away.  Asserted: smaller error
    at every N, by a factor above 100 from N = 200 on, and below 1e-5 at N = 533."""
    grid, mats = (12, 10, 6), [(1.0, 1.0), (1000.0, 1000.0)]
    ref = pr.make_polarization_oracle(grid, mats, scheme=scheme, tol=1e-13, maxiter=5000)
    assert ref.run_cg(E_LOAD) is False
    scale = np.abs(ref.eps).max()
    for N in (50, 200, 533):
        err = {}
        for method in ("polarization", "basic"):
            o = pr.make_polarization_oracle(grid, mats, scheme=scheme, tol=0.0, abs_tol=-1.0, maxiter=N)
            assert (o.run_polarization(E_LOAD) if method == "polarization" else o.run(E_LOAD)) is False
            assert o.iterations == N
            err[method] = np.abs(o.eps - ref.eps).max() / scale
        print("accuracy", scheme, N, err)
        assert err["polarization"] < err["basic"]
        if N >= 200:
            assert 100 * err["polarization"] < err["basic"]
        if N == 533:
            assert err["polarization"] <= 1e-5


@pytest.mark.parametrize("grid", GRIDS)
def test_the_reference_s_staggered_pass_as_written_does_not_converge_there(grid):
    """(e) GammaOperatorStaggered drops beta (F:20288-20300): the loop P <- mean - 4 mu_0 grad_s G0 div Q either blows up or
    ends far from the cell problem's solution (measured: the field overflows), which is why gamma_scheme staggered deviates"""
    o = pr.make_polarization_oracle(grid, [(1.0, 1.0), (10.0, 10.0)], scheme="staggered_as_written", tol=1e-10, maxiter=1500)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        failed = o.run_polarization(E_LOAD)
    bas, _ = converged(grid, 10.0, "staggered", "basic")
    with np.errstate(all="ignore"):
        d = np.abs(o.eps - bas.eps).max() / np.abs(bas.eps).max()
    assert failed or not np.isfinite(d) or d > 1e-2

"""mixing_rule "reuss" on the GPU against the NumPy restatement (reuss_reference.py): the stress stage and the reference-material
scan, the loops on every path that serves the rule (strain state, untiled sweep, tiled sweep on the moduli arrays and in its
in-sweep harmonic form, mixed boundary conditions, collocated and willot), the three scalar modes, and the oracle-free checks:
the series mean of layers, the bounds reuss <= laminate <= voigt, the homogeneous body, switching the rule on a live solver."""
import numpy as np
import pytest

import reuss_reference as rr
from helpers import rel_err, sphere_normals, sphere_phi

pytestmark = pytest.mark.gpu

ISO = [(0.4, 0.6), (6.0, 8.0), (1.5, 0.2)]
# test_gpu_general.py's grids: the smallest u_tile_supported accepts per tile shape <8,1>, <6,2>, <8,0>
TILE_GRIDS = [(6, 14, 128), (4, 14, 256), (4, 16, 80)]
E_LOAD = np.array([0.5, -0.25, 1.0, 0.1, 0.2, 0.3])


def phases(grid, nph):
    """a sphere (two phases, complementary bit for bit) or two nested spheres (three phases), composite voxels at the surfaces"""
    if nph == 2:
        phi = sphere_phi(grid, 0.3)
        return [1.0 - phi, phi], ISO[:2]
    core, both = sphere_phi(grid, 0.2), sphere_phi(grid, 0.35)
    return [1.0 - both, both - core, core], ISO


def gpu_solver(grid, phis, mats, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid)
    s.set_num_phases(len(mats))
    for p, m in enumerate(mats):
        s.set_phase(p, m[0], m[1], phis[p])
    s.set_options(mixing_rule="reuss", **opts)
    return s


def oracle(grid, phis, mats, cls=rr.ReussLSOracle, **kw):
    return cls(*grid, mats=mats, phis=phis, **kw)


# ---------------------------------------------------------------------------------------------- stage and scan
@pytest.mark.parametrize("nph", [2, 3])
@pytest.mark.parametrize("grid", [(8, 8, 8), (12, 10, 6), (6, 5, 7)])
def test_stress_stage(grid, nph):
    """k_stress through stress_voxel's kMixReuss branch; 1.4e-14 = 10 x the closed form's distance from the literal restatement
    (reuss_reference.py), the mean at the Voigt stage tests' 1e-12"""
    phis, mats = phases(grid, nph)
    s, o = gpu_solver(grid, phis, mats, mu_0=0.77, lambda_0=0.31), oracle(grid, phis, mats)
    eps = np.random.default_rng(10).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    e = rel_err(s.get_field("tau"), o.calc_stress(0.77, 0.31, eps))
    e2 = rel_err(s.get_field("sigma"), o.calc_stress(0.0, 0.0, eps))
    o.eps = eps
    e3 = rel_err(s.mean_stress(), o.mean_stress())
    print("stage", grid, nph, e, e2, e3)
    assert e < rr.STAGE_TOL and e2 < rr.STAGE_TOL and e3 < 1e-12
    s.close()


@pytest.mark.parametrize("nph", [2, 3])
def test_reference_material_scan(nph):
    grid = (12, 10, 6)
    phis, mats = phases(grid, nph)
    s, o = gpu_solver(grid, phis, mats), oracle(grid, phis, mats)
    o.calc_ref_material()
    mu_0, lam_0 = s.calc_ref_material()
    print("scan", nph, mu_0, o.mu_0)
    assert abs(mu_0 - o.mu_0) <= 1e-13 * o.mu_0 and lam_0 == 0.0
    s.close()


# ---------------------------------------------------------------------------------------------- loops
def run_both(grid, phis, mats, method, maxiter, P=None, cls=rr.ReussLSOracle, okw=None, **opts):
    o = oracle(grid, phis, mats, cls=cls, tol=1e-14, maxiter=maxiter, **(okw or {}))
    s = gpu_solver(grid, phis, mats, tol=1e-14, maxiter=maxiter, method=method, **opts)
    if P is not None:
        s.set_bc_projector(P)
        E = np.array([0.01, 0, 0, 0, 0, 0.002])
        fo = o.run(E, S0=np.zeros(6), P=P)
        fs = s.run(E, np.zeros(6))
    else:
        fo = o.run_cg(E_LOAD) if method == "cg" else o.run(E_LOAD)
        fs = s.run(E_LOAD)
    assert fs == fo and s.iterations == o.iterations == maxiter
    return s, o


def check_loop(s, o, method, what):
    # check_loop of test_gpu_general.py (test_gpu_parity's loop tolerances, cg / basic): residual history, strain field, mean stress
    rtol, etol, mtol = (1e-10, 1e-8, 1e-9) if method == "cg" else (1e-11, 1e-9, 1e-10)
    r = np.abs(np.array(s.residuals) - np.array(o.residuals)).max()
    e = rel_err(s.get_field("epsilon"), o.eps)
    m = rel_err(s.mean_stress(), o.mean_stress())
    print(what, method, "residuals", r, "eps", e, "mean stress", m)
    assert len(s.residuals) == len(o.residuals)
    assert r < rtol and e < etol and m < mtol


MIXED_P = np.zeros((6, 6))
MIXED_P[0, 0] = 1.0
MIXED_P[5, 5] = 0.5


@pytest.mark.parametrize("method,maxiter", [("basic", 5), ("cg", 4)])
@pytest.mark.parametrize("nph", [2, 3])
@pytest.mark.parametrize("u_loop", [0, 1, 2])
def test_loops_on_a_grid_the_tiles_do_not_fit(nph, method, maxiter, u_loop):
    """u_loop 0: the strain-state pass (k_stress); 1: the exact-order displacement sweep (k_u_stress); 2: the untiled fast sweep on
    the harmonic moduli arrays (k_u_fast)"""
    grid = (16, 12, 10)
    phis, mats = phases(grid, nph)
    s, o = run_both(grid, phis, mats, method, maxiter, u_loop=u_loop)
    check_loop(s, o, method, "untiled u_loop %d, %d phases" % (u_loop, nph))
    assert s.counter("u_tile_reuss") == 0
    s.close()


@pytest.mark.parametrize("grid", TILE_GRIDS)
@pytest.mark.parametrize("case", ["basic", "mixed_bc", "cg"])
@pytest.mark.parametrize("form", ["arrays", "in_sweep"])
def test_tiled_sweep(grid, case, form):
    """two complementary phases on every tile shape: k_u_tile on the moduli arrays (the default) and in its in-sweep harmonic form
    (option reuss_sweep, its counter), plain, with the sums of tau (mixed boundary conditions) and under the CG"""
    phis, mats = phases(grid, 2)
    method, maxiter = ("cg", 4) if case == "cg" else ("basic", 5)
    s, o = run_both(grid, phis, mats, method, maxiter, P=MIXED_P if case == "mixed_bc" else None, reuss_sweep=int(form == "in_sweep"))
    check_loop(s, o, method, "tile %s %s %s" % (grid, case, form))
    assert (s.counter("u_tile_reuss") > 0) == (form == "in_sweep")
    s.close()


def test_three_phases_on_a_tile_grid_read_the_arrays():
    grid = TILE_GRIDS[2]
    phis, mats = phases(grid, 3)
    s, o = run_both(grid, phis, mats, "basic", 5, reuss_sweep=1)
    check_loop(s, o, "basic", "three phases, tile grid")
    assert s.counter("u_tile_reuss") == 0
    s.close()


def test_mixed_boundary_conditions_in_the_strain_state():
    grid = (12, 10, 6)
    phis, mats = phases(grid, 3)
    s, o = run_both(grid, phis, mats, "basic", 5, P=MIXED_P)
    check_loop(s, o, "basic", "mixed bc, strain state")
    s.close()


def test_collocated_and_willot_schemes():
    """the Fourier-space schemes go through the same k_stress: five passes against the restatement"""
    from willot_reference import WillotMixin
    grid = (12, 10, 6)
    phis, mats = phases(grid, 3)

    class WillotReuss(WillotMixin, rr.ReussLSOracle):
        pass
    for scheme, cls in (("collocated", rr.ReussLSOracle), ("willot", WillotReuss)):
        s, o = run_both(grid, phis, mats, "basic", 5, cls=cls, okw={"gamma_scheme": scheme}, gamma_scheme=scheme)
        check_loop(s, o, "basic", scheme)
        s.close()


# ---------------------------------------------------------------------------------------------- scalar modes
def scalar_solver(mode, grid, mus, phis, **kw):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid)
    s.set_options(mode=mode)
    s.set_num_phases(len(mus))
    for p, (mu, phi) in enumerate(zip(mus, phis)):
        s.set_phase(p, mu, 0.0, phi)
    s.set_options(mixing_rule="reuss", **kw)
    return s


@pytest.mark.parametrize("mode", ["heat", "porous"])
@pytest.mark.parametrize("grid,u_loop", [((12, 10, 6), 1), ((9, 7, 5), 2), ((8, 14, 124), 2)])
def test_heat_and_porous(mode, grid, u_loop):
    """the flux of the state (the stage: k_sc_flux) and three iterations against the scalar model: the exact-order sweep, the
    fast sweep and the tiled sweep on the harmonic conductivity; tolerances of test_gpu_scalar.py"""
    phis, _ = phases(grid, 3)
    mus = [1.0, 12.0, 0.3]
    E = np.array([1.0, -0.5, 0.25])
    s = scalar_solver(mode, grid, mus, phis, tol=1e-14, maxiter=3, u_loop=u_loop)
    o = rr.ReussScalarOracle(*grid, mus=mus, phis=phis, tol=1e-14, maxiter=3)
    assert s.run(E) == o.run(E) and s.iterations == o.iterations == 3
    assert abs(s.ref_material[0] - o.mu_0) <= 1e-14 * o.mu_0
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    e = rel_err(s.get_field("epsilon"), o.eps)
    f = rel_err(s.get_field("sigma"), o.pk1(o.eps))
    m = rel_err(s.mean_stress(), o.mean_stress())
    print(mode, grid, u_loop, e, f, m)
    assert e < 1e-10 and f < 1e-10 and m < 1e-11
    s.close()


@pytest.mark.parametrize("grid", [(12, 10, 6), (8, 14, 124)])
def test_viscosity(grid):
    """the stress stage on a random field and three iterations against the viscosity model (the stored-polarisation pass)"""
    phis, _ = phases(grid, 3)
    mus = [1.0, 0.05, 0.4]
    E = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])
    s = scalar_solver("viscosity", grid, mus, phis, tol=1e-14, maxiter=3)
    o = rr.ReussViscosityOracle(*grid, mats=[(m, 0.0) for m in mus], phis=phis, tol=1e-14, maxiter=3)
    assert s.run(E) == o.run(E) and s.iterations == o.iterations == 3
    assert abs(s.ref_material[0] - o.mu_0) <= 1e-14 * o.mu_0
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    e = rel_err(s.get_field("epsilon"), o.eps)
    m = rel_err(s.mean_stress(), o.mean_stress())
    eps = np.random.default_rng(3).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    t = rel_err(s.get_field("tau"), o.calc_stress(o.mu_0, 0.0, eps))
    print("viscosity", grid, e, m, t)
    assert e < 1e-9 and m < 1e-10 and t < rr.STAGE_TOL
    s.close()


# ---------------------------------------------------------------------------------------------- oracle-free
def test_series_mean_of_two_layers_in_porous_mode():
    """phi depends on x only, the layer boundary lies inside a voxel (x = 3.4 of 8).  The flux of the 1-D problem is uniform, so
    the discrete problem with the harmonic voxel has K_eff,xx = 1 / sum(f_i / k_i) of the TRUE layers exactly; the arithmetic
    voxel short-circuits the boundary and gives a strictly larger value"""
    grid, k = (8, 4, 6), [1.0, 10.0]
    phi1 = np.zeros(grid)
    phi1[:3] = 1.0
    phi1[3] = 0.4
    exact = 1.0 / (0.425 / k[1] + 0.575 / k[0])
    got = {}
    for rule in ("reuss", "voigt"):
        s = scalar_solver("porous", grid, k, [1.0 - phi1, phi1], tol=1e-10, maxiter=5000)
        s.set_options(mixing_rule=rule)
        assert s.run(np.array([1.0, 0.0, 0.0])) is False
        got[rule] = s.mean_stress()[0]
        s.close()
    print("layers", got, exact)
    assert abs(got["reuss"] - exact) <= 1e-8
    assert got["voigt"] > got["reuss"] + 1e-3


def test_bounds_on_a_sphere():
    """16^3, composite voxels at the sphere's surface, converged: E : <sigma> under reuss <= laminate <= voigt, reuss < voigt"""
    from fibergen_amd import LSSolver
    grid = (16, 16, 16)
    phis, mats = phases(grid, 2)
    w = {}
    for rule in ("reuss", "laminate", "voigt"):
        s = LSSolver(*grid)
        s.set_num_phases(2)
        for p in range(2):
            s.set_phase(p, mats[p][0], mats[p][1], phis[p])
        s.set_normals(sphere_normals(grid))
        s.set_options(mixing_rule=rule, tol=1e-9, method="cg")
        assert s.run(E_LOAD) is False
        sig = s.mean_stress()
        w[rule] = float(sig[:3] @ E_LOAD[:3] + 2 * sig[3:] @ E_LOAD[3:])
        s.close()
    print("bounds", w)
    assert w["reuss"] <= w["laminate"] * (1 + 1e-7) and w["laminate"] <= w["voigt"] * (1 + 1e-7)
    assert w["reuss"] < w["voigt"] * (1 - 1e-4)


@pytest.mark.parametrize("grid", [(16, 16, 16), (6, 14, 128)])
def test_homogeneous_body_equals_voigt(grid):
    from fibergen_amd import LSSolver
    phis, _ = phases(grid, 2)
    out = {}
    for rule in ("reuss", "voigt"):
        s = LSSolver(*grid)
        s.set_num_phases(2)
        for p in range(2):
            s.set_phase(p, 6.0, 8.0, phis[p])
        s.set_options(mixing_rule=rule, tol=1e-10, method="basic")
        assert s.run(E_LOAD) is False
        out[rule] = (s.iterations, s.mean_stress(), s.get_field("epsilon"))
        s.close()
    m = rel_err(out["reuss"][1], out["voigt"][1])
    e = np.abs(out["reuss"][2] - out["voigt"][2]).max()
    print("homogeneous", grid, m, e)
    assert out["reuss"][0] == out["voigt"][0] and m <= 1e-13 and e <= 1e-13


@pytest.mark.parametrize("grid,nph", [((16, 12, 10), 2), ((4, 16, 80), 3), ((4, 16, 80), 2)])
def test_switching_the_rule_on_a_live_solver(grid, nph):
    """voigt -> reuss -> voigt: the moduli arrays follow the rule (mod_dirty_), the first result comes back"""
    phis, mats = phases(grid, nph)
    s = gpu_solver(grid, phis, mats, tol=1e-8, method="basic")
    res = []
    for rule in ("voigt", "reuss", "voigt", "reuss"):
        s.set_options(mixing_rule=rule)
        assert s.run(E_LOAD) is False
        res.append((s.iterations, s.mean_stress()))
    o = oracle(grid, phis, mats, tol=1e-8)
    assert o.run(E_LOAD) is False
    print("switch", grid, nph, [r[0] for r in res], rel_err(res[1][1], res[0][1]), rel_err(res[1][1], o.mean_stress()))
    assert res[2][0] == res[0][0] and rel_err(res[2][1], res[0][1]) <= 1e-14
    assert res[3][0] == res[1][0] and rel_err(res[3][1], res[1][1]) <= 1e-14
    assert rel_err(res[1][1], res[0][1]) > 1e-4
    assert res[1][0] == o.iterations and rel_err(res[1][1], o.mean_stress()) < 1e-9
    s.close()


def test_refusals_at_the_library():
    from fibergen_amd import LSSolver
    from fibergen_amd.distributed import SlabGroup
    from fibergen_amd.solver import REUSS_ERRORS
    import general_reference as gr
    grid = (8, 8, 8)
    phis, mats = phases(grid, 2)
    E = np.array([1.0, 0, 0, 0, 0, 0])

    def refused(s, key, scan=True):
        with pytest.raises(RuntimeError) as e:
            s.run(E)
        assert str(e.value) == REUSS_ERRORS[key]
        if scan:
            with pytest.raises(RuntimeError) as e:
                s.calc_ref_material()
            assert str(e.value) == REUSS_ERRORS[key]
        s.close()

    s = gpu_solver(grid, phis, mats)
    s.set_phase_stiffness(1, gr.distinct_stiffness())
    refused(s, "general")
    refused(gpu_solver(grid, phis, mats, gamma_scheme="full_staggered"), "dfg")
    refused(gpu_solver(grid, phis, mats, method="polarization"), "method")
    refused(gpu_solver(grid, phis, mats, error_estimator="energy"), "estimator")
    refused(gpu_solver(grid, phis, [mats[0], (0.0, 1.0)]), "moduli")
    refused(gpu_solver(grid, phis, [mats[0], (1.0, -0.7)]), "moduli")
    refused(scalar_solver("porous", grid, [1.0, 0.0], phis), "constant")
    refused(scalar_solver("viscosity", grid, [1.0, -2.0], phis), "constant")
    s = scalar_solver("heat", grid, [1.0, 2.0], phis)
    s.set_phase_conductivity(1, [3.0, 1.0, 1.0, 0.0, 0.0, 0.5])
    refused(s, "aniso")
    g = SlabGroup(*grid, nranks=1)
    with pytest.raises(RuntimeError) as e:
        g.set_options(mixing_rule="reuss")
    assert str(e.value) == REUSS_ERRORS["slab"]
    g.close()

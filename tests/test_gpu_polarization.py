"""method "polarization" on the GPU against the NumPy restatement (polarization_reference.py): every pass of the loop, the
converged run, the effective stiffness against the CG solver, the branch counter, the refusals of the C boundary."""
import numpy as np
import pytest

import general_reference as gr
import polarization_reference as pr
from helpers import rel_err

pytestmark = pytest.mark.gpu

E_LOAD = np.array([0.5, -0.25, 1.0, 0.1, 0.2, 0.3])
SCHEMES = ["collocated", "willot", "staggered"]
# 41 x 33 x 11: the DFT fall-back and an odd nz; 40 x 24 x 80: a grid the tiled displacement sweep accepts (u_tile_supported)
GRIDS = [(8, 8, 8), (12, 10, 6), (16, 16, 16), (41, 33, 11), (40, 24, 80)]
# Per-pass parity tolerance: 10 x the largest relative error measured on the MI355X over all cases below: 2.35e-14 (staggered,
# three phases with a general phase and contrast 1000, 40 x 24 x 80; collocated and willot stay below 3e-15)
PASS_TOL = 2.35e-13


def phases(kind, grid):
    """iso/iso at contrast 1000, iso/general (all 21 constants distinct, normal-shear coupling), three phases"""
    if kind == "iso":
        return pr.sphere_phi(grid), [(1.0, 1.0), (1000.0, 1000.0)]
    if kind == "general":
        return pr.sphere_phi(grid), [(0.4, 0.6), gr.distinct_stiffness(100.0)]
    core, both = pr.sphere_phi(grid, 0.2)[1], pr.sphere_phi(grid, 0.38)[1]
    return [1.0 - both, both - core, core], [(1.0, 1.0), gr.random_spd(np.random.default_rng(2), scale=0.1), (1000.0, 1000.0)]


def gpu_solver(grid, phis, mats, scheme, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid)
    s.set_num_phases(len(mats))
    for p, m in enumerate(mats):
        if gr.is_general(m):
            s.set_phase(p, 0.0, 0.0, phis[p])
            s.set_phase_stiffness(p, m)
        else:
            s.set_phase(p, m[0], m[1], phis[p])
    s.set_options(method="polarization", gamma_scheme=scheme, **opts)
    return s


@pytest.mark.parametrize("kind", ["iso", "general", "three"])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("grid", GRIDS)
def test_per_pass_parity(grid, scheme, kind):
    """three passes from P = 4 mu_0 E: P after each pass and the strain after the conversion, relative to max |field|.
    Measured on the MI355X: at most 2.35e-14 (PASS_TOL is 10 x that)."""
    phis, mats = phases(kind, grid)
    s = gpu_solver(grid, phis, mats, scheme)
    o = pr.make_polarization_oracle(grid, mats, phis, scheme)
    o.calc_ref_material_polarization()
    mu_0 = s.calc_ref_material()[0]
    assert abs(mu_0 - o.mu_0) <= 1e-13 * o.mu_0
    P0 = 4 * o.mu_0 * E_LOAD
    P = np.empty((6,) + grid)
    P[:] = P0[:, None, None, None]
    worst = 0.0
    for k in range(3):
        P = o.polarization_scheme(P0, P)
        s.iterate(E_LOAD, 1)
        worst = max(worst, rel_err(s.get_field("polarization"), P))
    e_eps = rel_err(s.get_field("epsilon"), o.calc_polarization(P, inv=True))
    print("parity", grid, scheme, kind, worst, e_eps)
    with pytest.raises(RuntimeError, match="polarization"):   # the state was converted: no polarisation field any more
        s.get_field("polarization")
    s.close()
    assert worst <= PASS_TOL and e_eps <= PASS_TOL


@pytest.mark.parametrize("scheme", SCHEMES)
def test_converged_run(scheme):
    """16^3 at tol 1e-8: iteration count and residual history equal the restatement's (the <= 1e-9 criterion of the estimator
    tests), the strain field agrees, and two load steps continue like the restatement's"""
    grid = (16, 16, 16)
    phis, mats = phases("general", grid)
    s = gpu_solver(grid, phis, mats, scheme, tol=1e-8, maxiter=2000)
    o = pr.make_polarization_oracle(grid, mats, phis, scheme, tol=1e-8, maxiter=2000)
    assert s.run(E_LOAD) is False and o.run_polarization(E_LOAD) is False
    print("converged", scheme, s.iterations, o.iterations, rel_err(s.get_field("epsilon"), o.eps))
    assert s.iterations == o.iterations
    assert np.abs(np.array(s.residuals) - np.array(o.residuals)).max() <= 1e-9
    assert rel_err(s.get_field("epsilon"), o.eps) <= 1e-9
    assert s.run_load_steps(E_LOAD, params=[0.5, 1.0], first=0) is False and o.run_polarization_steps(E_LOAD, [0.5, 1.0]) is False
    assert s.iterations == o.step_iterations[-1]
    assert np.abs(np.array(s.residuals) - np.array(o.residuals)).max() <= 1e-9
    s.close()


@pytest.mark.parametrize("kind", ["iso", "ortho"])
def test_effective_stiffness_equals_cg(kind):
    """C_eff from six load cases: the polarisation loop against the CG solver on the same operator; what separates them is the
    solvers' tolerance, asserted at 1e-6 relative.  Both run at tol 1e-11: the epsilon estimator watches increments of a NORM,
    which near the solution are of second order in the field's error, so at tol 1e-9 the polarisation loop stopped 5.8e-7
    (iso) and 1.4e-6 (ortho) away from CG -- the run is tightened, the bound stays (measured at tol 1e-11: 7.4e-8 and 5.4e-8).  The general phase here has no
    normal-shear coupling: with coupling the reference's full dPK1 matrix is the transpose-weighted D C instead of C D
     and the loop's fixed point is that of another material."""
    from fibergen_amd import LSSolver
    grid = (16, 16, 16)
    phis = pr.sphere_phi(grid)
    mats = [(1.0, 1.0), (20.0, 30.0)] if kind == "iso" else [(1.0, 1.0), gr.random_spd(np.random.default_rng(5), coupling=False, scale=3.0)]
    C = {}
    for method in ("polarization", "cg"):
        s = gpu_solver(grid, phis, mats, "staggered", tol=1e-11, maxiter=4000)
        s.set_options(method=method)
        cols = []
        for c in range(6):
            E = np.zeros(6)
            E[c] = 1.0
            assert s.run(E) is False
            cols.append(s.mean_stress())
        C[method] = np.array(cols).T
        s.close()
    d = np.abs(C["polarization"] - C["cg"]).max() / np.abs(C["cg"]).max()
    print("C_eff", kind, d)
    assert d <= 1e-6


def test_generic_voxel_counter():
    grid = (12, 10, 6)
    sharp = pr.sphere_phi(grid, smooth=False)
    smooth = pr.sphere_phi(grid)
    nmixed = int(((smooth[1] > 0) & (smooth[1] < 1)).sum())
    assert nmixed > 0
    iso = [(1.0, 1.0), (10.0, 10.0)]
    for phis, mats, want in ((sharp, iso, 0), (smooth, iso, nmixed),
                             (smooth, [iso[0], gr.distinct_stiffness(2.0)], nmixed + int((smooth[1] == 1).sum()))):
        s = gpu_solver(grid, phis, mats, "staggered")
        s.calc_ref_material()
        s.iterate(E_LOAD, 1)
        assert s.counter("polarization_generic_voxels") == want
        assert want == int(pr.generic_mask(phis, mats).sum())
        s.close()


def test_refusals_of_the_c_boundary():
    from fibergen_amd import LSSolver
    from fibergen_amd.solver import POLARIZATION_ERRORS as ERR
    import re
    grid = (8, 8, 8)
    phis, mats = pr.sphere_phi(grid), [(1.0, 1.0), (10.0, 10.0)]
    cases = [({"mixing_rule": "laminate"}, ERR["mixing"]), ({"gamma_scheme": "full_staggered"}, ERR["dfg"]),
             ({"mode": "viscosity"}, ERR["mode"]), ({"mode": "heat"}, ERR["mode"]), ({"error_estimator": "sigma"}, ERR["estimator"]),
             ({"error_estimator": "energy"}, ERR["estimator"]), ({"error_estimator": "residual"}, ERR["estimator"])]
    for opts, msg in cases:
        s = gpu_solver(grid, phis, mats, "staggered")
        s.set_options(**opts)
        for call in (lambda: s.run(E_LOAD), lambda: s.iterate(E_LOAD, 1)):
            with pytest.raises(RuntimeError, match=re.escape(msg)):
                call()
        s.close()
    s = gpu_solver(grid, phis, mats, "staggered")
    P = np.diag([1.0, 1.0, 0.0, 0.5, 0.5, 0.5])
    s.set_bc_projector(P)
    E_bc = E_LOAD.copy()
    E_bc[2] = 0.0   # compatible with the projector: the strain in the stress-controlled direction is not prescribed
    with pytest.raises(RuntimeError, match=re.escape(ERR["bc"])):
        s.run(E_bc, np.zeros(6))
    for name in ("nesterov", "basic+el", "nl_cg"):
        with pytest.raises(RuntimeError, match="Unknown solver method"):
            s.set_options(method=name)
    assert s._lib.fg_set_option_i(s._h, b"method", 3) != 0
    s.close()


def test_estimator_none_runs_to_maxiter():
    grid = (8, 8, 8)
    s = gpu_solver(grid, pr.sphere_phi(grid), [(1.0, 1.0), (10.0, 10.0)], "collocated", error_estimator="none", maxiter=7)
    assert s.run(E_LOAD) is False
    assert s.iterations == 7 and s.residuals == [1.0] * 7
    s.close()


def test_state_is_settled_when_method_phases_or_reference_material_change():
    """a polarisation state left by fg_iterate never reaches another loop as if it were a strain: switching the method converts
    it first; changing a phase converts it with the phases it was built with; a pass on another mu_0 starts afresh"""
    grid = (8, 8, 8)
    phis, mats = pr.sphere_phi(grid), [(1.0, 1.0), (10.0, 10.0)]
    s = gpu_solver(grid, phis, mats, "collocated", u_loop=0)
    mu_0 = s.calc_ref_material()[0]
    s.iterate(E_LOAD, 2)
    t = gpu_solver(grid, phis, mats, "collocated", u_loop=0)
    t.calc_ref_material()
    t.iterate(E_LOAD, 2)
    eps = t.get_field("epsilon")                 # the converted strain of the same two passes
    s.set_options(method="basic")
    s.iterate(E_LOAD, 1)                          # must run on eps, not on P
    t.set_options(method="basic")
    t.set_field("epsilon", eps)
    t.iterate(E_LOAD, 1)
    assert rel_err(s.get_field("epsilon"), t.get_field("epsilon")) <= 1e-13
    # a phase changes while the state is held: the conversion uses the old phase
    s.set_options(method="polarization")
    t.set_options(method="polarization")
    s.iterate(E_LOAD, 2)
    t.iterate(E_LOAD, 2)
    want = t.get_field("epsilon")
    s.set_phase(1, 3.0, 4.0, phis[1])
    assert rel_err(s.get_field("epsilon"), want) <= 1e-13
    # another mu_0: the held state is dropped (converted), the next pass starts from 4 mu_0 E
    t.iterate(E_LOAD, 1)
    t.set_options(mu_0=2.0 * mu_0)
    t.iterate(E_LOAD, 1)
    u = gpu_solver(grid, phis, mats, "collocated", u_loop=0, mu_0=2.0 * mu_0)
    u.iterate(E_LOAD, 1)
    assert rel_err(t.get_field("polarization"), u.get_field("polarization")) <= 1e-13
    for x in (s, t, u):
        x.close()


def test_counter_survives_a_cg_run():
    grid = (12, 10, 6)
    phis, mats = pr.sphere_phi(grid), [(1.0, 1.0), (10.0, 10.0)]
    s = gpu_solver(grid, phis, mats, "staggered", tol=1e-6)
    s.calc_ref_material()
    s.iterate(E_LOAD, 1)
    want = int(pr.generic_mask(phis, mats).sum())
    s.set_options(method="cg")
    assert s.run(E_LOAD) is False
    assert s.counter("polarization_generic_voxels") == want
    s.close()

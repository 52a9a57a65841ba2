"""law="general" on the GPU: phases with a constant 6x6 stiffness (fg_set_phase_stiffness) against the NumPy restatement
(general_reference.py) -- the stress stage, the reference-material scan, the strain-state loops, the tiled sweep's anisotropic
form on every tile shape -- and the oracle-free checks: isotropic equivalence, the homogeneous anisotropic body, the project."""
import numpy as np
import pytest

import general_reference as gr
from helpers import rel_err, sphere_phi, two_phase_setup

pytestmark = pytest.mark.gpu

ISO0 = (0.4, 0.6)
ISO2 = (6.0, 8.0)
# smallest grids u_tile_supported accepts per default tile shape of the isotropic sweeps (tests/test_gpu_dfg_stages.py): <8,1>,
# <6,2>, <8,0>.  The anisotropic form has no <6,2> instantiation (it does not fit 168 VGPRs without scratch): the
# second grid, rows of 128 pairs, runs it on <8,0> tiles (three z tiles, the last clamped) -- two shapes are exercised, not three.
TILE_GRIDS = [(6, 14, 128), (4, 14, 256), (4, 16, 80)]


def stiff(seed, scale=1.0, coupling=True):
    return gr.random_spd(np.random.default_rng(seed), coupling=coupling, scale=scale)


def three_phases(grid):
    core, both = sphere_phi(grid, 0.2), sphere_phi(grid, 0.35)
    return [1.0 - both, both - core, core], [stiff(1, 0.3), ISO2, stiff(2, 0.1, coupling=False)]


def two_phases(grid, fibre=None):
    phi = sphere_phi(grid, 0.3)
    return [1.0 - phi, phi], [ISO0, gr.distinct_stiffness(0.5) if fibre is None else fibre]


def gpu_solver(grid, phis, mats, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid)
    s.set_num_phases(len(mats))
    for p, m in enumerate(mats):
        if gr.is_general(m):
            s.set_phase(p, 0.0, 0.0, phis[p])
            s.set_phase_stiffness(p, m)
        else:
            s.set_phase(p, m[0], m[1], phis[p])
    s.set_options(**opts)
    return s


def oracle(grid, phis, mats, **kw):
    return gr.GeneralLSOracle(*grid, mats=mats, phis=phis, **kw)


# ---------------------------------------------------------------------------------------------- stage
@pytest.mark.parametrize("grid", [(8, 8, 8), (12, 10, 6), (6, 5, 7)])
def test_stress_stage_three_phases(grid):
    """k_stress through pk1_voigt's per-phase dispatch: two general phases and an isotropic one, at test_gpu_parity's tolerance"""
    phis, mats = three_phases(grid)
    s, o = gpu_solver(grid, phis, mats, mu_0=0.77, lambda_0=0.31), oracle(grid, phis, mats)
    eps = np.random.default_rng(10).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    e = rel_err(s.get_field("tau"), o.calc_stress(0.77, 0.31, eps))
    e2 = rel_err(s.get_field("sigma"), o.calc_stress(0.0, 0.0, eps))
    o.eps = eps
    e3 = rel_err(s.mean_stress(), o.mean_stress())
    print("stage", grid, e, e2, e3)
    assert e < 1e-14 and e2 < 1e-14 and e3 < 1e-12
    s.close()


@pytest.mark.parametrize("nph", [2, 3])
def test_reference_material_scan(nph):
    grid = (12, 10, 6)
    phis, mats = two_phases(grid) if nph == 2 else three_phases(grid)
    s, o = gpu_solver(grid, phis, mats), oracle(grid, phis, mats)
    o.calc_ref_material()
    mu_0, lam_0 = s.calc_ref_material()
    print("scan", nph, mu_0, o.mu_0)
    assert abs(mu_0 - o.mu_0) <= 1e-13 * o.mu_0 and lam_0 == 0.0
    s.set_options(ref_scale=0.5)
    o.ref_scale = 0.5
    o.calc_ref_material()
    assert abs(s.calc_ref_material()[0] - o.mu_0) <= 1e-13 * o.mu_0
    s.close()


# ---------------------------------------------------------------------------------------------- loops
E_LOAD = np.array([0.5, -0.25, 1.0, 0.1, 0.2, 0.3])


def run_both(grid, phis, mats, method, maxiter, P=None, **opts):
    o = oracle(grid, phis, mats, tol=1e-14, maxiter=maxiter)
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
    # test_gpu_parity's loop tolerances (cg / basic): residual history, strain field, mean stress
    rtol, etol, mtol = (1e-10, 1e-8, 1e-9) if method == "cg" else (1e-11, 1e-9, 1e-10)
    r = np.abs(np.array(s.residuals) - np.array(o.residuals)).max()
    e = rel_err(s.get_field("epsilon"), o.eps)
    m = rel_err(s.mean_stress(), o.mean_stress())
    print(what, method, "residuals", r, "eps", e, "mean stress", m)
    assert len(s.residuals) == len(o.residuals)
    assert r < rtol and e < etol and m < mtol


@pytest.mark.parametrize("method,maxiter", [("basic", 5), ("cg", 4)])
@pytest.mark.parametrize("nph", [2, 3])
def test_strain_state_loops(nph, method, maxiter):
    """grids the tiles do not fit, and three phases: basic_scheme and the strain-space CG through k_stress"""
    grid = (16, 12, 10)
    phis, mats = two_phases(grid) if nph == 2 else three_phases(grid)
    s, o = run_both(grid, phis, mats, method, maxiter)
    check_loop(s, o, method, "strain-state %d phases" % nph)
    assert s.counter("u_tile_aniso") == 0
    s.close()


def test_three_phases_on_a_tile_grid_take_the_strain_state_path():
    grid = TILE_GRIDS[2]
    phis, mats = three_phases(grid)
    s, o = run_both(grid, phis, mats, "basic", 5)
    check_loop(s, o, "basic", "three phases, tile grid")
    assert s.counter("u_tile_aniso") == 0
    s.close()


@pytest.mark.parametrize("grid", TILE_GRIDS)
@pytest.mark.parametrize("case", ["basic", "mixed_bc", "cg"])
def test_tiled_sweep_anisotropic_form(grid, case):
    """two complementary phases, the fibre with 21 distinct constants: k_u_tile ANISO (plain, with the sums of tau, with the CG
    direction) against the restatement, and against aniso_tile = 0 at the tolerance of test_tiled_displacement_sweep"""
    phis, mats = two_phases(grid)
    method, maxiter = ("cg", 4) if case == "cg" else ("basic", 5)
    P = None
    if case == "mixed_bc":
        P = np.zeros((6, 6))
        P[0, 0] = 1.0
        P[5, 5] = 0.5
    s, o = run_both(grid, phis, mats, method, maxiter, P=P)
    check_loop(s, o, method, "tile %s %s" % (grid, case))
    assert s.counter("u_tile_aniso") > 0
    s0, _ = run_both(grid, phis, mats, method, maxiter, P=P, aniso_tile=0)
    assert s0.counter("u_tile_aniso") == 0
    r = np.abs(np.array(s.residuals) - np.array(s0.residuals)).max()
    e = rel_err(s.get_field("epsilon"), s0.get_field("epsilon"))
    m = rel_err(s.mean_stress(), s0.mean_stress())
    print("tile vs strain state", grid, case, r, e, m)
    assert r < 1e-12 and e < 1e-11 and m < 1e-12
    s.close()
    s0.close()


# ---------------------------------------------------------------------------------------------- oracle-free
def c_eff(s):
    """calc_effective_properties F:26030-26088 through the C ABI: six unit load cases, shear columns halved"""
    S, its = np.empty((6, 6)), []
    for i in range(6):
        E = np.zeros(6)
        E[i] = 1.0
        assert s.run(E) is False
        S[:, i] = s.mean_stress()
        its.append(s.iterations)
    S[:, 3:] *= 0.5
    return S, its


@pytest.mark.parametrize("grid", [(16, 16, 16), (6, 14, 128)])
def test_isotropic_equivalence_end_to_end(grid):
    """(mu, lambda) against the equivalent C through fg_set_phase_stiffness, both at the default options (16^3: the untiled
    displacement loop against the strain-state pass; 6 x 14 x 128: the PHI2 sweep against its anisotropic form): every factor 2
    and every index of the general path, without an oracle.  The basic scheme is the method of this check: it is a contraction,
    so two evaluations that differ in rounding stay 1e-16-close through the run; the conjugate gradients amplify such
    differences (the suite holds its two isotropic CG forms to 1e-9 of each other) and are checked against the restatement
    above instead."""
    mats, phis, _ = two_phase_setup(grid)
    a = gpu_solver(grid, phis, mats, tol=1e-8, method="basic")
    b = gpu_solver(grid, phis, [gr.iso_stiffness(*m) for m in mats], tol=1e-8, method="basic")
    Ca, ia = c_eff(a)
    Cb, ib = c_eff(b)
    es = rel_err(b.get_field("sigma"), a.get_field("sigma"))
    ec = rel_err(Cb, Ca)
    print("iso equivalence", grid, ia, ib, es, ec, b.counter("u_tile_aniso"))
    assert ia == ib
    assert es <= 1e-12 and ec <= 1e-12
    assert abs(a.ref_material[0] - b.ref_material[0]) <= 1e-14 * a.ref_material[0]
    assert (b.counter("u_tile_aniso") > 0) == (grid[2] == 128)
    a.close()
    b.close()


@pytest.mark.parametrize("grid", [(16, 16, 16), (6, 14, 128)])
def test_homogeneous_anisotropic_body(grid):
    C = stiff(5, 2.0)
    phis, _ = two_phases(grid)
    s = gpu_solver(grid, phis, [C, C], tol=1e-10, method="basic")
    assert s.run(E_LOAD) is False
    # the first pass lands on the fixed point eps = E (residual 1: the change from the zero field), the second measures no change
    print("homogeneous", grid, s.iterations, s.residuals)
    assert s.iterations == 2 and s.residuals[0] == pytest.approx(1.0, abs=1e-14) and s.residuals[1] <= 1e-14
    assert np.abs(s.get_field("epsilon") - E_LOAD[:, None, None, None]).max() < 1e-13
    Ce, its = c_eff(s)
    print("homogeneous", grid, rel_err(Ce, C), its)
    assert its == [2] * 6 and rel_err(Ce, C) <= 1e-12
    s.close()


def test_set_phase_makes_the_phase_isotropic_again_and_rejections():
    from fibergen_amd import LSSolver
    from fibergen_amd.distributed import SlabGroup
    from helpers import make_oracle
    grid = (8, 8, 8)
    mats, phis, _ = two_phase_setup(grid)
    s = gpu_solver(grid, phis, [mats[0], stiff(3)], mu_0=0.77, lambda_0=0.31)
    s.set_phase(1, *mats[1])
    eps = np.random.default_rng(3).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    assert rel_err(s.get_field("tau"), make_oracle(grid).calc_stress(0.77, 0.31, eps)) < 1e-14
    C = stiff(4)
    with pytest.raises(RuntimeError, match="phase index out of range"):
        s.set_phase_stiffness(2, C)
    with pytest.raises(RuntimeError, match="phase index out of range"):
        s.set_phase_stiffness(-1, C)
    bad = C.copy()
    bad[0, 4] += 1e-11 * np.abs(C).max()
    with pytest.raises(RuntimeError, match="not symmetric"):
        s.set_phase_stiffness(1, bad)
    ok = C.copy()
    ok[0, 4] += 1e-13 * np.abs(C).max()
    s.set_phase_stiffness(1, ok)
    # the combinations general phases do not cover are refused when the run starts
    E = np.array([1.0, 0, 0, 0, 0, 0])
    for opts, msg in (({"mixing_rule": "laminate"}, "Voigt mixing only"), ({"gamma_scheme": "full_staggered"}, "full_staggered"),
                      ({"mode": "heat"}, "elasticity mode only"), ({"mode": "viscosity"}, "elasticity mode only")):
        t = gpu_solver(grid, phis, [mats[0], C], **opts)
        t.set_normals(np.zeros((3,) + grid))
        with pytest.raises(RuntimeError, match=msg):
            t.run(E)
        with pytest.raises(RuntimeError, match=msg):
            t.calc_ref_material()
        t.close()
    g = SlabGroup(*grid, nranks=1)
    g.set_num_phases(2)
    with pytest.raises(RuntimeError, match="slab-decomposed"):
        g.set_phase_stiffness(1, C)
    with pytest.raises(RuntimeError, match="slab-decomposed"):
        LSSolver.set_phase_stiffness(g.members[0], 1, C)
    g.close()
    s.close()


def test_collocated_and_willot_schemes_run_general_phases():
    """the Fourier-space schemes go through the same k_stress: five passes against the restatement"""
    from willot_reference import WillotMixin
    grid = (12, 10, 6)
    phis, mats = two_phases(grid)

    class WillotGeneral(WillotMixin, gr.GeneralLSOracle):
        pass
    for scheme, cls in (("collocated", gr.GeneralLSOracle), ("willot", WillotGeneral)):
        o = cls(*grid, mats=mats, phis=phis, tol=1e-14, maxiter=5, gamma_scheme=scheme)
        s = gpu_solver(grid, phis, mats, tol=1e-14, maxiter=5, method="basic", gamma_scheme=scheme)
        assert s.run(E_LOAD) == o.run(E_LOAD) and s.iterations == o.iterations == 5
        check_loop(s, o, "basic", scheme)
        s.close()


PROJECT_XML = """
<settings>
  <solver n="16">
    <method>basic</method><tol>1e-11</tol>
    <materials>
      <matrix E="1" nu="0.3" />
      <fibre law="general" c11="30" c22="12" c33="11" c12="5" c13="4.5" c23="4" c44="3.5" c55="5.5" c66="6" c14="0.3" c25="-0.2"
             c36="0.1" c45="0.15" />
    </materials>
  </solver>
  <actions><select_material name="fibre" /><place_fiber R="0.3" /><calc_effective_properties /></actions>
</settings>
"""


def test_project_with_a_general_fibre():
    from fibergen_amd import FG
    fg = FG()
    fg.set_xml(PROJECT_XML)
    fg.run()
    Cp = np.array(fg.get_effective_property())
    assert Cp.shape == (6, 6)
    C = np.array(materials_stiffness())
    phi = fg._lss.get_field("phi")
    from helpers import lame
    mu, lam = lame(1.0, 0.3)
    s = gpu_solver((16, 16, 16), [phi[0], phi[1]], [(mu, lam), C], tol=1e-11, method="basic")
    Cs, _ = c_eff(s)
    print("project", rel_err(Cp, Cs), np.abs(Cp - Cp.T).max() / np.abs(Cp).max())
    assert rel_err(Cp, Cs) <= 1e-12
    assert np.abs(Cp - Cp.T).max() <= 1e-10 * np.abs(Cp).max()
    # anisotropy arrives in the answer: the normal-shear coupling of the fibre is not averaged away
    assert abs(Cp[0, 3]) > 1e-4 and Cp[0, 0] > Cp[1, 1] > 1.0
    s.close()


def materials_stiffness():
    import xml.etree.ElementTree as ET
    from fibergen_amd import materials
    attrs = ET.fromstring(PROJECT_XML).find("solver/materials/fibre").attrib
    return materials.general_stiffness(attrs)

"""gamma_scheme full_staggered (the doubly fine grid, use_dfg F:14894-14897) on the GPU: the C ABI against the literal
fine-grid restatement of tests/dfg_reference.py, and the reference's viscosity demos through FG."""
import numpy as np
import pytest

from dfg_reference import (DfgLSOracle, DfgViscosityOracle, fine_images, input_kinds, replicate, restrict_component, split_input,
                           tile_shape)
from helpers import INCLUSION, MATRIX, lame, rel_err, sphere_phi

pytestmark = pytest.mark.gpu

E6 = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])


def _fine_random(grid, seed):
    f = np.random.default_rng(seed).random(tuple(2 * n for n in grid))
    return [1.0 - f, f]


def _gpu(grid, dims, mats, fine=None, coarse=None, mode="elasticity", **kw):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid, *dims)
    s.set_options(mode=mode, gamma_scheme="full_staggered")
    s.set_num_phases(len(mats))
    for p, (mu, lam) in enumerate(mats):
        s.set_phase(p, mu, lam, None if coarse is None else coarse[p])
        if fine is not None:
            s.set_phase_fine(p, fine[p])
    s.set_options(**kw)
    return s


def _check(s, o, E, S=None, cg=False, P=None):
    if P is not None:
        s.set_bc_projector(P)
    assert s.run(E, S) is False
    assert (o.run_cg(E, S, P) if cg else o.run(E, S0=S, P=P)) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-9
    assert rel_err(s.get_field("sigma"), o.pk1(o.eps)) < 1e-9
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-9
    assert rel_err(s.get_field("phi"), np.array(o.phis)) < 1e-15


# (16, 16, 128) and (8, 14, 124): the tiled sweeps (one wave per row / halo lanes)
GRIDS = [((16, 16, 16), (1, 1, 1)), ((12, 10, 6), (2.0, 1.0, 0.5)), ((9, 7, 5), (1, 1, 1)), ((16, 16, 128), (1, 1, 1)),
         ((8, 14, 124), (1.0, 2.0, 0.5))]


@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("grid,dims", GRIDS)
def test_elasticity_matches_fine_grid_oracle(grid, dims, method):
    mats = [lame(**MATRIX), lame(**INCLUSION)]
    fine = _fine_random(grid, 11)
    s = _gpu(grid, dims, mats, fine, tol=1e-6, method=method)
    o = DfgLSOracle(*grid, *dims, mats=mats, phis=[np.zeros(grid)] * 2, phis_fine=fine, tol=1e-6)
    _check(s, o, np.array([1.0, 0, 0, 0, 0, 0.5]), cg=method == "cg")
    s.close()


@pytest.mark.parametrize("grid", [(16, 16, 16), (16, 16, 128)])
def test_elasticity_mixed_bc(grid):
    mats = [lame(**MATRIX), lame(**INCLUSION)]
    fine = _fine_random(grid, 12)
    s = _gpu(grid, (1, 1, 1), mats, fine, tol=1e-8, bc_tol=1e-8)
    o = DfgLSOracle(*grid, mats=mats, phis=[np.zeros(grid)] * 2, phis_fine=fine, tol=1e-8, bc_tol=1e-8)
    P = np.diag([1.0, 0, 0, 0, 0, 0.5])   # Voigt projector: shear entries 1/2
    _check(s, o, np.array([1.0, 0, 0, 0, 0, 0.3]), np.zeros(6), P=P)
    s.close()


@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("grid,dims", [GRIDS[0], GRIDS[1], GRIDS[2], GRIDS[4]])
def test_viscosity_matches_fine_grid_oracle(grid, dims, method):
    fine = _fine_random(grid, 13)
    s = _gpu(grid, dims, [(1.0, 0.0), (0.05, 0.0)], fine, mode="viscosity", tol=1e-8, method=method)
    o = DfgViscosityOracle(*grid, *dims, mats=[(1.0, 0.0), (0.05, 0.0)], phis=[np.zeros(grid)] * 2, phis_fine=fine, tol=1e-8)
    _check(s, o, E6, cg=method == "cg")
    s.close()


@pytest.mark.parametrize("grid", [(12, 10, 6), (16, 16, 128)])
def test_replicated_fine_image_equals_coarse_input(grid):
    """half_staggered / raw data: a coarse field is taken as its piecewise-constant replica on the fine grid"""
    mats = [lame(**MATRIX), lame(**INCLUSION)]
    phi1 = sphere_phi(grid, 0.3)
    coarse = [1.0 - phi1, phi1]
    a = _gpu(grid, (1, 1, 1), mats, coarse=coarse, tol=1e-8)
    b = _gpu(grid, (1, 1, 1), mats, fine=[replicate(p) for p in coarse], tol=1e-8)
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    assert a.run(E) is False and b.run(E) is False
    assert a.iterations == b.iterations
    assert rel_err(a.get_field("epsilon"), b.get_field("epsilon")) < 1e-12
    assert rel_err(a.mean_stress(), b.mean_stress()) < 1e-12
    a.close()
    b.close()


def test_scheme_in_effect():
    """a sphere on the fine grid: full_staggered differs from the staggered run on its coarse field"""
    from fibergen_amd import LSSolver
    grid = (16, 16, 16)
    mats = [lame(**MATRIX), lame(**INCLUSION)]
    f1 = sphere_phi(tuple(2 * n for n in grid), 0.3)
    s = _gpu(grid, (1, 1, 1), mats, [1.0 - f1, f1], tol=1e-8)
    c1 = restrict_component(f1, (0, 0, 0))
    t = LSSolver(*grid)
    t.set_num_phases(2)
    t.set_phase(0, *mats[0], 1.0 - c1)
    t.set_phase(1, *mats[1], c1)
    t.set_options(tol=1e-8)
    E = np.array([0, 0, 0, 0, 0, 1.0])
    assert s.run(E) is False and t.run(E) is False
    assert rel_err(s.get_field("phi"), t.get_field("phi")) < 1e-15
    assert rel_err(s.mean_stress(), t.mean_stress()) > 1e-6
    s.close()
    t.close()


def test_out_of_scope_combinations_raise():
    from fibergen_amd import FG, LSSolver, _lib
    grid = (8, 8, 8)
    fine = _fine_random(grid, 14)
    mats = [lame(**MATRIX), lame(**INCLUSION)]
    s = _gpu(grid, (1, 1, 1), mats, fine, mixing_rule="laminate")
    s.set_normals(np.ones((3,) + grid) / np.sqrt(3))
    with pytest.raises(RuntimeError, match="Voigt mixing only"):
        s.run(np.array([1.0, 0, 0, 0, 0, 0]))
    s.close()
    s = _gpu(grid, (1, 1, 1), mats, fine, mode="heat")
    with pytest.raises(RuntimeError, match="heat / porous"):
        s.run(np.array([1.0, 0, 0, 0, 0, 0]))
    s.close()
    t = LSSolver(*grid)   # a fine image needs the scheme
    t.set_num_phases(1)
    with pytest.raises(RuntimeError, match="full_staggered"):
        t.set_phase_fine(0, np.ones((16, 16, 16)))
    t.close()
    lib = _lib.load()
    h = lib.fg_create_slab(8, 8, 8, 1.0, 1.0, 1.0, 0, 0, 1)
    assert h
    assert lib.fg_set_option_i(h, b"gamma_scheme", 2) != 0 and b"slab" in lib.fg_last_error(h)
    lib.fg_destroy(h)
    for mode, mix in (("heat", "voigt"), ("elasticity", "laminate")):
        fg = FG()
        fg.set_xml("""<settings><solver n="8"><mode>%s</mode><mixing_rule>%s</mixing_rule>
          <gamma_scheme>full_staggered</gamma_scheme><materials><a mu="1" lambda="1" /></materials></solver>
          <actions><run_load_case e11="1" /></actions></settings>""" % (mode, mix))
        with pytest.raises(RuntimeError, match="full_staggered"):
            fg.run()


NUNAN_KELLER_XML = """<?xml version="1.0" encoding="utf-8"?>
<settings>
  <print_precision>6</print_precision>
  <solver n="%d">
    <materials><matrix mu="1" /><fiber mu="0" /></materials>
    <mode>viscosity</mode>
    <gamma_scheme>full_staggered</gamma_scheme>
    <method>cg</method>
    <tol>1e-5</tol>
    <smooth_tol>1e-5</smooth_tol>
  </solver>
  <actions><select_material name="fiber" /><place_fiber V="0.2" /><calc_effective_properties /></actions>
</settings>"""


@pytest.mark.parametrize("n", [32, 64])
def test_fg_nunan_keller_full_staggered(n):
    """demo/viscosity/nunan_keller/project.xml with its full_staggered, at V = 0.2: alpha and beta within the staggered
    test's 3 % / 2.5 % of Nunan & Keller's table.  Measured: alpha -1.15 %, beta -0.46 % at 32^3; alpha -0.17 %,
    beta -0.01 % at the demo's 64^3 (the staggered scheme: +1.72 % / +1.33 % at 64^3)."""
    from fibergen_amd import FG
    from test_oracle_pins import NUNAN_KELLER
    fg = FG()
    fg.set_xml(NUNAN_KELLER_XML % n)
    assert fg.run() == 0
    mu_eff = fg.get_effective_property()
    alpha = 0.5 * (mu_eff[0][0] - mu_eff[0][1]) - 1
    beta = mu_eff[3][3] - 1
    print("nunan_keller full_staggered n=%d: alpha %+.4f %%, beta %+.4f %%"
          % (n, 100 * (alpha / NUNAN_KELLER[0.2][0] - 1), 100 * (beta / NUNAN_KELLER[0.2][1] - 1)))
    assert fg.get_volume_fraction("fiber") == pytest.approx(0.2, rel=2e-3)
    assert alpha == pytest.approx(NUNAN_KELLER[0.2][0], rel=0.03)
    assert beta == pytest.approx(NUNAN_KELLER[0.2][1], rel=0.025)


VISCOSITY_XML = """<settings>
  <solver n="%d">
    <tol>1e-4</tol>
    <maxiter>1000</maxiter>
    <materials><matrix mu="1" /><fiber mu="0.001" /></materials>
    <method>cg</method>
    <gamma_scheme>full_staggered</gamma_scheme>
    <mode>viscosity</mode>
  </solver>
  <actions><select_material name="fiber" /><place_fiber R="0.2" /><run_load_case e11="1" e22="-1" /></actions>
</settings>"""


def test_fg_viscosity_demo_full_staggered():
    """demo/viscosity/viscosity/project.xml as written but n = 16: converges; its result equals the fine-grid oracle on the
    same voxelisation (2n grid), whose restriction is the field FG reports as "phi"."""
    from fibergen_amd import FG, geometry
    from fibergen_amd.fg import _normalize_phi
    n = 16
    fg = FG()
    fg.set_xml(VISCOSITY_XML % n)
    assert fg.run() == 0
    lss = fg._lss
    phi = fg.get_field("phi")
    phif, _, _ = geometry.voxelize(fg._fibers, (2 * n,) * 3, fg._dims, fg._x0, 2, fg._matrix_mat)
    phif = _normalize_phi(phif)
    o = DfgViscosityOracle(n, n, n, mats=[(1.0, 0.0), (0.001, 0.0)], phis=[np.zeros((n,) * 3)] * 2, phis_fine=list(phif), tol=1e-4,
                           maxiter=1000)
    assert rel_err(np.asarray(phi).reshape(2, n, n, n), np.array(o.phis)) < 1e-14
    E = np.array([1.0, -1.0, 0, 0, 0, 0])
    assert o.run_cg(E) is False
    assert lss.iterations == o.iterations
    assert rel_err(lss.mean_stress(), o.mean_stress()) < 1e-8


TILED_GRIDS = [((6, 14, 128), (2.0, 1.0, 0.5)), ((16, 16, 128), (1, 1, 1)), ((4, 14, 256), (1.0, 1.5, 0.8)), ((5, 20, 256), (1, 1, 1)),
               ((5, 14, 100), (0.7, 1.3, 2.1)), ((4, 16, 80), (1, 1, 1)), ((4, 14, 200), (2.0, 1.0, 0.5)), ((6, 15, 130), (1, 1, 1)),
               ((8, 14, 124), (1.0, 2.0, 0.5))]


@pytest.mark.parametrize("variant", ["basic_mixed_bc", "cg", "cg_mixed_bc", "viscosity_mixed_bc"])
@pytest.mark.parametrize("grid,dims", TILED_GRIDS, ids=["%dx%dx%d-%s" % (g + (tile_shape(g).replace(" ", "-"),)) for g, _ in TILED_GRIDS])
def test_every_tile_shape_converged_runs(grid, dims, variant):
    """Converged runs on every shape of the five-moduli tiled sweeps, three phases (coarse, fine, coarse input) with pure cells:
    basic_mixed_bc -- the displacement loop with the sums of tau (k_u_tile<..., SUMT, 5>); cg -- the displacement-space CG
    (launch_u_tile_cg: k_u_tile<..., CGP, 5>); cg_mixed_bc -- a projector sends CG to strain space (plan::u_loop of fg_sweep_plan.h is false
    with a projector unless mixed BC are allowed, i.e. in run() of the basic scheme): k_eps_tile<..., 5> per operator
    application; viscosity_mixed_bc -- k_eps_tile<..., 5> with the recomputing tail and the adjusted sums"""
    rng = np.random.default_rng(15)
    viscosity = variant.startswith("viscosity")
    mats = [(1.0, 0.0), (0.05, 0.0), (3.0, 0.0)] if viscosity else [lame(**MATRIX), lame(**INCLUSION), (0.9, 1.7)]
    fine, coarse, ofine = split_input(fine_images(rng, grid, 3), input_kinds("mixed", 3))
    cg = variant.startswith("cg")
    kw = dict(tol=1e-6, bc_tol=1e-8) if variant.endswith("mixed_bc") else dict(tol=1e-6)
    from fibergen_amd import LSSolver
    s = LSSolver(*grid, *dims)
    s.set_options(mode="viscosity" if viscosity else "elasticity", gamma_scheme="full_staggered")
    s.set_num_phases(3)
    for p, (mu, lam) in enumerate(mats):
        s.set_phase(p, mu, lam, coarse[p])
        if fine[p] is not None:
            s.set_phase_fine(p, fine[p])
    s.set_options(method="cg" if cg else "basic", **kw)
    o = (DfgViscosityOracle if viscosity else DfgLSOracle)(*grid, *dims, mats=mats, phis=[np.zeros(grid)] * 3, phis_fine=ofine, **kw)
    if variant == "viscosity_mixed_bc":
        _check(s, o, np.array([0, 0, 0, 0.3, -0.2, 1.0]), np.zeros(6), P=np.diag([0.0, 0, 0, 0.5, 0.5, 0.5]))
    elif variant.endswith("mixed_bc"):
        _check(s, o, np.array([1.0, 0, 0, 0, 0, 0.3]), np.zeros(6), cg=cg, P=np.diag([1.0, 0, 0, 0, 0, 0.5]))
    else:
        _check(s, o, np.array([1.0, 0, 0, 0, 0, 0.5]), cg=cg)
    s.close()

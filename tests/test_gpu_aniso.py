"""GPU parity of law="aniso" in the scalar modes (a constant symmetric 3x3 conductivity per phase): the HIP path through the
C ABI against tests/aniso_reference.py on the same phase fields, and against closed forms that need no restatement.

K comes from a seeded random SPD 3x3 (six distinct constants, non-zero off-diagonals) at a contrast of about 10.  Two
complementary phases on grids the tiles fit run k_sc_tile_aniso (option aniso_sc_tile, counter "sc_tile_aniso"); everything else
the exact-order kernels (the 13-point sweep k_sc_sweep_aniso, k_sc_flux, k_sc_minmax_aniso)."""
import numpy as np
import pytest

from aniso_reference import AnisoScalarOracle, FixedRefOracle, check_laminate, k6, layer_problem, random_spd3, voigt_tangent3
from helpers import rel_err, sphere_phi
from test_gpu_fuzz import smooth_field

pytestmark = pytest.mark.gpu

E3 = np.array([1.0, -0.5, 0.25])


def two_K(seed=7):
    rng = np.random.default_rng(seed)
    return [random_spd3(rng, 1.0), random_spd3(rng, 10.0)]


def _solver(grid, mats, phis, dims=(1.0, 1.0, 1.0), mode="porous", **kw):
    """mats[p]: a number (law iso) or a symmetric 3x3 (law aniso)"""
    from fibergen_amd import LSSolver
    s = LSSolver(*grid, *dims)
    s.set_options(mode=mode)
    s.set_num_phases(len(mats))
    for p, (m, phi) in enumerate(zip(mats, phis)):
        if np.ndim(m) == 2:
            s.set_phase_conductivity(p, m if p % 2 else k6(m), phi)   # both input forms
        else:
            s.set_phase(p, m, 0.0, phi)
    s.set_options(**kw)
    return s


def _oracle(cls, grid, mats, phis, dims=(1.0, 1.0, 1.0), **kw):
    return cls(*grid, mus=mats, phis=phis, dx=dims[0], dy=dims[1], dz=dims[2], **kw)


def eig_mu0(phis, mats):
    w = np.linalg.eigvalsh(voigt_tangent3(phis, mats).reshape(-1, 3, 3))
    return 0.25 * (max(float(w.min()), 0.0) + float(w.max()))


@pytest.mark.parametrize("grid,dims", [((16, 16, 16), (1, 1, 1)), ((12, 10, 6), (2.0, 1.0, 0.5)), ((9, 7, 5), (1, 1, 1)),
                                       ((32, 16, 64), (1, 1, 1)), ((8, 16, 5), (1, 1, 1))])
@pytest.mark.parametrize("u_loop", [1, 2])
def test_aniso_run_matches_reference(grid, dims, u_loop):
    """the grids, cell sizes and bars of test_scalar_run_matches_oracle.  mu_0 is held against numpy's eigvalsh at 1e-13
    relative (symmetric eigenvalues are perfectly conditioned; about 450 ulp for the device's 3x3 solve), then handed to the
    restatement, so that its last bits do not decide the histories."""
    phi1 = sphere_phi(grid, 0.3)
    mats, phis = two_K(), [1 - phi1, phi1]
    s = _solver(grid, mats, phis, dims, tol=1e-9, u_loop=u_loop)
    assert s.run(E3) is False
    mu_0 = s.ref_material[0]
    assert abs(mu_0 - eig_mu0(phis, mats)) <= 1e-13 * mu_0
    o = _oracle(FixedRefOracle, grid, mats, phis, dims, tol=1e-9, mu_0=mu_0)
    assert o.run(E3) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    g = s.get_field("epsilon")
    assert g.shape == (3,) + grid
    assert rel_err(g, o.eps) < 1e-10
    assert rel_err(s.get_field("sigma"), o.pk1(o.eps)) < 1e-10
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-11
    np.testing.assert_allclose(s.mean_strain(), E3, atol=1e-12)
    T = s.get_field("u")
    To = o.potential()
    assert T.shape == (1,) + grid and np.abs(T[0] - To).max() < 1e-10 * max(1.0, np.abs(To).max())
    # raw passes continue from the state
    s.iterate(E3, 2)
    g2 = o.basic_scheme(E3, o.basic_scheme(E3, o.eps))
    assert rel_err(s.get_field("epsilon"), g2) < 1e-10
    s.close()


SHORT_GRIDS = [(1, 7, 5), (2, 7, 5), (6, 1, 5), (6, 2, 5), (6, 5, 1), (6, 5, 2), (2, 2, 2), (1, 1, 8), (1, 16, 1)]
_short_oracles = {}


def short_axis_phi(grid):
    """the sphere, or a smooth random field where the sphere's fraction is the same in every voxel of the grid"""
    phi1 = sphere_phi(grid, 0.3)
    if phi1.min() == phi1.max():
        phi1 = smooth_field(np.random.default_rng(5), grid)
    assert 0.0 <= phi1.min() < phi1.max() <= 1.0
    return phi1


@pytest.mark.parametrize("grid", SHORT_GRIDS)
@pytest.mark.parametrize("u_loop", [1, 2])
@pytest.mark.parametrize("method", ["basic", "cg"])
def test_aniso_short_axes(grid, u_loop, method):
    """axes of length 1 and 2: the 13-point stencil (k_sc_sweep_aniso, u_loop 1 and 2 alike for aniso phases off the tiled grids)
    wraps +-1 in two directions at once, and both neighbours along such an axis are the voxel itself (length 1) or one and the
    same voxel (length 2).  Against the restatement at the bars of test_aniso_run_matches_reference, for method basic and cg."""
    dims = (2.0, 1.0, 0.5)
    phi1 = short_axis_phi(grid)
    mats, phis = two_K(), [1 - phi1, phi1]
    s = _solver(grid, mats, phis, dims, tol=1e-9, u_loop=u_loop, method=method)
    assert s.run(E3) is False
    assert s.counter("sc_tile_aniso") == 0
    mu_0 = s.ref_material[0]
    assert abs(mu_0 - eig_mu0(phis, mats)) <= 1e-13 * mu_0
    key = (grid, method, mu_0)
    if key not in _short_oracles:     # one restatement run for both u_loop values (left unchanged)
        o = _oracle(FixedRefOracle, grid, mats, phis, dims, tol=1e-9, mu_0=mu_0)
        assert (o.run_cg(E3) if method == "cg" else o.run(E3)) is False
        _short_oracles[key] = o
    o = _short_oracles[key]
    g, T, To = s.get_field("epsilon"), s.get_field("u"), o.potential()
    print("short axes", grid, u_loop, method, "iterations", s.iterations, o.iterations, "residuals",
          np.abs(np.array(s.residuals) - np.array(o.residuals)).max() if s.iterations == o.iterations else None,
          "gradient", rel_err(g, o.eps), "flux", rel_err(s.get_field("sigma"), o.pk1(o.eps)),
          "mean flux", rel_err(s.mean_stress(), o.mean_stress()), "potential", np.abs(T[0] - To).max())
    assert s.iterations == o.iterations and o.iterations < 10000
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    assert g.shape == (3,) + grid
    assert rel_err(g, o.eps) < 1e-10
    assert rel_err(s.get_field("sigma"), o.pk1(o.eps)) < 1e-10
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-11
    np.testing.assert_allclose(s.mean_strain(), E3, atol=1e-12)
    assert T.shape == (1,) + grid and np.abs(T[0] - To).max() < 1e-10 * max(1.0, np.abs(To).max())
    s.close()


TILED_GRIDS = [((16, 16, 128), (1, 1, 1)), ((8, 14, 124), (1.0, 2.0, 0.5)), ((6, 20, 130), (1, 1, 1)),
               ((40, 30, 128), (1, 1, 1)), ((12, 16, 256), (1, 1, 1)), ((5, 14, 256), (2, 1, 1)),
               ((16, 16, 100), (1, 1, 1)), ((9, 14, 80), (1.0, 2.0, 0.5)), ((7, 20, 122), (1, 1, 1))]


@pytest.mark.parametrize("grid,dims", TILED_GRIDS)
@pytest.mark.parametrize("laws", ["aniso-aniso", "iso-aniso"])
def test_tiled_aniso_sweep(grid, dims, laws):
    """the nine grids of test_tiled_scalar_sweep (one per tile shape, overlapping last tiles, wrap in every direction) on
    k_sc_tile_aniso (aniso_sc_tile = 1, the default) against the exact-order 13-point sweep (= 0) and the restatement, at that
    test's bars; the counter reports the tiled form exactly where it runs.  Either phase may be iso or aniso."""
    phi1 = sphere_phi(grid, 0.3)
    mats, phis = two_K(), [1 - phi1, phi1]
    if laws == "iso-aniso":
        mats = [1.3, mats[1]]
    res = {}
    for flag in (0, 1):
        s = _solver(grid, mats, phis, dims, tol=1e-9, aniso_sc_tile=flag)
        assert s.run(E3) is False
        n = s.counter("sc_tile_aniso")
        assert (n > 0) if flag else (n == 0)
        res[flag] = (s.iterations, np.array(s.residuals), s.get_field("epsilon"), s.mean_stress(), s.get_field("u"), s.ref_material[0])
        s.close()
    a, b = res[0], res[1]
    assert a[0] == b[0]
    assert np.abs(a[1] - b[1]).max() < 1e-12
    assert rel_err(b[2], a[2]) < 1e-11 and rel_err(b[3], a[3]) < 1e-12
    assert np.abs(b[4] - a[4]).max() < 1e-11 * max(1.0, np.abs(a[4]).max())
    o = _oracle(FixedRefOracle, grid, mats, phis, dims, tol=1e-9, mu_0=b[5])
    assert o.run(E3) is False
    assert o.iterations == b[0] and rel_err(b[2], o.eps) < 1e-10


def test_tiled_form_falls_back():
    """three phases, a pair that is not complementary, u_loop = 1, a grid the tiles do not fit: the exact-order path, counter 0"""
    grid = (16, 16, 128)
    a, b = sphere_phi(grid, 0.3), sphere_phi(grid, 0.25, c=(0.2, 0.6, 0.4))
    p0 = np.clip(1 - a - b, 0, 1)
    tot = p0 + a + b
    K = two_K()
    cases = [([K[0], 6.0, K[1]], [p0 / tot, a / tot, b / tot], grid, {}),
             (K, [(1 - a) * (1 - 1e-9), a], grid, {}),
             (K, [1 - a, a], grid, {"u_loop": 1}),
             (K, [1 - sphere_phi((9, 7, 5), 0.3), sphere_phi((9, 7, 5), 0.3)], (9, 7, 5), {})]
    for mats, phis, gr, kw in cases:
        s = _solver(gr, mats, phis, tol=1e-9, **kw)
        assert s.run(E3) is False
        assert s.counter("sc_tile_aniso") == 0
        o = _oracle(FixedRefOracle, gr, mats, phis, tol=1e-9, mu_0=s.ref_material[0])
        assert o.run(E3) is False
        assert s.iterations == o.iterations and rel_err(s.get_field("epsilon"), o.eps) < 1e-10
        s.close()


def test_three_phases_mixed_laws():
    """iso and aniso phases mix (Voigt), three phases, fractions that are no complementary pair; a phase below the threshold"""
    grid = (9, 7, 5)
    a, b = sphere_phi(grid, 0.3), sphere_phi(grid, 0.25, c=(0.2, 0.6, 0.4))
    phis = [np.clip(1 - a - b, 0, 1), a, b]
    tot = phis[0] + phis[1] + phis[2]
    phis = [p / tot for p in phis]
    mats = [two_K()[0], 6.0, two_K(9)[1]]
    s = _solver(grid, mats, phis, tol=1e-9)
    assert s.run(E3) is False
    mu_0 = s.ref_material[0]
    assert abs(mu_0 - eig_mu0(phis, mats)) <= 1e-13 * mu_0
    o = _oracle(FixedRefOracle, grid, mats, phis, tol=1e-9, mu_0=mu_0)
    assert o.run(E3) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-10 and rel_err(s.get_field("sigma"), o.pk1(o.eps)) < 1e-10
    s.close()


def test_reference_medium_of_a_transversely_isotropic_phase():
    """repeated eigenvalues (a fibre that conducts ten times better along its oblique axis than across), where a closed
    trigonometric 3x3 solve loses half its digits: the device scan stays at 1e-13"""
    grid = (12, 10, 6)
    phi1 = sphere_phi(grid, 0.3)
    a = np.array([1.0, 2.0, -1.0]) / np.sqrt(6.0)
    Kf = 1.0 * np.eye(3) + 9.0 * np.outer(a, a)
    Kf = 0.5 * (Kf + Kf.T)
    mats, phis = [0.7, Kf], [1 - phi1, phi1]
    s = _solver(grid, mats, phis)
    s.calc_ref_material()
    mu_0 = s.ref_material[0]
    assert abs(mu_0 - eig_mu0(phis, mats)) <= 1e-13 * mu_0
    s.close()


@pytest.mark.parametrize("grid", [(16, 16, 16), (16, 16, 128)])
@pytest.mark.parametrize("estimator", ["epsilon", "residual"])
def test_aniso_cg_matches_reference(grid, estimator):
    """method=cg in potential space against the restatement's run_cg, at the bars of test_scalar_cg_matches_oracle"""
    phi1 = sphere_phi(grid, 0.3)
    mats, phis = two_K(), [1 - phi1, phi1]
    s = _solver(grid, mats, phis, tol=1e-10, method="cg", error_estimator=estimator)
    assert s.run(E3) is False
    o = _oracle(FixedRefOracle, grid, mats, phis, tol=1e-10, mu_0=s.ref_material[0])
    o.error_estimator = estimator
    assert o.run_cg(E3) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-10)
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-8
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-9
    # 16 x 16 x 128: the fused form with the direction update inside k_sc_tile_aniso<.., CGP>; 16^3: the four-kernel form
    assert (s.counter("sc_tile_aniso") > 0) == (grid == (16, 16, 128))
    s.close()


def test_homogeneous_body():
    grid = (16, 16, 128)
    K = two_K()[1]
    s = _solver(grid, [K], [np.ones(grid)], tol=1e-13)
    assert s.run(E3) is False
    w = np.linalg.eigvalsh(K)
    assert abs(s.ref_material[0] - 0.25 * (w[0] + w[-1])) <= 1e-13 * s.ref_material[0]
    assert rel_err(s.mean_stress(), K @ E3) <= 1e-13
    assert np.abs(s.get_field("epsilon") - E3[:, None, None, None]).max() <= 1e-13
    s.close()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_three_layers_reproduce_the_laminate(axis):
    """exact on this grid (every field depends on one coordinate only); the bar of
    test_scalar_effective_conductivity_of_layers_is_exact"""
    shape, fr, edges, phis, Ks = layer_problem(axis)
    s = _solver(shape, Ks, phis, tol=1e-13, maxiter=5000)
    assert s.run(E3) is False and s.iterations < 5000
    check_laminate(axis, s.get_field("epsilon"), s.get_field("sigma"), fr, edges, Ks, E3, 1e-10)
    s.close()


def test_isotropic_equivalence():
    """K = mu I through the aniso kernels gives the isotropic run: same iteration count, fields to 1e-11"""
    grid = (16, 16, 128)
    phi1 = sphere_phi(grid, 0.3)
    mus, phis = [1.0, 12.0], [1 - phi1, phi1]
    iso = _solver(grid, mus, phis, tol=1e-9)
    ani = _solver(grid, [m * np.eye(3) for m in mus], phis, tol=1e-9)
    assert iso.run(E3) is False and ani.run(E3) is False
    assert ani.counter("sc_tile_aniso") > 0 and iso.counter("sc_tile_aniso") == 0
    assert iso.iterations == ani.iterations
    assert abs(iso.ref_material[0] - ani.ref_material[0]) <= 1e-13 * iso.ref_material[0]
    assert rel_err(ani.get_field("epsilon"), iso.get_field("epsilon")) < 1e-11
    assert rel_err(ani.get_field("sigma"), iso.get_field("sigma")) < 1e-11
    iso.close()
    ani.close()


@pytest.mark.parametrize("perm", [(1, 2, 0), (2, 0, 1), (0, 2, 1)])
def test_axis_covariance(perm):
    """permuting grid axes, cell sizes, load and K together permutes the answer"""
    grid, dims = (12, 10, 6), (2.0, 1.0, 0.5)
    phi1 = sphere_phi(grid, 0.3)
    mats = two_K()
    s = _solver(grid, mats, [1 - phi1, phi1], dims, tol=1e-12)
    assert s.run(E3) is False
    g, q = s.get_field("epsilon"), s.mean_stress()
    s.close()
    perm = list(perm)
    pg, pd = tuple(grid[a] for a in perm), tuple(dims[a] for a in perm)
    pphi = np.ascontiguousarray(np.transpose(phi1, perm))
    pm = [K[np.ix_(perm, perm)] for K in mats]
    t = _solver(pg, pm, [1 - pphi, pphi], pd, tol=1e-12)
    assert t.run(E3[perm]) is False
    gp = t.get_field("epsilon")
    assert rel_err(np.transpose(gp, [0] + [a + 1 for a in np.argsort(perm)])[np.argsort(perm)], g) < 1e-10
    assert rel_err(t.mean_stress()[np.argsort(perm)], q) < 1e-10
    t.close()


@pytest.mark.parametrize("grid", [(12, 10, 6), (16, 16, 128)])
def test_aniso_mixed_boundary_conditions(grid):
    """a flux prescribed in x, gradients in y and z (method=basic): met to bc_tol, and the restatement's run (the tiled form has no
    variant with the sums of tau: the exact-order sweep plus the flux-mean sweep)"""
    phi1 = sphere_phi(grid, 0.3)
    mats, phis = two_K(), [1 - phi1, phi1]
    P3 = np.diag([0.0, 1.0, 1.0])
    P6 = np.diag([0.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    E, S = np.array([0.0, 0.3, -0.2]), np.array([1.5, 0.0, 0.0])
    s = _solver(grid, mats, phis, tol=1e-10, bc_tol=1e-9, maxiter=500)
    s.set_bc_projector(P6)
    assert s.run(E, S) is False
    o = _oracle(FixedRefOracle, grid, mats, phis, tol=1e-10, bc_tol=1e-9, maxiter=500, mu_0=s.ref_material[0])
    assert o.run(E, S, P3) is False
    assert s.iterations == o.iterations
    assert np.abs(np.array(s.residuals) - np.array(o.residuals)).max() < 1e-10
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-9
    assert abs(s.mean_stress()[0] - 1.5) <= 1e-9 * 1.5 and np.abs(s.mean_strain()[1:] - E[1:]).max() < 1e-12
    s.close()


def test_load_steps():
    """a linear law: two load steps end where the single load case ends (both converged to tol = 1e-11 in the relative change
    of the norm; the contraction of the scheme leaves the fields within 1e-8 of each other)"""
    grid = (12, 10, 6)
    phi1 = sphere_phi(grid, 0.3)
    mats, phis = two_K(), [1 - phi1, phi1]
    a = _solver(grid, mats, phis, tol=1e-11)
    b = _solver(grid, mats, phis, tol=1e-11)
    assert a.run(E3) is False
    assert b.run_load_steps(E3, params=(0.0, 0.5, 1.0)) is False
    assert rel_err(b.get_field("epsilon"), a.get_field("epsilon")) < 1e-8
    assert rel_err(b.mean_stress(), a.mean_stress()) < 1e-8
    a.close()
    b.close()


ANISO_XML = """
<settings><solver n="16"><mode>%s</mode><tol>1e-9</tol>
  <materials><matrix mu="1" />
    <incl law="aniso" c11="9" c22="3" c33="2" c23="0.5" c13="-0.7" c12="1.1" /></materials></solver>
  <actions><select_material name="incl" /><place_fiber R="0.3" />
  <calc_effective_properties /></actions></settings>"""


@pytest.mark.parametrize("mode", ["heat", "porous"])
def test_fg_aniso_project(mode):
    """an XML project with <place_fiber> and law="aniso" through FG: the 3x3 effective matrix is the restatement's on the same
    phase field, and an oblique K leaves non-zero off-diagonals"""
    from fibergen_amd import FG
    fg = FG()
    fg.set_xml(ANISO_XML % mode)
    assert fg.run() == 0
    K = np.array(fg.get_effective_property())
    assert K.shape == (3, 3)
    phi = fg.get_field("phi")
    Ki = np.array([[9, 1.1, -0.7], [1.1, 3, 0.5], [-0.7, 0.5, 2]])
    o = AnisoScalarOracle(16, 16, 16, mus=[1.0, Ki], phis=[phi[0], phi[1]], tol=1e-9)
    Ko = np.zeros((3, 3))
    for i in range(3):   # the project does not name a method: the reference's default, cg
        assert o.run_cg(np.eye(3)[i]) is False
        Ko[:, i] = o.mean_stress()
    assert rel_err(K, Ko) < 1e-9
    off = K - np.diag(np.diag(K))
    assert np.abs(off[np.triu_indices(3, 1)]).min() > 1e-3
    assert rel_err(K, K.T) < 1e-6   # the effective matrix of symmetric phases is symmetric (to the solver's tolerance)


def test_refusals():
    from fibergen_amd import LSSolver
    from fibergen_amd import materials
    from fibergen_amd.distributed import SlabMember
    grid = (8, 8, 8)
    s = LSSolver(*grid)
    s.set_num_phases(2)
    with pytest.raises(RuntimeError, match="heat / porous mode only"):   # elasticity (the default mode)
        s.set_phase_conductivity(1, np.eye(3))
    s.set_options(mode="heat")
    for bad in (float("nan"), float("inf")):
        c6 = np.array([1.0, 1.0, 1.0, 0.0, bad, 0.0])
        with pytest.raises(RuntimeError, match="phase conductivity is not finite"):
            s.set_phase_conductivity(1, c6)
    with pytest.raises(RuntimeError, match="phase index out of range"):
        s.set_phase_conductivity(2, np.eye(3))
    # a mode change after the fact is caught when the run starts, before any kernel
    phi1 = sphere_phi(grid, 0.3)
    s.set_phase(0, 1.0, 0.0, 1 - phi1)
    s.set_phase_conductivity(1, np.eye(3) * 4, phi1)
    s.set_options(mode="elasticity")
    with pytest.raises(RuntimeError, match="heat / porous mode only"):
        s.run([1.0, 0, 0, 0, 0, 0])
    # back to an isotropic phase: runs again
    s.set_options(mode="heat")
    s.set_phase(1, 4.0, 0.0)
    assert s.run([1.0, 0, 0]) is False
    s.close()
    m = SlabMember(8, 8, 8, nranks=1)
    try:
        m.set_options(mode="heat")
        m.set_num_phases(2)
        with pytest.raises(RuntimeError, match=materials.ANISO_SLAB_ERROR.replace("(", r"\(").replace(")", r"\)")):
            m.set_phase_conductivity(1, np.eye(3))
        # the library's own refusal, behind the Python one
        c6 = np.ones(6)
        from fibergen_amd import _lib
        assert m._lib.fg_set_phase_conductivity(m._h, 1, c6.ctypes.data_as(_lib.c_double_p)) != 0
        assert "slab-decomposed" in m._lib.fg_last_error(m._h).decode()
    finally:
        m.close()

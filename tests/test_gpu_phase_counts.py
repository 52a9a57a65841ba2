"""Four to eight phases on every GPU path against the oracles (the rest of the suite stops at three): the stress stage, one pass
and the reference material; every loop variant to convergence; the laminate rule's refusal of a third phase; k_polarize<NPH>
for NPH = 4 .. 8; general and aniso phases; the scalar and viscosity modes; full_staggered and willot; the phase count changed
on a live solver; the slab driver; the voxeliser (fg_voxelize, fg_voxelize_into coarse and fine) with eight materials and the
project layer with five and nine.  Inputs come from phase_draws.py: pairwise phases (laminate: pairs (0, k) and one pair
(j, j + 1) of two inclusions) and overlapping phases (Voigt: four and more phases in a voxel, a phase never placed, a phase
below the 10 eps threshold).

Every bar is the one the existing test of the same path uses; it is named where it is asserted.  Iteration counts of the
oracles alone are stated at the converged cases (all below the maxiter given)."""
import numpy as np
import pytest

import general_reference as gr
import polarization_reference as pr
from helpers import rel_err
from phase_draws import iso_mats, overlapping_phases, pairwise_phases, phase_pairs

pytestmark = pytest.mark.gpu

NPH = [4, 5, 8]
SMALL = (12, 10, 6)          # the tiles do not fit
TILED = (4, 14, 80)          # the smallest grid u_tile_supported accepts: even nz >= 80, ny >= 14, nx >= 4
E_LOAD = np.array([0.5, -0.25, 1.0, 0.1, 0.2, 0.3])

_cache = {}


def problem(grid, nph, mixing, seed=0):
    """(mats, phis, normals) of a (grid, nph, mixing): pairwise phases for the laminate rule, overlapping ones for Voigt"""
    key = ("problem", grid, nph, mixing, seed)
    if key not in _cache:
        rng = np.random.default_rng(4000 + 100 * seed + nph)
        mats = iso_mats(rng, nph)
        if mixing == "laminate":
            phis, normals = pairwise_phases(grid, nph, rng)
        else:
            phis, normals = overlapping_phases(grid, nph, rng), None
        _cache[key] = (mats, phis, normals)
    return _cache[key]


def gpu_solver(grid, mats, phis, normals=None, dims=(1.0, 1.0, 1.0), cls=None, **opts):
    """mats[p]: (mu, lambda) or a 6 x 6 stiffness"""
    from fibergen_amd import LSSolver
    s = LSSolver(*grid, *dims) if cls is None else cls
    s.set_num_phases(len(mats))
    for p, m in enumerate(mats):
        if gr.is_general(m):
            s.set_phase(p, 0.0, 0.0, phis[p])
            s.set_phase_stiffness(p, m)
        else:
            s.set_phase(p, m[0], m[1], phis[p])
    if normals is not None:
        s.set_normals(normals)
    s.set_options(**opts)
    return s


def ls_oracle(grid, mats, phis, normals, mixing, **kw):
    from oracle.ls_oracle import LSOracle
    return LSOracle(*grid, mats=mats, phis=phis, normals=normals, mixing_rule=mixing, **kw)


# ------------------------------------------------------------------------------------------------ 1. stages, strain state
@pytest.mark.parametrize("nph", NPH)
@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
@pytest.mark.parametrize("grid", [SMALL, (7, 5, 9), (1, 6, 8)])
def test_stress_stage_one_pass_and_reference_material(grid, mixing, nph):
    """k_stress<mixing, kMaxPhases>, one basic pass and k_tangent_minmax against LSOracle.  Bars of
    test_gpu_parity.test_stress_stage (1e-14 on tau and sigma, 1e-12 on the means) and test_one_iteration (1e-12 on the strain
    after the pass); the reference material at 1e-14 relative (test_gpu_fullsize_oracle)."""
    mats, phis, normals = problem(grid, nph, mixing)
    o = ls_oracle(grid, mats, phis, normals, mixing)
    s = gpu_solver(grid, mats, phis, normals, mixing_rule=mixing, mu_0=0.77, lambda_0=0.31)
    eps = np.random.default_rng(10).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    e_tau = rel_err(s.get_field("tau"), o.calc_stress(0.77, 0.31, eps))
    e_sig = rel_err(s.get_field("sigma"), o.calc_stress(0.0, 0.0, eps))
    o.eps = eps
    e_ms, e_me = rel_err(s.mean_stress(), o.mean_stress()), rel_err(s.mean_strain(), o.mean_strain())
    print("stage", grid, mixing, nph, e_tau, e_sig, e_ms, e_me)
    assert e_tau < 1e-14 and e_sig < 1e-14
    assert e_ms < 1e-12 and e_me < 1e-12 + 1e-13
    for p in range(nph):
        assert s.volume_fraction(p) == pytest.approx(phis[p].mean(), rel=1e-13, abs=1e-30)
    s.close()
    o = ls_oracle(grid, mats, phis, normals, mixing)
    s = gpu_solver(grid, mats, phis, normals, mixing_rule=mixing)
    o.calc_ref_material()
    mu_0, lam_0 = s.calc_ref_material()
    assert mu_0 == pytest.approx(o.mu_0, rel=1e-14) and lam_0 == 0.0
    eps = 0.1 * np.random.default_rng(15).standard_normal((6,) + grid)
    E = np.array([1.0, 0.2, -0.3, 0.1, 0.0, 0.4])
    s.set_field("epsilon", eps)
    s.run_stage("iteration", E)
    e_it = rel_err(s.get_field("epsilon"), o.basic_scheme(E, eps))
    print("pass", grid, mixing, nph, e_it)
    assert e_it < 1e-12
    s.close()


def test_laminate_second_fraction_is_one_minus_the_first():
    """get_mix F:13523 sets c2 = 1 - c1 whatever the second phase's stored fraction is.  Fractions that sum to one cannot tell
    that from reading it, so here the second phase of every pair (j, j + 1) stores half of what it should: the oracle and
    the product both have to take 1 - c1.  Bar: test_stress_stage's."""
    grid, nph = SMALL, 8
    mats, phis, normals = problem(grid, nph, "laminate")
    phis = [p.copy() for p in phis]
    pair = [k for k in phase_pairs(phis)[0] if k[0] > 0][0]
    both = (phis[pair[0]] != 0) & (phis[pair[1]] != 0)
    assert both.any()
    phis[pair[1]][both] *= 0.5
    o = ls_oracle(grid, mats, phis, normals, "laminate")
    s = gpu_solver(grid, mats, phis, normals, mixing_rule="laminate", mu_0=0.77, lambda_0=0.31)
    eps = np.random.default_rng(11).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    assert rel_err(s.get_field("tau"), o.calc_stress(0.77, 0.31, eps)) < 1e-14
    s.close()


# ------------------------------------------------------------------------------------------------ 2. every loop variant
VARIANTS = [dict(u_loop=u, u_tile=t, fuse_stress_div=f) for u in (0, 1, 2) for t in (0, 1) for f in (0, 1)]
PROJECTORS = {"uniaxial_stress_x": [1, 0, 0, 0, 0, 0], "plane_strain_free_z": [1, 1, 0, 0.5, 0.5, 0.5]}


def run_pair(s, o, method, E, bc=None, steps=None, tag=None):
    """test_gpu_fuzz._run_combination's comparison: a combination the oracle rejects must be rejected with the same message;
    else iteration counts equal, residual histories within 1e-9, strain within 1e-8, mean stress within 1e-9"""
    E, S0, P = E.copy(), np.zeros(6), None
    if bc is not None:
        keep = np.array(PROJECTORS[bc], dtype=float)
        P = np.diag(keep)
        E = E * (keep > 0)
        s.set_bc_projector(P)
    params = steps or [0.0, 1.0]
    if not hasattr(o, "ref_run"):     # one oracle run for all the variants of a combination (left unchanged afterwards)
        try:
            o.ref_run = (o.run_load_steps(E, S0, P, params=params, method=method), None)
        except RuntimeError as e:
            o.ref_run = (None, e)
    ref_failed, err = o.ref_run
    if err is not None:
        with pytest.raises(RuntimeError) as got:
            s.run_load_steps(E, S0, params=params)
        assert str(err).split(":")[0][:24] in str(got.value), tag
        return
    failed = s.run_load_steps(E, S0, params=params)
    assert failed == ref_failed and ref_failed is False, tag
    assert s.iterations == o.iterations, (tag, s.iterations, o.iterations)
    r, rr = np.array(s.residuals), np.array(o.residuals)
    assert r.shape == rr.shape and np.abs(r - rr).max() < 1e-9, tag
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-8, tag
    assert np.abs(s.mean_stress() - o.mean_stress()).max() < 1e-9 * max(1.0, np.abs(o.mean_stress()).max()), tag


@pytest.mark.parametrize("nph", NPH)
@pytest.mark.parametrize("scheme", ["staggered", "collocated"])
@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
@pytest.mark.parametrize("grid", [SMALL, TILED])
def test_every_loop_variant_converged(grid, mixing, method, scheme, nph):
    """u_loop x u_tile x fuse_stress_div at tol 1e-7 against one oracle run; the fuzz file's bars (run_pair).  The oracle alone
    converges in 5 to 109 iterations over these combinations (maxiter 400); it refuses none of them (collocated with laminate
    mixing included), so every variant of every combination is a converged run held against it."""
    mats, phis, normals = problem(grid, nph, mixing)
    common = dict(tol=1e-7, maxiter=400)
    o = ls_oracle(grid, mats, phis, normals, mixing, gamma_scheme=scheme, **common)
    for v in VARIANTS:
        s = gpu_solver(grid, mats, phis, normals, mixing_rule=mixing, gamma_scheme=scheme, method=method, **common, **v)
        run_pair(s, o, method, E_LOAD, tag=(grid, mixing, method, scheme, nph, v))
        assert o.ref_run[1] is None, o.ref_run[1]      # a converged comparison, not a matched refusal
        if mixing == "laminate" and scheme == "staggered" and v["u_loop"] == 2 and o.ref_run[1] is None:
            # the interface lists of the laminate correction (test_counters_report_the_laminate_lists)
            mixed = int(np.any([(p != 0) & (p != 1) for p in phis], axis=0).sum())
            assert s.counter("interface_voxels") == mixed > 0, v
            assert mixed <= s.counter("affected_voxels") <= 7 * mixed, v
        s.close()


@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
@pytest.mark.parametrize("what", ["uniaxial_stress_x", "plane_strain_free_z", "steps"])
def test_mixed_boundary_conditions_and_load_steps_five_phases(what, mixing):
    """once each at nph = 5 on the tiled grid (u_loop 2, the default) and the small one; the fuzz file's bars.  Oracle alone:
    20 to 48 iterations (maxiter 400)."""
    for grid in (SMALL, TILED):
        mats, phis, normals = problem(grid, 5, mixing)
        common = dict(tol=1e-7, maxiter=400)
        o = ls_oracle(grid, mats, phis, normals, mixing, **common)
        s = gpu_solver(grid, mats, phis, normals, mixing_rule=mixing, **common)
        if what == "steps":
            run_pair(s, o, "basic", E_LOAD, steps=[0.0, 0.4, 1.0], tag=(grid, what, mixing))
        else:
            run_pair(s, o, "basic", E_LOAD, bc=what, tag=(grid, what, mixing))
        s.close()


# ------------------------------------------------------------------------------------------------ 3. laminate refusal
@pytest.mark.parametrize("nph", [4, 8])
@pytest.mark.parametrize("u_loop", [0, 1, 2])
def test_laminate_refuses_a_third_phase(nph, u_loop):
    """one voxel with three non-zero phases: the oracle raises "The laminate mixing rule supports only two phase mixtures", and
    so do the strain-state pass (u_loop 0), k_u_stress (1) and k_interface_solve (2); matched as _run_combination matches"""
    grid = TILED
    mats, phis, normals = problem(grid, nph, "laminate")
    phis = [p.copy() for p in phis]
    at = tuple(int(v[0]) for v in np.nonzero((phis[0] != 0) & (phis[1] != 0)))   # a (0, 1) voxel gets phase nph - 1 as well
    phis[0][at] -= 0.125 * phis[0][at]
    phis[nph - 1][at] = 1.0 - phis[0][at] - phis[1][at]
    assert sum(int(p[at] != 0) for p in phis) == 3
    o = ls_oracle(grid, mats, phis, normals, "laminate", tol=1e-7, maxiter=50)
    with pytest.raises(RuntimeError) as want:
        o.run(E_LOAD)
    assert str(want.value).startswith("The laminate mixing rule supports only two phase mixtures")
    s = gpu_solver(grid, mats, phis, normals, mixing_rule="laminate", tol=1e-7, maxiter=50, u_loop=u_loop)
    with pytest.raises(RuntimeError) as got:
        s.run(E_LOAD)
    assert str(want.value).split(":")[0][:24] in str(got.value)
    s.close()


# ------------------------------------------------------------------------------------------------ 4. polarisation
from test_gpu_polarization import PASS_TOL, SCHEMES   # noqa: E402  (the per-pass bar of that file: 10 x its largest measured error)


def polar_problem(grid, nph):
    """overlapping phases; the last phase is general, from five phases on phase 3 as well, from six on the never-placed one too"""
    key = ("polar", grid, nph)
    if key not in _cache:
        rng = np.random.default_rng(7000 + nph)
        mats = iso_mats(rng, nph)
        mats[nph - 1] = gr.random_spd(rng, scale=0.3)
        if nph >= 5:
            mats[3] = gr.distinct_stiffness(0.5)
        if nph >= 6:
            mats[2] = gr.random_spd(rng, coupling=False, scale=2.0)
        _cache[key] = (mats, overlapping_phases(grid, nph, rng))
    return _cache[key]


@pytest.mark.parametrize("nph", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("grid", [SMALL, (41, 33, 11)])
def test_polarization_per_pass_parity(grid, scheme, nph):
    """k_polarize<NPH, INV> for every NPH the switch of launch_polarize has beyond three: test_per_pass_parity of
    test_gpu_polarization.py (three passes, P after each, the converted strain) at that file's PASS_TOL, and the counter of
    the voxels that took the 6 x 6 solve."""
    mats, phis = polar_problem(grid, nph)
    s = gpu_solver(grid, mats, phis, method="polarization", gamma_scheme=scheme)
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
    want = int(pr.generic_mask(phis, mats).sum())
    assert 0 < want and s.counter("polarization_generic_voxels") == want
    e_eps = rel_err(s.get_field("epsilon"), o.calc_polarization(P, inv=True))
    print("parity", grid, scheme, nph, worst, e_eps)
    s.close()
    assert worst <= PASS_TOL and e_eps <= PASS_TOL


@pytest.mark.parametrize("scheme", SCHEMES)
def test_polarization_converged_eight_phases(scheme):
    """16^3, tol 1e-8, as test_converged_run: iterations equal, residuals within 1e-9, strain within 1e-9.  The restatement
    alone: 26 iterations with each of the three schemes (maxiter 2000)."""
    grid = (16, 16, 16)
    mats, phis = polar_problem(grid, 8)
    s = gpu_solver(grid, mats, phis, method="polarization", gamma_scheme=scheme, tol=1e-8, maxiter=2000)
    o = pr.make_polarization_oracle(grid, mats, phis, scheme, tol=1e-8, maxiter=2000)
    assert s.run(E_LOAD) is False and o.run_polarization(E_LOAD) is False
    print("converged", scheme, s.iterations, o.iterations, rel_err(s.get_field("epsilon"), o.eps))
    assert s.iterations == o.iterations < 2000
    assert np.abs(np.array(s.residuals) - np.array(o.residuals)).max() <= 1e-9
    assert rel_err(s.get_field("epsilon"), o.eps) <= 1e-9
    s.close()


# ------------------------------------------------------------------------------------------------ 5. general and aniso laws
def general_problem(grid, nph):
    key = ("general", grid, nph)
    if key not in _cache:
        rng = np.random.default_rng(8000 + nph)
        mats = iso_mats(rng, nph)
        for p in (0, 3, 7):                     # general and isotropic phases interleaved
            if p < nph:
                mats[p] = gr.random_spd(rng, scale=0.2) if p else gr.distinct_stiffness(0.5)
        _cache[key] = (mats, overlapping_phases(grid, nph, rng))
    return _cache[key]


@pytest.mark.parametrize("nph", [5, 8])
@pytest.mark.parametrize("scheme", ["staggered", "collocated", "willot"])
@pytest.mark.parametrize("method,maxiter", [("basic", 5), ("cg", 4)])
def test_general_phases_passes_and_converged_run(method, maxiter, scheme, nph):
    """pk1_voigt over pt.C[p] for p up to 7 and k_tangent_minmax<GENERAL>: a few passes (test_gpu_general.run_both) and a run
    to tol 1e-7, at test_gpu_general.check_loop's bars.  The restatement alone converges in 5 to 34 iterations (maxiter 400)."""
    from test_gpu_general import check_loop
    grid = SMALL
    mats, phis = general_problem(grid, nph)
    for kw in (dict(tol=1e-14, maxiter=maxiter), dict(tol=1e-7, maxiter=400)):
        o = pr.PolarizationOracle(*grid, mats=mats, phis=phis, gamma_scheme=scheme, **kw)
        s = gpu_solver(grid, mats, phis, gamma_scheme=scheme, method=method, **kw)
        fo = o.run_cg(E_LOAD) if method == "cg" else o.run(E_LOAD)
        assert s.run(E_LOAD) == fo is False and s.iterations == o.iterations
        assert abs(s.ref_material[0] - o.mu_0) <= 1e-13 * o.mu_0         # test_reference_material_scan's bar
        if kw["maxiter"] == 400:
            assert o.iterations < 400
        check_loop(s, o, method, "general %d phases %s %s" % (nph, scheme, kw))
        s.close()


@pytest.mark.parametrize("nph", [5, 8])
@pytest.mark.parametrize("u_loop", [1, 2])
@pytest.mark.parametrize("mode", ["heat", "porous"])
def test_aniso_phases(mode, u_loop, nph):
    """K[8][6] read by phase index: aniso phases at 1, 4 and 7 against aniso_reference, as test_aniso_run_matches_reference
    (mu_0 at 1e-13 against eigvalsh, then handed to the restatement; its bars).  The restatement alone: 69 (five phases) and 52 (eight) iterations."""
    from aniso_reference import FixedRefOracle, random_spd3
    from test_gpu_aniso import E3, _oracle, _solver, eig_mu0
    grid = SMALL
    rng = np.random.default_rng(8500 + nph)
    mats = [float(rng.uniform(0.5, 5.0)) for _ in range(nph)]
    for p in (1, 4, 7):
        if p < nph:
            mats[p] = random_spd3(rng, float(rng.uniform(1.0, 10.0)))
    phis = overlapping_phases(grid, nph, rng)
    s = _solver(grid, mats, phis, mode=mode, tol=1e-9, u_loop=u_loop)
    assert s.run(E3) is False
    mu_0 = s.ref_material[0]
    assert abs(mu_0 - eig_mu0(phis, mats)) <= 1e-13 * mu_0
    o = _oracle(FixedRefOracle, grid, mats, phis, tol=1e-9, mu_0=mu_0)
    assert o.run(E3) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-10
    assert rel_err(s.get_field("sigma"), o.pk1(o.eps)) < 1e-10
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-11
    s.close()


# ------------------------------------------------------------------------------------------------ 6. scalar and viscosity
@pytest.mark.parametrize("nph", [4, 8])
@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("mode", ["heat", "porous", "viscosity"])
@pytest.mark.parametrize("grid", [SMALL, TILED])
def test_scalar_and_viscosity_modes(grid, mode, method, nph):
    """for q < sp.n in the scalar sweeps (u_loop 1 and 2) and the viscosity loop against ScalarOracle / ViscosityOracle; bars of
    test_random_scalar_and_viscosity_problems_match_their_oracles.  The oracles alone: 2 to 35 iterations (maxiter 300)."""
    from fibergen_amd import LSSolver
    rng = np.random.default_rng(9500 + nph)
    mus = [float(rng.uniform(0.05, 20.0)) for _ in range(nph)]
    phis = overlapping_phases(grid, nph, rng)
    common = dict(tol=1e-7, maxiter=300)
    E6 = np.array([0.3, -0.7, 0.4, 0.5, -0.2, 0.9])
    if mode == "viscosity":
        from oracle.viscosity_oracle import ViscosityOracle
        o = ViscosityOracle(*grid, mats=[(m, 0.0) for m in mus], phis=phis, **common)
        E, loops = E6.copy(), [None]
        E[:3] -= E[:3].mean()
    else:
        from oracle.scalar_oracle import ScalarOracle
        o = ScalarOracle(*grid, mus=mus, phis=phis, **common)
        E, loops = E6[:3].copy(), [1, 2]
    assert (o.run_cg(E) if method == "cg" else o.run(E)) is False and o.iterations < 300
    for u_loop in loops:
        s = LSSolver(*grid)
        s.set_options(mode=mode)
        s.set_num_phases(nph)
        for p in range(nph):
            s.set_phase(p, mus[p], 0.0, phis[p])
        s.set_options(method=method, **common, **({} if u_loop is None else {"u_loop": u_loop}))
        tag = (grid, mode, method, nph, u_loop)
        assert s.run(E) is False, tag
        assert s.iterations == o.iterations, tag
        assert np.abs(np.array(s.residuals) - np.array(o.residuals)).max() < 1e-9, tag
        assert rel_err(s.get_field("epsilon"), o.eps) < 1e-8, tag
        ms = np.asarray(s.mean_stress())[:len(np.atleast_1d(o.mean_stress()))]
        assert np.abs(ms - o.mean_stress()).max() < 1e-9 * max(1.0, np.abs(o.mean_stress()).max()), tag
        s.close()


# ------------------------------------------------------------------------------------------------ 7. full_staggered, willot
def dfg_problem(grid, nph):
    """fine images of nph overlapping phases; the odd phases arrive as fine fields, the even ones as coarse input"""
    from dfg_reference import split_input
    rng = np.random.default_rng(9800 + nph)
    mats = iso_mats(rng, nph)
    images = overlapping_phases(tuple(2 * n for n in grid), nph, rng)
    return (mats,) + split_input(images, ["coarse" if p % 2 == 0 else "fine" for p in range(nph)])


def dfg_solver(grid, mats, fine, coarse, cls=None, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid) if cls is None else cls
    s.set_options(gamma_scheme="full_staggered")
    s.set_num_phases(len(mats))
    for p, (mu, lam) in enumerate(mats):
        s.set_phase(p, mu, lam, coarse[p])
        if fine[p] is not None:
            s.set_phase_fine(p, fine[p])
    s.set_options(**opts)
    return s


@pytest.mark.parametrize("nph", [4, 8])
@pytest.mark.parametrize("grid", [(4, 16, 80), SMALL])
def test_full_staggered(grid, nph):
    """launch_dfg_moduli over p < pt.n and the 3 * pt.n fine fields: the stress stage (test_gpu_dfg_stages' bars: 1e-14 against
    the fractions form, 1e-12 on the mean) and a converged run (the dfg fuzz file's bars).  (4, 16, 80) is the smallest grid of
    test_gpu_dfg.py's tile shapes.  The oracle alone: 9 to 14 iterations (maxiter 400)."""
    from dfg_reference import DfgLSOracle, calc_stress_fractions
    mats, fine, coarse, ofine = dfg_problem(grid, nph)
    o = DfgLSOracle(*grid, mats=mats, phis=[np.zeros(grid)] * nph, phis_fine=ofine, tol=1e-7, maxiter=400)
    s = dfg_solver(grid, mats, fine, coarse, mu_0=0.77, lambda_0=0.31)
    eps = np.random.default_rng(12).standard_normal((6,) + grid)
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    assert rel_err(s.get_field("tau"), calc_stress_fractions(eps, ofine, mats, 0.77, 0.31)) < 1e-14
    assert rel_err(s.mean_stress(), o.mean_stress(eps)) < 1e-12
    assert rel_err(s.get_field("phi"), np.array(o.phis)) < 1e-15
    s.close()
    s = dfg_solver(grid, mats, fine, coarse, tol=1e-7, maxiter=400)
    assert s.run(E_LOAD) is False and o.run(E_LOAD) is False
    assert s.iterations == o.iterations < 400
    assert np.abs(np.array(s.residuals) - np.array(o.residuals)).max() < 1e-9
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-8
    assert np.abs(s.mean_stress() - o.mean_stress()).max() < 1e-9 * max(1.0, np.abs(o.mean_stress()).max())
    s.close()


@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
def test_willot_eight_phases(mixing):
    """one converged run against willot_reference at test_willot_pass_and_run_match_restatement's bars.  The restatement
    alone: 35 (voigt) and 58 (laminate) iterations."""
    from willot_reference import WillotLSOracle
    grid = SMALL
    mats, phis, normals = problem(grid, 8, mixing)
    o = WillotLSOracle(*grid, mats=mats, phis=phis, normals=normals, mixing_rule=mixing, gamma_scheme="willot", tol=1e-8)
    s = gpu_solver(grid, mats, phis, normals, mixing_rule=mixing, gamma_scheme="willot", tol=1e-8)
    assert s.run(E_LOAD) is False and o.run(E_LOAD) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-9
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-10
    s.close()


# ------------------------------------------------------------------------------------------------ 8. live phase count
def test_phase_count_changes_on_a_live_solver():
    """8 phases (laminate, u_loop 2) -> set_num_phases(2) -> set_num_phases(5) with full_staggered and fine fields on ONE solver:
    every run equals the run of a fresh solver bit for bit (phi_, phis_, the effective moduli and the laminate lists are
    rebuilt, nothing of the earlier count is left behind)."""
    from fibergen_amd import LSSolver
    grid = (4, 16, 80)
    m8, p8, n8 = problem(grid, 8, "laminate")
    m2 = iso_mats(np.random.default_rng(77), 2)
    p2 = [p8[0] + sum(p8[2:]), p8[1]]
    m5, fine5, coarse5, _ = dfg_problem(grid, 5)

    def stages(make):
        out = []
        for k in range(3):
            s = make(k)
            assert s.run(E_LOAD) is False
            out.append((s.iterations, np.array(s.residuals), s.get_field("epsilon"), s.mean_stress().copy(), s.get_field("phi"),
                        np.array([s.counter("interface_voxels"), s.counter("affected_voxels")])))
            if s is not live:
                s.close()
        return out

    live = LSSolver(*grid)

    def configure(s, k):
        if k == 0:
            return gpu_solver(grid, m8, p8, n8, cls=s, gamma_scheme="staggered", mixing_rule="laminate", u_loop=2, tol=1e-7)
        if k == 1:
            return gpu_solver(grid, m2, p2, None, cls=s, gamma_scheme="staggered", mixing_rule="voigt", u_loop=2, tol=1e-7)
        return dfg_solver(grid, m5, fine5, coarse5, cls=s, mixing_rule="voigt", u_loop=2, tol=1e-7)

    got = stages(lambda k: configure(live, k))
    want = stages(lambda k: configure(LSSolver(*grid), k))
    for k, (a, b) in enumerate(zip(got, want)):
        assert a[0] == b[0], k
        for x, y in zip(a[1:], b[1:]):
            assert x.shape == y.shape and np.array_equal(x, y), k
    assert got[0][4].shape[0] == 8 and got[1][4].shape[0] == 2 and got[2][4].shape[0] == 5
    # the laminate lists: those of the eight phases after stage 0 (k_mixed_list's criterion, as test_every_loop_variant_converged
    # counts them), and after set_num_phases(2) what a fresh two-phase solver reports (compared above), not the earlier lists
    mixed = int(np.any([(p != 0) & (p != 1) for p in p8], axis=0).sum())
    assert got[0][5][0] == mixed > 0 and mixed <= got[0][5][1] <= 7 * mixed
    assert np.array_equal(got[1][5], want[1][5]) and np.array_equal(got[2][5], want[2][5])
    live.close()


# ------------------------------------------------------------------------------------------------ 9. slab driver
@pytest.mark.parametrize("nph", [4, 8])
@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
@pytest.mark.parametrize("grid", [(8, 16, 124), (4, 6, 8)])
def test_slab_group_two_ranks(grid, mixing, method, nph):
    """SlabGroup, P = 2, one tiled and one small grid of draw_slab's ranges: the interface planes carry pairs other than
    (0, 1).  Bars of test_random_slab_group_matches_oracle.  The oracle alone: 5 to 109 iterations (maxiter 400)."""
    from fibergen_amd.distributed import SlabGroup
    mats, phis, normals = problem(grid, nph, mixing)
    if normals is None:
        from phase_draws import random_normals
        normals = random_normals(np.random.default_rng(3), grid)
    common = dict(tol=1e-7, maxiter=400)
    o = ls_oracle(grid, mats, phis, normals, mixing, **common)
    g = SlabGroup(*grid, nranks=2)
    g.set_num_phases(nph)
    for p, (m, phi) in enumerate(zip(mats, phis)):
        g.set_phase(p, m[0], m[1], phi)
    g.set_normals(normals)
    g.set_options(mixing_rule=mixing, method=method, **common)
    tag = (grid, mixing, method, nph)
    if method == "cg":
        assert o.run_cg(E_LOAD) is False and g.run(E_LOAD) is False, tag
    else:
        assert o.run(E_LOAD) is False and g.run(E_LOAD) is False, tag
    assert g.iterations == o.iterations < 400, tag
    assert np.abs(np.array(g.residuals) - np.array(o.residuals)).max() < 1e-9, tag
    assert rel_err(g.get_field("epsilon"), o.eps) < 1e-8, tag
    mtol = 1e-8 if method == "cg" else 1e-9
    assert np.abs(g.mean_stress() - o.mean_stress()).max() < mtol * max(1.0, np.abs(o.mean_stress()).max()), tag
    g.close()


# ------------------------------------------------------------------------------------------------ 10. geometry
@pytest.mark.parametrize("matrix", [0, 3])
@pytest.mark.parametrize("shape", [(20, 20, 20), (24, 20, 12)])
def test_voxelizer_eight_materials(shape, matrix):
    """fg_voxelize with seven inclusion materials and the matrix (k_vox_normalize(nph = 8)), overlapping capsules, against
    voxel_oracle as test_gpu_voxelize.test_product_equals_checker compares (its TOL); (24, 20, 12) is the (2n)^3 grid
    full_staggered voxelises for the small grid of this file"""
    from oracle import voxel_oracle
    from test_gpu_voxelize import TOL, both, random_capsules
    fibers = random_capsules(21, 8, tuple(m for m in range(8) if m != matrix))
    (phi, nrm, real), (phi_c, nrm_c, real_c) = both(fibers, shape, nph=8, matrix=matrix)
    assert phi.shape == (8,) + shape and all(phi[m].max() > 0 for m in range(8))
    assert np.abs(phi - phi_c).max() <= TOL
    assert np.abs(voxel_oracle.normalize_phi(phi) - voxel_oracle.normalize_phi(phi_c)).max() <= TOL
    assert np.abs(nrm - nrm_c).max() <= 1e-13
    assert real == real_c
    assert ((phi >= 0) & (phi <= 1)).all()


def eight_phase_solver(shape, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*shape)
    s.set_num_phases(8)
    for p, (mu, lam) in enumerate(iso_mats(np.random.default_rng(5), 8)):
        s.set_phase(p, mu, lam)
    s.set_options(mu_0=2.0, lambda_0=1.5, **opts)
    return s


@pytest.mark.parametrize("matrix", [0, 3])
def test_voxelize_into_eight_materials(matrix):
    """fg_voxelize_into with nph = 8 on 20^3: the solver's normalised fractions and normals against voxel_oracle at
    test_gpu_voxelize's bars, and exactly equal to the host path (geometry.voxelize, normalised, set_phase) as
    test_gpu_voxelize_into.test_fields_equal_host_path asserts"""
    from fibergen_amd import geometry
    from fibergen_amd.fg import _normalize_phi
    from oracle import voxel_oracle
    from test_gpu_voxelize import TOL, random_capsules
    shape, dims, x0 = (20, 20, 20), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    fibers = random_capsules(21, 8, tuple(m for m in range(8) if m != matrix))
    dev = eight_phase_solver(shape)
    real_dev = dev.voxelize_into(fibers, x0, matrix, want_normals=True)
    phi_c, nrm_c, real_c = voxel_oracle.voxelize(fibers, shape, dims, x0, 8, matrix, want_normals=True)
    phi = dev.get_field("phi")
    # (the normalisation walks the materials from the last to the first and the matrix takes all that is left: with the matrix
    # at 3 the materials before it end up empty, in the oracle as here)
    assert phi.shape == (8,) + shape and all(phi[m].max() > 0 for m in range(matrix, 8))
    assert np.abs(phi - voxel_oracle.normalize_phi(phi_c)).max() <= TOL
    assert np.abs(dev.get_field("normals") - nrm_c).max() <= 1e-13
    raw, nrm, real = geometry.voxelize(fibers, shape, dims, x0, 8, matrix, want_normals=True)
    assert real_dev == real == real_c
    assert np.delete(raw, matrix, axis=0).sum(axis=0).max() > 1 + 1e-6      # the capsules overlap: the normalisation acts
    assert np.array_equal(phi, _normalize_phi(raw)) and np.array_equal(dev.get_field("normals"), nrm)
    assert dev.counter("phase_uploads") == 0
    dev.close()


@pytest.mark.parametrize("matrix", [0, 3])
def test_voxelize_into_eight_materials_fine(matrix):
    """FG_VOX_FINE with nph = 8: the (2n)^3 images of full_staggered, normalised on the device; the solver's coarse fractions
    (8-cell means) against the normalised images of voxel_oracle at test_gpu_voxelize's TOL, and exactly equal to a solver
    that got the host-normalised images through set_phase_fine (test_fine_form_full_staggered)"""
    from dfg_reference import restrict_component
    from fibergen_amd import geometry
    from fibergen_amd.fg import _normalize_phi
    from oracle import voxel_oracle
    from test_gpu_voxelize import TOL, random_capsules
    shape, dims, x0 = (12, 10, 6), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    fshape = tuple(2 * n for n in shape)
    fibers = random_capsules(21, 8, tuple(m for m in range(8) if m != matrix))
    dev = eight_phase_solver(shape, gamma_scheme="full_staggered")
    real_dev = dev.voxelize_into(fibers, x0, matrix, fine=True)
    phi_c, _n, real_c = voxel_oracle.voxelize(fibers, fshape, dims, x0, 8, matrix)
    want = np.stack([restrict_component(f, (0, 0, 0)) for f in voxel_oracle.normalize_phi(phi_c)])
    phi = dev.get_field("phi")
    assert phi.shape == (8,) + shape and all(phi[m].max() > 0 for m in range(matrix, 8))
    assert np.abs(phi - want).max() <= TOL
    raw, _n, real = geometry.voxelize(fibers, fshape, dims, x0, 8, matrix)
    assert real_dev == real == real_c
    host = eight_phase_solver(shape, gamma_scheme="full_staggered")
    for p, f in enumerate(_normalize_phi(raw)):
        host.set_phase_fine(p, f)
    assert np.array_equal(phi, host.get_field("phi"))
    for s in (dev, host):
        s.iterate(E_LOAD, 3)
    assert np.array_equal(dev.get_field("epsilon"), host.get_field("epsilon"))
    dev.close()
    host.close()


def project_xml(nmat, extra=""):
    """a <place_fiber> project with nmat <materials> entries: the matrix and nmat - 1 inclusion materials, one overlapping
    capsule each"""
    rng = np.random.default_rng(40 + nmat)
    mats = '<matrix E="1" nu="0.3" />' + "".join('<m%d E="%.3f" nu="%.3f" />' % (k, rng.uniform(2.0, 20.0), rng.uniform(0.1, 0.35))
                                                 for k in range(1, nmat))
    acts = ""
    for k in range(1, nmat):
        c, a = rng.uniform(0.25, 0.75, 3), rng.standard_normal(3)
        acts += ('<select_material name="m%d" /><place_fiber type="capsule" cx="%.3f" cy="%.3f" cz="%.3f" ax="%.3f" ay="%.3f" '
                 'az="%.3f" L="%.3f" R="%.3f" />' % (k, c[0], c[1], c[2], a[0], a[1], a[2], rng.uniform(0.3, 0.6), rng.uniform(0.1, 0.18)))
    return ('<settings><solver n="12"><tol>1e-6</tol><method>cg</method><mixing_rule>voigt</mixing_rule><materials>%s</materials>'
            '</solver><actions>%s%s<calc_effective_properties /></actions></settings>' % (mats, acts, extra))


def test_project_with_five_materials_device_geometry_on_and_off():
    """FG with five <materials> entries: the geometry voxelised inside the solver (device_geometry, the default) and handed over
    through host arrays give bit-identical fractions, volume fractions and C_eff (test_gpu_fg_device_geometry.test_results_identical)"""
    from test_gpu_fg_device_geometry import run
    xml = project_xml(5)
    dev, host = run(xml, True), run(xml, False)
    assert dev._lss.counter("phase_uploads") == 0 and host._lss.counter("phase_uploads") >= 5
    names = dev.get_phase_names()
    assert len(names) == 5 and names == host.get_phase_names()
    phi = dev.get_field("phi")
    assert phi.shape == (5, 12, 12, 12) and np.array_equal(phi, host.get_field("phi"))
    assert ((phi > 0) & (phi < 1)).any() and all(phi[m].max() > 0 for m in range(5))
    for name in names:
        assert dev.get_volume_fraction(name) == host.get_volume_fraction(name) > 0
        a, b = dev.get_real_volume_fraction(name), host.get_real_volume_fraction(name)
        assert a == b or (np.isnan(a) and np.isnan(b))
        assert np.array_equal(dev.get_field(name), host.get_field(name))
    C = np.array(dev.get_effective_property())
    assert C.shape == (6, 6) and np.array_equal(C, np.array(host.get_effective_property()))
    assert dev.get_residuals() == host.get_residuals()


@pytest.mark.parametrize("device", [True, False])
def test_project_with_nine_materials_is_refused(device):
    """one material more than kMaxPhases: fg_set_num_phases refuses with "number of phases must be in [1, 8]" on both paths"""
    from fibergen_amd import FG
    fg = FG()
    fg.device_geometry = device
    fg.set_xml(project_xml(9))
    with pytest.raises(RuntimeError, match=r"number of phases must be in \[1, 8\]"):
        fg.run()

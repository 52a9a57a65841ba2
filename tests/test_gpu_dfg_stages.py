"""gamma_scheme full_staggered stage by stage: every kernel of one pass against the literal fine-grid chain of
tests/dfg_reference.py (DfgLSOracle / DfgViscosityOracle) and against the coarse fraction form the library evaluates, on every
tile shape of the five-moduli sweeps (k_u_tile / k_eps_tile with NMOD = 5) and on the untiled path, with one to three phases
given as fine images, coarse fields (k_dfg_fractions_replica) or a mix of both (the fine_set_ mask).

Bars (the rules of test_gpu_parity.py and test_dfg_oracle.py): an element-wise stage against the same algebraic form
(pk1_fractions, C0 subtracted as calc_stress does) 1e-14; against the literal prolong -> PK1 -> restrict chain 1e-13;
means 1e-12; a stage that contains transforms 1e-12.

That these files can fail was checked with seven value-only changes to the library, one at a time (first red test of
test_gpu_dfg_stages / _state / _fuzz / _project in that order):
  k_u_tile NMOD = 5 with Sc[2] for t4 and Sc[1] for t5       test_iteration_stage_and_iterate[6x14x128-2ph-fine-<8,1>]
  k_dfg_moduli reading phis + (3 (p & 1) + c) n              test_stress_stage[16x16x128-3ph-mixed-<8,1>]
  k_dfg_moduli without the threshold on the shear groups     test_voigt_threshold_drops_a_stiff_trace_phase[elasticity-4x16x80-tiled]
  k_dfg_stress<2> with shear weight 1                        test_gpu_dfg_state::test_estimators_and_load_steps[5x14x100-tiled-basic-energy]
  k_dfg_fractions_replica: phi_s.p[1] with yb for xb         test_stress_stage[16x16x128-3ph-mixed-<8,1>]
  set_phase_field keeping the fine_set_ bit                  test_gpu_dfg_state::test_one_solver_through_reconfigurations[4x16x80-tiled-basic]
  launch_eps_tile nz = 256 on <8,0,5> with A_23 <-> A_13     test_iteration_stage_and_iterate[4x14x256-2ph-coarse-<6,2>]"""
import numpy as np
import pytest

from dfg_reference import (DfgLSOracle, DfgViscosityOracle, calc_stress_fractions, fine_images, input_kinds, split_input,
                           tile_shape)
from helpers import rel_err

gpu = pytest.mark.gpu

MU0, LAM0 = 0.77, 0.31
ISO, A1, A2, A3 = (1.0, 1.0, 1.0), (2.0, 1.0, 0.5), (1.0, 1.5, 0.8), (0.7, 1.3, 2.1)

# grid, cell, what it reaches
GRIDS = [
    ((6, 14, 128), A1, "<8,1>, last march of 2 planes, surplus workgroups"),
    ((16, 16, 128), ISO, "<8,1>"),
    ((4, 14, 256), A2, "<6,2>"),
    ((5, 20, 256), ISO, "<6,2>, partial march"),
    ((5, 14, 100), A3, "<8,0> short, nz/2 = 50: wrapped surplus lanes"),
    ((4, 16, 80), ISO, "<8,0> short, nz/2 = 40: the lower edge of u_tile_supported"),
    ((4, 14, 200), A1, "<8,0> two z tiles, the second clamped"),
    ((6, 15, 130), ISO, "<8,0> two z tiles, clamped last y tile"),
    ((8, 14, 124), (1.0, 2.0, 0.5), "<8,0> exact: one tile of 62 pairs"),
    ((9, 7, 5), ISO, "untiled: odd nz"),
    ((12, 10, 6), A1, "untiled"),
    ((8, 16, 78), A2, "untiled: nz/2 = 39 just below the tile limit"),
    ((8, 12, 128), ISO, "untiled: ny = 12 just below the tile limit"),
    ((1, 1, 4), A3, "untiled: degenerate x and y (the shifted 8-cell block wraps onto itself)"),
    ((10, 1, 1), ISO, "untiled: degenerate y and z"),
]
# (phases, input) per grid, in the order of GRIDS: every phase count and every input kind meets every tile shape and the
# untiled path (test_case_table_covers_every_shape)
CONFIGS = [
    [(1, "coarse"), (2, "fine")], [(3, "mixed"), (2, "mixed")],          # <8,1>
    [(1, "fine"), (2, "coarse")], [(3, "mixed"), (3, "fine")],           # <6,2>
    [(2, "mixed"), (3, "coarse")], [(1, "fine"), (3, "fine")],           # <8,0> short
    [(3, "fine"), (1, "coarse")], [(2, "mixed"), (2, "coarse")],         # <8,0> two
    [(1, "fine"), (2, "coarse"), (3, "mixed")],                          # <8,0> exact
    [(3, "fine"), (2, "mixed")], [(2, "coarse"), (3, "mixed")], [(1, "fine"), (3, "coarse")], [(2, "fine"), (3, "mixed")],
    [(3, "fine"), (2, "mixed"), (1, "coarse")], [(3, "mixed"), (2, "coarse"), (1, "fine")],
]
CASES = [(g, d, nph, kind) for (g, d, _), cfgs in zip(GRIDS, CONFIGS) for nph, kind in cfgs]
IDS = ["%s-%dph-%s-%s" % ("x".join(map(str, g)), nph, kind, tile_shape(g).replace(" ", "-")) for g, _d, nph, kind in CASES]
cases = pytest.mark.parametrize("grid,dims,nph,kind", CASES, ids=IDS)

ELASTIC = [(0.38, 0.58), (4.2, 2.8), (1.7, 0.4)]
FLUID = [(1.0, 0.0), (0.05, 0.0), (3.0, 0.0)]


def test_case_table_covers_every_shape():
    """CPU: the table above holds what its comment says, on grids of the classes the issue names"""
    assert len(GRIDS) == len(CONFIGS) == 15 and len(CASES) >= 30
    assert sum(1 for _g, d, _ in GRIDS if len(set(d)) > 1) >= 8          # anisotropic cells on at least half
    seen = {}
    for g, _d, nph, kind in CASES:
        seen.setdefault(tile_shape(g), set()).update([nph, kind])
    assert set(seen) == {"<8,1>", "<6,2>", "<8,0> short", "<8,0> exact", "<8,0> two", "untiled"}
    for shape, have in seen.items():
        assert have >= {1, 2, 3, "fine", "coarse", "mixed"}, shape
    for g, _d, what in GRIDS:
        assert what.startswith(tile_shape(g)), (g, what)


def _pair(grid, dims, nph, kind, viscosity=False, seed=0, **opts):
    """the product and the fine-grid oracle of one case, both with the reference medium (0.77, 0.31)"""
    from fibergen_amd import LSSolver
    rng = np.random.default_rng(700 + seed)
    mats = (FLUID if viscosity else ELASTIC)[:nph]
    fine, coarse, ofine = split_input(fine_images(rng, grid, nph), input_kinds(kind, nph))
    s = LSSolver(*grid, *dims)
    s.set_options(mode="viscosity" if viscosity else "elasticity", gamma_scheme="full_staggered")
    s.set_num_phases(nph)
    for p, (mu, lam) in enumerate(mats):
        s.set_phase(p, mu, lam, coarse[p])
        if fine[p] is not None:
            s.set_phase_fine(p, fine[p])
    s.set_options(mu_0=MU0, lambda_0=LAM0, **opts)
    cls = DfgViscosityOracle if viscosity else DfgLSOracle
    o = cls(*grid, *dims, mats=mats, phis=[np.zeros(grid)] * nph, phis_fine=ofine)
    o.mu_0, o.lambda_0 = MU0, LAM0
    return s, o, ofine, mats, rng


def _stress_checks(s, o, ofine, mats, eps, viscosity):
    s.set_field("epsilon", eps)
    s.run_stage("stress")
    tau = s.get_field("tau")
    assert rel_err(tau, calc_stress_fractions(eps, ofine, mats, MU0, LAM0, viscosity)) < 1e-14
    assert rel_err(tau, o.calc_stress(MU0, LAM0, eps)) < 1e-13
    sigma = s.get_field("sigma")
    assert rel_err(sigma, calc_stress_fractions(eps, ofine, mats, 0.0, 0.0, viscosity)) < 1e-14
    assert rel_err(sigma, o.pk1(eps)) < 1e-13
    assert rel_err(s.mean_stress(), o.mean_stress(eps)) < 1e-12
    assert rel_err(s.get_field("phi"), np.array(o.phis)) < 1e-15


@gpu
@cases
def test_stress_stage(grid, dims, nph, kind):
    """k_dfg_fractions_fine / k_dfg_fractions_replica -> k_dfg_moduli -> k_dfg_stress<0> (tau, sigma) and
    k_dfg_stress<1> (mean stress); "phi" is the restriction of the fine image"""
    s, o, ofine, mats, rng = _pair(grid, dims, nph, kind)
    _stress_checks(s, o, ofine, mats, rng.standard_normal((6,) + grid), False)
    s.close()


E_EL = np.array([1.0, 0.2, -0.3, 0.1, 0.0, 0.4])
E_FL = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])


@gpu
@cases
def test_iteration_stage_and_iterate(grid, dims, nph, kind):
    """One pass of Solver::basic_scheme (run_stage "iteration": the strain-state pipeline -- k_eps_tile<...,5> on tiled
    grids, k_dfg_stress<0> + k_div on the others and with fuse_stress_div = 0), then iterate(E, n) for n = 1 and 3 from the same
    strain field.  Solver::iterate from a SET strain field has no displacement yet (u_valid_ is false): its first pass is
    basic_scheme, the passes after it are the displacement loop where plan::u_loop (fg_sweep_plan.h) admits it -- under full_staggered
    that is the tiled grids with u_loop = 2 and u_tile = 1 (the five-moduli k_u_tile); with u_tile = 0, and on untiled grids,
    every pass is basic_scheme.  So n = 3 with the default options runs k_eps_tile<...,5> once and k_u_tile<...,5> twice,
    n = 3 with u_tile = 0 runs k_eps_tile<...,5> three times: both against three passes of the oracle."""
    s, o, _ofine, _mats, rng = _pair(grid, dims, nph, kind, seed=1)
    eps0 = 0.1 * rng.standard_normal((6,) + grid)
    ref = [eps0]
    for _ in range(3):
        ref.append(o.basic_scheme(E_EL, ref[-1]))
    tiled = tile_shape(grid) != "untiled"
    variants = [{}] + ([{"u_tile": 0}, {"fuse_stress_div": 0}] if tiled else [{"fuse_stress_div": 0}])
    for opts in variants:
        s.set_options(**{"u_tile": 1, "fuse_stress_div": 1, **opts})
        s.set_field("epsilon", eps0)
        s.run_stage("iteration", E_EL)
        assert rel_err(s.get_field("epsilon"), ref[1]) < 1e-12, opts
        for n in (1, 3):
            s.set_field("epsilon", eps0)
            s.iterate(E_EL, n)
            assert rel_err(s.get_field("epsilon"), ref[n]) < 1e-12, (opts, n)
    s.close()


@gpu
@pytest.mark.parametrize("grid,dims", [(g, d) for g, d, _ in GRIDS if tile_shape(g) != "untiled"],
                         ids=["x".join(map(str, g)) + "-" + tile_shape(g).replace(" ", "-") for g, _d, _ in GRIDS
                              if tile_shape(g) != "untiled"])
def test_displacement_loop_from_the_uniform_field(grid, dims):
    """the five-moduli k_u_tile from the state run() starts it in: iterate(E, n) on the zero strain field gives eps_1 = E
    by one strain-state pass and n - 1 tiled displacement passes; three phases, mixed input"""
    s, o, _ofine, _mats, _rng = _pair(grid, dims, 3, "mixed", seed=2)
    s.set_field("epsilon", np.zeros((6,) + grid))
    s.iterate(E_EL, 4)
    ref = np.zeros((6,) + grid)
    for _ in range(4):
        ref = o.basic_scheme(E_EL, ref)
    assert rel_err(s.get_field("epsilon"), ref) < 1e-12
    s.close()


@gpu
@cases
def test_viscosity_stress_and_iteration_stages(grid, dims, nph, kind):
    """mode = viscosity: the five-moduli branch of the strain-state pass (k_eps_tile<...,5> + the recomputing tail
    launch_eps_delta_recompute on tiled grids; k_dfg_stress<0> + k_div + k_eps_delta elsewhere and with fuse_stress_div = 0)
    against DfgViscosityOracle; iterate() never enters the displacement loop in this mode (plan::u_loop, fg_sweep_plan.h: mode 0 only)"""
    s, o, ofine, mats, rng = _pair(grid, dims, nph, kind, viscosity=True, seed=3)
    _stress_checks(s, o, ofine, mats, rng.standard_normal((6,) + grid), True)
    eps0 = rng.standard_normal((6,) + grid)
    ref1 = o.basic_scheme(E_FL, eps0)
    ref2 = o.basic_scheme(E_FL, ref1)
    for opts in ({}, {"fuse_stress_div": 0}):
        s.set_options(**{"fuse_stress_div": 1, **opts})
        s.set_field("epsilon", eps0)
        s.run_stage("iteration", E_FL)
        assert rel_err(s.get_field("epsilon"), ref1) < 1e-12, opts
        s.set_field("epsilon", eps0)
        s.iterate(E_FL, 2)
        assert rel_err(s.get_field("epsilon"), ref2) < 1e-12, opts
    s.close()


@gpu
@pytest.mark.parametrize("grid", [(4, 16, 80), (9, 7, 5)], ids=["4x16x80-tiled", "9x7x5-untiled"])
@pytest.mark.parametrize("mode", ["elasticity", "viscosity"])
def test_voigt_threshold_drops_a_stiff_trace_phase(grid, mode):
    """The Voigt rule skips a phase whose fraction is <= 10 eps (F:12736), in k_dfg_moduli for each of the four component
    groups.  A block of fine cells holds 1.5e-15 of a phase of modulus 1e14 (zero elsewhere), so every group fraction of that
    phase is below the threshold and the phase must not contribute at all; taken into the sum it would add up to 0.3 to moduli
    of order one.  The chain (threshold per fine cell) and the fraction form (threshold per group mean) agree here."""
    from fibergen_amd import LSSolver
    viscosity = mode == "viscosity"
    rng = np.random.default_rng(710)
    fshape = tuple(2 * n for n in grid)
    trace = np.zeros(fshape)
    trace[: max(1, fshape[0] // 2), : max(1, fshape[1] // 2), 1:fshape[2] // 2] = 1.5e-15
    images = fine_images(rng, grid, 2) + [trace]
    mats = [(1.0, 0.0 if viscosity else 0.6), (0.2, 0.0 if viscosity else 1.1), (1e14, 0.0 if viscosity else 1e14)]
    s = LSSolver(*grid, 1.0, 1.5, 0.8)
    s.set_options(mode=mode, gamma_scheme="full_staggered")
    s.set_num_phases(3)
    for p, (mu, lam) in enumerate(mats):
        s.set_phase(p, mu, lam)
        s.set_phase_fine(p, images[p])
    s.set_options(mu_0=MU0, lambda_0=LAM0)
    cls = DfgViscosityOracle if viscosity else DfgLSOracle
    o = cls(*grid, 1.0, 1.5, 0.8, mats=mats, phis=[np.zeros(grid)] * 3, phis_fine=images)
    o.mu_0, o.lambda_0 = MU0, LAM0
    eps = rng.standard_normal((6,) + grid)
    two = cls(*grid, 1.0, 1.5, 0.8, mats=mats[:2], phis=[np.zeros(grid)] * 2, phis_fine=images[:2])
    assert rel_err(o.pk1(eps), two.pk1(eps)) == 0.0          # the reference drops the trace phase
    _stress_checks(s, o, images, mats, eps, viscosity)
    s.set_field("epsilon", eps)
    s.run_stage("iteration", E_FL)
    assert rel_err(s.get_field("epsilon"), o.basic_scheme(E_FL, eps)) < 1e-12
    s.close()

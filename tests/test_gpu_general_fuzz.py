"""law="general" in the randomised draws, against the restatement tests/general_reference.py.

Seeds 0 ... 29: the draw of test_gpu_fuzz.py (grid, cell, fractions, method, loop options, mixed boundary conditions, load steps,
load) with at least one phase -- any phase, also the first -- turned into a random 6x6 stiffness, the Green operator drawn among
staggered / collocated / willot, the error estimator among epsilon / sigma / residual / energy, and linear load-step extrapolation.
Mixing is Voigt, the only rule general phases have.  The restatement alone converges for all 30 within maxiter = 400 (at most
114 passes; checked on the CPU), none is left out.

Tile draws, 12 seeds: two complementary phases on the grids of test_gpu_general.TILE_GRIDS, the general law on the fibre, the
matrix or both, basic or CG, mixed boundary conditions with probability 0.3 and, with probability 0.25, one switch that takes
the run off the tiled sweep's anisotropic form (u_loop = 1, u_tile = 0, phi_sweep = 0, aniso_tile = 0); the counter "u_tile_aniso" must report
that form exactly where the draw says it runs.

The reference medium: the device scan is held against the restatement's at 1e-13 relative (the bar of
test_gpu_general.test_reference_material_scan), then both sides run on the device's value, so that its last bits do not decide
an iteration count.

Bars as in test_gpu_fuzz.py: the failed flag and iteration counts equal, residual histories 1e-9, strain fields 1e-8, mean stress
1e-9 (runs to tol 1e-7)."""
from dataclasses import dataclass

import numpy as np
import pytest

import general_reference as gr
from helpers import lame, rel_err
from test_gpu_fuzz import PROJECTORS, draw, smooth_field
from test_gpu_general import TILE_GRIDS
from willot_reference import WillotMixin

COMMON = dict(tol=1e-7, maxiter=400)
N_TILE = 12
# chosen so that the tiled form is expected in at least 6 of the 12 tile draws and all four switches are drawn (the CPU test
# test_tile_draws_cover_the_tiled_form_and_every_way_off_it)
TILE_OFFSET = 11
SWITCHES = (("u_loop", 1), ("u_tile", 0), ("phi_sweep", 0), ("aniso_tile", 0))


@dataclass
class FixedRefGeneral(gr.GeneralLSOracle):
    """the restatement on a reference medium handed in (the product's): calc_ref_material keeps mu_0 and does the rest of its
    work, the matrices of the boundary-condition projector"""

    def calc_ref_material(self):
        if np.isnan(self.mu_0):
            raise RuntimeError("FixedRefGeneral needs mu_0")
        self._set_bc_projector(self.BC_P)


@dataclass
class FixedRefWillotGeneral(WillotMixin, FixedRefGeneral):
    pass


def draw_general(seed):
    c = dict(draw(seed))
    rng = np.random.default_rng(21000 + seed)
    nph = len(c["mats"])
    forced = int(rng.integers(nph))
    mats, general = [], []
    for p in range(nph):
        g = p == forced or rng.random() < 0.5
        C = gr.random_spd(rng, coupling=rng.random() < 0.7, scale=rng.uniform(0.05, 1.0))   # drawn whether used or not
        mats.append(C if g else c["mats"][p])
        general.append(bool(g))
    c["mats"], c["general"] = mats, general
    c["scheme"] = str(rng.choice(["staggered", "staggered", "staggered", "collocated", "willot"]))
    c["estimator"] = str(rng.choice(["epsilon", "epsilon", "sigma", "residual" if c["method"] == "cg" else "epsilon"]))
    c["extrapolation"] = 1 if (c["steps"] is not None and rng.random() < 0.3) else 0
    if rng.random() < 0.15:
        c["estimator"] = "energy"
    # laminate mixing and full_staggered are refused for general phases (test_gpu_general.py tests the refusals)
    c["mixing"], c["normals"] = "voigt", None
    return c


def draw_general_tile(seed):
    rng = np.random.default_rng(23000 + 100 * TILE_OFFSET + seed)
    shape = tuple(int(v) for v in TILE_GRIDS[int(rng.integers(len(TILE_GRIDS)))])
    dims = tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3))
    p1 = smooth_field(rng, shape)
    general = [(False, True), (True, False), (True, True)][seed % 3]   # (matrix, fibre)
    mats = []
    for p in range(2):
        C = gr.random_spd(rng, coupling=rng.random() < 0.7, scale=rng.uniform(0.05, 1.0))
        iso = lame(E=float(rng.uniform(0.5, 20.0)), nu=float(rng.uniform(0.05, 0.4)))
        mats.append(C if general[p] else iso)
    method = "cg" if rng.random() < 0.5 else "basic"
    bc = str(rng.choice(list(PROJECTORS))) if rng.random() < 0.3 else None
    opts = {}
    if rng.random() < 0.25:      # one switch that must send the run off the tiled form
        name, value = SWITCHES[int(rng.integers(len(SWITCHES)))]
        opts[name] = value
    return dict(shape=shape, dims=dims, mats=mats, general=list(general), phis=[1.0 - p1, p1], normals=None, mixing="voigt",
                scheme="staggered", method=method, opts=opts, bc=bc, steps=None, E=rng.uniform(-1.0, 1.0, size=6),
                estimator="epsilon", extrapolation=0)


def tiled_form_expected(c):
    """Whether k_u_tile's ANISO form must run, from the draw alone.  A general phase enters the displacement loop only through
    plan::aniso_tile (fg_sweep_plan.h): option aniso_tile, elasticity, the staggered operator, Voigt mixing, u_loop >= 2, u_tile, one GPU, a grid
    u_tile_supported takes (even nz >= 80, ny >= 14, nx >= 4) and two phases whose fractions are complementary bit for bit with
    phi_sweep on (two_phase_complementary).  method basic: plan::u_loop with mixed boundary conditions allowed then admits pure strain
    and, on these grids, mixed boundary conditions (the sweep's form with the sums of tau), and the first pass of a fresh step
    already runs u_pass_front.  method cg: run_cg enters run_cg_u (whose operator is u_pass_front, or the sweep's form with the CG
    direction) only if plan::u_loop without mixed boundary conditions holds and the estimator is epsilon or residual;
    otherwise CG runs in strain space through k_stress."""
    o = c["opts"]
    nx, ny, nz = c["shape"]
    grid_ok = nz % 2 == 0 and nz // 2 >= 40 and ny >= 14 and nx >= 4
    complementary = len(c["phis"]) == 2 and bool(np.all(c["phis"][0] == 1.0 - c["phis"][1]))
    ok = (any(c["general"]) and o.get("aniso_tile", 1) and c["scheme"] == "staggered" and c["mixing"] == "voigt"
          and o.get("u_loop", 2) >= 2 and o.get("u_tile", 1) and grid_ok and complementary and o.get("phi_sweep", 1))
    if c["method"] == "cg":
        ok = ok and c["bc"] is None and c["estimator"] in ("epsilon", "residual")
    return bool(ok)


def test_tile_draws_cover_the_tiled_form_and_every_way_off_it():
    cs = [draw_general_tile(seed) for seed in range(N_TILE)]
    tiled = [seed for seed, c in enumerate(cs) if tiled_form_expected(c)]
    print("general tile draws: tiled form expected in seeds", tiled)
    assert len(tiled) >= 6
    assert {tuple(cs[seed]["general"]) for seed in tiled} == {(False, True), (True, False), (True, True)}
    assert {cs[seed]["method"] for seed in tiled} == {"basic", "cg"}
    assert any(cs[seed]["bc"] is not None for seed in tiled)
    # off the tiled form: by every switch, and by CG with mixed boundary conditions
    assert {name for c in cs for name in c["opts"]} == {name for name, _ in SWITCHES}
    assert any(c["method"] == "cg" and c["bc"] is not None and not c["opts"] for c in cs)


def _tag(seed, c):
    return "seed %d: %s" % (seed, {k: c[k] for k in ("shape", "general", "scheme", "method", "estimator", "extrapolation", "opts",
                                                     "bc", "steps")})


def _run_and_compare(seed, c):
    """the product and the restatement on the draw c at the bars of test_gpu_fuzz.py; returns the solver (None if both refused)"""
    from fibergen_amd import LSSolver
    shape, dims, tag = c["shape"], c["dims"], _tag(seed, c)
    s = LSSolver(*shape, *dims)
    s.set_num_phases(len(c["mats"]))
    for p, (m, phi) in enumerate(zip(c["mats"], c["phis"])):
        if gr.is_general(m):
            s.set_phase(p, 0.0, 0.0, phi)
            s.set_phase_stiffness(p, m)
        else:
            s.set_phase(p, m[0], m[1], phi)
    s.set_options(mixing_rule="voigt", gamma_scheme=c["scheme"], method=c["method"], error_estimator=c["estimator"],
                  loadstep_extrapolation_order=c["extrapolation"], **COMMON, **c["opts"])
    E, S0, P = c["E"].copy(), np.zeros(6), None
    if c["bc"] is not None:
        keep = np.array(PROJECTORS[c["bc"]], dtype=float)
        P = np.diag(keep)
        E = E * (keep > 0)
        s.set_bc_projector(P)
    kw = dict(mats=c["mats"], phis=c["phis"], mixing_rule="voigt", gamma_scheme=c["scheme"], error_estimator=c["estimator"],
              loadstep_extrapolation_order=c["extrapolation"], **COMMON)
    scan = gr.GeneralLSOracle(*shape, *dims, **kw)
    scan.calc_ref_material()
    mu_0, lam_0 = s.calc_ref_material()
    print(tag, "mu_0", mu_0, scan.mu_0)
    assert abs(mu_0 - scan.mu_0) <= 1e-13 * scan.mu_0 and lam_0 == 0.0, tag
    cls = FixedRefWillotGeneral if c["scheme"] == "willot" else FixedRefGeneral
    o = cls(*shape, *dims, mu_0=mu_0, **kw)
    params = c["steps"] or [0.0, 1.0]
    try:
        ref_failed = o.run_load_steps(E, S0, P, params=params, method=c["method"])
    except RuntimeError as e:
        # a combination the restatement rejects must be rejected by the product with the same leading message
        with pytest.raises(RuntimeError) as got:
            s.run_load_steps(E, S0, params=params)
        assert str(e).split(":")[0][:24] in str(got.value), tag
        s.close()
        return None
    assert max(o.step_iterations) < COMMON["maxiter"], tag   # converged, not cut off
    failed = s.run_load_steps(E, S0, params=params)
    assert s.ref_material[0] == mu_0, tag       # the run's own scan gave the value the restatement ran on
    r, rr = np.array(s.residuals), np.array(o.residuals)
    e = rel_err(s.get_field("epsilon"), o.eps)
    m = np.abs(s.mean_stress() - o.mean_stress()).max() / max(1.0, np.abs(o.mean_stress()).max())
    print(tag, "iterations", s.iterations, o.iterations, "residuals", np.abs(r - rr).max() if r.shape == rr.shape else None,
          "eps", e, "mean stress", m)
    assert failed == ref_failed, tag
    assert s.iterations == o.iterations, tag
    assert r.shape == rr.shape and np.abs(r - rr).max() < 1e-9, tag
    assert e < 1e-8, tag
    assert m < 1e-9, tag
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(30))
def test_random_combination_with_general_phases_matches_restatement(seed):
    s = _run_and_compare(seed, draw_general(seed))
    if s is not None:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_TILE))
def test_random_tile_draw_with_general_phases(seed):
    """the run against the restatement, and the dispatch: the tiled sweep's anisotropic form runs exactly where
    tiled_form_expected (computed from the draw, never from the solver's answer) says it must"""
    c = draw_general_tile(seed)
    expected = tiled_form_expected(c)
    s = _run_and_compare(seed, c)
    assert s is not None, _tag(seed, c)
    n = s.counter("u_tile_aniso")
    print(_tag(seed, c), "u_tile_aniso", n, "expected", expected)
    assert (n > 0) == expected, _tag(seed, c)
    s.close()

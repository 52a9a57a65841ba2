"""law="aniso" (heat / porous) in the randomised draws, against the restatement tests/aniso_reference.py.

Seeds 0 ... 29: the draw of test_gpu_fuzz.draw_scalar (grid with axes from length 1 on, non-cubic cell, one to three phases, mode,
method, u_loop, mixed boundary condition, load; mode viscosity mapped to porous) with at least one phase -- any phase -- turned into
a random symmetric positive definite 3x3 conductivity of scale 0.05 ... 20.  The restatement alone converges for all 30 within
maxiter = 300 (at most 100 passes; checked on the CPU), none is left out.

Tile draws, 12 seeds: two complementary phases on the grids and cells of test_gpu_aniso.TILED_GRIDS, the laws aniso / aniso,
iso / aniso, aniso / iso, basic or CG and, with probability 0.25, one switch that takes the run off k_sc_tile_aniso (u_loop = 1,
u_tile = 0, phi_sweep = 0, aniso_sc_tile = 0); the counter "sc_tile_aniso" must report the tiled form exactly where the draw says it
runs.

The reference medium: the device's mu_0 is held against numpy's eigvalsh at 1e-13 relative (test_gpu_aniso.py), then handed to the
restatement, so that its last bits do not decide an iteration count.

Bars as in test_random_scalar_and_viscosity_problems_match_their_oracles: the failed flag and iteration counts equal, residual
histories 1e-9, gradient fields 1e-8, mean flux 1e-9; and the potential 1e-8 (runs to tol 1e-7)."""
import numpy as np
import pytest

from aniso_reference import FixedRefOracle, is_aniso, k6, random_spd3
from helpers import rel_err
from test_gpu_aniso import TILED_GRIDS, eig_mu0
from test_gpu_fuzz import draw_scalar, smooth_field

COMMON = dict(tol=1e-7, maxiter=300)
N_TILE = 12
# chosen so that the tiled form is expected in at least 6 of the 12 tile draws and all four switches are drawn (the CPU test
# test_tile_draws_cover_the_tiled_form_and_every_way_off_it)
TILE_OFFSET = 18
SWITCHES = (("u_loop", 1), ("u_tile", 0), ("phi_sweep", 0), ("aniso_sc_tile", 0))


def draw_aniso(seed):
    c = dict(draw_scalar(seed))
    if c["mode"] == "viscosity":
        c["mode"] = "porous"
    rng = np.random.default_rng(22000 + seed)
    nph = len(c["mus"])
    forced = int(rng.integers(nph))
    mats = []
    for p in range(nph):
        a = p == forced or rng.random() < 0.5
        K = random_spd3(rng, rng.uniform(0.05, 20.0))    # drawn whether used or not
        mats.append(K if a else c["mus"][p])
    c["mats"], c["opts"] = mats, {"u_loop": c["u_loop"]}
    return c


def draw_aniso_tile(seed):
    rng = np.random.default_rng(24000 + 100 * TILE_OFFSET + seed)
    shape, dims = TILED_GRIDS[int(rng.integers(len(TILED_GRIDS)))]
    p1 = smooth_field(rng, shape)
    aniso = [(True, True), (False, True), (True, False)][seed % 3]
    mats = []
    for p in range(2):
        K = random_spd3(rng, rng.uniform(0.05, 20.0))
        mu = float(rng.uniform(0.05, 20.0))
        mats.append(K if aniso[p] else mu)
    method = "cg" if rng.random() < 0.5 else "basic"
    opts = {}
    if rng.random() < 0.25:      # one switch that must send the run off the tiled form
        name, value = SWITCHES[int(rng.integers(len(SWITCHES)))]
        opts[name] = value
    return dict(shape=tuple(shape), dims=tuple(float(d) for d in dims), mats=mats, phis=[1.0 - p1, p1],
                mode=str(rng.choice(["heat", "porous"])), method=method, opts=opts, bc=False, E=rng.uniform(-1.0, 1.0, size=6))


def tiled_form_expected(c):
    """Whether k_sc_tile_aniso must run, from the draw alone: plan::sc_tile_aniso (fg_sweep_plan.h) -- option aniso_sc_tile, heat / porous, an
    aniso phase, u_loop >= 2, u_tile, no mixed boundary condition, one GPU, a grid sc_sweep_tiled takes (= u_tile_supported: even
    nz >= 80, ny >= 14, nx >= 4) and two phases whose fractions are complementary bit for bit with phi_sweep on
    (two_phase_complementary).  method basic asks it in every u_pass_front; method cg (run_cg_scalar) asks it for the fused form,
    whose operator sweep is k_sc_tile_aniso with the direction update, and otherwise applies the operator through u_pass_front,
    which asks again: the same predicate for both methods."""
    o = c["opts"]
    nx, ny, nz = c["shape"]
    grid_ok = nz % 2 == 0 and nz // 2 >= 40 and ny >= 14 and nx >= 4
    complementary = len(c["phis"]) == 2 and bool(np.all(c["phis"][0] == 1.0 - c["phis"][1]))
    mixed_bc = c["bc"] and c["method"] == "basic"
    return bool(o.get("aniso_sc_tile", 1) and any(is_aniso(m) for m in c["mats"]) and o.get("u_loop", 2) >= 2 and o.get("u_tile", 1)
                and not mixed_bc and grid_ok and complementary and o.get("phi_sweep", 1))


def test_tile_draws_cover_the_tiled_form_and_every_way_off_it():
    cs = [draw_aniso_tile(seed) for seed in range(N_TILE)]
    tiled = [seed for seed, c in enumerate(cs) if tiled_form_expected(c)]
    print("aniso tile draws: tiled form expected in seeds", tiled)
    assert len(tiled) >= 6
    assert len({tuple(is_aniso(m) for m in cs[seed]["mats"]) for seed in tiled}) == 3
    assert {cs[seed]["method"] for seed in tiled} == {"basic", "cg"}
    assert {name for c in cs for name in c["opts"]} == {name for name, _ in SWITCHES}


def _tag(seed, c):
    d = {k: c[k] for k in ("shape", "mode", "method", "opts", "bc")}
    d["laws"] = ["aniso" if is_aniso(m) else "iso" for m in c["mats"]]
    return "seed %d: %s" % (seed, d)


def _run_and_compare(seed, c, common):
    """the product and the restatement on the draw c; returns the solver"""
    from fibergen_amd import LSSolver
    shape, dims, tag = c["shape"], c["dims"], _tag(seed, c)
    s = LSSolver(*shape, *dims)
    s.set_options(mode=c["mode"])
    s.set_num_phases(len(c["mats"]))
    for p, (m, phi) in enumerate(zip(c["mats"], c["phis"])):
        if is_aniso(m):
            s.set_phase_conductivity(p, m if p % 2 else k6(m), phi)   # both input forms
        else:
            s.set_phase(p, m, 0.0, phi)
    s.set_options(method=c["method"], **common, **c["opts"])
    mu_0 = s.calc_ref_material()[0]
    want = eig_mu0(c["phis"], c["mats"])
    print(tag, "mu_0", mu_0, want)
    assert abs(mu_0 - want) <= 1e-13 * mu_0, tag
    o = FixedRefOracle(*shape, mus=c["mats"], phis=c["phis"], dx=dims[0], dy=dims[1], dz=dims[2], mu_0=mu_0, **common)
    E = c["E"][:3].copy()
    if c["bc"] and c["method"] == "basic":
        P3 = np.diag([1.0, 0.0, 1.0])   # gradient prescribed along x and z, zero mean flux along y
        P6 = np.zeros((6, 6))
        P6[:3, :3] = P3
        E = E * np.array([1.0, 0.0, 1.0])
        s.set_bc_projector(P6)
        s.set_options(bc_tol=1e-8)
        o.bc_tol = 1e-8
        ref_failed = o.run(E, np.zeros(3), P3)
        failed = s.run(E, np.zeros(6))
    else:
        ref_failed = o.run_cg(E) if c["method"] == "cg" else o.run(E)
        failed = s.run(E)
    assert s.ref_material[0] == mu_0, tag       # the run's own scan gave the value the restatement ran on
    r, rr = np.array(s.residuals), np.array(o.residuals)
    e = rel_err(s.get_field("epsilon"), o.eps)
    ms = np.asarray(s.mean_stress())[:3]
    m = np.abs(ms - o.mean_stress()).max() / max(1.0, np.abs(o.mean_stress()).max())
    T, To = s.get_field("u"), o.potential()
    t = np.abs(T[0] - To).max() / max(1.0, np.abs(To).max())
    print(tag, "iterations", s.iterations, o.iterations, "residuals", np.abs(r - rr).max() if r.shape == rr.shape else None,
          "gradient", e, "mean flux", m, "potential", t)
    assert failed == ref_failed, tag
    assert s.iterations == o.iterations, tag
    assert r.shape == rr.shape and np.abs(r - rr).max() < 1e-9, tag
    assert e < 1e-8, tag
    assert m < 1e-9, tag
    assert T.shape == (1,) + tuple(shape) and t < 1e-8, tag
    return s, o


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(30))
def test_random_scalar_problem_with_aniso_phases_matches_restatement(seed):
    c = draw_aniso(seed)
    s, o = _run_and_compare(seed, c, COMMON)
    assert o.iterations < COMMON["maxiter"], _tag(seed, c)   # converged, not cut off
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_TILE))
def test_random_tile_draw_with_aniso_phases(seed):
    """the run against the restatement, and the dispatch: k_sc_tile_aniso runs exactly where tiled_form_expected (computed from the
    draw, never from the solver's answer) says it must"""
    c = draw_aniso_tile(seed)
    expected = tiled_form_expected(c)
    s, o = _run_and_compare(seed, c, COMMON)   # (converged runs: the restatement takes 1.3 s on the largest grid, at most 47 passes)
    assert o.iterations < COMMON["maxiter"], _tag(seed, c)
    n = s.counter("sc_tile_aniso")
    print(_tag(seed, c), "sc_tile_aniso", n, "expected", expected)
    assert (n > 0) == expected, _tag(seed, c)
    s.close()

"""Randomised gamma_scheme full_staggered combinations through the C ABI against the fine-grid oracles
(tests/dfg_reference.py), in the style of test_gpu_fuzz.py and with its bars: iteration counts equal, residual histories
1e-9, strain fields 1e-8, mean stress 1e-9 (runs to tol 1e-7, maxiter 400).

A seed draws: the grid (even seeds from the small lists of test_gpu_fuzz.py, odd seeds walk a list of thin grids that take
the tiled five-moduli sweeps -- all three tile shapes, nx not a multiple of 4), the cell, one to three phases, per phase
fine or coarse input (fine images: smooth fields with pure cells, for a quarter of the seeds a sharp 0/1 image), the mode
(elasticity / viscosity), the method (basic / cg), the error estimator (epsilon, sigma, energy; residual with cg; viscosity
without energy: the oracle has no fluid energy to compare with), the loop switches (u_loop, u_tile, fuse_stress_div, fuse_x),
optionally a projector (mixed boundary conditions) and load steps.  The draw is deterministic per seed; no seed is skipped or
filtered by its outcome.  test_draw_covers_every_path (CPU) pins what the kept seeds reach."""
import os

import numpy as np
import pytest

from dfg_reference import DfgLSOracle, DfgViscosityOracle, fine_images, split_input, tile_shape
from helpers import lame, rel_err
from test_gpu_fuzz import LENGTHS_XY, LENGTHS_Z, PROJECTORS

N_DFG = int(os.environ.get("FG_FUZZ_SEEDS", "60"))

gpu = pytest.mark.gpu

# thin grids on the tiled sweeps: <8,1>, <6,2>, <8,0> short / exact / two z tiles, twice each, nx = 5, 6, 7 among them
TILED = [(6, 14, 128), (4, 14, 256), (5, 14, 100), (8, 14, 124), (4, 14, 200), (5, 16, 128), (5, 15, 256), (4, 16, 80),
         (7, 14, 124), (6, 15, 130)]
SHEAR = [0, 0, 0, 0.5, 0.5, 0.5]   # viscosity: shear stresses prescribed, normal shear rates zero (as the scalar fuzz)


def draw_dfg(seed, fields=True):
    rng = np.random.default_rng(21000 + seed)
    if seed % 2:
        shape = TILED[(seed // 2) % len(TILED)]
    else:
        while True:
            shape = (int(rng.choice(LENGTHS_XY)), int(rng.choice(LENGTHS_XY)), int(rng.choice(LENGTHS_Z)))
            if 8 <= shape[0] * shape[1] * shape[2] <= 8000:
                break
    dims = tuple(float(v) for v in rng.uniform(0.5, 2.0, size=3))
    nph = int(rng.choice([1, 2, 3], p=[0.15, 0.4, 0.45]))   # one phase is the homogeneous problem: one or two passes
    kinds = [str(rng.choice(["fine", "coarse"])) for _ in range(nph)]
    sharp = bool(rng.random() < 0.25)
    mode = "viscosity" if rng.random() < 0.3 else "elasticity"
    if mode == "viscosity":
        mats = [(float(rng.uniform(0.05, 5.0)), 0.0) for _ in range(nph)]
    else:
        mats = [lame(E=float(rng.uniform(0.5, 20.0)), nu=float(rng.uniform(0.05, 0.4))) for _ in range(nph)]
    method = "cg" if rng.random() < 0.4 else "basic"
    estimators = ["epsilon", "sigma"] + (["energy"] if mode == "elasticity" else []) + (["residual"] if method == "cg" else [])
    estimator = str(rng.choice(estimators))
    opts = {}
    if rng.random() < 0.5:
        opts["u_loop"] = int(rng.integers(0, 3))
    if rng.random() < 0.3:
        opts["fuse_x"] = int(rng.integers(0, 2))
    if rng.random() < 0.3:
        opts["u_tile"] = int(rng.choice([0, 1]))
    if rng.random() < 0.3:
        opts["fuse_stress_div"] = int(rng.integers(0, 2))
    bc = None
    if rng.random() < 0.4:
        bc = "shear_stress" if mode == "viscosity" else str(rng.choice(list(PROJECTORS)))
    steps = [0.0, 0.4, 1.0] if rng.random() < 0.3 else None
    E = rng.uniform(-1.0, 1.0, size=6)
    if mode == "viscosity":
        E[:3] -= E[:3].mean()               # the prescribed fluid stress is traceless
    c = dict(shape=shape, dims=dims, nph=nph, kinds=kinds, sharp=sharp, mode=mode, mats=mats, method=method,
             estimator=estimator, opts=opts, bc=bc, steps=steps, E=E)
    if fields:   # a stream of its own: the combination above does not depend on the images' size
        c["images"] = fine_images(np.random.default_rng(31000 + seed), shape, nph, sharp)
    return c


def oracle_and_load(c):
    """the fine-grid oracle of a draw and its load (E, S0, P, params)"""
    common = dict(tol=1e-7, maxiter=400, error_estimator=c["estimator"])
    _fine, _coarse, ofine = split_input(c["images"], c["kinds"])
    cls = DfgViscosityOracle if c["mode"] == "viscosity" else DfgLSOracle
    o = cls(*c["shape"], *c["dims"], mats=c["mats"], phis=[np.zeros(c["shape"])] * c["nph"], phis_fine=ofine, **common)
    E, S0, P = c["E"].copy(), np.zeros(6), None
    if c["bc"] is not None:
        keep = np.array(SHEAR if c["bc"] == "shear_stress" else PROJECTORS[c["bc"]], dtype=float)
        P = np.diag(keep)
        E = E * (keep > 0)                 # prescribed strain lives in the range of P, the stress (zero) in its complement
        if c["bc"] == "shear_stress":
            o.bc_tol = 1e-8
    return o, E, S0, P, c["steps"] or [0.0, 1.0]


def test_draw_covers_every_path():
    """CPU, no oracle run: what the kept seeds reach.  A thinner seed count must keep all of it."""
    draws = [draw_dfg(seed, fields=False) for seed in range(N_DFG)]
    shapes = [tile_shape(c["shape"]) for c in draws]
    for t in ("<8,1>", "<6,2>", "<8,0> short", "<8,0> exact", "<8,0> two"):
        assert shapes.count(t) >= 2, t
    assert "untiled" in shapes
    assert any(c["shape"][0] % 4 for c, t in zip(draws, shapes) if t != "untiled")   # a march that does not divide nx
    assert {c["estimator"] for c in draws} >= {"epsilon", "sigma", "energy", "residual"}
    assert {(c["mode"], c["method"]) for c in draws} == {(m, k) for m in ("elasticity", "viscosity") for k in ("basic", "cg")}
    assert {c["nph"] for c in draws} == {1, 2, 3}
    assert any(len(set(c["kinds"])) == 2 for c in draws)                             # mixed fine / coarse input
    assert any(set(c["kinds"]) == {"fine"} for c in draws) and any(set(c["kinds"]) == {"coarse"} for c in draws)
    assert any(c["sharp"] and c["nph"] > 1 for c in draws)
    assert any(c["bc"] and c["method"] == "cg" and c["mode"] == "elasticity" and c["nph"] > 1 for c in draws)   # CG with mixed BC
    assert any(c["bc"] and c["mode"] == "viscosity" and c["nph"] > 1 for c in draws)                  # viscosity with mixed BC
    assert any(c["bc"] and t != "untiled" and c["mode"] == "elasticity" and c["method"] == "basic"
               and c["opts"].get("u_loop", 2) == 2 and c["opts"].get("u_tile", 1) == 1 for c, t in zip(draws, shapes))   # SUMT
    assert any(c["steps"] for c in draws)
    assert any(c["opts"].get("u_tile") == 0 and t != "untiled" for c, t in zip(draws, shapes))
    assert any(c["opts"].get("fuse_stress_div") == 0 and t != "untiled" for c, t in zip(draws, shapes))
    assert {c["opts"].get("u_loop") for c in draws} >= {0, 1, 2}
    assert {c["opts"].get("fuse_x") for c in draws} >= {0, 1}
    assert any(c["mode"] == "viscosity" and t in ("<8,1>", "<6,2>") for c, t in zip(draws, shapes))


@gpu
@pytest.mark.parametrize("seed", range(N_DFG))
def test_random_full_staggered_combination_matches_fine_grid_oracle(seed):
    from fibergen_amd import LSSolver
    c = draw_dfg(seed)
    o, E, S0, P, params = oracle_and_load(c)
    fine, coarse, _ofine = split_input(c["images"], c["kinds"])
    s = LSSolver(*c["shape"], *c["dims"])
    s.set_options(mode=c["mode"], gamma_scheme="full_staggered")
    s.set_num_phases(c["nph"])
    for p, (mu, lam) in enumerate(c["mats"]):
        s.set_phase(p, mu, lam, coarse[p])
        if fine[p] is not None:
            s.set_phase_fine(p, fine[p])
    s.set_options(method=c["method"], error_estimator=c["estimator"], tol=1e-7, maxiter=400, **c["opts"])
    if P is not None:
        s.set_bc_projector(P)
        if c["bc"] == "shear_stress":
            s.set_options(bc_tol=1e-8)
    tag = "seed %d: %s" % (seed, {k: c[k] for k in ("shape", "nph", "kinds", "sharp", "mode", "method", "estimator", "opts",
                                                      "bc", "steps")})
    try:
        ref_failed = o.run_load_steps(E, S0, P, params=params, method=c["method"])
    except RuntimeError as e:
        # a combination the reference rejects must be rejected by the product with the same message
        with pytest.raises(RuntimeError) as got:
            s.run_load_steps(E, S0, params=params)
        assert str(e).split(":")[0][:24] in str(got.value), tag
        s.close()
        return
    failed = s.run_load_steps(E, S0, params=params)
    assert failed == ref_failed, tag
    assert s.iterations == o.iterations, tag
    r, rr = np.array(s.residuals), np.array(o.residuals)
    assert r.shape == rr.shape and np.abs(r - rr).max() < 1e-9, tag
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-8, tag
    assert np.abs(s.mean_stress() - o.mean_stress()).max() < 1e-9 * max(1.0, np.abs(o.mean_stress()).max()), tag
    assert rel_err(s.get_field("phi"), np.array(o.phis)) < 1e-15, tag
    s.close()

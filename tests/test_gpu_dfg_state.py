"""gamma_scheme full_staggered: the solver's state across reconfiguration (phis_, mod5_, mod5_dirty_, the fine_set_ mask).
ONE solver object is taken through a sequence of changes; after each step its run equals a FRESHLY built fine-grid oracle
of that configuration (never a second product run), at the bars of _check in test_gpu_dfg.py."""
import numpy as np
import pytest

from dfg_reference import DfgLSOracle, fine_images, replicate, restrict_component
from helpers import INCLUSION, MATRIX, lame, rel_err
from test_gpu_dfg import _check

pytestmark = pytest.mark.gpu

E = np.array([1.0, 0, 0, 0, 0, 0.5])


@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("grid,dims", [((4, 16, 80), (1.0, 1.5, 0.8)), ((12, 10, 6), (2.0, 1.0, 0.5))],
                         ids=["4x16x80-tiled", "12x10x6-untiled"])
def test_one_solver_through_reconfigurations(grid, dims, method):
    """fine images -> phase 1 replaced by a coarse field (set_phase clears the fine_set_ bit: k_dfg_fractions_replica next to
    k_dfg_fractions_fine) -> new moduli for phase 0 (mod5_dirty_ by set_phase_material) -> set_num_phases(3) with new fine
    images (phis_ freed and reallocated, mod5_ kept) -> gamma_scheme staggered (the plain oracle on the coarse "phi") ->
    full_staggered again (the fine fractions are still there)"""
    from fibergen_amd import LSSolver
    from oracle.ls_oracle import LSOracle
    rng = np.random.default_rng(720)
    tol = dict(tol=1e-6)
    cg = method == "cg"
    mats = [lame(**MATRIX), lame(**INCLUSION)]
    img = fine_images(rng, grid, 2)
    s = LSSolver(*grid, *dims)
    s.set_options(gamma_scheme="full_staggered", method=method, **tol)
    s.set_num_phases(2)
    for p in range(2):
        s.set_phase(p, *mats[p])
        s.set_phase_fine(p, img[p])

    def oracle(mats, fine):
        return DfgLSOracle(*grid, *dims, mats=mats, phis=[np.zeros(grid)] * len(mats), phis_fine=fine, **tol)

    _check(s, oracle(mats, img), E, cg=cg)                                   # 1: all fine

    c1 = restrict_component(fine_images(rng, grid, 2)[1], (0, 0, 0))         # 2: phase 1 from another, coarse field
    s.set_phase(1, *mats[1], c1)
    mixed = [img[0], replicate(c1)]
    _check(s, oracle(mats, mixed), E, cg=cg)

    mats = [(2.3, 1.1), mats[1]]                                             # 3: new moduli, fields untouched
    s.set_phase(0, *mats[0])
    _check(s, oracle(mats, mixed), E, cg=cg)

    mats3 = [mats[0], mats[1], (0.9, 1.7)]                                   # 4: three phases, new fine images
    img3 = fine_images(rng, grid, 3)
    s.set_num_phases(3)
    for p in range(3):
        s.set_phase(p, *mats3[p])
        s.set_phase_fine(p, img3[p])
    o3 = oracle(mats3, img3)
    _check(s, o3, E, cg=cg)

    s.set_options(gamma_scheme="staggered")                                  # 5: the staggered scheme on the coarse field
    _check(s, LSOracle(*grid, *dims, mats=mats3, phis=o3.phis, **tol), E, cg=cg)

    s.set_options(gamma_scheme="full_staggered")                             # 6: and back
    _check(s, oracle(mats3, img3), E, cg=cg)
    s.close()


@pytest.mark.parametrize("estimator", ["sigma", "energy"])
@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("grid", [(5, 14, 100), (9, 7, 5)], ids=["5x14x100-tiled", "9x7x5-untiled"])
def test_estimators_and_load_steps(grid, method, estimator):
    """error_estimator sigma (k_dfg_stress<1> after every pass) and energy (k_dfg_stress<2>, reachable through this estimator
    only) under load steps: on the tiled grid with method basic the estimator's ensure_eps materialises the strain inside the
    five-moduli displacement loop at every iteration.  Three phases with pure cells."""
    from fibergen_amd import LSSolver
    rng = np.random.default_rng(721)
    mats = [lame(**MATRIX), lame(**INCLUSION), (0.9, 1.7)]
    img = fine_images(rng, grid, 3)
    kw = dict(tol=1e-7, maxiter=400, error_estimator=estimator)
    s = LSSolver(*grid, 1.0, 1.5, 0.8)
    s.set_options(gamma_scheme="full_staggered", method=method, **kw)
    s.set_num_phases(3)
    for p in range(3):
        s.set_phase(p, *mats[p])
        s.set_phase_fine(p, img[p])
    o = DfgLSOracle(*grid, 1.0, 1.5, 0.8, mats=mats, phis=[np.zeros(grid)] * 3, phis_fine=img, **kw)
    params = [0.0, 0.4, 1.0]
    assert o.run_load_steps(E, params=params, method=method) is False and o.iterations < 400
    assert s.run_load_steps(E, params=params) is False
    assert s.iterations == o.iterations
    np.testing.assert_allclose(s.residuals, o.residuals, rtol=0, atol=1e-11)
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-9
    assert rel_err(s.mean_stress(), o.mean_stress()) < 1e-9
    s.close()

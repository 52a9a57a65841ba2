"""The randomised draw of test_gpu_fuzz.py (grid, cell, phases, mixing rule, method, loop options, mixed boundary conditions,
load steps) with the Green operator forced to willot, against the restatement tests/willot_reference.py: seeds 0 ... 29.
The restatement alone converges for all 30 within maxiter = 400 (at most 85 passes; checked on the CPU), none is left out.

Bars as in test_gpu_fuzz.py: iteration counts equal, residual histories 1e-9, strain fields 1e-8, mean stress 1e-9."""
import numpy as np
import pytest

from helpers import rel_err
from test_gpu_fuzz import PROJECTORS, draw
from willot_reference import WillotLSOracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(30))
def test_random_combination_with_willot_matches_restatement(seed):
    from fibergen_amd import LSSolver
    c = draw(seed)
    shape, dims = c["shape"], c["dims"]
    common = dict(tol=1e-7, maxiter=400)
    o = WillotLSOracle(*shape, *dims, mats=c["mats"], phis=c["phis"], normals=c["normals"], mixing_rule=c["mixing"], **common)
    s = LSSolver(*shape, *dims)
    s.set_num_phases(len(c["mats"]))
    for p, (m, phi) in enumerate(zip(c["mats"], c["phis"])):
        s.set_phase(p, m[0], m[1], phi)
    if c["normals"] is not None:
        s.set_normals(c["normals"])
    s.set_options(mixing_rule=c["mixing"], gamma_scheme="willot", method=c["method"], **common, **c["opts"])
    E, S0, P = c["E"].copy(), np.zeros(6), None
    if c["bc"] is not None:
        keep = np.array(PROJECTORS[c["bc"]], dtype=float)
        P = np.diag(keep)
        E = E * (keep > 0)
        s.set_bc_projector(P)
    params = c["steps"] or [0.0, 1.0]
    tag = "seed %d: %s" % (seed, {k: c[k] for k in ("shape", "mixing", "method", "opts", "bc", "steps")})
    assert o.run_load_steps(E, S0, P, params=params, method=c["method"]) is False, tag
    assert max(o.step_iterations) < common["maxiter"], tag   # converged, not cut off
    assert s.run_load_steps(E, S0, params=params) is False, tag
    assert s.iterations == o.iterations, tag
    r, rr = np.array(s.residuals), np.array(o.residuals)
    assert r.shape == rr.shape and np.abs(r - rr).max() < 1e-9, tag
    assert rel_err(s.get_field("epsilon"), o.eps) < 1e-8, tag
    assert np.abs(s.mean_stress() - o.mean_stress()).max() < 1e-9 * max(1.0, np.abs(o.mean_stress()).max()), tag
    s.close()

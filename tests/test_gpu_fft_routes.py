"""Every transform family of fg_fft_route.h on every axis, on the GPU: per axis the shortest length of each family and both
sides of the thresholds (helpers.fft_route_grids, from tests/golden/fft_routes.txt.gz), thin on the other axes -- the path
counters against the golden table, the forward and the inverse transform against numpy.

Tolerance: the project's 1e-13 relative max-norm for a transform stage, the bar of
tests/test_gpu_bluestein.py::test_fft_forward_inverse for every family."""
import numpy as np
import pytest

from helpers import fft_route_grids, make_gpu_solver, rel_err

pytestmark = pytest.mark.gpu

GRIDS = fft_route_grids()


@pytest.mark.parametrize("grid,axis,family,path", GRIDS, ids=["%s-%s-%s" % ("x".join(map(str, g)), "xyz"[a], f) for g, a, f, _ in GRIDS])
def test_fft_forward_inverse(grid, axis, family, path):
    rng = np.random.default_rng(21)
    s = make_gpu_solver(grid)
    assert s.counter("fft_path_" + "xyz"[axis]) == path
    f = rng.standard_normal((3,) + grid)
    s.set_field("f", f)
    s.run_stage("fft_forward")
    err = rel_err(s.get_field("f_hat"), np.fft.rfftn(f, axes=(1, 2, 3)) / float(np.prod(grid)))
    print("forward", grid, family, err)
    assert err <= 1e-13
    # inverse of an arbitrary (non-Hermitian) spectrum: FFTW c2r semantics
    nzc = grid[2] // 2 + 1
    spec = rng.standard_normal((3,) + grid[:2] + (nzc,)) + 1j * rng.standard_normal((3,) + grid[:2] + (nzc,))
    s.set_field("f_hat", spec)
    s.run_stage("fft_inverse")
    err = rel_err(s.get_field("f"), np.fft.irfftn(spec, s=grid, axes=(1, 2, 3)) * float(np.prod(grid)))
    print("inverse", grid, family, err)
    assert err <= 1e-13
    s.close()


def test_bluestein_switch_moves_only_its_family():
    for grid, axis, family, path in GRIDS:
        if family in ("bluestein", "sub_lds", "tile"):
            s = make_gpu_solver(grid, bluestein=0)
            assert s.counter("fft_path_" + "xyz"[axis]) == (5 if family == "bluestein" else path)
            s.close()

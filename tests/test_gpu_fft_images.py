"""fft_images = 1 (ONE exchange plane in LDS, crossed by the real and then the imaginary parts: Line<N, 1> in the power-of-two
y, x and mirrored z passes) against fft_images = 2 (both planes side by side): the same butterflies in the same order, so every
result is bit-identical -- array_equal, no tolerance.  This is the race check of the one-plane form: the host emulation
(tests/emulate/test_fft_images_emulate.py) cannot see a missing barrier.  plane_fft = 0 keeps small grids on the y and z
kernels under test instead of the plane kernels."""
import numpy as np
import pytest

from helpers import make_gpu_solver

pytestmark = pytest.mark.gpu

GRIDS = [(64, 64, 64),      # short lines, wide tiles (TileCols > 8), M = 32 z lines on the two-plane fall-back
         (128, 256, 64),    # y and x lines of different pass counts
         (256, 128, 128),   # x on the k_strided path when fuse_x = 0; M = 64 mirrored z lines
         (64, 64, 512),     # M = 256 z lines
         (64, 72, 128),     # nzc = 65: the last tile has invalid columns whose threads must reach every barrier
         (128, 64, 80)]     # nzc = 41; nz / 2 = 40 is no power of two: z on another path


def transforms(grid, images, fuse_x):
    rng = np.random.default_rng(5)
    s = make_gpu_solver(grid, fft_images=images, fuse_x=fuse_x, plane_fft=0)
    s.set_field("f", rng.standard_normal((3,) + grid))
    s.run_stage("fft_forward")
    spec = s.get_field("f_hat").copy()
    s.run_stage("fft_inverse")
    back = s.get_field("f").copy()
    s.close()
    return spec, back


def passes(grid, images, fuse_x, mixing):
    s = make_gpu_solver(grid, mixing=mixing, fft_images=images, fuse_x=fuse_x, plane_fft=0)
    s.calc_ref_material()
    s.set_field("epsilon", np.random.default_rng(7).standard_normal((6,) + grid))
    s.iterate(np.array([1.0, 0.0, 0.0, 0.0, 0.0, 0.5]), 3)
    out = s.get_field("epsilon").copy(), s.get_field("sumsq").copy()
    s.close()
    return out


@pytest.mark.parametrize("fuse_x", [0, 1])
@pytest.mark.parametrize("grid", GRIDS)
def test_transforms_bit_identical(grid, fuse_x):
    spec2, back2 = transforms(grid, 2, fuse_x)
    spec1, back1 = transforms(grid, 1, fuse_x)
    assert np.isfinite(spec2).all() and np.isfinite(back2).all()
    assert np.array_equal(spec1, spec2)
    assert np.array_equal(back1, back2)


@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
@pytest.mark.parametrize("fuse_x", [0, 1])
@pytest.mark.parametrize("grid", GRIDS)
def test_iterate_bit_identical(grid, fuse_x, mixing):
    eps2, norm2 = passes(grid, 2, fuse_x, mixing)
    eps1, norm1 = passes(grid, 1, fuse_x, mixing)
    assert np.isfinite(eps2).all()
    assert np.array_equal(eps1, eps2)
    assert np.array_equal(norm1, norm2)


@pytest.mark.parametrize("grid", [(40, 40, 40), (32, 32, 45)])
def test_no_op_on_other_lengths(grid):
    """a decimal grid and an odd nz: the forced option changes nothing and raises nothing"""
    spec2, back2 = transforms(grid, 2, 1)
    spec1, back1 = transforms(grid, 1, 1)
    assert np.array_equal(spec1, spec2)
    assert np.array_equal(back1, back2)

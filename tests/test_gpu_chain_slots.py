"""The timing slots of the transform chain (fg_g0_chain.h, Solver::fft_g0_chain): every variant of the schedule charges exactly
the slots DESIGN.md's table names for it.  bench.py reads the slots by position, so a pass that moves to another slot -- or a
slot that is opened around nothing -- changes what its per-kernel table says without changing any result.

Twenty passes of fg_iterate with stage timing on; slots 2..8 are the chain's (0, 1 and 9 belong to the sweeps around it).  A
slot the variant does not use is never opened and reads exactly 0.0; a slot it uses sums twenty kernel durations, each above the
reading of an empty event pair (on 16 x 8 x 16 the shortest pass, the one-component y transform, still runs about 2 us against
a bias the solver measures and subtracts).  x_layout needs rows of at least 64 points (the complex pitch a multiple of 8), so
that variant runs on 16 x 8 x 64, the smallest grid Fft3::can_xlayout accepts together with the power-of-two passes; the
plane kernels start at 16 lines of 8 complex points (plane_dispatch), so that variant runs on 16 x 16 x 16."""
import numpy as np
import pytest

from helpers import make_gpu_solver, sphere_phi

pytestmark = pytest.mark.gpu

PASSES = 20
CHAIN = ["r2c_z", "c2c_y_fwd", "c2c_x_fwd", "g0", "c2c_x_inv", "c2c_y_inv", "c2r_z"]   # slots 2 .. 8
G16, GPL, G64 = (16, 8, 16), (16, 16, 16), (16, 8, 64)

# variant -> (options, grid, slots of the chain that are charged)
VARIANTS = {
    "plain": (dict(fuse_x=0, plane_fft=0), G16, ["r2c_z", "c2c_y_fwd", "c2c_x_fwd", "g0", "c2c_x_inv", "c2c_y_inv", "c2r_z"]),
    "fused": (dict(fuse_x=1, plane_fft=0), G16, ["r2c_z", "c2c_y_fwd", "g0", "c2c_y_inv", "c2r_z"]),
    "plane": (dict(fuse_x=1, plane_fft=1), GPL, ["r2c_z", "g0", "c2r_z"]),
    # (the plane kernel wins over the chunked pairs, so it is switched off)
    "pair_chunk": (dict(fuse_x=1, plane_fft=0, pair_chunk=4), G16, ["r2c_z", "g0", "c2c_y_inv"]),
    "x_layout": (dict(fuse_x=1, plane_fft=0, x_layout=1), G64, ["r2c_z", "c2c_y_fwd", "g0", "c2c_y_inv", "c2r_z"]),
}


def _heat_solver(grid, **kw):
    from fibergen_amd import LSSolver
    phi = sphere_phi(grid, 0.3)
    s = LSSolver(*grid)
    s.set_options(mode="heat")
    s.set_num_phases(2)
    s.set_phase(0, 1.0, 0.0, 1 - phi)
    s.set_phase(1, 7.0, 0.0, phi)
    s.set_options(**kw)
    return s


@pytest.mark.parametrize("mode,variant", [("elasticity", v) for v in VARIANTS] + [("heat", v) for v in ("plain", "fused", "plane")])
def test_chain_slots(mode, variant):
    opts, grid, named = VARIANTS[variant]
    if mode == "heat":
        s, E = _heat_solver(grid, **opts), np.array([1.0, -0.5, 0.25])
    else:
        s, E = make_gpu_solver(grid, **opts), np.array([1.0, 0, 0, 0, 0, 0.5])
    s.calc_ref_material()
    s.enable_stage_timing(True)
    s.iterate(E, PASSES)
    ms, count = s.stage_times()
    s.close()
    print(mode, variant, grid, {k: ms[k] for k in CHAIN}, count)
    assert count == PASSES
    for k in CHAIN:
        if k in named:
            assert ms[k] > 0.0, (k, ms)
        else:
            assert ms[k] == 0.0, (k, ms)

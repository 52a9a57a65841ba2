"""Bluestein tile kernels on the GPU (fg_fft_bluestein.hip): axes whose length has a prime factor above 13 and at least 64
points (z: nz / 2 for even nz) -- path counters, the transforms against numpy, the loop against the oracles, the option
bluestein = 0 (the O(n^2) sums) as an A/B partner, one slab case.  Grids are thin on the axes a case is not about.

Tolerances: the project's 1e-13 relative max-norm for a transform stage (tests/test_gpu_parity.py::test_fft_forward_inverse),
1e-11 for a loop pass against the NumPy oracle (test_fft_random_grids_with_small_prime_factors)."""
import numpy as np
import pytest

from helpers import make_gpu_solver, make_oracle, rel_err, sphere_phi, two_phase_setup

pytestmark = pytest.mark.gpu

AXES = "xyz"


def paths(s):
    return [s.counter("fft_path_" + a) for a in AXES]


def padded(s):
    return [s.counter("fft_bluestein_m_" + a) for a in AXES]


def test_path_counters_and_option_is_per_solver():
    s = make_gpu_solver((67, 68, 134))
    assert paths(s) == [4, 4, 4]
    m = padded(s)
    assert m[0] >= 2 * 67 - 1 and m[1] >= 2 * 68 - 1 and m[2] >= 2 * 67 - 1   # z: nz / 2 = 67 packed points
    s.close()
    # lines below 64 points keep the kernels they had: 41 and 62 = nz / 2 (2 * 31) the O(n^2) sums -- and 33 = 3 * 11, which is
    # 13-smooth, the tile kernels it has been running on
    s = make_gpu_solver((41, 33, 124))
    assert paths(s) == [5, 3, 5] and padded(s) == [0, 0, 0]
    s.close()
    s = make_gpu_solver((41, 37, 124))   # a prime on y too: all three axes on the O(n^2) sums
    assert paths(s) == [5, 5, 5] and padded(s) == [0, 0, 0]
    s.close()
    s = make_gpu_solver((64, 100, 96))   # power of two, tile kernels, sub-lines 3 * 16
    assert all(p not in (4, 5) for p in paths(s)) and padded(s) == [0, 0, 0]
    s.close()
    off = make_gpu_solver((67, 8, 8), bluestein=0)
    assert off.counter("fft_path_x") == 5 and off.counter("fft_bluestein_m_x") == 0
    on = make_gpu_solver((67, 8, 8))     # created while `off` lives: the switch is the solver's, not the process's
    assert on.counter("fft_path_x") == 4 and on.counter("fft_bluestein_m_x") >= 133
    assert off.counter("fft_path_x") == 5
    off.set_options(bluestein=1)
    assert off.counter("fft_path_x") == 4
    on.close()
    off.close()


@pytest.mark.parametrize("grid,want", [   # want: the path of the axes the case is about
    ((67, 68, 134), {"x": 4, "y": 4, "z": 4}),
    ((127, 8, 254), {"x": 4, "y": 1, "z": 4}),
    ((8, 170, 10), {"x": 1, "y": 4}),     # y pass with nzc = 6 columns: one ragged tile per x plane
    ((340, 6, 67), {"x": 4, "z": 4}),     # odd nz: the rows as nz complex points
    ((6, 10, 211), {"z": 4}),
    ((631, 6, 4), {"x": 4}),              # 4-column tiles
    ((4, 1259, 4), {"y": 4}),             # 2-column tiles
    ((10, 4, 1018), {"z": 4}),            # nz / 2 = 509
    ((2503, 2, 2), {"x": 5}),             # no plan beyond ~2 490 points: the O(n^2) sums, still correct
])
def test_fft_forward_inverse(grid, want):
    rng = np.random.default_rng(12)
    s = make_gpu_solver(grid)
    assert {a: s.counter("fft_path_" + a) for a in want} == want
    f = rng.standard_normal((3,) + grid)
    s.set_field("f", f)
    s.run_stage("fft_forward")
    got = s.get_field("f_hat")
    ref = np.fft.rfftn(f, axes=(1, 2, 3)) / float(np.prod(grid))
    err = rel_err(got, ref)
    print("forward", grid, err)
    assert err <= 1e-13
    # inverse of an arbitrary (non-Hermitian) spectrum: FFTW c2r semantics
    nzc = grid[2] // 2 + 1
    spec = rng.standard_normal((3,) + grid[:2] + (nzc,)) + 1j * rng.standard_normal((3,) + grid[:2] + (nzc,))
    s.set_field("f_hat", spec)
    s.run_stage("fft_inverse")
    got = s.get_field("f")
    ref = np.fft.irfftn(spec, s=grid, axes=(1, 2, 3)) * float(np.prod(grid))
    err = rel_err(got, ref)
    print("inverse", grid, err)
    assert err <= 1e-13
    s.close()


@pytest.mark.parametrize("grid", [(67, 8, 10), (8, 10, 134)])
@pytest.mark.parametrize("mixing", ["voigt", "laminate"])
def test_one_iteration_against_oracle(grid, mixing):
    rng = np.random.default_rng(15)
    s = make_gpu_solver(grid, mixing=mixing)
    assert 4 in paths(s)
    o = make_oracle(grid, mixing=mixing)
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    s.calc_ref_material()
    o.calc_ref_material()
    eps0 = rng.standard_normal((6,) + grid)
    s.set_field("epsilon", eps0)
    s.iterate(E, 1)
    err = rel_err(s.get_field("epsilon"), o.basic_scheme(E, eps0))
    print("iterate", grid, mixing, err)
    assert err <= 1e-11
    s.close()


def test_heat_mode_passes_against_oracle():
    from fibergen_amd import LSSolver
    from oracle.scalar_oracle import ScalarOracle
    grid = (67, 10, 134)
    phi1 = sphere_phi(grid, 0.3)
    mus, phis = [1.0, 12.0], [1 - phi1, phi1]
    s = LSSolver(*grid)
    s.set_options(mode="heat")
    s.set_num_phases(2)
    for p in range(2):
        s.set_phase(p, mus[p], 0.0, phis[p])
    s.set_options(tol=1e-14, maxiter=2)
    assert paths(s) == [4, 3, 4]   # 67 and nz / 2 = 67 on Bluestein, 10 on the tile kernels
    o = ScalarOracle(*grid, mus=mus, phis=phis, tol=1e-14, maxiter=2)
    E = np.array([1.0, -0.5, 0.25])
    s.run(E)
    o.run(E)
    assert s.iterations == o.iterations == 2
    err = rel_err(s.get_field("epsilon"), o.eps)
    print("heat", err)
    assert err <= 1e-11
    s.close()


def test_four_cg_iterations_against_oracle():
    grid = (68, 8, 10)
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    o = make_oracle(grid, tol=1e-14, maxiter=4)
    s = make_gpu_solver(grid, tol=1e-14, maxiter=4, method="cg")
    assert paths(s)[0] == 4
    o.run_cg(E)
    s.run(E)
    assert s.iterations == o.iterations == 4 and len(s.residuals) == len(o.residuals)
    err = np.abs(np.array(s.residuals) - np.array(o.residuals)).max()
    print("cg residual history", err)
    assert err <= 1e-9
    s.close()


def test_bluestein_against_the_quadratic_sums():
    grid = (67, 68, 38)
    rng = np.random.default_rng(16)
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    eps0 = rng.standard_normal((6,) + grid)
    out = {}
    for flag in (1, 0):
        s = make_gpu_solver(grid, bluestein=flag)
        out[flag] = [paths(s)]
        s.calc_ref_material()
        s.set_field("epsilon", eps0)
        s.iterate(E, 3)
        out[flag].append(s.get_field("epsilon"))
        s.close()
    assert out[1][0] == [4, 4, 5] and out[0][0] == [5, 5, 5]
    err = rel_err(out[1][1], out[0][1])
    print("bluestein on / off", err)
    assert err <= 1e-12


def test_two_slabs_equal_the_single_gpu_solver():
    from fibergen_amd.distributed import SlabGroup
    grid = (8, 68, 134)
    E = np.array([1.0, 0, 0, 0, 0, 0.5])
    mats, phis, normals = two_phase_setup(grid, "voigt")
    g = SlabGroup(*grid, nranks=2)
    g.set_num_phases(2)
    for p in range(2):
        g.set_phase(p, mats[p][0], mats[p][1], phis[p])
    g.set_normals(normals)
    g.set_options(mixing_rule="voigt", tol=1e-6)
    s = make_gpu_solver(grid, tol=1e-6)
    assert paths(s) == [1, 4, 4]
    assert s.run(E) is False and g.run(E) is False
    for m in g.members:
        assert [m.counter("fft_path_" + a) for a in AXES] == [1, 4, 4]
    assert g.iterations == s.iterations
    err = rel_err(g.get_field("epsilon"), s.get_field("epsilon"))
    print("slabs", err)
    assert err <= 1e-11
    s.close()
    g.close()

"""The pressure of mode viscosity on the GPU: get_field("p") of the C ABI (k_div_vector, the one-component transform pair,
k_poisson_symbol) against the NumPy restatement tests/pressure_reference.py, oracle-free against the 7-point Laplacian, the
accessor's side effects, its refusals, and the project layer (FG.get_field, the "p" array of the VTK file).

Tolerances.  Parity: 1e-8 relative to max |p|, what tests/test_gpu_viscosity.py asks of "u" against ViscosityOracle.velocity().
Oracle-free: p comes back from two transforms with a relative error of a few 1e-16; applying L_h to it amplifies that by at most
cond(L_h) = 4 sum_a n_a^2/d_a^2 / (2 pi / d_max)^2 -- 465 on the largest grid here, (8, 6, 67) -- so 1e-11 of max |f| leaves more
than a decade over 465 x 5e-16."""
import gzip
import os

import numpy as np
import pytest

import pressure_reference as pr
from helpers import rel_err, sphere_phi

pytestmark = pytest.mark.gpu

E6 = np.array([0.5, -0.5, 0.0, 0.2, 0.0, 1.0])
MUS = [1.0, 0.05, 0.4]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pressure_elasticity_n16.vtk.gz")

# (6, 5, 7): odd nz, no z-Nyquist bin; (16, 16, 16): tiled sweep, plane kernels; (10, 12, 20): smooth tile kernels;
# (8, 6, 67): a prime axis
GRIDS = [((8, 8, 8), (1.0, 1.0, 1.0)), ((12, 10, 6), (2.0, 1.0, 0.5)), ((6, 5, 7), (1.0, 1.0, 1.0)), ((16, 16, 16), (1.0, 1.0, 1.0)),
         ((10, 12, 20), (1.0, 2.0, 0.5)), ((8, 6, 67), (1.0, 1.0, 1.0))]


def phases(grid, nph):
    """a sphere (two phases) or two nested spheres (three), composite voxels at the surfaces"""
    if nph == 2:
        phi = sphere_phi(grid, 0.3)
        return [1.0 - phi, phi]
    core, both = sphere_phi(grid, 0.2), sphere_phi(grid, 0.35)
    return [1.0 - both, both - core, core]


def gpu_solver(grid, dims, phis, **opts):
    from fibergen_amd import LSSolver
    s = LSSolver(*grid, *dims)
    s.set_options(mode="viscosity")
    s.set_num_phases(len(phis))
    for p, phi in enumerate(phis):
        s.set_phase(p, MUS[p], 0.0, phi)
    s.set_options(**opts)
    return s


def oracle(grid, dims, phis, mixing="voigt", **kw):
    from oracle.viscosity_oracle import ViscosityOracle
    from reuss_reference import ReussViscosityOracle
    cls = ReussViscosityOracle if mixing == "reuss" else ViscosityOracle
    return cls(*grid, *dims, mats=[(m, 0.0) for m in MUS[:len(phis)]], phis=phis, **kw)


_PAIRS = {}


def pair_after(grid, dims, nph, mixing, method):
    """(solver, oracle) after three iterations of the method, computed once and shared (the tests read, never write)"""
    key = (grid, dims, nph, mixing, method)
    if key not in _PAIRS:
        phis = phases(grid, nph)
        s = gpu_solver(grid, dims, phis, mixing_rule=mixing, method=method, tol=1e-14, maxiter=3)
        o = oracle(grid, dims, phis, mixing, tol=1e-14, maxiter=3)
        assert s.run(E6) == (o.run_cg(E6) if method == "cg" else o.run(E6))
        assert s.iterations == o.iterations == 3
        _PAIRS[key] = (s, o)
    return _PAIRS[key]


# ---------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("mixing", ["voigt", "reuss"])
@pytest.mark.parametrize("nph", [2, 3])
@pytest.mark.parametrize("grid,dims", GRIDS)
def test_pressure_matches_restatement(grid, dims, nph, mixing, method):
    s, o = pair_after(grid, dims, nph, mixing, method)
    assert s.ref_material[0] == pytest.approx(o.mu_0, rel=1e-14)
    assert s._lib.fg_field_components(s._h, b"p") == 1
    p = s.get_field("p")
    assert p.shape == (1,) + grid and np.isfinite(p).all()
    want = pr.pressure(o)
    e = rel_err(p[0], want)
    print("p", grid, nph, mixing, method, "fft_path_z", s.counter("fft_path_z"), "rel err", e, "max |p|", np.abs(want).max())
    assert np.abs(want).max() > 1e-3
    assert e < 1e-8


def test_prime_axis_pass():
    """(8, 6, 67): which pass served the prime z axis -- 4 = Bluestein, 5 = the O(n^2) sums (67 points: below or above
    fft::kBluesteinMin decides); either way not one of the smooth families the other grids take"""
    s, _ = pair_after((8, 6, 67), (1.0, 1.0, 1.0), 2, "voigt", "basic")
    path = s.counter("fft_path_z")
    print("fft_path_z of nz = 67:", path, "bluestein m:", s.counter("fft_bluestein_m_z"))
    assert path in (4, 5)


def test_full_staggered():
    """gamma_scheme full_staggered on (16, 16, 16): the five-moduli stress stage feeds the accessor as it feeds "u" """
    from dfg_reference import DfgViscosityOracle
    grid = (16, 16, 16)
    f = np.random.default_rng(13).random(tuple(2 * n for n in grid))
    fine = [1.0 - f, f]
    from fibergen_amd import LSSolver
    s = LSSolver(*grid)
    s.set_options(mode="viscosity", gamma_scheme="full_staggered")
    s.set_num_phases(2)
    for p in range(2):
        s.set_phase(p, MUS[p], 0.0, None)
        s.set_phase_fine(p, fine[p])
    s.set_options(tol=1e-14, maxiter=3)
    o = DfgViscosityOracle(*grid, mats=[(m, 0.0) for m in MUS[:2]], phis=[np.zeros(grid)] * 2, phis_fine=fine, tol=1e-14, maxiter=3)
    assert s.run(E6) == o.run(E6) and s.iterations == o.iterations == 3
    want = pr.pressure(o)
    e = rel_err(s.get_field("p")[0], want)
    print("p full_staggered", e, np.abs(want).max())
    assert np.abs(want).max() > 1e-3 and e < 1e-8
    s.close()


# ---------------------------------------------------------------------------------------------- oracle-free
@pytest.mark.parametrize("mixing", ["voigt", "reuss"])
@pytest.mark.parametrize("grid,dims", GRIDS)
def test_laplacian_of_the_pressure_is_its_right_hand_side(grid, dims, mixing):
    """L_h p = SCALE * f in NumPy, f rebuilt from the solver's own strain state, phase fields and mu_0"""
    s, _ = pair_after(grid, dims, 3, mixing, "basic")
    o = oracle(grid, dims, list(s.get_field("phi")), mixing)
    o.mu_0 = s.ref_material[0]
    f = pr.pressure_rhs(o, s.get_field("epsilon"))
    p = s.get_field("p")[0]
    d = np.abs(pr.laplacian7(p, dims) - pr.SCALE * (f - f.mean())).max() / np.abs(f).max()
    print("L p - f", grid, mixing, d, "mean p / max", abs(p.mean()) / np.abs(p).max())
    assert d < 1e-11
    assert abs(p.mean()) < 1e-13 * np.abs(p).max()


# ---------------------------------------------------------------------------------------------- side effects
@pytest.mark.parametrize("grid", [(12, 10, 6), (16, 16, 16), (8, 14, 124)])   # untiled / plane kernels / tiled fused sweep
def test_loop_state_is_untouched(grid):
    """fg_iterate x 2, get_field("p"), fg_iterate x 2 against fg_iterate x 4: the sums of squares behind the residuals, the
    residual history and the strain field bit for bit"""
    phis = phases(grid, 2)
    out = []
    for read in (False, True):
        s = gpu_solver(grid, (1.0, 1.0, 1.0), phis)
        s.calc_ref_material()
        s.iterate(E6, 2)
        sums = [s.get_field("sumsq")]
        if read:
            assert np.isfinite(s.get_field("p")).all()
        s.iterate(E6, 2)
        sums.append(s.get_field("sumsq"))
        out.append((np.array(sums), np.array(s.residuals), s.get_field("epsilon")))
        s.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def test_repeatable():
    s, _ = pair_after((12, 10, 6), (2.0, 1.0, 0.5), 2, "voigt", "cg")
    a = s.get_field("p")
    u = s.get_field("u")
    b = s.get_field("p")
    assert np.array_equal(a, b)
    assert np.array_equal(u, s.get_field("u"))   # the two accessors share their front half and their buffers


# ---------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("mode", ["elasticity", "porous"])
def test_other_modes_refuse(mode):
    from fibergen_amd import LSSolver, _lib
    grid = (8, 8, 8)
    s = LSSolver(*grid)
    s.set_options(mode=mode)
    s.set_num_phases(1)
    s.set_phase(0, 1.0, 0.0 if mode == "porous" else 1.0, np.ones(grid))
    assert s._lib.fg_field_components(s._h, b"p") == 0
    with pytest.raises(RuntimeError, match="field 'p'.*%s" % ("heat / porous" if mode == "porous" else "elasticity")):
        s.get_field("p")
    out = np.full(grid, 7.0)
    assert s._lib.fg_get_field(s._h, b"p", out.ctypes.data_as(_lib.c_double_p)) != 0
    assert "field 'p'" in s._lib.fg_last_error(s._h).decode() and (out == 7.0).all()
    with pytest.raises(RuntimeError, match="Unknown field 'nope'"):
        s.get_field("nope")
    s.close()


def test_pressure_cannot_be_set():
    s, _ = pair_after((8, 8, 8), (1.0, 1.0, 1.0), 2, "voigt", "basic")
    with pytest.raises(RuntimeError, match="field 'p' cannot be set"):
        s.set_field("p", np.zeros((1, 8, 8, 8)))


def test_slab_solver_refuses():
    """two x-slabs of (16, 8, 8) on one GPU (the members a GlobalViewSolver drives, one per rank, here both in this process)"""
    from fibergen_amd.distributed import SlabGroup
    grid = (16, 8, 8)
    phi = sphere_phi(grid, 0.3)
    g = SlabGroup(*grid, nranks=2)
    g.set_options(mode="viscosity")
    g.set_num_phases(2)
    g.set_phase(0, 1.0, 0.0, 1.0 - phi)
    g.set_phase(1, 0.05, 0.0, phi)
    g.set_options(tol=1e-14, maxiter=2)
    g.run(E6)
    assert g.get_field("epsilon").shape == (6,) + grid
    with pytest.raises(RuntimeError, match="field 'p'.*slab-decomposed"):
        g.get_field("p")
    g.close()


# ---------------------------------------------------------------------------------------------- project layer
def project(mode, outfile):
    mats = ('<matrix E="1" nu="0.3" /><inclusion E="10" nu="0.2" />' if mode == "elasticity" else
            '<matrix mu="1" /><inclusion mu="0.05" />')
    load = 'e11="1" e12="0.5"' if mode == "elasticity" else 'e11="0.5" e22="-0.5" e12="1"'
    return """<settings><solver n="16"><mode>%s</mode><tol>1e-8</tol><method>basic</method><materials>%s</materials></solver>
      <actions><select_material name="inclusion" /><place_fiber R="0.3" /><run_load_case %s outfile="%s" /></actions>
    </settings>""" % (mode, mats, load, outfile)


def test_fg_get_field_and_vtk_file(tmp_path):
    from fibergen_amd import FG, vtk
    out = str(tmp_path / "viscosity.vtk")
    fg = FG()
    fg.set_xml(project("viscosity", out))
    assert fg.run() == 0
    p = fg.get_field("p")
    assert p.shape == (1, 16, 16, 16) and np.abs(p).max() > 1e-3
    assert np.array_equal(fg.get_field("p", range_x=[0, 5]), p[:, [0, 5]])
    assert np.array_equal(fg.get_field("p", range_x=[0, 5], range_z=[3], components=[0]), p[:, [0, 5]][:, :, :, [3]])
    raw = open(out, "rb").read()
    assert raw.count(b"SCALARS p float") == 1 and raw.index(b"VECTORS u float") < raw.index(b"SCALARS p float")
    _, fields = vtk.read_legacy(out)
    assert list(fields)[-2:] == ["u", "p"]
    assert np.array_equal(fields["p"], p.astype(">f4").astype(np.float64))


def test_elasticity_file_is_unchanged(tmp_path):
    """the same project in elasticity mode: no "p", the file byte for byte the one the code wrote before the pressure existed
    (tests/golden/pressure_elasticity_n16.vtk.gz)"""
    from fibergen_amd import FG
    out = str(tmp_path / "elasticity.vtk")
    fg = FG()
    fg.set_xml(project("elasticity", out))
    assert fg.run() == 0
    raw = open(out, "rb").read()
    assert b"SCALARS p " not in raw
    assert raw == gzip.open(GOLDEN, "rb").read()
    with pytest.raises(RuntimeError, match="field 'p'.*elasticity"):
        fg.get_field("p")

"""The project layer (FG, XML) under the doubly fine grid schemes: half_staggered, the alias full-staggered, raw / injected
coarse phase data under full_staggered, and three materials with overlapping <place_fiber> groups -- each against the
fine-grid oracle of tests/dfg_reference.py built from the voxelisation the scheme prescribes."""
import numpy as np
import pytest

from dfg_reference import DfgLSOracle
from helpers import rel_err

pytestmark = pytest.mark.gpu

XML = """<settings>
  <solver nx="%d" ny="%d" nz="%d">
    <tol>1e-6</tol>
    <method>%s</method>
    <gamma_scheme>%s</gamma_scheme>
    <materials><matrix E="1" nu="0.3" /><incl E="10" nu="0.2" /></materials>
  </solver>
  <actions>%s<run_load_case e11="1" e22="-0.5" /></actions>
</settings>"""
FIBER = '<select_material name="incl" /><place_fiber R="0.3" />'
E = np.array([1.0, -0.5, 0, 0, 0, 0])


def _run_fg(grid, method, scheme, actions=FIBER, inject=None):
    from fibergen_amd import FG
    fg = FG()
    fg.set_xml(XML % (grid + (method, scheme, actions)))
    for name, phi in (inject or {}).items():
        fg.set_phase_field(name, phi)
    assert fg.run() == 0
    return fg


def _mats(fg):
    return [(m["mu"], m["lambda"]) for m in fg._phase_materials]


def _voxelise(fg, shape, nph=2):
    from fibergen_amd import geometry
    from fibergen_amd.fg import _normalize_phi
    phi, _, _ = geometry.voxelize(fg._fibers, shape, fg._dims, fg._x0, nph, fg._matrix_mat)
    return _normalize_phi(phi)


def _against_oracle(fg, o, method):
    lss = fg._lss
    assert (o.run_cg(E) if method == "cg" else o.run(E)) is False
    assert lss.iterations == o.iterations
    assert rel_err(lss.get_field("phi"), np.array(o.phis)) < 1e-14
    assert rel_err(lss.mean_stress(), o.mean_stress()) < 1e-8
    assert rel_err(lss.get_field("epsilon"), o.eps) < 1e-8


@pytest.mark.parametrize("method", ["basic", "cg"])
@pytest.mark.parametrize("grid", [(12, 10, 8), (4, 16, 80)], ids=["12x10x8-untiled", "4x16x80-tiled"])
def test_fg_half_staggered_is_the_replica_of_the_coarse_voxelisation(grid, method):
    """<gamma_scheme>half_staggered: the geometry is voxelised on the COARSE grid and taken as its piecewise-constant replica
    on the fine one -- equal to LSSolver with gamma_scheme full_staggered fed that coarse field (k_dfg_fractions_replica), and
    to the fine-grid oracle built from it; and not what full_staggered computes from the same geometry"""
    from fibergen_amd import LSSolver
    fg = _run_fg(grid, method, "half_staggered")
    coarse = _voxelise(fg, grid)
    mats = _mats(fg)
    o = DfgLSOracle(*grid, *fg._dims, mats=mats, phis=list(coarse), tol=1e-6)
    _against_oracle(fg, o, method)
    s = LSSolver(*grid, *fg._dims)
    s.set_options(gamma_scheme="full_staggered", method=method, tol=1e-6)
    s.set_num_phases(2)
    for p in range(2):
        s.set_phase(p, *mats[p], coarse[p])
    assert s.run(E) is False
    assert s.iterations == fg._lss.iterations
    assert rel_err(s.get_field("epsilon"), fg._lss.get_field("epsilon")) < 1e-12
    assert rel_err(s.mean_stress(), fg._lss.mean_stress()) < 1e-12
    s.close()
    full = _run_fg(grid, method, "full_staggered")
    assert rel_err(full._lss.mean_stress(), fg._lss.mean_stress()) > 1e-6


@pytest.mark.parametrize("grid", [(12, 10, 8), (4, 16, 80)], ids=["12x10x8-untiled", "4x16x80-tiled"])
def test_fg_full_staggered_alias_with_a_dash(grid):
    """<gamma_scheme>full-staggered (F:15068) is full_staggered: the geometry voxelised on the fine grid"""
    a = _run_fg(grid, "basic", "full-staggered")
    b = _run_fg(grid, "basic", "full_staggered")
    assert a._lss.iterations == b._lss.iterations
    assert rel_err(a._lss.get_field("epsilon"), b._lss.get_field("epsilon")) < 1e-12
    assert rel_err(a._lss.mean_stress(), b._lss.mean_stress()) < 1e-12
    fine = _voxelise(a, tuple(2 * n for n in grid))
    o = DfgLSOracle(*grid, *a._dims, mats=_mats(a), phis=[np.zeros(grid)] * 2, phis_fine=list(fine), tol=1e-6)
    _against_oracle(a, o, "basic")


@pytest.mark.parametrize("grid", [(12, 10, 8), (4, 16, 80)], ids=["12x10x8-untiled", "4x16x80-tiled"])
def test_fg_injected_coarse_phase_under_full_staggered(grid):
    """raw / injected phase data (FG.set_phase_field, the path of read_raw_data: _raw_phase) under full_staggered has no fine
    image: the coarse array is normalised and replicated (initFullStageredRawPhases F:17648-17710)"""
    from fibergen_amd.fg import _normalize_phi
    from test_gpu_fuzz import smooth_field
    phi1 = smooth_field(np.random.default_rng(730), grid)
    fg = _run_fg(grid, "basic", "full_staggered", actions="", inject={"incl": phi1})
    coarse = _normalize_phi(np.stack([np.ones(grid), phi1]))
    o = DfgLSOracle(*grid, *fg._dims, mats=_mats(fg), phis=list(coarse), tol=1e-6)
    _against_oracle(fg, o, "basic")


THREE_XML = """<settings>
  <solver nx="%d" ny="%d" nz="%d">
    <tol>1e-6</tol>
    <method>basic</method>
    <gamma_scheme>full_staggered</gamma_scheme>
    <materials><matrix mu="1" lambda="1.5" /><shell mu="3" lambda="2" /><core mu="8" lambda="4" /></materials>
  </solver>
  <actions>
    <select_material name="shell" /><place_fiber R="0.3" cx="0.4" cy="0.5" cz="0.5" />
    <select_material name="core" /><place_fiber R="0.25" cx="0.65" cy="0.5" cz="0.5" />
    <run_load_case e11="1" e22="-0.5" />
  </actions>
</settings>"""


@pytest.mark.parametrize("grid", [(12, 10, 8), (4, 16, 80)], ids=["12x10x8-untiled", "4x16x80-tiled"])
def test_fg_three_materials_overlapping_fibers_full_staggered(grid):
    """three materials, two <place_fiber> groups that overlap: normalizePhi ("the last material wins") acts on the FINE image;
    "phi" is its restriction, the volume fractions sum to one, the run equals DfgLSOracle on that image"""
    from fibergen_amd import FG
    fg = FG()
    fg.set_xml(THREE_XML % grid)
    assert fg.run() == 0
    fgrid = tuple(2 * n for n in grid)
    raw_image = _voxelise_raw(fg, fgrid)
    assert (raw_image[1] + raw_image[2]).max() > 1.0 + 1e-6        # the two groups do overlap: the normalisation acts
    fine = _voxelise(fg, fgrid, 3)
    assert abs(sum(fg.get_volume_fraction(n) for n in ("matrix", "shell", "core")) - 1.0) < 1e-12
    for p, name in enumerate(("matrix", "shell", "core")):
        assert fg.get_volume_fraction(name) == pytest.approx(fine[p].mean(), rel=1e-12)
    o = DfgLSOracle(*grid, *fg._dims, mats=_mats(fg), phis=[np.zeros(grid)] * 3, phis_fine=list(fine), tol=1e-6)
    _against_oracle(fg, o, "basic")


def _voxelise_raw(fg, shape):
    from fibergen_amd import geometry
    phi, _, _ = geometry.voxelize(fg._fibers, shape, fg._dims, fg._x0, 3, fg._matrix_mat)
    return phi

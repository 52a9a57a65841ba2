"""law="aniso" (heat / porous) at the project layer and at the C boundary, without a GPU: XML parsing of c11 c22 c33 c23 c13 c12
(MatrixLinearAnisotropicMaterialLaw::readSettings F:11097-11105), what is handed to the solver, the refusals, the ABI's
rejections."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from fibergen_amd import materials
from fibergen_amd.fg import FG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fibergen_amd.h")

XML = """
<settings>
  <variables><c type="float" value="3" /></variables>
  <solver n="8">
    <mode>%s</mode>
    <method>basic</method>
    <materials>
      <matrix mu="2" />
      <fiber law="aniso" %s />
    </materials>
  </solver>
  <actions><select_material name="fiber" /><place_fiber R="0.3" /></actions>
</settings>
"""


class FakeSolver:
    """records what init_lss hands to the solver"""
    made = []

    def __init__(self, *a, **k):
        self.calls = []
        FakeSolver.made.append(self)

    def set_num_phases(self, n):
        self.calls.append(("n", n))

    def set_phase(self, p, mu, lam, phi=None):
        self.calls.append(("iso", p, mu, lam))

    def set_phase_stiffness(self, p, C):
        self.calls.append(("general", p, np.array(C, dtype=float)))

    def set_phase_conductivity(self, p, K, phi=None):
        self.calls.append(("aniso", p, np.array(K, dtype=float)))

    def set_options(self, **kw):
        self.calls.append(("opts", kw))

    def set_convergence_callback(self, fn):
        pass


@pytest.fixture
def fake(monkeypatch):
    import fibergen_amd.fg as fgmod
    FakeSolver.made = []
    monkeypatch.setattr(fgmod, "LSSolver", FakeSolver)
    return FakeSolver


def conductivity_of(attrs, fake, mode="heat"):
    fg = FG()
    fg.set_xml(XML % (mode, attrs))
    fg._init_python()
    fg.init_lss()
    calls = fake.made[-1].calls
    an = [c for c in calls if c[0] == "aniso"]
    assert len(an) == 1 and an[0][1] == 1
    # the library takes a conductivity in heat / porous mode only: the mode is set before the phase
    first_mode = min(i for i, c in enumerate(calls) if c[0] == "opts" and "mode" in c[1])
    assert calls[first_mode][1]["mode"] == mode and first_mode < calls.index(an[0])
    assert [c for c in calls if c[0] == "iso" and c[1] == 0][0][2:] == (2.0, 0.0)   # the matrix stays isotropic
    return an[0][2]


@pytest.mark.parametrize("mode", ["heat", "porous"])
def test_aniso_is_a_law_of_the_scalar_modes(fake, mode):
    """before the feature: Unknown material law 'aniso'"""
    K = conductivity_of('c11="3" c12="0.5"', fake, mode)
    assert list(K) == [3, 1, 1, 0, 0, 0.5]


def test_defaults_are_the_identity(fake):
    assert list(conductivity_of("", fake)) == [1, 1, 1, 0, 0, 0]
    assert materials.aniso_conductivity({}) == [1, 1, 1, 0, 0, 0]


def test_order_is_11_22_33_23_13_12(fake):
    K = conductivity_of('c11="1.5" c22="2.5" c33="3.5" c23="0.23" c13="0.13" c12="0.12"', fake)
    assert list(K) == [1.5, 2.5, 3.5, 0.23, 0.13, 0.12]


def test_symmetric_storage_reads_the_upper_names_only(fake):
    """six constants of a symmetric matrix: readSettings F:11097-11105 knows c23, c13, c12 and not their mirror names"""
    K = conductivity_of('c12="0.4" c21="7" c32="9" c31="8"', fake)
    assert list(K) == [1, 1, 1, 0, 0, 0.4]
    from fibergen_amd.solver import conductivity6
    M = np.array([[1.5, 0.12, 0.13], [0.12, 2.5, 0.23], [0.13, 0.23, 3.5]])
    assert list(conductivity6(M)) == [1.5, 2.5, 3.5, 0.23, 0.13, 0.12]
    assert list(conductivity6([1.5, 2.5, 3.5, 0.23, 0.13, 0.12])) == [1.5, 2.5, 3.5, 0.23, 0.13, 0.12]
    with pytest.raises(ValueError, match="symmetric"):
        conductivity6(M + np.triu(np.ones((3, 3)), 1))
    with pytest.raises(ValueError, match="six numbers"):
        conductivity6(np.eye(4))


def test_values_are_expressions(fake):
    K = conductivity_of('c11="2*c+1" c23="c/2" c33="math.sqrt(16)"', fake)
    assert list(K) == [7, 1, 4, 1.5, 0, 0]


@pytest.mark.parametrize("mode", ["elasticity", "viscosity"])
def test_aniso_outside_the_scalar_modes_still_raises(fake, mode):
    fg = FG()
    xml = XML % (mode, 'c11="3"')
    if mode == "elasticity":   # (a complete elastic matrix, so that the fibre's law is what fails)
        xml = xml.replace('<matrix mu="2" />', '<matrix E="1" nu="0.3" />')
    fg.set_xml(xml)
    with pytest.raises(RuntimeError, match="Unknown material law 'aniso'"):
        fg.init_lss()


def test_other_laws_still_raise_in_heat_mode(fake):
    for law in ("tiso", "Aniso", "matrix"):
        fg = FG()
        fg.set_xml((XML % ("heat", "")).replace('law="aniso"', 'law="%s"' % law))
        with pytest.raises(RuntimeError, match="Unknown material law '%s'" % law):
            fg.init_lss()


def test_refused_on_slabs(fake):
    fg = FG()
    fg.set_xml(XML % ("heat", 'c11="3"'))
    fg._slabs = True
    with pytest.raises(RuntimeError, match=re.escape(materials.ANISO_SLAB_ERROR)):
        fg.init_lss()
    assert not fake.made, "refused before a solver is created"
    from fibergen_amd.distributed import GlobalViewSolver, SlabGroup
    with pytest.raises(RuntimeError, match=re.escape(materials.ANISO_SLAB_ERROR)):
        GlobalViewSolver.set_phase_conductivity(object.__new__(GlobalViewSolver), 0, np.ones(6))
    with pytest.raises(RuntimeError, match=re.escape(materials.ANISO_SLAB_ERROR)):
        SlabGroup.set_phase_conductivity(object.__new__(SlabGroup), 0, np.ones(6))


def test_messages_are_the_library_s():
    # the solver's setter and the slab driver's check_members raise the one constant of fg_sweep_plan.h
    src = open(os.path.join(ROOT, "fibergen_amd", "csrc", "fg_sweep_plan.h")).read()
    src = re.sub(r'"\s*\n\s*"', "", src)
    assert 'kAnisoSlab = "%s"' % materials.ANISO_SLAB_ERROR in src
    assert "plan::kAnisoSlab" in open(os.path.join(ROOT, "fibergen_amd", "csrc", "fg_solver.hip")).read()
    slab = open(os.path.join(ROOT, "fibergen_amd", "csrc", "fg_slab.hip")).read()
    assert "require_plan(plan::Entry::Slab)" in slab


# ---- the C boundary
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fibergen_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    from fibergen_amd import _lib
    return _lib.load()


def test_declared_and_bound(lib):
    from fibergen_amd import LSSolver, _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+fg_set_phase_conductivity\s*\(([^)]*)\)", text)
    assert m, "fg_set_phase_conductivity is not declared in the header"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 3 and params[0].startswith("fg_solver*") and params[2].startswith("const double*")
    assert "F:11089-11156" in open(HEADER).read()
    res, args = _lib.SIGNATURES["fg_set_phase_conductivity"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, _lib.c_double_p]
    assert hasattr(lib, "fg_set_phase_conductivity") and callable(LSSolver.set_phase_conductivity)
    assert lib.fg_abi_version() == 1


def test_fails_loudly_without_a_solver(lib):
    """a NULL handle gives FG_ERROR, never a crash; the rejections that need a solver run in tests/test_gpu_aniso.py"""
    from fibergen_amd import _lib
    fg_error = int(re.search(r"#define\s+FG_ERROR\s+\(?(-?\d+)", open(HEADER).read()).group(1))
    c6 = np.ones(6)
    assert lib.fg_set_phase_conductivity(None, 0, c6.ctypes.data_as(_lib.c_double_p)) == fg_error
    assert lib.fg_set_phase_conductivity(None, -1, None) == fg_error

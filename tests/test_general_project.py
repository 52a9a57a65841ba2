"""law="general" at the project layer and at the C boundary, without a GPU: XML parsing of c11 ... c66 (read_matrix F:1101-1119
on Voigt::Id4(6) F:501-512), what is handed to the solver, every refusal, and the ABI's rejections."""
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
    <method>basic</method>
    <materials>
      <matrix E="1" nu="0.3" />
      <fiber law="general" %s />
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


def stiffness_of(attrs, fake, **settings):
    fg = FG()
    fg.set_xml(XML % attrs)
    for k, v in settings.items():
        fg.set("solver." + k, v)
    fg._init_python()
    fg.init_lss()
    calls = fake.made[-1].calls
    gen = [c for c in calls if c[0] == "general"]
    assert len(gen) == 1 and gen[0][1] == 1
    # the general phase's stiffness arrives after its (placeholder) isotropic call, the matrix stays isotropic
    order = [c[0] for c in calls if c[0] in ("iso", "general") and c[1] == 1]
    assert order == ["iso", "general"]
    assert [c for c in calls if c[0] == "iso" and c[1] == 0][0][2] == pytest.approx(1 / 2.6)
    return gen[0][2]


def test_defaults_are_id4_not_the_identity(fake):
    C = stiffness_of("", fake)
    assert np.array_equal(C, np.diag([1, 1, 1, 0.5, 0.5, 0.5]))
    assert materials.general_stiffness({}) == np.diag([1, 1, 1, 0.5, 0.5, 0.5]).tolist()


def test_symmetric_fill_and_later_attribute_wins(fake):
    C = stiffness_of('c11="10" c12="4" c16="0.5" c44="2" c53="-1"', fake)
    assert C[0, 0] == 10 and C[0, 1] == C[1, 0] == 4 and C[0, 5] == C[5, 0] == 0.5 and C[3, 3] == 2
    assert C[4, 2] == C[2, 4] == -1 and C[1, 1] == 1 and C[4, 4] == 0.5
    # c12 and c21 both given: the loop runs i, j row-major, (2, 1) comes after (1, 2) and sets both entries -- whatever the
    # order of the attributes in the file
    for attrs in ('c12="4" c21="7"', 'c21="7" c12="4"'):
        C = stiffness_of(attrs, fake)
        assert C[0, 1] == C[1, 0] == 7
    C = stiffness_of('c36="1" c63="2" c45="3" c54="5"', fake)
    assert C[2, 5] == C[5, 2] == 2 and C[3, 4] == C[4, 3] == 5


def test_values_are_expressions(fake):
    C = stiffness_of('c11="2*c+1" c23="c/2" c66="math.sqrt(16)"', fake)
    assert C[0, 0] == 7 and C[1, 2] == C[2, 1] == 1.5 and C[5, 5] == 4


def test_other_laws_still_raise(fake):
    for law in ("tiso", "neohooke", "General"):
        fg = FG()
        fg.set_xml((XML % "").replace('law="general"', 'law="%s"' % law))
        with pytest.raises(RuntimeError, match="Unknown material law '%s'" % law):
            fg.init_lss()


@pytest.mark.parametrize("settings,message", [
    ({"mode": "heat"}, materials.GENERAL_MODE_ERROR),
    ({"mode": "porous"}, materials.GENERAL_MODE_ERROR),
    ({"mode": "viscosity"}, materials.GENERAL_MODE_ERROR),
    ({"mixing_rule": "laminate"}, materials.GENERAL_MIXING_ERROR),
    ({"gamma_scheme": "full_staggered"}, materials.GENERAL_DFG_ERROR),
    ({"gamma_scheme": "half_staggered"}, materials.GENERAL_DFG_ERROR),
])
def test_refusals_of_the_project_layer(fake, settings, message):
    fg = FG()
    fg.set_xml(XML % 'c11="3"')
    for k, v in settings.items():
        fg.set("solver." + k, v)
    with pytest.raises(RuntimeError, match=re.escape(message)):
        fg.init_lss()
    assert not fake.made, "refused before a solver is created"


def test_refused_on_slabs(fake):
    fg = FG()
    fg.set_xml(XML % 'c11="3"')
    fg._slabs = True
    with pytest.raises(RuntimeError, match=re.escape(materials.GENERAL_SLAB_ERROR)):
        fg.init_lss()
    from fibergen_amd.distributed import SlabGroup
    with pytest.raises(RuntimeError, match=re.escape(materials.GENERAL_SLAB_ERROR)):
        SlabGroup.set_phase_stiffness(object.__new__(SlabGroup), 0, np.eye(6))


def test_messages_are_the_library_s():
    """the project layer raises in the wording of the solver library (law_refusal in fg_sweep_plan.h)"""
    src = open(os.path.join(ROOT, "fibergen_amd", "csrc", "fg_sweep_plan.h")).read()
    src = re.sub(r'"\s*\n\s*"', "", src)
    for msg in (materials.GENERAL_MODE_ERROR, materials.GENERAL_MIXING_ERROR, materials.GENERAL_DFG_ERROR,
                materials.GENERAL_SLAB_ERROR):
        assert '"%s"' % msg in src, msg


# ---- the C boundary
@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fibergen_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    from fibergen_amd import _lib
    return _lib.load()


def test_declared_and_bound(lib):
    from fibergen_amd import LSSolver, _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+fg_set_phase_stiffness\s*\(([^)]*)\)", text)
    assert m, "fg_set_phase_stiffness is not declared in the header"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 3 and params[0].startswith("fg_solver*") and params[2].startswith("const double*")
    assert "F:11233" in open(HEADER).read()
    res, args = _lib.SIGNATURES["fg_set_phase_stiffness"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int, _lib.c_double_p]
    assert hasattr(lib, "fg_set_phase_stiffness") and callable(LSSolver.set_phase_stiffness)


def test_fails_loudly_without_a_solver(lib):
    """a NULL handle gives FG_ERROR, never a crash.  The library cannot create a solver without a device, so the rejections
    that need one -- an asymmetric C, p out of range -- run in tests/test_gpu_general.py."""
    from fibergen_amd import _lib
    fg_error = int(re.search(r"#define\s+FG_ERROR\s+\(?(-?\d+)", open(HEADER).read()).group(1))
    C = np.eye(6)
    assert lib.fg_set_phase_stiffness(None, 0, C.ctypes.data_as(_lib.c_double_p)) == fg_error
    assert lib.fg_set_phase_stiffness(None, -1, None) == fg_error
    from fibergen_amd import LSSolver
    with pytest.raises(ValueError, match="6x6"):
        LSSolver.set_phase_stiffness(object.__new__(LSSolver), 0, np.eye(5))

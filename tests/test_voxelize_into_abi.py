"""CPU checks of fg_voxelize_into at the boundary: declared in the header, bound in _lib.py, and failing loudly (never
crashing, never falling back) where no solver can exist."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fibergen_amd.h")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "fibergen_amd", "csrc"), "-j4"], stdout=subprocess.DEVNULL)
    from fibergen_amd import _lib
    return _lib.load()


def test_declared_and_bound(lib):
    from fibergen_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+fg_voxelize_into\s*\(([^)]*)\)", text)
    assert m, "fg_voxelize_into is not declared in the header"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9 and params[0].startswith("fg_solver*") and params[1].startswith("const fg_fiber*")
    res, args = _lib.SIGNATURES["fg_voxelize_into"]
    assert res is ctypes.c_int and len(args) == 9
    assert args[1] == ctypes.POINTER(_lib.FgFiber) and args[3] == _lib.c_double_p and args[6] is ctypes.c_double
    assert hasattr(lib, "fg_voxelize_into")


def test_flags_defined():
    from fibergen_amd import _lib
    text = open(HEADER).read()
    flags = dict(re.findall(r"#define\s+(FG_VOX_[A-Z]+)\s+(\d+)", text))
    assert flags == {"FG_VOX_NORMALS": "1", "FG_VOX_FINE": "2"}
    assert (_lib.FG_VOX_NORMALS, _lib.FG_VOX_FINE) == (1, 2)


def test_python_surface():
    from fibergen_amd import FG, LSSolver
    assert callable(LSSolver.voxelize_into)
    assert FG.device_geometry is True


def test_fails_loudly_without_a_solver(lib):
    """The entry needs a solver, and a solver needs a GPU.  A NULL handle gives FG_ERROR (not a crash, whatever else is
    passed), and where no GPU is present no handle can be made: the wrapper's call chain ends in the library's message.
    Only the NULL-handle calls reach fg_voxelize_into itself; without a GPU LSSolver's constructor already raises, so that
    leg checks the Python wrapper chain (LSSolver(...).voxelize_into), not the entry."""
    from fibergen_amd import _lib
    fib = (_lib.FgFiber * 1)()
    x0 = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    fg_error = int(re.search(r"#define\s+FG_ERROR\s+\(?(-?\d+)", open(HEADER).read()).group(1))
    for fibers, n, origin in ((fib, 1, ctypes.cast(x0, _lib.c_double_p)), (None, 0, None)):
        assert lib.fg_voxelize_into(None, fibers, n, origin, 0, -1, 1e-3, _lib.FG_VOX_NORMALS | _lib.FG_VOX_FINE, None) == fg_error
    import torch
    if not torch.cuda.is_available():
        from fibergen_amd import LSSolver

        def voxelise():
            LSSolver(4, 4, 4).voxelize_into([], (0, 0, 0), 0)
        # (a machine without any device: the runtime's own "no ROCm-capable device"; one whose devices are hidden: the
        # library's "needs an AMD GPU" -- the same pattern as test_cabi.py::test_fails_loudly_without_gpu)
        with pytest.raises(RuntimeError, match="HIP|device|GPU"):
            voxelise()

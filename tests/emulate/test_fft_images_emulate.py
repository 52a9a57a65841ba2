"""Host emulation of the strided pass on ONE exchange plane (Line<N, 1>: the real parts cross the plane, then the imaginary
parts) against numpy.fft, at the tolerance of tests/test_fft_emulation.py, and bit for bit against the two-plane form.  CPU
only: checks the indexing and the phase order; a missing barrier is invisible here (tests/test_gpu_fft_images.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import emulation_build_flags  # noqa: E402

dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_images") / "emu_fft_images.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, os.path.join(ROOT, "tests", "emulate", "emu_fft_images.cpp")])
    return ctypes.CDLL(out)


def run(emu, x, N, d, images):
    y = x.copy()
    lds = ctypes.c_int(0)
    nouter, _, ncols = x.shape
    assert emu.emu_strided_images(N, d, y.view(np.float64).ctypes.data_as(dp), ncols, nouter, ctypes.c_double(0.5), images,
                                  ctypes.byref(lds)) == 0
    return y, lds.value


@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024])
@pytest.mark.parametrize("d", [-1, 1])
def test_strided_one_plane(emu, N, d):
    rng = np.random.default_rng(N)
    ncols, nouter = 11, 2  # ragged last tile
    x = rng.standard_normal((nouter, N, ncols)) + 1j * rng.standard_normal((nouter, N, ncols))
    y1, lds1 = run(emu, x, N, d, 1)
    ref = (np.fft.fft(x, axis=1) if d < 0 else np.fft.ifft(x, axis=1) * N) * 0.5
    assert np.abs(y1 - ref).max() / np.abs(ref).max() < 1e-14
    y2, lds2 = run(emu, x, N, d, 2)
    assert np.array_equal(y1.view(np.float64), y2.view(np.float64))
    assert 2 * lds1 == lds2

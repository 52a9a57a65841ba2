"""Bluestein tile kernels (fg_fft_bluestein.h) on the host: the planner, and the kernels' per-thread phase code run thread by
thread (tests/emulate/emu_bluestein.cpp) against numpy.fft.  CPU only.

Tolerance: the project's 1e-13 relative max-norm for transforms.  The algorithm itself (chirp with the index reduced mod 2n,
long double tables, two M-point transforms) gives <= 1.5e-15 in numpy for n up to 2018, so 1e-13 leaves two decades."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emulate")
dp = ctypes.POINTER(ctypes.c_double)
TOL = 1e-13


def P(a):
    return a.ctypes.data_as(dp)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_bluestein") / "emu_bluestein.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, os.path.join(EMU_DIR, "emu_bluestein.cpp")])
    lib = ctypes.CDLL(out)
    lib.emu_bluestein_lds_max.restype = ctypes.c_long
    return lib


def largest_prime_factor(n):
    f, p = 1, 2
    while p * p <= n:
        while n % p == 0:
            f, n = p, n // p
        p += 1
    return max(f, n) if n > 1 else f


def plan(emu, kind, n):
    out = (ctypes.c_long * 5)()
    if emu.emu_bluestein_plan(kind, n, out) != 0:
        return None
    return dict(M=out[0], lines=out[1], threads=out[2], npass=out[3], lds=out[4])


@pytest.mark.parametrize("kind", [0, 1])
def test_planner(emu, kind):
    lds_max = emu.emu_bluestein_lds_max()
    assert emu.emu_bluestein_min() == 64
    nplans = 0
    for n in range(64, 2401):
        if largest_prime_factor(n) <= 13:
            continue
        p = plan(emu, kind, n)
        if p is None:
            continue
        nplans += 1
        assert p["M"] >= 2 * n - 1, (n, p)
        assert largest_prime_factor(p["M"]) <= 13, (n, p)
        assert p["lds"] <= lds_max, (n, p)
        assert p["lines"] >= (2 if kind == 0 else 1), (n, p)
    assert nplans > 1000   # (every such length up to 2400 is expected to have a plan; the exact count is the planner's)
    for n in (11, 33, 41, 62, 63):
        assert plan(emu, kind, n) is None


def test_planner_examples_and_fallback(emu):
    # the padded lengths of some sizes users meet: the smallest 13-smooth M >= 2 n - 1 where the tile planner has a plan for it
    for n, M in ((67, 135), (127, 256), (170, 343), (340, 686), (1009, 2025)):
        assert plan(emu, 0, n)["M"] == M
    # tile widths follow the LDS limit (16 bytes per point)
    assert plan(emu, 0, 631)["lines"] == 4
    assert plan(emu, 0, 1259)["lines"] == 2
    # beyond ~2490 points a strided line pair no longer fits: the O(n^2) kernels keep such axes
    assert plan(emu, 0, 2503) is None
    assert any(plan(emu, 0, n) is None for n in range(2491, 2600))


@pytest.mark.parametrize("n", [67, 68, 127, 170, 631, 1259])
@pytest.mark.parametrize("d", [-1, 1])
def test_strided(emu, n, d):
    rng = np.random.default_rng(n)
    ncols, nouter = (11 if n < 600 else 5), 2   # ragged last tile (8-, 4- and 2-column tiles), two outer blocks
    x = rng.standard_normal((nouter, n, ncols)) + 1j * rng.standard_normal((nouter, n, ncols))
    y = x.copy()
    assert emu.emu_bluestein_strided(n, d, P(y.view(np.float64)), ncols, nouter, ctypes.c_double(0.37)) == 0
    ref = (np.fft.fft(x, axis=1) if d < 0 else np.fft.ifft(x, axis=1) * n) * 0.37
    err = np.abs(y - ref).max() / np.abs(ref).max()
    print("strided n=%d dir=%+d: %.3g" % (n, d, err))
    assert err <= TOL


@pytest.mark.parametrize("nz", [134, 136, 254, 340, 67, 127, 211])
def test_z(emu, nz):
    rng = np.random.default_rng(nz)
    nzc = nz // 2 + 1
    nrows = 2 * plan(emu, 1, nz if nz % 2 else nz // 2)["lines"] - 3   # two tiles, the second ragged
    assert nrows >= 1
    x = rng.standard_normal((nrows, nz))
    buf = np.full((nrows, 2 * nzc), np.nan)
    buf[:, :nz] = x
    assert emu.emu_bluestein_z(nz, 1, P(buf), ctypes.c_long(nrows)) == 0
    ref = np.fft.rfft(x, axis=1)
    err = np.abs(buf.view(np.complex128) - ref).max() / np.abs(ref).max()
    print("r2c nz=%d: %.3g" % (nz, err))
    assert err <= TOL
    # non-Hermitian input: imaginary parts of DC / Nyquist must be ignored like FFTW's c2r
    X = rng.standard_normal((nrows, nzc)) + 1j * rng.standard_normal((nrows, nzc))
    buf = X.copy().view(np.float64).copy()
    assert emu.emu_bluestein_z(nz, 0, P(buf), ctypes.c_long(nrows)) == 0
    ref = np.fft.irfft(X, n=nz, axis=1) * nz
    err = np.abs(buf[:, :nz] - ref).max() / np.abs(ref).max()
    print("c2r nz=%d: %.3g" % (nz, err))
    assert err <= TOL


def test_sanitized_standalone(tmp_path):
    """The same emulation code as a stand-alone program built with AddressSanitizer + UBSan (lengths 67, nz = 136, odd
    nz = 127): clean exit, results checked against direct sums inside the program.  The program links its
    sanitizer runtime itself."""
    exe = str(tmp_path / "bluestein_main")
    sanitize = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    flags = sanitize + [f for f in emulation_build_flags() if f not in ["-shared", "-fPIC", "-O2"] + sanitize]
    subprocess.check_call(["g++"] + flags + ["-o", exe, os.path.join(EMU_DIR, "bluestein_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr

"""law="general" on the host: the per-voxel arithmetic of fg_stage_math.h (general6, pk1_voigt with mixed isotropic / general
phases, the Jacobi eigenvalue routine of the reference-material scan) against the NumPy restatement (general_reference.py),
and the restatement against the isotropic oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import general_reference as gr
from helpers import emulation_build_flags, make_oracle, two_phase_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emulate", "emu_general.cpp")
NCASE = 200


def make_cases():
    """200 seeded cases of three phases; every second stiffness couples normal and shear components"""
    rng = np.random.default_rng(20241)
    cases = []
    for i in range(NCASE):
        law = np.array([1.0, float(i % 3 != 0), 0.0])           # phase 0 general, phase 1 mostly, phase 2 isotropic
        mu = rng.uniform(0.5, 5.0, 3)
        lam = rng.uniform(0.1, 4.0, 3)
        C = np.stack([gr.random_spd(rng, coupling=(i % 2 == 0), scale=10.0 ** rng.integers(-2, 3)) for _ in range(3)])
        phi = rng.dirichlet(np.ones(3))
        if i % 5 == 0:
            phi = np.array([phi[0] + phi[1], 0.0, phi[2]])     # a phase below the Voigt threshold is skipped
        if i % 7 == 0:
            phi = np.array([0.0, 0.0, 1.0]) if i % 14 else np.array([1.0, 0.0, 0.0])
        F = rng.standard_normal(6)
        cases.append((law, mu, lam, C, phi, F))
    return cases


def pack(cases):
    return np.concatenate([np.concatenate([law, mu, lam, C.ravel(), phi, F]) for law, mu, lam, C, phi, F in cases])


def expected(cases):
    out = np.empty((len(cases), 14))
    for k, (law, mu, lam, C, phi, F) in enumerate(cases):
        mats = [C[p] if law[p] else (mu[p], lam[p]) for p in range(3)]
        phis = [np.full((1, 1, 1), phi[p]) for p in range(3)]
        eps = F.reshape(6, 1, 1, 1)
        out[k, :6] = gr.general6(eps, C[0]).ravel()
        out[k, 6:12] = gr.pk1_voigt_general(eps, phis, mats).ravel()
        w = np.linalg.eigvalsh(gr.voigt_tangent_matrices(phis, mats)[0, 0, 0])
        out[k, 12], out[k, 13] = w[0], w[-1]
    return out


def check(out, cases):
    exp = expected(cases)
    for k in range(len(cases)):
        for sl in (slice(0, 6), slice(6, 12)):
            scale = np.abs(exp[k, sl]).max()
            assert np.abs(out[k, sl] - exp[k, sl]).max() <= 1e-14 * scale, (k, out[k, sl], exp[k, sl])
        big = max(abs(exp[k, 12]), abs(exp[k, 13]))
        assert abs(out[k, 12] - exp[k, 12]) <= 1e-13 * big and abs(out[k, 13] - exp[k, 13]) <= 1e-13 * big, (k, out[k, 12:], exp[k, 12:])


@pytest.fixture(scope="module")
def cases():
    return make_cases()


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "emu_general.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, SRC])
    lib = ctypes.CDLL(out)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_general_batch.restype = None
    lib.emu_general_batch.argtypes = [ctypes.c_long, dp, dp]
    lib.emu_jacobi_minmax6.restype = None
    lib.emu_jacobi_minmax6.argtypes = [dp, dp, dp]
    return lib


def test_stress_and_scan_against_restatement(emu, cases):
    dp = ctypes.POINTER(ctypes.c_double)
    data = np.ascontiguousarray(pack(cases))
    out = np.zeros((len(cases), 14))
    emu.emu_general_batch(len(cases), data.ctypes.data_as(dp), out.ctypes.data_as(dp))
    check(out, cases)


def test_jacobi_against_eigvalsh(emu):
    dp = ctypes.POINTER(ctypes.c_double)
    rng = np.random.default_rng(7)
    mats = [gr.scan_matrix(gr.random_spd(rng, coupling=bool(i % 2), scale=10.0 ** rng.integers(-3, 4))) for i in range(200)]
    mats += [np.diag([3.0, 1.0, 2.0, 2.0, 5.0, 4.0]), np.zeros((6, 6)), np.ones((6, 6)), gr.scan_matrix(gr.iso_stiffness(1.2, 0.7)),
             -gr.random_spd(rng)]   # already diagonal, zero, rank one, degenerate (isotropic), negative definite
    for A in mats:
        A = np.ascontiguousarray(A)
        lo, hi = ctypes.c_double(), ctypes.c_double()
        emu.emu_jacobi_minmax6(A.ctypes.data_as(dp), ctypes.byref(lo), ctypes.byref(hi))
        w = np.linalg.eigvalsh(A)
        big = np.abs(w).max()
        assert abs(lo.value - w[0]) <= 1e-13 * big and abs(hi.value - w[-1]) <= 1e-13 * big, (A, lo.value, hi.value, w)


def test_standalone_program_under_sanitizers(tmp_path, cases):
    """the same code as a program of its own, built with AddressSanitizer + UBSan linked statically, so that it runs in the
    inherited environment whatever else is loaded first (no Python loading involved)"""
    exe = str(tmp_path / "emu_general")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DFG_HOST_EMULATION", "-DEMU_GENERAL_MAIN", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-o", exe, SRC])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    pack(cases).tofile(fin)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-2000:])
    check(np.fromfile(fout).reshape(len(cases), 14), cases)


# ---- the restatement itself: phases given as C(mu, lambda) reproduce the isotropic oracle
@pytest.mark.parametrize("grid", [(8, 8, 8), (12, 10, 6)])
def test_isotropic_equivalence_in_the_restatement(grid):
    mats, phis, normals = two_phase_setup(grid)
    iso = make_oracle(grid, tol=1e-6)
    gen = gr.GeneralLSOracle(*grid, mats=[gr.iso_stiffness(*m) for m in mats], phis=phis, normals=normals, tol=1e-6)
    E = np.array([1.0, 0.2, -0.3, 0.1, 0.25, 0.5])
    assert iso.run(E) is False and gen.run(E) is False
    assert abs(gen.mu_0 - iso.mu_0) <= 1e-14 * iso.mu_0
    assert gen.iterations == iso.iterations
    assert np.abs(gen.eps - iso.eps).max() <= 1e-12 * np.abs(iso.eps).max()


def test_scan_matrix_layout():
    """[[C_nn, C_ns], [C_ns^T, 2 C_ss]]"""
    C = gr.distinct_stiffness()
    A = gr.scan_matrix(C)
    assert np.array_equal(A[:3, :3], C[:3, :3]) and np.array_equal(A[:3, 3:], C[:3, 3:])
    assert np.array_equal(A[3:, :3], C[:3, 3:].T) and np.array_equal(A[3:, 3:], 2 * C[3:, 3:])
    assert len({round(v, 12) for v in C[np.triu_indices(6)]}) == 21

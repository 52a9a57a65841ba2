"""method "polarization" on the host: the per-voxel arithmetic of fg_stage_math.h (polarize_iso, polarize_generic and the
dispatch polarize_voxel) compiled for the host against the NumPy restatement (polarization_reference.py).

Tolerance.  Both sides solve (C + 2 mu_0 Id) R = F by Gaussian elimination with partial pivoting, which is backward stable:
each computed R is the exact solution of a system perturbed by O(n eps) relative, so two such solutions differ by at most
c n eps cond(A) |R|.  With n = 6 the bound used is 64 eps cond(A), on max |R| for the strain and on (|C|_inf + 2 mu_0) max |R|
for Q = C R - 2 mu_0 R (a product with the matrix adds its norm times the error of R).  The closed form of an isotropic voxel
is restated in the same operation order: 4 eps."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import general_reference as gr
import polarization_reference as pr
from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emulate", "emu_polar.cpp")
EPS = np.finfo(np.float64).eps
NCASE = 400


def make_cases():
    """seeded cases of three phases (general, mostly general, isotropic): pure voxels of each kind (phi == 1 exactly, the others
    0), mixed voxels, a fraction below the 10 eps threshold of the Voigt rule, mu_0 spread over four decades"""
    rng = np.random.default_rng(20251)
    cases = []
    for i in range(NCASE):
        law = np.array([1.0, float(i % 3 != 0), 0.0])
        mu = rng.uniform(0.5, 5.0, 3) * 10.0 ** rng.integers(-1, 3)
        lam = rng.uniform(0.1, 4.0, 3)
        C = np.stack([gr.random_spd(rng, coupling=(i % 2 == 0), scale=10.0 ** rng.integers(-2, 3)) for _ in range(3)])
        phi = rng.dirichlet(np.ones(3))
        kind = i % 8
        if kind == 0:
            phi = np.array([0.0, 0.0, 1.0])            # pure isotropic: the closed form
        elif kind == 1:
            phi = np.array([1.0, 0.0, 0.0])            # pure general: no form of its own, the 6 x 6 solve
        elif kind == 2:
            phi = np.array([phi[0] + phi[1], 0.0, phi[2]])
        elif kind == 3:
            phi = np.array([1.0 - 1e-15, 1e-15, 0.0])  # a fraction below the threshold is skipped; phi_0 != 1: generic
        elif kind == 4:
            phi = np.array([0.0, 1.0, 0.0])            # phase 1: general or isotropic by case
        mu_0 = 10.0 ** rng.uniform(-2, 2)
        F = rng.standard_normal(6)
        cases.append((law, mu, lam, C, phi, F, mu_0))
    return cases


def pack(cases):
    return np.concatenate([np.concatenate([law, mu, lam, C.ravel(), phi, F, [mu_0]]) for law, mu, lam, C, phi, F, mu_0 in cases])


@pytest.fixture(scope="module")
def emu_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "emu_polar.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, SRC])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def results(emu_lib):
    cases = make_cases()
    lib = emu_lib
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_polar_batch.restype = None
    lib.emu_polar_batch.argtypes = [ctypes.c_long, dp, dp]
    data = np.ascontiguousarray(pack(cases))
    res = np.zeros((len(cases), 25))
    lib.emu_polar_batch(len(cases), data.ctypes.data_as(dp), res.ctypes.data_as(dp))
    lib.emu_polar2_batch.restype = None
    lib.emu_polar2_batch.argtypes = [ctypes.c_long, dp, dp]
    two = two_phase_cases(cases)
    data2 = np.ascontiguousarray(pack(two))
    res2 = np.zeros((len(two), 13))
    lib.emu_polar2_batch(len(two), data2.ctypes.data_as(dp), res2.ctypes.data_as(dp))
    return cases, res, (two, res2)


def two_phase_cases(cases):
    """the same draws as two-phase voxels (phases 1 and 2 of each record moved to 0 and 1: mostly general + isotropic): pure of
    either kind, mixed, and a fraction below the threshold"""
    out = []
    for i, (law, mu, lam, C, phi, F, mu_0) in enumerate(cases):
        f = phi[1] + phi[2]
        phi2 = np.array([phi[1] / f, 1.0 - phi[1] / f, 0.0]) if f > 0 else np.array([1.0, 0.0, 0.0])
        if i % 8 == 3:
            phi2 = np.array([1e-15, 1.0 - 1e-15, 0.0])
        if i % 8 == 5:
            phi2 = np.array([0.0, 1.0, 0.0])
        out.append((np.roll(law, -1), np.roll(mu, -1), np.roll(lam, -1), np.roll(C, -1, axis=0), phi2, F, mu_0))
    return out


def n_phase_cases(cases, nph):
    """the same draws as nph-phase voxels: record i gives phases 0 .. 2, the records after it the rest (laws, moduli,
    stiffnesses and fractions in that order); the fractions are scaled to sum 1.  Every eighth voxel is pure in its last
    phase (the dispatch walks past nph - 1 zeros), the next has a fraction below the threshold there and phase 0 at zero,
    the next is pure in its last isotropic phase (the closed form)"""
    out = []
    for i, (law, mu, lam, C, phi, F, mu_0) in enumerate(cases):
        take = [cases[(i + j) % len(cases)] for j in range((nph + 2) // 3)]
        cat = lambda k: np.concatenate([t[k] for t in take])[:nph]   # noqa: E731
        phin = cat(4) / cat(4).sum() if cat(4).sum() > 0 else np.eye(nph)[0]
        pure = np.eye(nph)
        if i % 8 == 0:
            phin = pure[nph - 1]
        elif i % 8 == 1:
            phin = np.concatenate([[0.0], phin[1:nph - 1], [1e-15]])
            phin[1] += 1.0 - phin.sum()
        elif i % 8 == 2:
            phin = pure[max(p for p in range(nph) if cat(0)[p] == 0)]
        out.append((cat(0), cat(1), cat(2), cat(3), phin, F, mu_0))
    return out


@pytest.mark.parametrize("nph", [4, 5, 6, 7])
def test_four_to_seven_phase_instantiations(results, emu_lib, nph):
    """polarize_voxel<NPH> for NPH = 4 .. 7 (one kernel per phase count in launch_polarize; 2 and kMaxPhases are held above):
    the unrolled phase loops on nph-phase voxels, same bounds as the two-phase instantiation"""
    cases, lib = results[0], emu_lib
    many = n_phase_cases(cases, nph)
    data = np.ascontiguousarray(np.concatenate([np.concatenate([law, mu, lam, C.ravel(), phi, F, [mu_0]])
                                                for law, mu, lam, C, phi, F, mu_0 in many]))
    assert data.size == len(many) * (40 * nph + 7)
    res = np.zeros((len(many), 13))
    dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_polarn_batch.restype = ctypes.c_int
    lib.emu_polarn_batch.argtypes = [ctypes.c_int, ctypes.c_long, dp, dp]
    assert lib.emu_polarn_batch(nph, len(many), data.ctypes.data_as(dp), res.ctypes.data_as(dp)) == 0
    check_instantiation(many, res, nph)


def check_instantiation(cases, res, nph):
    """polarize_voxel<NPH> on nph-phase records against the restatement: the branch taken, then the strain and the polarisation
    at 64 eps cond(A) (6 x 6 solve) or 4 eps (closed form), as the module docstring derives"""
    ngeneric = 0
    for k, (law, mu, lam, C, phi, F, mu_0) in enumerate(cases):
        mats = [C[p] if law[p] else (mu[p], lam[p]) for p in range(nph)]
        phis = [np.full((1, 1, 1), phi[p]) for p in range(nph)]
        Fv = F.reshape(6, 1, 1, 1)
        M = pr.tangent_full(phis, mats)[0, 0, 0]
        generic = bool(pr.generic_mask(phis, mats)[0, 0, 0])
        assert res[k, 12] == float(generic), (k, phi)
        ngeneric += generic
        Q = pr.calc_polarization(Fv, phis, mats, mu_0).ravel()
        R = pr.calc_polarization(Fv, phis, mats, mu_0, inv=True).ravel()
        bound = 64 * EPS * np.linalg.cond(M + 2 * mu_0 * np.eye(6)) if generic else 4 * EPS
        sR = np.abs(R).max()
        sQ = (np.abs(M).sum(axis=1).max() + 2 * mu_0) * sR if generic else np.abs(Q).max()
        assert np.abs(res[k, 6:12] - R).max() <= bound * sR, (k, "inv")
        assert np.abs(res[k, :6] - Q).max() <= bound * sQ, (k, "forward")
    assert 0 < ngeneric < len(cases)


def restate(case):
    law, mu, lam, C, phi, F, mu_0 = case
    mats = [C[p] if law[p] else (mu[p], lam[p]) for p in range(3)]
    phis = [np.full((1, 1, 1), phi[p]) for p in range(3)]
    Fv = F.reshape(6, 1, 1, 1)
    M = pr.tangent_full(phis, mats)
    return mats, phis, Fv, M[0, 0, 0]


def test_against_restatement(results):
    cases, res, _ = results
    ngeneric = 0
    for k, case in enumerate(cases):
        mats, phis, Fv, M = restate(case)
        mu_0 = case[6]
        generic = bool(pr.generic_mask(phis, mats)[0, 0, 0])
        assert res[k, 12] == float(generic), (k, case[4])
        ngeneric += generic
        A = M + 2 * mu_0 * np.eye(6)
        bound = 64 * EPS * np.linalg.cond(A)
        Rg = pr.polarize_generic(Fv, M[None, None, None], mu_0, inv=True).ravel()
        Qg = pr.polarize_generic(Fv, M[None, None, None], mu_0).ravel()
        sR = np.abs(Rg).max()
        sQ = (np.abs(M).sum(axis=1).max() + 2 * mu_0) * sR
        assert np.abs(res[k, 19:25] - Rg).max() <= bound * sR, (k, "generic inv")
        assert np.abs(res[k, 13:19] - Qg).max() <= bound * sQ, (k, "generic")
        Q = pr.calc_polarization(Fv, phis, mats, mu_0).ravel()
        R = pr.calc_polarization(Fv, phis, mats, mu_0, inv=True).ravel()
        if generic:
            assert np.array_equal(res[k, :6], res[k, 13:19]) and np.array_equal(res[k, 6:12], res[k, 19:25])
        else:   # the closed form in the reference's operation order
            assert np.abs(res[k, 6:12] - R).max() <= 4 * EPS * np.abs(R).max(), (k, "iso inv")
            assert np.abs(res[k, :6] - Q).max() <= 4 * EPS * np.abs(Q).max(), (k, "iso")
    assert 0 < ngeneric < len(cases)


def test_inverse_undoes_forward(results):
    """P = (C + C0) eps  ->  inv gives eps back: the emulated strain of P, multiplied out, returns P"""
    cases, res, _ = results
    for k, case in enumerate(cases):
        mats, phis, Fv, M = restate(case)
        mu_0 = case[6]
        A = M + 2 * mu_0 * np.eye(6)
        back = A @ res[k, 19:25]
        assert np.abs(back - case[5]).max() <= 64 * EPS * np.linalg.cond(A) * np.abs(case[5]).max(), k


def test_two_phase_instantiation(results):
    """polarize_voxel<2>, the instantiation of every two-phase run: same bounds as above"""
    two, res2 = results[2]
    check_instantiation(two, res2, 2)

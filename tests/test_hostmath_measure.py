"""The measurement arithmetic Solver and SlabGroup share (fibergen_amd/csrc/fg_hostmath.h: bc_error_value, check_bc_compatible,
ref_mu0, extrapolation_weights and the load-step helpers) through a C shim, against literal Python restatements of the code it
replaced in fg_solver.hip / fg_slab.hip: the same float64 operations in the same order, compared exactly.  CPU only."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = ctypes.POINTER(ctypes.c_double)
EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "emu_hostmath_measure.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, os.path.join(ROOT, "tests", "emulate", "emu_hostmath_measure.cpp")])
    lib = ctypes.CDLL(out)
    lib.emu_bc_error_value.restype = ctypes.c_double
    lib.emu_bc_error_value.argtypes = [dp, dp, ctypes.c_double, dp, dp, dp, dp]
    lib.emu_check_bc_compatible.argtypes = [dp, dp, dp, dp]
    lib.emu_ref_mu0.restype = ctypes.c_double
    lib.emu_ref_mu0.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_double]
    lib.emu_extrapolation_weights.argtypes = [dp, ctypes.c_int, ctypes.c_double, dp]
    lib.emu_check_load_steps.argtypes = [dp, ctypes.c_int, ctypes.c_int]
    lib.emu_load_step_values.argtypes = [ctypes.c_double, dp, dp, dp, dp]
    return lib


def ptr(a):
    return a.ctypes.data_as(dp)


def arr(v):
    return np.ascontiguousarray(v, dtype=np.float64)


# ---- restatements (sequential sums, the order of the C++ text)
def voigt_mv(M, v):
    vc = [v[0], v[1], v[2], v[3] * 2, v[4] * 2, v[5] * 2]
    out = []
    for i in range(6):
        s = 0.0
        for j in range(6):
            s += M[i][j] * vc[j]
        out.append(s)
    return out


def voigt_norm2(v):
    s = 0.0
    for x in v:
        s += x * x
    return math.sqrt(s + v[3] * v[3] + v[4] * v[4] + v[5] * v[5])


def norm2(v):
    s = 0.0
    for x in v:
        s += x * x
    return math.sqrt(s)


def bc_error_restated(P, Q, bc_tol, Emean, Smean, E_cur, S_cur):
    PE, QS, PEc = voigt_mv(P, Emean), voigt_mv(Q, Smean), voigt_mv(P, E_cur)
    norm_E = voigt_norm2(PEc)
    err_F = voigt_norm2([PE[i] - E_cur[i] for i in range(6)]) / (1 if norm_E < bc_tol else norm_E)
    norm_S = voigt_norm2(S_cur)
    err_S = voigt_norm2([QS[i] - S_cur[i] for i in range(6)]) / (1 if norm_S < bc_tol else norm_S)
    return err_F if err_F > err_S else err_S


def compatible_restated(P, Q, Emax, Smax):
    se = math.sqrt(EPS)
    if norm2(voigt_mv(P, Smax)) > se * norm2(Smax):
        return 1
    if norm2(voigt_mv(Q, Emax)) > se * norm2(Emax):
        return 2
    return 0


def ref_mu0_restated(lmin, lmax, method, ref_scale):
    if lmin < 0:
        lmin = 0
    mu_0 = math.sqrt(lmin * lmax) if method == 2 else 0.5 * (lmin + lmax)
    mu_0 *= 0.5 * ref_scale
    return mu_0


def weights_restated(t, t_new):
    """the elimination as Solver::run_load_steps wrote it out; (weights, pivot rows) or None for a zero pivot"""
    n = len(t)
    A = [[math.pow(t[j], i) for j in range(n)] + [math.pow(t_new, i)] for i in range(n)]
    pivots = []
    for c in range(n):
        piv = c
        for r in range(c + 1, n):
            if abs(A[r][c]) > abs(A[piv][c]):
                piv = r
        if A[piv][c] == 0.0:
            return None
        pivots.append(piv)
        A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, n):
            m = A[r][c] / A[c][c]
            for j in range(c, n + 1):
                A[r][j] -= m * A[c][j]
    w = [0.0] * n
    for r in range(n - 1, -1, -1):
        v = A[r][n]
        for j in range(r + 1, n):
            v -= A[r][j] * w[j]
        w[r] = v / A[r][r]
    return w, pivots


def projectors():
    """pure strain, sigma_11 prescribed, all stresses prescribed, a rotated rank-one stress direction"""
    Id = np.diag([1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    out = [Id.copy(), np.diag([0.0, 1.0, 1.0, 0.5, 0.5, 0.5]), np.zeros((6, 6))]
    n = np.array([1.0, 2.0, -1.0, 0.5, 0.25, -0.75])
    n = n / math.sqrt(n[:3] @ n[:3] + 2 * n[3:] @ n[3:])
    out.append(Id - np.outer(n, n))
    return [(arr(P), arr(Id - P)) for P in out]


def test_bc_error_value(emu):
    rng = np.random.default_rng(2)
    seen = set()
    for P, Q in projectors():
        for bc_tol in (1e-8, 10.0):   # 10: both norms count as zero and divide by 1
            for _ in range(5):
                Em, Sm, Ec, Sc = (arr(rng.standard_normal(6)) for _ in range(4))
                if _ == 4:
                    Sc = arr(np.zeros(6))
                got = emu.emu_bc_error_value(ptr(P), ptr(Q), bc_tol, ptr(Em), ptr(Sm), ptr(Ec), ptr(Sc))
                want = bc_error_restated(P.tolist(), Q.tolist(), bc_tol, Em.tolist(), Sm.tolist(), Ec.tolist(), Sc.tolist())
                assert got == want
                seen.add(got)
    assert len(seen) > 30


def test_check_bc_compatible(emu):
    rng = np.random.default_rng(3)
    answers = []
    for P, Q in projectors():
        for _ in range(6):
            E, S = rng.standard_normal(6), rng.standard_normal(6)
            for Emax, Smax in ((E, S), (voigt_mv(P.tolist(), E), voigt_mv(Q.tolist(), S)), (voigt_mv(P.tolist(), E), S),
                               (E, voigt_mv(Q.tolist(), S)), (E, np.zeros(6))):
                Emax, Smax = arr(Emax), arr(Smax)
                got = emu.emu_check_bc_compatible(ptr(P), ptr(Q), ptr(Emax), ptr(Smax))
                assert got == compatible_restated(P.tolist(), Q.tolist(), Emax.tolist(), Smax.tolist())
                answers.append(got)
    assert set(answers) == {0, 1, 2}   # the stress condition is asked first


def test_ref_mu0(emu):
    rng = np.random.default_rng(4)
    cases = [(-0.5, 3.0), (0.0, 0.0), (0.0, 2.0), (1.0, 1.0)] + [tuple(sorted(rng.uniform(0.01, 50.0, 2))) for _ in range(20)]
    for lmin, lmax in cases:
        for method in (0, 1, 2):
            for ref_scale in (1.0, 0.7, 2.5):
                assert emu.emu_ref_mu0(lmin, lmax, method, ref_scale) == ref_mu0_restated(lmin, lmax, method, ref_scale)
    assert emu.emu_ref_mu0(-0.5, 3.0, 0, 1.0) == 0.75          # the clamp at 0, arithmetic mean / 2
    assert emu.emu_ref_mu0(1.0, 4.0, 2, 1.0) == 1.0            # polarisation: geometric mean / 2
    assert emu.emu_ref_mu0(1.0, 4.0, 1, 1.0) == 1.25


def weights(emu, t, t_new):
    t, w = arr(t), np.full(len(t), 7.0)
    ok = emu.emu_extrapolation_weights(ptr(t), len(t), t_new, ptr(w))
    return ok, w


@pytest.mark.parametrize("n", range(2, 9))
def test_extrapolation_weights(emu, n):
    rng = np.random.default_rng(n)
    ascending = np.linspace(0.1, 1.0, n)                       # |t_j^i| grows with j in every row: the pivot search moves
    paths = [ascending, ascending[::-1].copy(), np.sort(rng.uniform(0.05, 1.0, n)), rng.permutation(np.linspace(0.2, 1.5, n))]
    orders, checked = set(), []
    for t in paths:
        t_new = float(t.max() + 0.1)
        ok, w = weights(emu, t, t_new)
        want, pivots = weights_restated(t.tolist(), t_new)
        assert ok == 1 and w.tolist() == want
        orders.add(tuple(pivots))
        V = np.vander(t, n, increasing=True)                   # V_ij = t_i^j
        ref = np.linalg.solve(V.T, t_new ** np.arange(n))
        # against LAPACK where the forward error bound cond(V) eps |w| of either solver stays under 1e-12: n <= 5 on these nodes
        # (cond about 1.3e3, |w| < 3); from n = 6 on (cond 1e4 ... 1e6, |w| up to 40) only the exact comparison above holds
        if np.linalg.cond(V) * np.abs(ref).max() * np.finfo(float).eps < 1e-12:
            checked.append(n)
            assert np.abs(w - ref).max() <= 1e-12
    assert n > 5 or len(checked) >= 3                          # (random nodes may lie close together)
    assert any(p != tuple(range(n)) for p in orders)           # a pivot order that is not the natural one was taken
    t = paths[0].copy()
    t[-1] = t[0]                                               # two equal parameters: the matrix is singular
    ok, w = weights(emu, t, 2.0)
    assert ok == 0 and weights_restated(t.tolist(), 2.0) is None and (w == 7.0).all()


def test_load_step_helpers(emu):
    p = arr([0.5, 1.0])
    assert emu.emu_check_load_steps(ptr(p), 2, 0) == 0 and emu.emu_check_load_steps(ptr(p), 2, 1) == 0
    assert emu.emu_check_load_steps(ptr(p), 0, 0) == 1 and emu.emu_check_load_steps(ptr(p), 2, -1) == 1
    assert emu.emu_check_load_steps(None, 2, 0) == 1
    rng = np.random.default_rng(6)
    Emax, Smax, E, S = arr(rng.standard_normal(6)), arr(rng.standard_normal(6)), np.zeros(6), np.zeros(6)
    for t in (0.0, 0.3, 1.0, 1.7):
        emu.emu_load_step_values(t, ptr(Emax), ptr(Smax), ptr(E), ptr(S))
        assert E.tolist() == [t * x for x in Emax.tolist()] and S.tolist() == [t * x for x in Smax.tolist()]

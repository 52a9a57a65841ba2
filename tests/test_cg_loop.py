"""The CG iteration skeleton the five pipelined conjugate-gradient loops share (fibergen_amd/csrc/fg_cg_loop.h) driven through
a C shim on a small dense problem, against a literal Python restatement of the loop as the solver wrote it out before the
skeleton existed (Solver::run_cg_u), and against the host-scalar loop (Solver::run_cg's tail) restated likewise.  The shim and
the restatement do the same float64 operations in the same order (sequential sums, no contraction), so call traces, alpha /
beta sequences and iterates are compared for equality.  CPU only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = sys.float_info.min
K = 24   # first CG slot (kSlotCg)
APPLY_P, APPLY_DIR, DIRECTION, DOT_PW, UPDATE, FETCH, MAY_RUN_AHEAD, SUMS, ESTIMATOR, CONVERGED, ADVANCE, RR_AFTER, WAIT, BC_OK = range(1, 15)
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int)
NEVER = -1


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "emu_cg_loop.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, os.path.join(ROOT, "tests", "emulate", "emu_cg_loop.cpp")])
    lib = ctypes.CDLL(out)
    lib.emu_cg_pipelined.restype = ctypes.c_long
    lib.emu_cg_pipelined.argtypes = [ctypes.c_int, dp, dp, ctypes.c_double, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_long, dp, ip, ctypes.c_int, dp, dp, ip]
    return lib


def problem(n, seed=3):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, n))
    a = m @ m.T / n + np.eye(n)   # symmetric positive definite, condition number about 5
    return np.ascontiguousarray(a), rng.standard_normal(n)


def run_header(emu, a, b, tol=-1.0, maxiter=1000, fused_dir=False, run_ahead=False, fail_at=NEVER):
    n = len(b)
    cap = 4 * 16 * (maxiter + 2)
    x, trace = np.zeros(n), np.zeros(cap, dtype=np.int32)
    alphas, betas, out = np.zeros(maxiter + 2), np.zeros(maxiter + 2), np.zeros(4, dtype=np.int32)
    args = (x.ctypes.data_as(dp), trace.ctypes.data_as(ip), cap, alphas.ctypes.data_as(dp), betas.ctypes.data_as(dp),
            out.ctypes.data_as(ip))
    it = emu.emu_cg_pipelined(n, a.ctypes.data_as(dp), b.ctypes.data_as(dp), tol, maxiter, K, int(fused_dir), int(run_ahead), fail_at,
                              *args)
    assert out[1] <= cap
    return dict(iter=it, failed=bool(out[0]), trace=[tuple(r) for r in trace[:out[1]].reshape(-1, 4).tolist()], x=x,
                alphas=alphas[:out[2]].tolist(), betas=betas[:out[3]].tolist())


class Vectors:
    """the vector work of the shim, sums taken in index order"""

    def __init__(self, a, b):
        self.a, self.n = a, len(b)
        self.x, self.r, self.p, self.w = [0.0] * self.n, list(b), list(b), [0.0] * self.n
        self.alphas, self.betas = [], []

    def apply(self):
        for i in range(self.n):
            s = 0.0
            for j in range(self.n):
                s += self.a[i, j] * self.p[j]
            self.w[i] = self.p[i] - s

    @staticmethod
    def dot(u, v):
        s = 0.0
        for ui, vi in zip(u, v):
            s += ui * vi
        return s

    def pw(self):
        return self.dot(self.p, [pi - wi for pi, wi in zip(self.p, self.w)])

    def axpy_x(self, alpha):
        self.alphas.append(alpha)
        self.x = [xi + alpha * pi for xi, pi in zip(self.x, self.p)]

    def axpy_r(self, alpha):
        self.r = [ri - alpha * (pi - wi) for ri, pi, wi in zip(self.r, self.p, self.w)]

    def direction(self, beta):
        self.betas.append(beta)
        self.p = [ri + beta * pi for ri, pi in zip(self.r, self.p)]


class Rule:
    """StopRule::measure + decide with the shim's hooks (nothing requested, no callback, bc_ok) and its scripted failure"""

    def __init__(self, tol, maxiter, fail_at):
        self.tol, self.maxiter, self.fail_at, self.prev = tol, maxiter, fail_at, 0.0

    def measure(self, cur):
        self.abs_err = abs(self.prev - cur)
        self.rel_err = self.abs_err / (TINY + cur)
        self.prev = cur

    def converged(self, it, t=None):
        """(the loop ends, failed); bc_ok is asked -- and traced -- only when a tolerance is met"""
        if it == self.fail_at:
            return True, True
        if self.rel_err != self.rel_err:
            return True, True
        if it >= self.maxiter:
            return True, False
        met = self.rel_err <= self.tol or self.abs_err <= -1.0
        if met and t is not None:
            t.append((BC_OK, 0, 0, 0))
        return met, False


def run_python_pipelined(a, b, tol, maxiter, fused_dir, run_ahead, fail_at):
    """Solver::run_cg_u's loop as it stood, on the shim's problem: cb_ is `not run_ahead`, the kernels are the Vectors' methods"""
    v, rule, t, nvox = Vectors(a, b), Rule(tol, maxiter, fail_at), [], float(len(b))
    d = {}
    blk, s0 = (K, K + 8), K + 16
    d[blk[0] + 6] = v.dot(v.r, v.r)

    def beta(num, den):
        return (d[num] / nvox + TINY) / (d[den] / nvox + TINY)

    def apply_p():
        t.append((APPLY_P, 0, 0, 0))
        v.apply()

    def apply_dir(num, den):
        t.append((APPLY_DIR, num, den, 0))
        v.direction(beta(num, den))
        v.apply()

    def direction(num, den):
        t.append((DIRECTION, num, den, 0))
        v.direction(beta(num, den))

    it, failed, applied = 0, False, False
    beta_num = beta_den = 0
    while True:
        cur = it & 1
        nxt = cur ^ 1
        if not applied:
            if fused_dir and it > 0:
                apply_dir(beta_num, beta_den)
            else:
                apply_p()
        applied = False
        t.append((DOT_PW, s0, 0, 0))
        d[s0] = v.pw()
        t.append((UPDATE, blk[cur] + 6, s0, blk[nxt]))
        alpha = (d[blk[cur] + 6] / nvox + TINY) / (d[s0] / nvox + TINY)
        v.axpy_x(alpha)
        v.axpy_r(alpha)
        d[blk[nxt]], d[blk[nxt] + 6] = v.dot(v.x, v.x), v.dot(v.r, v.r)
        t.append((FETCH, blk[nxt], 0, 0))
        h0 = d[blk[nxt]]
        t.append((MAY_RUN_AHEAD, 0, 0, 0))
        if run_ahead and it < maxiter:
            if fused_dir:
                apply_dir(blk[nxt] + 6, blk[cur] + 6)
            else:
                direction(blk[nxt] + 6, blk[cur] + 6)
                apply_p()
            applied = True
        t.append((WAIT, 0, 0, 0))
        t.append((SUMS, 0, 0, 0))
        rule.measure(np.sqrt(h0 / nvox))
        t.append((ESTIMATOR, 0, 0, 0))
        t.append((CONVERGED, it, 0, 0))
        stop, failed = rule.converged(it, t)
        if stop:
            break
        it += 1
        if not applied:
            if fused_dir:
                beta_num, beta_den = blk[nxt] + 6, blk[cur] + 6
            else:
                direction(blk[nxt] + 6, blk[cur] + 6)
    return dict(iter=it, failed=failed, trace=t, x=np.array(v.x), alphas=v.alphas, betas=v.betas)


def run_python_host(a, b, tol, maxiter, r_late, fail_at):
    """the host-scalar loops as they stood: SlabGroup::run_cg_scalar's tail (r updated with the iterate) and, r_late, Solver::run_cg's
    tail (r updated after the stop test)"""
    v, rule, t, nvox = Vectors(a, b), Rule(tol, maxiter, fail_at), [], float(len(b))
    gamma = v.dot(v.r, v.r) / nvox + TINY
    it, failed = 0, False
    while True:
        t.append((APPLY_P, 0, 0, 0))
        v.apply()
        t.append((DOT_PW, 0, 0, 0))
        alpha = gamma / (v.pw() / nvox + TINY)
        t.append((ADVANCE, 0, 0, 0))
        v.axpy_x(alpha)
        if not r_late:
            v.axpy_r(alpha)
            rr = v.dot(v.r, v.r)
        rule.measure(np.sqrt(v.dot(v.x, v.x) / nvox))
        t.append((ESTIMATOR, 0, 0, 0))
        t.append((CONVERGED, it, 0, 0))
        stop, failed = rule.converged(it)
        if stop:
            break
        it += 1
        t.append((RR_AFTER, 0, 0, 0))
        if r_late:
            v.axpy_r(alpha)
            rr = v.dot(v.r, v.r)
        delta = rr / nvox + TINY
        beta = delta / gamma
        gamma = delta
        t.append((DIRECTION, 0, 0, 0))
        v.direction(beta)
    return dict(iter=it, failed=failed, trace=t, x=np.array(v.x), alphas=v.alphas, betas=v.betas)


def same(got, want):
    assert got["iter"] == want["iter"] and got["failed"] == want["failed"]
    assert got["trace"] == want["trace"]
    assert got["alphas"] == want["alphas"] and got["betas"] == want["betas"]
    assert np.array_equal(got["x"], want["x"])


# (tol, maxiter, fail_at, iteration the run must end in, failed): tolerance never met and maxiter reached (the deferred direction is
# seen on iterations 1, 2 and 3); convergence on the first iteration (rel_err = 1 there: the estimate starts from the zero field);
# a tolerance met in between; a `converged` that fails
ENDINGS = [(-1.0, 4, NEVER, 4, False), (2.0, 50, NEVER, 0, False), (1e-3, 50, NEVER, None, False), (-1.0, 50, 2, 2, True)]


@pytest.mark.parametrize("tol,maxiter,fail_at,last,failed", ENDINGS)
@pytest.mark.parametrize("run_ahead", [False, True])
@pytest.mark.parametrize("fused_dir", [False, True])
def test_pipelined_trace(emu, fused_dir, run_ahead, tol, maxiter, fail_at, last, failed):
    a, b = problem(7)
    got = run_header(emu, a, b, tol=tol, maxiter=maxiter, fused_dir=fused_dir, run_ahead=run_ahead, fail_at=fail_at)
    same(got, run_python_pipelined(a, b, tol, maxiter, fused_dir, run_ahead, fail_at))
    assert got["failed"] == failed
    assert got["iter"] == last if last is not None else 0 < got["iter"] < maxiter
    if last == maxiter:   # nothing is enqueued behind the last iteration's fetch
        assert [c[0] for c in got["trace"][-6:]] == [FETCH, MAY_RUN_AHEAD, WAIT, SUMS, ESTIMATOR, CONVERGED]
    assert (got["trace"][-1][0] == BC_OK) == (last is None or last == 0)   # bc_ok is asked only when a tolerance is met
    if fused_dir:         # the direction is never formed point-wise, and from the second iteration on always inside the sweep
        codes = [c[0] for c in got["trace"]]
        assert DIRECTION not in codes and codes.count(APPLY_P) == 1
        if last == maxiter:
            dirs = [c[1:3] for c in got["trace"] if c[0] == APPLY_DIR]
            assert dirs == [(K + 14, K + 6), (K + 6, K + 14), (K + 14, K + 6), (K + 6, K + 14)]


@pytest.mark.parametrize("n", [6, 9, 12])
def test_iterate_is_plain_cg(emu, n):
    """A stop rule that never stops before maxiter = n: the iterate is that of textbook CG written with numpy (the matrix-vector
    product and the inner products through BLAS, i.e. the same operations in another summation order).  Bound: 16 eps |x|, a few
    ulp of the solution norm -- the matrix has a condition number of about 5, so the rounding of the n-term sums (a few eps
    each) reaches x hardly amplified; a wrong slot or a wrong order of the calls shows at 1e-2 |x| or more."""
    a, b = problem(n)
    x, r = np.zeros(n), b.copy()
    p, gamma = r.copy(), r @ r / n + TINY
    for _ in range(n + 1):
        ap = a @ p
        alpha = gamma / (p @ ap / n + TINY)
        x, r = x + alpha * p, r - alpha * ap
        delta = r @ r / n + TINY
        p, gamma = r + delta / gamma * p, delta
    bound = 16 * np.finfo(float).eps * np.linalg.norm(x)
    for kw in (dict(fused_dir=False, run_ahead=False), dict(fused_dir=True, run_ahead=True)):
        got = run_header(emu, a, b, maxiter=n, **kw)
        assert got["iter"] == n and not got["failed"]
        assert np.linalg.norm(got["x"] - x) <= bound
        assert np.linalg.norm(a @ got["x"] - b) <= 1e-9 * np.linalg.norm(b)   # and it solves the system: CG ends after n steps


@pytest.mark.parametrize("n", [6, 12])
def test_both_forms_take_the_same_steps(emu, n):
    """the pipelined skeleton forms the alpha / beta sequence of the host-scalar loops (restated above, both placements of the r
    update), to the bit"""
    a, b = problem(n, seed=5)
    host = run_python_host(a, b, -1.0, n, False, NEVER)
    assert len(host["alphas"]) == n + 1 and len(host["betas"]) == n
    late = run_python_host(a, b, -1.0, n, True, NEVER)
    assert late["alphas"] == host["alphas"] and late["betas"] == host["betas"]
    for fused_dir in (False, True):
        for run_ahead in (False, True):
            pipe = run_header(emu, a, b, maxiter=n, fused_dir=fused_dir, run_ahead=run_ahead)
            assert pipe["alphas"] == host["alphas"] and pipe["betas"] == host["betas"]
            assert np.array_equal(pipe["x"], host["x"])

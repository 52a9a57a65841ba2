"""The basic-scheme iteration Solver::run_one_step and SlabGroup::run_step share (fibergen_amd/csrc/fg_basic_loop.h) driven
through a C shim on a toy contraction, against two literal Python restatements: the loop of each site as it was written out
before the skeleton existed.  The shim's hooks and the restatements do the same float64 operations in the same order, so call
traces (hook, argument, the E / E_next handed over), residual histories and final fields are compared for equality.  CPU only."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import emulation_build_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emulate", "emu_basic_loop.cpp")
TINY = sys.float_info.min
(REFRESH, MIXED_ASKED, START_FROM, CARRY, U_PASS, STRAIN, WAIT, MQ_TAU, NORM, ESTIMATOR, CONVERGED, BC_OK, ADOPT, CHAIN, PREPARE, F00,
 FINISH) = range(1, 18)
E0 = [0.5, -0.2, 0.1, 0.05, -0.1, 0.3]
N = 5
LONE, GROUP = 0, 1
dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu") / "emu_basic_loop.so")
    subprocess.check_call(["g++"] + emulation_build_flags() + ["-o", out, SRC])
    lib = ctypes.CDLL(out)
    lib.emu_basic_loop.restype = ctypes.c_int
    lib.emu_basic_loop.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_long), ctypes.c_double, dp, dp, ctypes.c_int, dp,
                                   dp]
    return lib


def scenario(site, fresh=1, u_space=1, have_u=None, mixed=0, update_ref=0, voting=0, estimator=0, leaves_u=1, bc_fail=0, maxiter=40,
             nan_at=-1, stop_at=-1, tol=1e-6):
    if have_u is None:
        have_u = int(bool(fresh and u_space))   # a fresh step in displacement space starts from u = 0
    return dict(site=site, fresh=fresh, u_space=u_space, have_u=have_u, mixed=mixed, update_ref=update_ref, voting=voting,
                estimator=estimator, leaves_u=leaves_u, bc_fail=bc_fail, maxiter=maxiter, nan_at=nan_at, stop_at=stop_at, tol=tol)


def run_header(emu, sc):
    ints = (ctypes.c_int * 10)(*[sc[k] for k in ("site", "fresh", "u_space", "have_u", "mixed", "update_ref", "voting", "estimator",
                                                  "leaves_u", "bc_fail")])
    longs = (ctypes.c_long * 3)(sc["maxiter"], sc["nan_at"], sc["stop_at"])
    cap = 8 * 16 * (sc["maxiter"] + 4)
    trace, res, out, e0 = np.zeros(cap), np.zeros(sc["maxiter"] + 2), np.zeros(3 + N), np.array(E0)
    n = emu.emu_basic_loop(ints, longs, sc["tol"], e0.ctypes.data_as(dp), trace.ctypes.data_as(dp), cap, res.ctypes.data_as(dp),
                           out.ctypes.data_as(dp))
    assert 0 < n <= cap and n % 8 == 0
    return dict(iter=int(out[0]), failed=bool(out[1]), trace=[tuple(r) for r in trace[:n].reshape(-1, 8).tolist()],
                residuals=res[:int(out[2])].tolist(), eps=out[3:].tolist())


class Toy:
    """the shim's field and its estimator, sums taken in index order"""

    def __init__(self, sc):
        self.sc, self.t, self.residuals = sc, [], []
        self.eps = [0.0 if sc["fresh"] else 0.3 + 0.1 * i for i in range(N)]
        self.dev, self.ss, self.tau, self.have_u, self.bc_asked, self.calls = [0.0] * N, 0.0, 0.0, bool(sc["have_u"]), 0, 0
        self.m_prev, self.m_pp, self.w_prev, self.est_iter = [0.0] * 6, [0.0] * 6, 0.0, 0

    def rec(self, code, a=0.0, E=None):
        self.t.append((float(code), float(a)) + tuple(float(x) for x in (E if E is not None else [0.0] * 6)))

    def sum(self):
        s = 0.0
        for x in self.eps:
            s += x
        return s

    def sumsq(self):
        s = 0.0
        for x in self.eps:
            s += x * x
        return s

    def sweep(self):
        t = [0.5 * (1.0 + 0.2 * i) * self.eps[(i + 1) % N] for i in range(N)]
        m = 0.0
        for x in t:
            m += x
        m /= N
        self.dev = [x - m for x in t]

    def take(self, mean):
        self.eps = [mean + d for d in self.dev]

    # MeanEstimator and the two templates beside it (fg_stop_rule.h)
    def mean_stress(self):
        return [self.sum() * (c + 1) / N for c in range(6)]

    @staticmethod
    def norm9_diff(a, b):
        s = 0.0
        for c in range(6):
            s += (a[c] - b[c]) * (a[c] - b[c]) * (2.0 if c >= 3 else 1.0)
        return math.sqrt(s)

    def estimator_begin(self):
        k, fresh = self.sc["estimator"], self.sc["fresh"]
        if k == 2:
            m = [0.0] * 6 if fresh else self.mean_stress()
            self.m_prev, self.m_pp, self.est_iter = list(m), list(m), 0
        elif k == 3:
            self.w_prev, self.est_iter = 0.0 if fresh else self.sumsq() / N, 0

    def estimator_update(self, rule):
        k = self.sc["estimator"]
        if k == 2:
            m = self.mean_stress()
            if self.est_iter > 1:
                rule.abs_err = 0.5 * (self.norm9_diff(self.m_pp, m) + self.norm9_diff(self.m_prev, m))
            else:
                rule.abs_err = self.norm9_diff(self.m_prev, m)
            rule.rel_err = rule.abs_err / (TINY + self.norm9_diff(m, [0.0] * 6))
            self.m_pp, self.m_prev = self.m_prev, list(m)
            self.est_iter += 1
        elif k == 3:
            w = self.sumsq() / N
            rule.abs_err = abs(self.w_prev - w)
            rule.rel_err = rule.abs_err / (TINY + abs(w))
            self.w_prev = w
            self.est_iter += 1
        elif k == 4:
            rule.abs_err = rule.rel_err = 1.0

    # the device work of the hooks
    def do_carry(self, E):
        self.rec(CARRY, 0, E)
        self.sweep()
        self.take(E[0])

    def do_u_pass(self, E, mixed, chain_now):
        self.rec(U_PASS, chain_now, E)
        self.ss = self.sumsq()
        if mixed:
            self.tau = 0.25 * self.sum() / N
        self.sweep()

    def do_strain_pass(self, E, mixed):
        self.rec(STRAIN, mixed, E)
        shift = 0.3 * (0.25 * self.sum() / N) if mixed else 0.0
        self.sweep()
        self.take(E[0] - shift)
        self.ss = self.sumsq()
        self.have_u = bool(self.sc["leaves_u"]) and not mixed

    def do_refresh(self):
        E = [E0[c] + 0.01 * (c + 1) for c in range(6)]
        self.rec(REFRESH, 0, E)
        return E

    def do_norm(self):
        self.rec(NORM)
        self.calls += 1
        return float("nan") if self.calls == self.sc["nan_at"] else math.sqrt(self.ss / N)

    def do_adopt(self, E_next):
        self.rec(ADOPT, 0, E_next)
        self.take(E_next[0])
        self.have_u = True

    def bc_ok(self):
        self.rec(BC_OK)
        self.bc_asked += 1
        return self.bc_asked > self.sc["bc_fail"]


class Rule:
    """StopRule::measure + decide with the shim's hooks: a stop request at iteration stop_at, no callback"""

    def __init__(self, q):
        sc = q.sc
        self.q, self.tol, self.maxiter, self.stop_at = q, sc["tol"], sc["maxiter"], sc["stop_at"]
        self.prev = 0.0 if sc["fresh"] else math.sqrt(q.sumsq() / N)
        self.abs_err = self.rel_err = 0.0

    def measure(self, cur):
        self.abs_err = abs(self.prev - cur)
        self.rel_err = self.abs_err / (TINY + cur)
        self.prev = cur

    def converged(self, it):
        """(the loop ends, failed)"""
        self.q.rec(CONVERGED, it)
        if self.rel_err != self.rel_err:
            return True, True
        if it == self.stop_at:
            return True, True
        self.q.residuals.append(self.rel_err)
        if it >= self.maxiter:
            return True, False
        if (self.rel_err <= self.tol or self.abs_err <= -1.0) and self.q.bc_ok():
            return True, False
        return False, False


def finish(q, it, failed):
    q.rec(FINISH, it, [float(failed), 0, 0, 0, 0, 0])
    return dict(iter=it, failed=failed, trace=q.t, residuals=q.residuals, eps=q.eps)


def run_python_lone(sc):
    """Solver::run_one_step as it stood (method basic), from `for (int i = 0; i < 6; ++i) F00_[i] = 0.0;` to its return"""
    q = Toy(sc)
    fresh_step = bool(sc["fresh"])
    q.rec(F00)
    uloop = bool(sc["u_space"])
    q.rec(MIXED_ASKED)
    mixed_bc = bool(sc["mixed"])   # asked once, before calc_ref_material
    rule = Rule(q)
    if sc["estimator"] >= 2:
        q.estimator_begin()
    it = 1
    carry = uloop and not fresh_step and q.have_u
    update_ref = bool(sc["update_ref"])
    E = list(E0)
    E_next_ = list(E0)   # (the member: u_pass_front sets it, the correction overwrites it)
    failed = False
    while True:
        if update_ref:
            E = q.do_refresh()
            update_ref = False
        pending_back = False
        if carry:
            if mixed_bc:
                carry = False
                uloop = False
            else:
                q.do_carry(E)   # u_pass_front(E); u_pass_back()
                carry = False
        if uloop and q.have_u:
            if it == 1 and fresh_step:
                q.rec(START_FROM, 0, E)
                q.take(E[0])
            q.do_u_pass(E, mixed_bc, False)
            E_next_ = list(E)
            pending_back = True
        else:
            q.do_strain_pass(E, mixed_bc)
            if uloop and q.have_u and not mixed_bc:
                carry = True
            else:
                uloop = False
        q.rec(WAIT, pending_back)   # fetch_norms_and_errors: if (pending_back_) launch_pending_back()
        if pending_back and mixed_bc:
            q.rec(MQ_TAU)
            t1 = [0.3 * q.tau if c == 0 else 0.0 for c in range(6)]
            E_next_ = [E[c] - t1[c] for c in range(6)]
        rule.measure(q.do_norm())
        q.rec(ESTIMATOR, sc["estimator"])
        if sc["estimator"] >= 2:
            q.estimator_update(rule)
        stop, failed = rule.converged(it)
        if stop:
            break
        if pending_back:
            q.do_adopt(E_next_)   # adopt_back()
        it += 1
    return finish(q, it, failed)


def run_python_group(sc):
    """SlabGroup::run_step as it stood, from `StopRule rule = a.stop_rule(prev0);` to its return"""
    q = Toy(sc)
    fresh = bool(sc["fresh"])
    fast = bool(sc["u_space"])
    rule = Rule(q)
    if sc["estimator"] >= 2:
        q.estimator_begin()
    carry = (not fresh) and fast
    carry = carry and q.have_u
    voting = bool(sc["voting"])
    it = 1
    update_ref = bool(sc["update_ref"])
    E = list(E0)
    failed = False
    while True:
        if update_ref:
            E = q.do_refresh()
            update_ref = False
            if fast:
                q.rec(PREPARE)
        q.rec(MIXED_ASKED)
        mixed_bc = bool(sc["mixed"])   # asked on every iteration, after calc_ref_material
        if carry:
            carry = False
            if mixed_bc:
                fast = False
            else:
                q.do_carry(E)   # pass_fast(a.E_cur_, false, true); slab_adopt(E, true)
        all_u = q.have_u
        pending = False
        if fast and all_u:
            if it == 1 and fresh:
                q.rec(START_FROM, 0, E)
                q.take(E[0])
            q.do_u_pass(E, mixed_bc, not voting)
            pending = True
        else:
            q.do_strain_pass(E, mixed_bc)
            have_u = fast and not mixed_bc
            have_u = have_u and q.have_u
            if have_u:
                carry = True
            else:
                fast = False
        q.rec(WAIT, 0)   # wait_norms()
        E_next = list(E)
        if pending and mixed_bc:
            q.rec(MQ_TAU)
            t1 = [0.3 * q.tau if c == 0 else 0.0 for c in range(6)]
            E_next = [E[c] - t1[c] for c in range(6)]
        rule.measure(q.do_norm())
        q.rec(ESTIMATOR, sc["estimator"])
        if sc["estimator"] >= 2:
            q.estimator_update(rule)
        stop, failed = rule.converged(it)
        if stop:
            break
        if pending:
            if voting:
                q.rec(CHAIN)   # pass_fast_chain()
            q.do_adopt(E_next)
        it += 1
    return finish(q, it, failed)


RESTATED = {LONE: run_python_lone, GROUP: run_python_group}


def same(got, want):
    assert got["iter"] == want["iter"] and got["failed"] == want["failed"]
    assert got["trace"] == want["trace"], next((i, a, b) for i, (a, b) in enumerate(zip(got["trace"], want["trace"])) if a != b)
    assert got["residuals"] == want["residuals"]
    assert got["eps"] == want["eps"]


def common(trace):
    """The hook table of DESIGN.md section 4 as a filter: what remains of a site's trace once the calls that exist on one site only
    are taken out -- the lone solver clears F00_ and asks mixed_bc() once, before the loop; the group asks in every iteration and
    prepares again behind a refreshed reference material; the lone wait enqueues the chain, the group's pass does, or (voting) its
    adopt."""
    keep = []
    for r in trace:
        if r[0] in (F00, MIXED_ASKED, PREPARE, CHAIN):
            continue
        keep.append((r[0], 0.0) + r[2:] if r[0] in (U_PASS, WAIT) else r)
    return keep


def codes(trace):
    return [int(r[0]) for r in trace]


SCENARIOS = {
    "fresh, prescribed strain": dict(),
    "fresh, mixed bc": dict(mixed=1),
    "continuing, carries": dict(fresh=0, have_u=1),
    "continuing, mixed bc: displacement space is left": dict(fresh=0, have_u=1, mixed=1),
    "no displacement: strain pass, carry, displacement passes": dict(fresh=0, have_u=0),
    "no displacement and the pass leaves none": dict(fresh=0, have_u=0, leaves_u=0),
    "no displacement loop": dict(u_space=0),
    "no displacement loop, mixed bc, continuing": dict(fresh=0, u_space=0, mixed=1),
    "update_ref": dict(update_ref=1),
    "update_ref, mixed bc, continuing": dict(fresh=0, have_u=1, mixed=1, update_ref=1),
    "voting": dict(voting=1),
    "voting, mixed bc": dict(voting=1, mixed=1),
    "voting, maxiter": dict(voting=1, maxiter=3, tol=-1.0),
    "maxiter": dict(maxiter=4, tol=-1.0),
    "maxiter at once": dict(maxiter=1, tol=-1.0),
    "nan": dict(nan_at=3),
    "stop request": dict(stop_at=2),
    "estimator sigma": dict(estimator=2),
    "estimator sigma, continuing": dict(estimator=2, fresh=0, have_u=1),
    "estimator energy": dict(estimator=3),
    "estimator energy, continuing, mixed bc": dict(estimator=3, fresh=0, have_u=1, mixed=1),
    "estimator none": dict(estimator=4, maxiter=5),
    "bc_ok false twice, then true": dict(mixed=1, bc_fail=2),
}


@pytest.mark.parametrize("site", [LONE, GROUP], ids=["lone", "group"])
@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_trace_equals_the_loop_as_it_stood(emu, name, site):
    sc = scenario(site, **SCENARIOS[name])
    got = run_header(emu, sc)
    same(got, RESTATED[site](sc))


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_sites_differ_as_the_hook_table_says(emu, name):
    lone, group = (RESTATED[s](scenario(s, **SCENARIOS[name])) for s in (LONE, GROUP))
    assert common(lone["trace"]) == common(group["trace"])
    assert lone["residuals"] == group["residuals"] and lone["eps"] == group["eps"] and lone["iter"] == group["iter"]
    got = run_header(emu, scenario(GROUP, **SCENARIOS[name]))
    assert common(got["trace"]) == common(lone["trace"])
    # the calls of one site only
    assert codes(lone["trace"]).count(F00) == 1 and codes(lone["trace"]).count(MIXED_ASKED) == 1
    assert codes(lone["trace"])[:2] == [F00, MIXED_ASKED]
    assert codes(group["trace"]).count(MIXED_ASKED) == group["iter"] and F00 not in codes(group["trace"])
    assert CHAIN not in codes(lone["trace"]) and PREPARE not in codes(lone["trace"])


def test_scenarios_reach_what_they_name(emu):
    def run(name, site=GROUP):
        return run_header(emu, scenario(site, **SCENARIOS[name]))

    t = run("fresh, prescribed strain")
    assert codes(t["trace"])[:4] == [MIXED_ASKED, START_FROM, U_PASS, WAIT] and STRAIN not in codes(t["trace"]) and not t["failed"]
    assert 3 < t["iter"] < 40 and codes(t["trace"])[-2:] == [BC_OK, FINISH]
    t = run("fresh, mixed bc")
    adopted = [r[2] for r in t["trace"] if r[0] == ADOPT]
    assert MQ_TAU in codes(t["trace"]) and all(e != E0[0] for e in adopted[1:])   # E_next = E - MQ:<tau> reaches the adopt
    t = run("continuing, carries")
    assert codes(t["trace"])[:3] == [MIXED_ASKED, CARRY, U_PASS] and codes(t["trace"]).count(CARRY) == 1
    t = run("continuing, mixed bc: displacement space is left")
    assert CARRY not in codes(t["trace"]) and U_PASS not in codes(t["trace"]) and codes(t["trace"]).count(STRAIN) == t["iter"]
    t = run("no displacement: strain pass, carry, displacement passes")
    c = [x for x in codes(t["trace"]) if x in (STRAIN, CARRY, U_PASS)]
    assert c[:3] == [STRAIN, CARRY, U_PASS] and set(c[3:]) == {U_PASS}
    t = run("no displacement and the pass leaves none")
    assert U_PASS not in codes(t["trace"]) and CARRY not in codes(t["trace"])
    for name in ("update_ref", "update_ref, mixed bc, continuing"):
        t = run(name)
        assert codes(t["trace"])[:2] == [REFRESH, PREPARE] and codes(t["trace"]).count(REFRESH) == 1
        assert [r[2] for r in t["trace"] if r[0] in (U_PASS, STRAIN)][0] == E0[0] + 0.01   # the pass runs on the refreshed mean
    for name in ("voting", "voting, mixed bc", "voting, maxiter"):
        t = run(name)
        c = codes(t["trace"])
        assert all(r[1] == 0.0 for r in t["trace"] if r[0] == U_PASS)                       # no chain with the sweep
        assert c.count(CHAIN) == c.count(ADOPT) == t["iter"] - 1                             # none on the breaking iteration
        assert all(c[i - 1] in (CONVERGED, BC_OK) and c[i + 1] == ADOPT for i, x in enumerate(c) if x == CHAIN)   # after the stop decision
    t = run("maxiter")
    assert t["iter"] == 4 and not t["failed"] and BC_OK not in codes(t["trace"])
    assert run("maxiter at once")["iter"] == 1
    t = run("nan")
    assert t["iter"] == 3 and t["failed"] and len(t["residuals"]) == 2
    t = run("stop request")
    assert t["iter"] == 2 and t["failed"] and len(t["residuals"]) == 1
    plain = run("fresh, prescribed strain")
    for name in ("estimator sigma", "estimator energy"):
        t = run(name)
        assert t["residuals"] != plain["residuals"][:len(t["residuals"])] and not t["failed"]
    t = run("estimator none")
    assert t["residuals"] == [1.0] * 5 and t["iter"] == 5
    t = run("bc_ok false twice, then true")
    assert codes(t["trace"]).count(BC_OK) == 3 and codes(t["trace"])[-2:] == [BC_OK, FINISH]
    lone = run("fresh, prescribed strain", LONE)
    assert all(r[1] == 1.0 for r in lone["trace"] if r[0] == WAIT)   # the lone wait enqueues the chain


def test_stand_alone_driver_under_the_sanitizers(tmp_path):
    """every combination of the switches on both sites, each way to stop, in a program of its own built with ASan + UBSan"""
    flags = [f for f in emulation_build_flags() if f not in ("-shared", "-fPIC") and not f.startswith("-O")]
    exe = str(tmp_path / "emu_basic_loop")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DFG_EMU_MAIN"] + flags +
                          ["-o", exe, SRC])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stdout.split() == ["OK", "8192"]

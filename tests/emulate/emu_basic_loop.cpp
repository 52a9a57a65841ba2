// C shim around fibergen_amd/csrc/fg_basic_loop.h for tests/test_basic_loop.py: the header is host code, so the very skeleton
// Solver::run_one_step and SlabGroup::run_step call runs here on a toy field of n values,
//   pass:  dev_i = 0.5 c_i eps_{i+1} - mean(0.5 c eps_{+1}),  eps'_i = E[0] + dev_i   (a contraction: residuals are real numbers)
// with the hooks of either site (site 0: the lone solver, 1: the group) doing on it what the real hooks do on the device.  Every
// call is recorded as eight doubles {code, a, E[0..5]}:
//   1 refresh_ref (E after) | 2 mixed_bc asked | 3 start_from E | 4 carry_pass E | 5 u_pass chain-now E | 6 strain_pass mixed E |
//   7 wait chain-enqueued-here | 8 mq_mean_tau | 9 norm | 10 estimator kind | 11 converged iter | 12 bc_ok | 13 adopt E_next |
//   14 deferred chain | 15 prepare | 16 F00 cleared | 17 finish iter failed
// With main(): the same scenarios run once more in a stand-alone program (built with the sanitizers by the test).
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../fibergen_amd/csrc/fg_basic_loop.h"

using namespace fg;

namespace {

struct Scenario {
  int site, fresh, u_space, have_u, mixed, update_ref, voting, estimator, leaves_u, bc_fail;
  long maxiter, nan_at, stop_at;
  double tol;
};

struct Toy {
  static constexpr int n = 5;
  const Scenario& sc;
  double eps[n], dev[n], ss = 0.0, tau = 0.0;
  bool have_u, chain_pending = false;
  MeanEstimator est;
  std::vector<double> trace, residuals;
  int bc_asked = 0;
  explicit Toy(const Scenario& s) : sc(s), have_u(s.have_u != 0) {
    for (int i = 0; i < n; ++i) eps[i] = s.fresh ? 0.0 : 0.3 + 0.1 * i, dev[i] = 0.0;
  }
  void rec(int code, double a = 0.0, const double* E = nullptr) {
    trace.push_back(code), trace.push_back(a);
    for (int c = 0; c < 6; ++c) trace.push_back(E ? E[c] : 0.0);
  }
  double sum() const {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += eps[i];
    return s;
  }
  double sumsq() const {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += eps[i] * eps[i];
    return s;
  }
  void sweep() {   // the fluctuation of the next field from the current one
    double t[n], m = 0.0;
    for (int i = 0; i < n; ++i) t[i] = 0.5 * (1.0 + 0.2 * i) * eps[(i + 1) % n];
    for (int i = 0; i < n; ++i) m += t[i];
    m /= n;
    for (int i = 0; i < n; ++i) dev[i] = t[i] - m;
  }
  void take(double mean) {
    for (int i = 0; i < n; ++i) eps[i] = mean + dev[i];
  }
  // what the estimator templates of fg_stop_rule.h ask of a site
  void mean_stress(double* m6) const {
    for (int c = 0; c < 6; ++c) m6[c] = sum() * (c + 1) / n;
  }
  double mean_energy() const { return sumsq() / n; }
  template <class F>
  void each_estimator(F f) { f(est); }
  bool converged(const StopRule& rule, long iter, const std::function<bool()>& bc_ok, bool* failed) {
    rec(11, (double)iter);
    const StopDecision d = rule.decide(iter, stop_hooks([&] { return iter == sc.stop_at; }, [&](double r) { residuals.push_back(r); },
                                                        [] { return StopPoll(); }, bc_ok));
    *failed = d == StopDecision::kFail;
    return d != StopDecision::kContinue;
  }
};

BasicResult run(Toy& q, const double* E0) {
  const Scenario& sc = q.sc;
  const double abs_tol = -1.0;
  const bool lone = sc.site == 0;
  if (lone) q.rec(16);
  bool mixed_before = false;
  if (lone) q.rec(2), mixed_before = sc.mixed != 0;
  StopRule rule(sc.tol, abs_tol, sc.maxiter, sc.estimator, sc.fresh ? 0.0 : std::sqrt(q.sumsq() / q.n));
  if (sc.estimator >= 2) estimator_begin(q, sc.estimator, sc.fresh != 0);
  long calls = 0;   // of norm: the iteration being measured
  BasicLoopOps ops;
  ops.refresh_ref = [&](double* E) {
    for (int c = 0; c < 6; ++c) E[c] = E0[c] + 0.01 * (c + 1);
    q.rec(1, 0, E);
    if (!lone && sc.u_space) q.rec(15);
  };
  ops.have_u = [&] { return q.have_u; };
  ops.mixed_bc = [&] {
    if (lone) return mixed_before;
    return q.rec(2), sc.mixed != 0;
  };
  ops.start_from = [&](const double* E) { q.rec(3, 0, E), q.take(E[0]); };
  ops.carry_pass = [&](const double* E) { q.rec(4, 0, E), q.sweep(), q.take(E[0]); };
  ops.u_pass = [&](const double* E, bool mixed) {
    const bool now = !lone && !sc.voting;   // the lone solver enqueues the chain behind the copies of its wait
    q.rec(5, now, E);
    q.ss = q.sumsq();
    if (mixed) q.tau = 0.25 * q.sum() / q.n;
    q.sweep();
    q.chain_pending = !now;
  };
  ops.strain_pass = [&](const double* E, bool mixed) {
    q.rec(6, mixed, E);
    const double shift = mixed ? 0.3 * (0.25 * q.sum() / q.n) : 0.0;
    q.sweep(), q.take(E[0] - shift);
    q.ss = q.sumsq();
    q.have_u = sc.leaves_u && !mixed;
  };
  ops.wait = [&] {
    q.rec(7, lone && q.chain_pending);
    if (lone) q.chain_pending = false;
  };
  ops.mq_mean_tau = [&](double* t6) {
    q.rec(8);
    for (int c = 0; c < 6; ++c) t6[c] = c == 0 ? 0.3 * q.tau : 0.0;
  };
  ops.norm = [&] {
    q.rec(9);
    return ++calls == sc.nan_at ? std::numeric_limits<double>::quiet_NaN() : std::sqrt(q.ss / q.n);
  };
  ops.estimator = [&](StopRule& r) {
    q.rec(10, sc.estimator);
    if (sc.estimator >= 2) estimator_update(q, sc.estimator, &r.abs_err, &r.rel_err);
  };
  ops.bc_ok = [&] { return q.rec(12), ++q.bc_asked > sc.bc_fail; };
  ops.adopt = [&](const double* E_next) {
    if (q.chain_pending) q.rec(14), q.chain_pending = false;
    q.rec(13, 0, E_next), q.take(E_next[0]), q.have_u = true;
  };
  const BasicResult end = basic_loop(q, ops, rule, E0, sc.fresh != 0, sc.u_space != 0, sc.update_ref != 0);
  q.rec(17, (double)end.iter, nullptr), q.trace[q.trace.size() - 6] = end.failed;
  return end;
}

}  // namespace

extern "C" {

// ints: site fresh u_space have_u mixed update_ref voting estimator leaves_u bc_fail; longs: maxiter nan_at stop_at.
// Returns the trace length (doubles), -1 if it does not fit; out: [0] iter, [1] failed, [2] residuals recorded, then the field.
int emu_basic_loop(const int* ints, const long* longs, double tol, const double* E0, double* trace, int cap, double* residuals,
                   double* out) {
  const Scenario sc{ints[0], ints[1], ints[2], ints[3], ints[4], ints[5], ints[6], ints[7], ints[8], ints[9],
                    longs[0], longs[1], longs[2], tol};
  Toy q(sc);
  const BasicResult end = run(q, E0);
  if ((int)q.trace.size() > cap) return -1;
  for (size_t i = 0; i < q.trace.size(); ++i) trace[i] = q.trace[i];
  for (size_t i = 0; i < q.residuals.size(); ++i) residuals[i] = q.residuals[i];
  out[0] = (double)end.iter, out[1] = end.failed, out[2] = (double)q.residuals.size();
  for (int i = 0; i < Toy::n; ++i) out[3 + i] = q.eps[i];
  return (int)q.trace.size();
}

}  // extern "C"

#ifdef FG_EMU_MAIN
// every combination of the switches on both sites, with each way to stop: prints one line per run (iter failed trace-length)
int main() {
  const double E0[6] = {0.5, -0.2, 0.1, 0.05, -0.1, 0.3};
  long runs = 0;
  for (int bits = 0; bits < 512; ++bits)
    for (int est : {0, 2, 3, 4})
      for (int end = 0; end < 4; ++end) {
        Scenario sc{bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1, (bits >> 4) & 1, (bits >> 5) & 1, (bits >> 6) & 1,
                    est, (bits >> 7) & 1, (bits >> 8) & 1, end == 1 ? 3 : 40, end == 2 ? 3 : -1, end == 3 ? 2 : -1, 1e-6};
        Toy q(sc);
        const BasicResult r = run(q, E0);
        if (r.iter < 1 || r.iter > sc.maxiter || q.trace.size() % 8 != 0) return std::printf("FAIL %d %d %d\n", bits, est, end), 1;
        ++runs;
      }
  std::printf("OK %ld\n", runs);
  return 0;
}
#endif

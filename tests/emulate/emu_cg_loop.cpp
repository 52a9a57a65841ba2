// C shim around fibergen_amd/csrc/fg_cg_loop.h for tests/test_cg_loop.py: the header is host code, so the very skeleton
// the pipelined CG loops call runs here on host vectors.  The problem is A x = b with a dense symmetric positive definite A of
// order n, the operator written like the solver's: w = G p with G = I - A, so that p - w = A p.  The "device" slots of the
// pipelined form are a host array.  Every operation call is recorded as four ints {code, a, b, c}:
//   1 apply_p | 2 apply_dir num den | 3 direction num den | 4 dot_pw out | 5 update gamma pw out | 6 fetch slot |
//   7 cg_may_run_ahead | 8 sums | 9 estimator | 10 converged iter | 13 cg_wait | 14 bc_ok
#include <vector>

#include "../../fibergen_amd/csrc/fg_cg_loop.h"

using namespace fg;

namespace {

struct Problem {
  int n;
  const double* A;
  std::vector<double> x, r, p, w;
  double nvox, tiny = std::numeric_limits<double>::min();
  int *trace, cap, len = 0;
  double *alphas, *betas;
  int na = 0, nb = 0;
  Problem(int n_, const double* A_, const double* b, int* trace_, int cap_, double* alphas_, double* betas_)
      : n(n_), A(A_), x(n_, 0.0), r(b, b + n_), p(b, b + n_), w(n_, 0.0), nvox((double)n_), trace(trace_), cap(cap_),
        alphas(alphas_), betas(betas_) {}
  void rec(int code, int a = 0, int b = 0, int c = 0) {
    if (len + 4 <= cap) trace[len] = code, trace[len + 1] = a, trace[len + 2] = b, trace[len + 3] = c;
    len += 4;
  }
  void apply() {   // w = p - A p
    for (int i = 0; i < n; ++i) {
      double s = 0.0;
      for (int j = 0; j < n; ++j) s += A[i * n + j] * p[j];
      w[i] = p[i] - s;
    }
  }
  double pw() const {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += p[i] * (p[i] - w[i]);
    return s;
  }
  double rr() const {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += r[i] * r[i];
    return s;
  }
  double xx() const {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += x[i] * x[i];
    return s;
  }
  void axpy_x(double alpha) {
    alphas[na++] = alpha;
    for (int i = 0; i < n; ++i) x[i] += alpha * p[i];
  }
  void axpy_r(double alpha) {
    for (int i = 0; i < n; ++i) r[i] -= alpha * (p[i] - w[i]);
  }
  void dir(double beta) {
    betas[nb++] = beta;
    for (int i = 0; i < n; ++i) p[i] = r[i] + beta * p[i];
  }
};

// the class side of the skeleton: the shim's "device" d, its "host" copy h, and the real stop rule with a failure scripted
// at iteration fail_at
struct Site {
  Problem& q;
  double *d, *h;
  bool run_ahead;
  long fail_at;
  void cg_fetch(int from) {
    q.rec(6, from);
    for (int c = 0; c < 7; ++c) h[c] = d[from + c];
  }
  void cg_wait() { q.rec(13); }
  bool cg_may_run_ahead() { return q.rec(7), run_ahead; }
  bool converged(const StopRule& rule, long iter, const std::function<bool()>& bc_ok, bool* failed) {
    q.rec(10, (int)iter);
    if (iter == fail_at) {
      *failed = true;
      return true;
    }
    const StopDecision dec = rule.decide(iter, stop_hooks([] { return false; }, [](double) {}, [] { return StopPoll(); }, bc_ok));
    *failed = dec == StopDecision::kFail;
    return dec != StopDecision::kContinue;
  }
};

}  // namespace

extern "C" {

// Returns the loop counter at the end.  out: [0] failed, [1] trace length (ints), [2] alphas, [3] betas recorded.
long emu_cg_pipelined(int n, const double* A, const double* b, double tol, long maxiter, int first_slot, int fused_dir,
                      int run_ahead, long fail_at, double* x, int* trace, int cap, double* alphas, double* betas, int* out) {
  Problem q(n, A, b, trace, cap, alphas, betas);
  const double abs_tol = -1.0;
  double d[64] = {0}, h[7] = {0};
  const CgSlots slot = cg_slots(first_slot);
  d[slot.rr(0)] = q.rr();
  StopRule rule(tol, abs_tol, maxiter, 0, 0.0);
  auto beta = [&](int num, int den) { return (d[num] / q.nvox + q.tiny) / (d[den] / q.nvox + q.tiny); };
  CgPipelinedOps ops;
  ops.fused_dir = fused_dir != 0;
  ops.apply_p = [&] { q.rec(1), q.apply(); };
  ops.apply_dir = [&](int num, int den) { q.rec(2, num, den), q.dir(beta(num, den)), q.apply(); };
  ops.direction = [&](int num, int den) { q.rec(3, num, den), q.dir(beta(num, den)); };
  ops.dot_pw = [&](int o) { q.rec(4, o), d[o] = q.pw(); };
  ops.update = [&](int gamma, int pw, int o) {
    q.rec(5, gamma, pw, o);
    const double alpha = (d[gamma] / q.nvox + q.tiny) / (d[pw] / q.nvox + q.tiny);
    q.axpy_x(alpha), q.axpy_r(alpha);
    for (int c = 0; c < 6; ++c) d[o + c] = c == 0 ? q.xx() : 0.0;
    d[o + 6] = q.rr();
  };
  ops.sums = [&] { return q.rec(8), CgSums{std::sqrt(h[0] / q.nvox), h[6]}; };
  ops.estimator = [&](StopRule&) { q.rec(9); };
  ops.bc_ok = [&] { return q.rec(14), true; };
  Site site{q, d, h, run_ahead != 0, fail_at};
  const CgResult end = cg_pipelined(site, ops, rule, slot, q.nvox);
  for (int i = 0; i < n; ++i) x[i] = q.x[i];
  out[0] = end.failed, out[1] = q.len, out[2] = q.na, out[3] = q.nb;
  return end.iter;
}

}  // extern "C"

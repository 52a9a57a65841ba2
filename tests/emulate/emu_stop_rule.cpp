// C shim around fibergen_amd/csrc/fg_stop_rule.h for tests/test_stop_rule.py: the header is host code, so the very
// functions the solver loops call run here on scripted sequences.
#include "../../fibergen_amd/csrc/fg_stop_rule.h"

using namespace fg;

extern "C" {

double emu_norm9_of_sums(const double* sumsq6, double nglobal) { return norm9_of_sums(sumsq6, nglobal); }
double emu_norm3_of_sums(const double* sumsq3, double nglobal) { return norm3_of_sums(sumsq3, nglobal); }

// One load step of n scripted iterations (iteration i runs with loop counter iter0 + i), ended by the first decision that is
// not "continue".  Per iteration: cur[i], gamma_next[i] (the r:r-based gamma after the update; ignored unless use_gamma),
// stop_req[i] (stop_requested()'s answer), cb[i] (bit 0: the callback asks to stop, bit 1: cancel raised inside it),
// bc[i] (bc_ok()'s answer).  group != 0: poll() goes through agree_poll with a fake vote that adds remote[i] (same bits: what
// the other ranks contribute).  Returns the number of iterations run; decision: 0 continue, 1 stop, 2 fail.
// counts: [0] record calls, [1] poll calls, [2] bc_ok calls, [3] vote calls.
int emu_stop_run(double tol, double abs_tol, long maxiter, int estimator, double prev0, double gamma0, int use_gamma, int n,
                 long iter0, const double* cur, const double* gamma_next, const int* stop_req, const int* cb, const int* bc,
                 int group, int nranks, int voting, const int* remote, double* abs_err, double* rel_err, int* decision,
                 double* recorded, int* counts) {
  StopRule rule(tol, abs_tol, maxiter, estimator, prev0, gamma0);
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  for (int i = 0; i < n; ++i) {
    if (use_gamma) rule.measure(cur[i], gamma_next[i]);
    else rule.measure(cur[i]);
    abs_err[i] = rule.abs_err;
    rel_err[i] = rule.rel_err;
    const StopDecision d = rule.decide(iter0 + i, stop_hooks([&] { return stop_req[i] != 0; },
                                                             [&](double r) { recorded[counts[0]++] = r; },
                                                             [&] {
                                                               ++counts[1];
                                                               StopPoll p;
                                                               p.stop = (cb[i] & 1) != 0;
                                                               p.cancelled = (cb[i] & 2) != 0;
                                                               if (!group) return p;
                                                               return agree_poll(p, nranks, voting != 0, [&](double* v) {
                                                                 ++counts[3];
                                                                 v[0] += (remote[i] & 1) ? 1.0 : 0.0;
                                                                 v[1] += (remote[i] & 2) ? 1.0 : 0.0;
                                                               });
                                                             },
                                                             [&] {
                                                               ++counts[2];
                                                               return bc[i] != 0;
                                                             }));
    decision[i] = d == StopDecision::kContinue ? 0 : d == StopDecision::kStop ? 1 : 2;
    if (d != StopDecision::kContinue) return i + 1;
  }
  return n;
}

// MeanEstimator: started on m0 / w0, then n updates
void emu_sigma(int n, const double* m0, const double* m, double* abs_err, double* rel_err) {
  MeanEstimator e;
  e.start_sigma(m0);
  for (int i = 0; i < n; ++i) e.update_sigma(m + 6 * i, abs_err + i, rel_err + i);
}

void emu_energy(int n, double w0, const double* w, double* abs_err, double* rel_err) {
  MeanEstimator e;
  e.start_energy(w0);
  for (int i = 0; i < n; ++i) e.update_energy(w[i], abs_err + i, rel_err + i);
}

}  // extern "C"

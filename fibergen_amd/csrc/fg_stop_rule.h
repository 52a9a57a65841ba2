// The convergence test every solver loop ends its iteration with: the measurement of EpsilonErrorEstimator F:14591-14637 or
// ResidualErrorEstimator F:14382-14405 followed by _converged F:21177-21244.  Host code without any HIP in it, shared by the
// loops of Solver (fg_solver.hip) and SlabGroup (fg_slab.hip) and driven on its own by tests/test_stop_rule.py.
#pragma once

#include <cmath>
#include <limits>

namespace fg {

// component_norm + fix_dim + norm_2 over the 9 mirrored entries (F:10127-10138, F:14600-14609, F:14627) from the six sums
// of squares of the strain field: m_c = sqrt(ss_c / N), all six m_c^2, then the three shear terms once more
inline double norm9_of_sums(const double* sumsq6, double nglobal) {
  double m[6], s9 = 0.0;
  for (int c = 0; c < 6; ++c) m[c] = std::sqrt(sumsq6[c] / nglobal);
  for (int c = 0; c < 6; ++c) s9 += m[c] * m[c];
  for (int c = 3; c < 6; ++c) s9 += m[c] * m[c];
  return std::sqrt(s9);
}

// the scalar modes' sibling (three gradient components, nothing to mirror)
inline double norm3_of_sums(const double* sumsq3, double nglobal) {
  double s3 = 0.0;
  for (int c = 0; c < 3; ++c) {
    const double m = std::sqrt(sumsq3[c] / nglobal);
    s3 += m * m;
  }
  return std::sqrt(s3);
}

// The error estimators that re-measure a mean of the strain field every iteration (create_error_estimator F:14940-14972):
// SigmaErrorEstimator F:14514-14587 (created with _mode = 2: from its third update on, the mean of the distances to the
// last two mean stresses), EnergyErrorEstimator F:14410-14468, NoneErrorEstimator F:14370-14378 (always 1).  The solver
// (one GPU or the slab group) supplies the measurement; norm_2 runs over the 9 mirrored entries (fix_dim).
struct MeanEstimator {
  double m_prev[6] = {0, 0, 0, 0, 0, 0}, m_pp[6] = {0, 0, 0, 0, 0, 0}, w_prev = 0.0;
  long iter = 0;
  static double norm9_diff(const double* a, const double* b) {
    double s = 0.0;
    for (int c = 0; c < 6; ++c) s += (a[c] - b[c]) * (a[c] - b[c]) * (c >= 3 ? 2.0 : 1.0);
    return std::sqrt(s);
  }
  void start_sigma(const double* m) {
    for (int c = 0; c < 6; ++c) m_prev[c] = m_pp[c] = m[c];
    iter = 0;
  }
  void update_sigma(const double* m, double* abs_err, double* rel_err) {
    const double zero[6] = {0, 0, 0, 0, 0, 0};
    *abs_err = iter > 1 ? 0.5 * (norm9_diff(m_pp, m) + norm9_diff(m_prev, m)) : norm9_diff(m_prev, m);
    *rel_err = *abs_err / (std::numeric_limits<double>::min() + norm9_diff(m, zero));
    for (int c = 0; c < 6; ++c) m_pp[c] = m_prev[c], m_prev[c] = m[c];
    ++iter;
  }
  void start_energy(double w) { w_prev = w, iter = 0; }
  void update_energy(double w, double* abs_err, double* rel_err) {
    *abs_err = std::fabs(w_prev - w);
    *rel_err = *abs_err / (std::numeric_limits<double>::min() + std::fabs(w));
    w_prev = w;
    ++iter;
  }
};

// create_error_estimator  F:14940-14972 for these estimators, on a site (Solver, SlabGroup) that supplies mean_stress(m6),
// mean_energy() and each_estimator(f), which applies f to its estimator (the group: to every member's; all hold the same
// all-reduced means).  Their constructors run on the field the step starts from (zero for a first step: <sigma> = 0, <W> = 0),
// update() after every iteration.
template <class Site>
void estimator_begin(Site& site, int error_estimator, bool fresh) {
  if (error_estimator == 2) {
    double m[6] = {0, 0, 0, 0, 0, 0};
    if (!fresh) site.mean_stress(m);
    site.each_estimator([&](MeanEstimator& e) { e.start_sigma(m); });
  } else if (error_estimator == 3) {
    const double w = fresh ? 0.0 : site.mean_energy();
    site.each_estimator([&](MeanEstimator& e) { e.start_energy(w); });
  }
}

template <class Site>
void estimator_update(Site& site, int error_estimator, double* abs_err, double* rel_err) {
  if (error_estimator == 2) {
    double m[6];
    site.mean_stress(m);
    site.each_estimator([&](MeanEstimator& e) { e.update_sigma(m, abs_err, rel_err); });
  } else if (error_estimator == 3) {
    const double w = site.mean_energy();
    site.each_estimator([&](MeanEstimator& e) { e.update_energy(w, abs_err, rel_err); });
  } else if (error_estimator == 4) {
    *abs_err = *rel_err = 1.0;
  }
}

enum class StopDecision { kContinue, kStop, kFail };

// what the callbacks answered after an iteration
struct StopPoll {
  bool stop = false;        // a callback asked to stop: the run ends as a success
  bool cancelled = false;   // fg_cancel was called (from inside a callback or from another thread): the run fails
};

// What differs between a lone solver and a group of slabs, as four callables:
//   bool stop_requested()    a stop was asked for before this iteration's residual is recorded
//   void record(double)      the residual joins the history
//   StopPoll poll()          the convergence callbacks, then the cancel flag once more
//   bool bc_ok()             bc_error F:21129-21161 within its tolerance; called only when a tolerance is met, after maxiter
template <class StopRequested, class Record, class Poll, class BcOk>
struct StopHooks {
  StopRequested stop_requested;
  Record record;
  Poll poll;
  BcOk bc_ok;
};

template <class StopRequested, class Record, class Poll, class BcOk>
StopHooks<StopRequested, Record, Poll, BcOk> stop_hooks(StopRequested a, Record b, Poll c, BcOk d) {
  return {a, b, c, d};
}

// The group's part of poll(): the answers of this process' members are agreed over the ranks when the run votes (vote(v2)
// replaces two host values by their sums over the ranks).  Without a vote an asynchronous fg_cancel on one of several ranks
// is not acted upon here -- it travels with the flag word of the next reduction, so that every rank sees it.
template <class Vote>
StopPoll agree_poll(StopPoll local, int nranks, bool voting, Vote vote) {
  if (voting) {
    double v[2] = {local.stop ? 1.0 : 0.0, local.cancelled ? 1.0 : 0.0};
    vote(v);
    local.stop = v[0] != 0.0;
    local.cancelled = v[1] != 0.0;
  }
  if (nranks > 1 && !voting) local.cancelled = false;
  return local;
}

// State of the stop rule over one load step.  prev0: norm of the field the step starts from (the estimators are constructed
// on it); gamma_0: r:r / N + tiny at the start of CG (read under the residual estimator only).  The limits are the caller's
// options themselves (references, they must outlive the rule): they are read when a decision is taken, so a convergence
// callback that changes them is heard in the same iteration.
struct StopRule {
  const double &tol, &abs_tol;
  const long& maxiter;
  bool residual;   // error_estimator 1: update_cg(gamma, gamma_0)  F:14397-14401
  double prev, gamma_cur, gamma_0;
  double abs_err = 0.0, rel_err = 0.0;

  StopRule(const double& tol_, const double& abs_tol_, const long& maxiter_, int error_estimator, double prev0, double gamma0 = 0.0)
      : tol(tol_), abs_tol(abs_tol_), maxiter(maxiter_), residual(error_estimator == 1), prev(prev0), gamma_cur(gamma0),
        gamma_0(gamma0) {}

  // cur: norm of the strain field after this iteration.  The residual estimator reports the gamma the iteration started from.
  void measure(double cur) {
    abs_err = std::fabs(prev - cur);
    rel_err = abs_err / (std::numeric_limits<double>::min() + cur);
    prev = cur;
    if (residual) {
      abs_err = std::sqrt(gamma_cur);
      rel_err = std::sqrt(gamma_cur / gamma_0);
    }
  }
  // loops that know r:r after the update at this point: gamma_next = r:r / N + tiny is what the next iteration starts from
  void measure(double cur, double gamma_next) {
    measure(cur);
    gamma_cur = gamma_next;
  }

  // _converged  F:21177-21244 on (abs_err, rel_err) -- the loop may have replaced them (estimators 2 to 4) in between
  template <class Hooks>
  StopDecision decide(long iter, Hooks&& h) const {
    if (std::isnan(rel_err)) return StopDecision::kFail;   // "NaN detected in solution. Aborting."
    if (h.stop_requested()) return StopDecision::kFail;
    h.record(rel_err);
    const StopPoll p = h.poll();
    if (p.stop) return StopDecision::kStop;
    if (p.cancelled) return StopDecision::kFail;
    if (iter >= maxiter) return StopDecision::kStop;
    if ((rel_err <= tol || abs_err <= abs_tol) && h.bc_ok()) return StopDecision::kStop;
    return StopDecision::kContinue;
  }
};

}  // namespace fg

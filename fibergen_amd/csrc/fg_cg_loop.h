// The pipelined iteration of runCGElasticity F:23153-23247 (alpha and beta formed on the device, the next operator application
// enqueued before the host waits) as five conjugate-gradient loops of Solver (fg_solver.hip) and SlabGroup (fg_slab.hip) run it,
// written once: the skeleton owns the counters, the slots and the order of the calls; what a site does in a call it assigns to
// a named hook, and what is the same for every loop of a class it takes from the class (DESIGN.md has the table).  Host code
// without any HIP in it, like fg_stop_rule.h, and driven on its own by tests/test_cg_loop.py.
#pragma once

#include <cmath>
#include <functional>
#include <limits>

#include "fg_stop_rule.h"

namespace fg {

struct CgResult {
  long iter;   // the counter the loop ended with (the iterations are counted from 0)
  bool failed;
};
struct CgSums {
  double norm, rr;   // norm of the iterate for the stop rule; r:r after the update
};

// Device slots of the pipelined form, from the solver's first CG slot: two blocks of 8 that alternate per iteration (the six
// sums of squares of the iterate, then r:r), and p:(p - w).  gamma of iteration k is rr(k & 1), its update leaves delta in
// rr(~k & 1).
struct CgSlots {
  int blk[2], pw;
  int rr(int b) const { return blk[b] + 6; }
};
constexpr CgSlots cg_slots(int first) { return CgSlots{{first, first + 8}, first + 16}; }

// Slot arguments are device slots; alpha and beta are quotients of the sums there, each as sum / N + tiny.
// Before the call: p = r, r:r in slot.rr(0), rule.gamma_0 set where the residual estimator reads it.
struct CgPipelinedOps {
  bool fused_dir = false;                             // the direction is formed inside the operator's sweep, not point-wise
  std::function<void()> apply_p;                      // w = operator(p)
  std::function<void(int num, int den)> apply_dir;    // fused_dir: p = r + beta p inside the sweep, then w = operator(p)
  std::function<void(int num, int den)> direction;    // otherwise: p = r + beta p, point-wise
  std::function<void(int out)> dot_pw;                // p:(p - w) -> out
  std::function<void(int gamma, int pw, int out)> update;   // x += alpha p, r -= alpha (p - w); the seven sums -> out .. out + 6
  std::function<CgSums()> sums;                       // the seven sums have arrived: state for the accessors, sumsq_, the norm
  std::function<void(StopRule&)> estimator;           // optional: the estimators that replace the rule's measurement
  std::function<bool()> bc_ok;                        // the stop rule's last question (may have to bring the iterate home first)
};

// Site (Solver, SlabGroup) supplies what all its loops share: cg_fetch(slot) starts the copy of the seven sums and the error
// words to the host, cg_wait() waits for it and throws on a device error, cg_may_run_ahead() says that nothing looks at the
// state between two iterations (no callback, no vote), converged(rule, iter, bc_ok, &failed) is its side of the stop rule.
template <class Site>
CgResult cg_pipelined(Site& site, const CgPipelinedOps& ops, StopRule& rule, const CgSlots& slot, double nvox) {
  const double tiny = std::numeric_limits<double>::min();
  long iter = 0;
  bool failed = false;
  bool applied = false;           // w = operator(p) of the coming iteration is already enqueued
  int dir_num = 0, dir_den = 0;   // fused_dir: slots of the direction the next operator application forms
  for (;;) {
    const int cur = (int)(iter & 1), nxt = cur ^ 1;
    if (!applied) {
      if (ops.fused_dir && iter > 0) ops.apply_dir(dir_num, dir_den);
      else ops.apply_p();   // (the first iteration: p = r)
    }
    applied = false;
    ops.dot_pw(slot.pw);
    ops.update(slot.rr(cur), slot.pw, slot.blk[nxt]);
    site.cg_fetch(slot.blk[nxt]);
    if (site.cg_may_run_ahead() && iter < rule.maxiter) {   // enqueued behind the copies
      if (ops.fused_dir) {
        ops.apply_dir(slot.rr(nxt), slot.rr(cur));
      } else {
        ops.direction(slot.rr(nxt), slot.rr(cur));
        ops.apply_p();
      }
      applied = true;
    }
    site.cg_wait();
    const CgSums s = ops.sums();
    rule.measure(s.norm, s.rr / nvox + tiny);   // delta = r:r after the update is the next gamma
    if (ops.estimator) ops.estimator(rule);
    if (site.converged(rule, iter, ops.bc_ok, &failed)) break;
    iter++;
    if (!applied) {
      if (ops.fused_dir) dir_num = slot.rr(nxt), dir_den = slot.rr(cur);
      else ops.direction(slot.rr(nxt), slot.rr(cur));
    }
  }
  return {iter, failed};
}

}  // namespace fg

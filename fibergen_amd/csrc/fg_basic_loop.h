// The iteration of runBasic F:21716-21805 for one load step as Solver::run_one_step (fg_solver.hip) and SlabGroup::run_step
// (fg_slab.hip) run it -- in displacement space where the configuration allows it, with the transform chain enqueued before the
// host has seen the norms --, written once: the skeleton owns the counter, the flags and the prescribed mean of the pass and of
// the next one, the order of the calls and the break; what a site does in a call it assigns to a named hook, and its side of the
// stop rule the skeleton takes from the class (DESIGN.md has the table).  Host code without any HIP in it, like fg_cg_loop.h,
// and driven on its own by tests/test_basic_loop.py.
#pragma once

#include <functional>

#include "fg_stop_rule.h"

namespace fg {

struct BasicResult {
  long iter;   // the counter the loop ended with (the iterations are counted from 1)
  bool failed;
};

// E is the prescribed mean strain of the pass, six values the skeleton owns.  Before the call: the state of the step (a fresh
// step: u = 0), rule constructed on the field the step starts from.
struct BasicLoopOps {
  std::function<void(double* E)> refresh_ref;   // update_ref: calcRefMaterial, then E = calcBCMean; before the first pass only
  std::function<bool()> have_u;                 // every member holds the displacement of its state (no side effect)
  std::function<bool()> mixed_bc;               // asked once per iteration, behind refresh_ref; the moment it is read is the site's
  std::function<void(const double* E)> start_from;    // first iteration of a fresh step: eps_1 = E (u_1 = 0)
  std::function<void(const double* E)> carry_pass;    // u -> u' with eps' = E + sym grad u', adopted, nothing measured
  std::function<void(const double* E, bool mixed_bc)> u_pass;        // norms of eps_k (mixed_bc: + sums of tau_k), chain to u_{k+1}
  std::function<void(const double* E, bool mixed_bc)> strain_pass;   // eps_k -> eps_{k+1}, adopted; may leave a displacement
  std::function<void()> wait;                          // the sums of the pass have reached the host; throws on a device error
  std::function<void(double* t6)> mq_mean_tau;         // MQ:<tau_k> of the displacement pass waited for
  std::function<double()> norm;                        // the norm of eps_k from the sums of squares (which become sumsq_)
  std::function<void(StopRule&)> estimator;            // the estimators that replace the rule's measurement, where one is chosen
  std::function<bool()> bc_ok;                         // the stop rule's last question
  std::function<void(const double* E_next)> adopt;     // u_{k+1} (chain enqueued now if it was deferred) becomes the state
};

// Site (Solver, SlabGroup) supplies converged(rule, iter, bc_ok, &failed), its side of the stop rule.  fresh: the step starts
// from the zero field; u_space: the configuration has a displacement loop (it is left for the step where a pass needs <tau> or
// leaves no displacement).
template <class Site>
BasicResult basic_loop(Site& site, const BasicLoopOps& ops, StopRule& rule, const double* E0, bool fresh, bool u_space,
                       bool update_ref) {
  long iter = 1;
  bool failed = false;
  // a continuing load step in the displacement loop: the state is u of the previous step (eps = E_old + sym grad u); one
  // unrecorded pass turns it into u' with eps' = E_new + sym grad u' -- the field the reference's first iteration of the step
  // produces -- and the loop then measures eps' in its first pass
  bool carry = u_space && !fresh && ops.have_u();
  double E[6], E_next[6];
  for (int i = 0; i < 6; ++i) E[i] = E0[i];
  for (;;) {
    if (update_ref) {
      ops.refresh_ref(E);
      update_ref = false;
    }
    const bool mixed_bc = ops.mixed_bc();
    if (carry) {
      carry = false;
      if (mixed_bc) u_space = false;   // the correction of the prescribed mean needs <tau> of the old field: strain-state passes
      else ops.carry_pass(E);
    }
    bool pending = false;
    if (u_space && ops.have_u()) {
      if (iter == 1 && fresh) ops.start_from(E);
      ops.u_pass(E, mixed_bc);
      pending = true;
    } else {
      // no displacement behind the strain field (a step that starts from a given / extrapolated field, mixed boundary
      // conditions with their correction term in the strain): strain-state pass.  If it leaves a displacement, the loop goes
      // on in displacement space after the unrecorded pass of a continuing state (carry).
      ops.strain_pass(E, mixed_bc);
      if (u_space && !mixed_bc && ops.have_u()) carry = true;
      else u_space = false;
    }
    ops.wait();
    for (int c = 0; c < 6; ++c) E_next[c] = E[c];
    if (pending && mixed_bc) {
      // applyBCProjector  F:20247-20270 with bc_relax = 1: eps_{k+1} = E + alpha MQ:<tau_k> + sym grad u_{k+1}
      double t[6];
      ops.mq_mean_tau(t);
      for (int c = 0; c < 6; ++c) E_next[c] = E[c] - t[c];   // alpha = -1  (F:20575)
    }
    rule.measure(ops.norm());
    ops.estimator(rule);   // sigma / energy / none: F:14410-14587
    if (site.converged(rule, iter, ops.bc_ok, &failed)) break;
    if (pending) ops.adopt(E_next);
    iter++;
  }
  return {iter, failed};
}

}  // namespace fg

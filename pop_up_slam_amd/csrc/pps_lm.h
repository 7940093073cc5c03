// pps_lm.h -- the Levenberg-Marquardt rule of Optimizer::levenberg_marquardt (Thirdparty/isam/isamlib/Optimizer.cpp:371-467), once.
// Host only, no HIP: the three host loops (lm_solve, lm_solve_dual: pps_solve.cpp; the rounds of pps_multi.cpp) decide WHEN a trial's
// chi2 is on the host and what to launch next; what a chi2 means -- accept / reject / stop, the lambda schedule, the trace, the trial
// counters, the not-PD report -- is here (LmControl), and so is the scheme lm_solve_dual and the batched rounds share (LmDualWalk): the walk
// over the two records of a launch set that solved the step for lambda and for lambda * factor, and the rotation of the three state copies
// that an accepted trial causes.  tests/test_host_lm.py replays recorded trajectories through both without a device.
#pragma once
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../include/pps.h"

namespace pps_impl {

// what the rule writes besides its own state (a handle's properties, LM trace and stats record), gathered once per solve
struct LmSink {
  const pps_props* prop;
  std::vector<double>*tr_lambda, *tr_chi2;
  std::vector<int>* tr_acc;
  pps_stats* stats;
  bool verbose;                  // the "LM Iteration" line per trial (the batched rounds print none)
};

enum class LmVerdict { Rejected, Accepted, Converged };

constexpr const char* kLmNotPdMessage = "normal equations not positive definite at the last LM trial";

struct LmControl {
  double lambda, error = 0.0, dnorm = 0.0;      // error: chi2 at the linearisation point; dnorm: |delta| of the trial judged next
  int num_iter = 0;
  // Not-PD is a property of ONE factorisation (one lambda): every result record carries the flag of the solve that produced
  // its step, and the chi2 kernel clears it.  CHOLMOD is silent here and LM simply rejects such a step and raises lambda
  // (Optimizer.cpp:448-455), so only a solve whose LAST trial was still not PD reports PPS_ENOTPD.
  bool last_notpd = false;
  int n_notpd = 0;

  explicit LmControl(const pps_props& p) : lambda(p.lm_lambda0) {}

  // the loop condition (:398)
  bool running(const pps_props& p) const { return (p.max_iterations <= 0 || num_iter < p.max_iterations) && dnorm > p.epsilon2 && error > p.epsilon_abs; }

  // a trial's result record (chi2, |delta|^2, status word) is on the host: the step it stands for is the one judged next
  void take_step(const double* rec) {
    dnorm = std::sqrt(rec[1]);
    last_notpd = rec[2] != 0.0;
    n_notpd += last_notpd ? 1 : 0;
  }

  // One pass of the loop body (:400-456) for the trial whose chi2 is error_new, in two halves.  decide() is the rule -- verdict, lambda
  // schedule, the new error -- and touches nothing but this object; note() is what the trial leaves behind (trace, counters, the verbose
  // line) and needs nothing the rule changes: a loop that has a launch waiting for the verdict calls decide(), launches, then note().
  struct Trial { double lambda, chi2; int iter; bool accepted; };      // a judged trial as note() records it
  __attribute__((always_inline)) LmVerdict decide(const pps_props& p, double error_new, Trial* t) {
    num_iter++;
    const double error_diff = error - error_new;
    const bool accepted = error_diff > 0.;
    *t = Trial{lambda, error_new, num_iter, accepted};
    if (!accepted) {
      lambda *= p.lm_lambda_factor;                              // (:452)
      return LmVerdict::Rejected;
    }
    const bool converged = error_diff < p.epsilon_rel * error;   // (:431-434) against the chi2 the step started from
    error = error_new;
    if (converged) return LmVerdict::Converged;
    lambda /= p.lm_lambda_factor;                                // (:438)
    return LmVerdict::Accepted;
  }
  static void note(const LmSink& s, const Trial& t) {
    s.tr_lambda->push_back(t.lambda); s.tr_chi2->push_back(t.chi2); s.tr_acc->push_back(t.accepted ? 1 : 0);
    if (s.verbose) fprintf(stderr, "LM Iteration %d: (lambda=%g) %s %.12g\n", t.iter, t.lambda, t.accepted ? "residual:" : "rejected", t.chi2);
    if (t.accepted) s.stats->lm_trials_accepted++; else s.stats->lm_trials_rejected++;
  }
  // both halves at once (the one-step loop, the batched rounds, tests/cpp/lm_host.cpp).  Forced inline: with its three push_backs the compiler
  // otherwise emits it out of line, a call per trial between a record's arrival and the next launch that the loops did not have before
  __attribute__((always_inline)) LmVerdict judge(const LmSink& s, double error_new) {
    Trial t;
    const LmVerdict v = decide(*s.prop, error_new, &t);
    note(s, t);
    return v;
  }

  // the solve is over: its figures -> stats; PPS_ENOTPD (the caller sets kLmNotPdMessage on its handle) when the last trial was not PD
  int finish(const LmSink& s, int* iterations) const {
    pps_stats& st = *s.stats;
    st.lm_iterations = num_iter;
    st.chi2_final = error; st.lambda_final = lambda; st.last_delta_norm = dnorm;
    st.lm_trials_notpd = n_notpd;
    if (iterations) *iterations = num_iter;
    return last_notpd ? PPS_ENOTPD : PPS_OK;
  }
};

// The dual-trial walk.  A launch set solves the step for lambda (record 0) and, when it carries two trials, for lambda * factor (record 1):
// the step LM asks for next if it rejects the first.  One object per graph: the rule, which record is judged next, whether record 1 is such
// a step, whether the solve ended on an accepted, converged trial -- and x, the place of the linearisation point among the three copies of
// the state.  The copies rotate by index (the batch kernels read x: BatchArgs::xsel): trial k of a set is written to copy (x + 1 + k) % 3, an
// accepted trial's copy is the next x.  What judge() says the caller owes:
enum class LmNext {
  Done,          // nothing: the solve is over (converged on this trial)
  Second,        // the set's second record: once it is on the host, lm.take_step on it, then lm.running / judge again
  Relaunch,      // both rejected: a new launch set (begin_set) on the same J and H
  Relinearise    // accepted: x is that trial's copy now (cur still names the trial); relinearise there, then a new launch set
};

struct LmDualWalk {
  LmControl lm;
  int cur = 0, x = 0;              // record of the launch set that is judged next | copy that holds the linearisation point
  bool have_next = false;          // record 1 of the set holds the step for the next lambda
  bool trial_taken = false;        // ended on an accepted, converged trial: the estimate is that trial, not the linearisation point

  explicit LmDualWalk(const pps_props& p) : lm(p) {}

  // the copy trial k of a launch set goes to: (x + 1 + k) % 3, without the division (judge() rotates between a record and the launch it triggers)
  int trial(int k) const { const int c = x + 1 + k; return c < 3 ? c : c - 3; }
  int final_copy() const { return trial_taken ? trial(cur) : x; }    // linpoint_to_estimate (:466), or x when the pending step is dropped
  void begin_set(bool two_trials) { cur = 0; have_next = two_trials; }
  // the trial `cur` has chi2 error_new; *t is that trial for LmControl::note (at once, or behind the launch the answer asks for)
  __attribute__((always_inline)) LmNext judge(const pps_props& p, double error_new, LmControl::Trial* t) {
    const LmVerdict v = lm.decide(p, error_new, t);
    if (v == LmVerdict::Converged) { trial_taken = true; return LmNext::Done; }
    if (v == LmVerdict::Accepted) { x = trial(cur); return LmNext::Relinearise; }
    if (!have_next) return LmNext::Relaunch;
    cur = 1; have_next = false;
    return LmNext::Second;
  }
};

}  // namespace pps_impl

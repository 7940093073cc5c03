// lm_host.cpp -- csrc/pps_lm.h on the host (test infrastructure, tests/test_host_lm.py).
// Walks the LM controller over a recorded sequence of trial results the way the three host loops of the library do -- take_step on a
// record's arrival, running / judge per trial, finish at the end -- with no device behind it: the chi2 values, step norms and not-PD
// words come from the caller.  lm_host_replay is the one-step loop on LmControl alone; lm_host_replay_walk is the dual-trial scheme of
// lm_solve_dual and the batched rounds on LmDualWalk; lm_host_rotation drives the walk's rotation of the three state copies.
#include "pps_lm.h"

using namespace pps_impl;

namespace {

// what both replays share: the properties, the sink the rule writes to, and the way the results go back to the caller
struct Replay {
  pps_props p{};
  pps_stats st{};
  std::vector<double> tr_lambda, tr_chi2;
  std::vector<int> tr_acc;
  LmSink sink{&p, &tr_lambda, &tr_chi2, &tr_acc, &st, false};
  explicit Replay(const double* props6) {
    p.epsilon2 = props6[0]; p.epsilon_abs = props6[1]; p.epsilon_rel = props6[2]; p.max_iterations = (int)props6[3];
    p.lm_lambda0 = props6[4]; p.lm_lambda_factor = props6[5];
  }
  int finish(const LmControl& lm, int k, double* lambda_out, double* chi2_out, int* acc_out, double* summary) {
    for (int i = 0; i < k; i++) { lambda_out[i] = tr_lambda[i]; chi2_out[i] = tr_chi2[i]; acc_out[i] = tr_acc[i]; }
    int iterations = -1;
    summary[0] = lm.finish(sink, &iterations);
    summary[1] = iterations; summary[2] = st.lm_iterations; summary[3] = st.chi2_final; summary[4] = st.lambda_final;
    summary[5] = st.last_delta_norm; summary[6] = st.lm_trials_notpd; summary[7] = st.lm_trials_accepted; summary[8] = st.lm_trials_rejected;
    return (int)tr_lambda.size() == k ? k : -1;
  }
};

}  // namespace

// props6 = epsilon2, epsilon_abs, epsilon_rel, max_iterations, lm_lambda0, lm_lambda_factor.  Trial k has chi2[k], |delta|^2 dn2[k] and
// status word notpd[k].  Out, per judged trial: the trace triple the controller pushed (lambda, chi2, accepted) and its verdict
// (0 rejected | 1 accepted | 2 converged); summary[9] = return code of finish, *iterations, then the stats it wrote: lm_iterations,
// chi2_final, lambda_final, last_delta_norm, lm_trials_notpd, lm_trials_accepted, lm_trials_rejected.  Returns the trials judged.
extern "C" int lm_host_replay(const double* props6, double chi2_initial, int n, const double* chi2, const double* dn2, const double* notpd,
                              double* lambda_out, double* chi2_out, int* acc_out, int* verdict_out, double* summary) {
  Replay r(props6);
  const pps_props& p = r.p;
  LmControl lm(p);
  lm.error = chi2_initial;
  int k = 0;
  auto record = [&](int i) { const double rec[4] = {chi2[i], dn2[i], notpd[i], 0.0}; lm.take_step(rec); };
  if (n > 0) record(0);
  while (k < n && lm.running(p)) {
    const LmVerdict v = lm.judge(r.sink, chi2[k]);
    verdict_out[k] = v == LmVerdict::Rejected ? 0 : (v == LmVerdict::Accepted ? 1 : 2);
    k++;
    if (v == LmVerdict::Converged) break;
    if (k < n) record(k);            // (the step for the next lambda: solved after a verdict, as in the reference's loop)
  }
  return r.finish(lm, k, lambda_out, chi2_out, acc_out, summary);
}

// The same sequence through LmDualWalk, driven the way lm_solve_dual and the rounds of pps_multi.cpp drive it.  A launch set that begins when k
// trials are judged offers trial k as its record 0 and, if it carries two trials, trial k + 1 as its record 1.  mode: 0 one trial in every set |
// 1 two in every set | 2 lm_solve_dual's adaptive choice (one trial at first and after a trial accepted at once, two after a rejection).
// Outputs as lm_host_replay, and counts[6] = launch sets, second records taken, relaunches after both trials were rejected, relinearisations,
// sets with one trial, the final copy index (LmDualWalk::final_copy).
extern "C" int lm_host_replay_walk(const double* props6, double chi2_initial, int n, const double* chi2, const double* dn2, const double* notpd, int mode,
                                   double* lambda_out, double* chi2_out, int* acc_out, int* verdict_out, double* summary, int* counts) {
  Replay r(props6);
  const pps_props& p = r.p;
  LmDualWalk w(p);
  w.lm.error = chi2_initial;
  int k = 0;
  int &n_sets = counts[0], &n_second = counts[1], &n_relaunch = counts[2], &n_relin = counts[3], &n_single = counts[4];
  for (int i = 0; i < 6; i++) counts[i] = 0;
  bool two = mode == 1;
  // a record is on the host: the step it stands for is the one judged next (false: the recorded sequence has ended)
  auto record = [&]() { if (k >= n) return false; const double rec[4] = {chi2[k], dn2[k], notpd[k], 0.0}; w.lm.take_step(rec); return true; };
  auto launch = [&]() { w.begin_set(two); n_sets++; n_single += two ? 0 : 1; return record(); };
  bool more = launch();
  while (more && w.lm.running(p)) {
    LmControl::Trial t;
    const int cur = w.cur;
    const LmNext next = w.judge(p, chi2[k], &t);
    LmControl::note(r.sink, t);
    verdict_out[k] = !t.accepted ? 0 : (next == LmNext::Done ? 2 : 1);
    k++;
    if (next == LmNext::Done) break;
    if (next == LmNext::Second) { more = record(); n_second += more ? 1 : 0; continue; }      // (taken only now, when it is about to be judged)
    if (next == LmNext::Relinearise) { n_relin++; if (mode == 2) two = cur != 0; }
    else { n_relaunch++; if (mode == 2) two = true; }
    more = launch();
  }
  counts[5] = w.final_copy();
  return r.finish(w.lm, k, lambda_out, chi2_out, acc_out, summary);
}

// The rotation alone: n launch sets of two trials, in set i trial cur[i] (0 / 1) is accepted -- after trial 0 was rejected when it is trial 1 --;
// then one more set that ends the solve on its trial `end` accepted and converged (0 / 1), or with its pending step dropped (end < 0: the loop
// condition failed).  places[3 (n + 1)]: per set, the copy of the linearisation point and the copies its trials 0 and 1 are written to.
// Returns LmDualWalk::final_copy, or -1 when the walk asked for something else than this sequence implies.
extern "C" int lm_host_rotation(int n, const int* cur, int end, int* places) {
  pps_props p{};
  p.epsilon_rel = 1e-6; p.lm_lambda0 = 1e-6; p.lm_lambda_factor = 10.0;
  LmDualWalk w(p);
  w.lm.error = 1.0;
  LmControl::Trial t;
  for (int i = 0; i <= n; i++) {
    w.begin_set(true);
    places[3 * i] = w.x; places[3 * i + 1] = w.trial(0); places[3 * i + 2] = w.trial(1);
    const int c = i < n ? cur[i] : end;
    if (c < 0) break;
    if (c == 1 && (w.judge(p, 2.0 * w.lm.error, &t) != LmNext::Second || w.cur != 1)) return -1;
    const LmNext next = w.judge(p, w.lm.error * (i < n ? 0.5 : 1.0 - 1e-9), &t);
    if (next != (i < n ? LmNext::Relinearise : LmNext::Done)) return -1;
  }
  return w.final_copy();
}

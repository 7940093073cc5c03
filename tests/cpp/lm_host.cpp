// lm_host.cpp -- csrc/pps_lm.h on the host (test infrastructure, tests/test_host_lm.py).
// Walks the LM controller over a recorded sequence of trial results the way the three host loops of the library do -- take_step on a
// record's arrival, running / judge per trial, finish at the end -- with no device behind it: the chi2 values, step norms and not-PD
// words come from the caller.
#include "pps_lm.h"

using namespace pps_impl;

// props6 = epsilon2, epsilon_abs, epsilon_rel, max_iterations, lm_lambda0, lm_lambda_factor.  Trial k has chi2[k], |delta|^2 dn2[k] and
// status word notpd[k].  Out, per judged trial: the trace triple the controller pushed (lambda, chi2, accepted) and its verdict
// (0 rejected | 1 accepted | 2 converged); summary[9] = return code of finish, *iterations, then the stats it wrote: lm_iterations,
// chi2_final, lambda_final, last_delta_norm, lm_trials_notpd, lm_trials_accepted, lm_trials_rejected.  Returns the trials judged.
extern "C" int lm_host_replay(const double* props6, double chi2_initial, int n, const double* chi2, const double* dn2, const double* notpd,
                              double* lambda_out, double* chi2_out, int* acc_out, int* verdict_out, double* summary) {
  pps_props p{};
  p.epsilon2 = props6[0]; p.epsilon_abs = props6[1]; p.epsilon_rel = props6[2]; p.max_iterations = (int)props6[3];
  p.lm_lambda0 = props6[4]; p.lm_lambda_factor = props6[5];
  pps_stats st{};
  std::vector<double> tr_lambda, tr_chi2;
  std::vector<int> tr_acc;
  const LmSink sink{&p, &tr_lambda, &tr_chi2, &tr_acc, &st, false};
  LmControl lm(p);
  lm.error = chi2_initial;
  int k = 0;
  auto record = [&](int i) { const double rec[4] = {chi2[i], dn2[i], notpd[i], 0.0}; lm.take_step(rec); };
  if (n > 0) record(0);
  while (k < n && lm.running(p)) {
    const LmVerdict v = lm.judge(sink, chi2[k]);
    verdict_out[k] = v == LmVerdict::Rejected ? 0 : (v == LmVerdict::Accepted ? 1 : 2);
    k++;
    if (v == LmVerdict::Converged) break;
    if (k < n) record(k);            // (the step for the next lambda: solved after a verdict, as in the reference's loop)
  }
  for (int i = 0; i < k; i++) { lambda_out[i] = tr_lambda[i]; chi2_out[i] = tr_chi2[i]; acc_out[i] = tr_acc[i]; }
  int iterations = -1;
  summary[0] = lm.finish(sink, &iterations);
  summary[1] = iterations; summary[2] = st.lm_iterations; summary[3] = st.chi2_final; summary[4] = st.lambda_final;
  summary[5] = st.last_delta_norm; summary[6] = st.lm_trials_notpd; summary[7] = st.lm_trials_accepted; summary[8] = st.lm_trials_rejected;
  return (int)tr_lambda.size() == k ? k : -1;
}

// pps_solve.cpp -- the solve drivers.  Host control flow follows the reference line by line where it matters for parity:
//   pps_batch_optimize  == Optimizer::levenberg_marquardt  (Thirdparty/isam/isamlib/Optimizer.cpp:371-467)
//   pps_update          == Optimizer::relinearize          (Optimizer.cpp:114-185) via Slam::update, mod_batch = 1
// Everything numeric runs on the device; per LM trial one 32-byte result record (chi2, |delta|^2, not-PD flag) returns to the
// host for the accept / reject decision.
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

struct PhaseTimer {
  pps_graph* g; double* acc; bool on;
  PhaseTimer(pps_graph* g_, double* a) : g(g_), acc(a), on(g_->profiling >= 2) { if (on) (void)hipEventRecord(g->ev[0], g->stream); }
  ~PhaseTimer() {
    if (!on) return;
    (void)hipEventRecord(g->ev[1], g->stream);
    (void)hipEventSynchronize(g->ev[1]);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, g->ev[0], g->ev[1]);
    *acc += 1e-3 * ms;
  }
};

// the next start / stop pair of a launch's own events (profiling level 1), the vector grown by two when all are handed out; events = false: none
static int take_event_pair(pps_graph* g, bool events, std::vector<hipEvent_t>& evs, int& used, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!events) return PPS_OK;
  if (used + 2 > (int)evs.size()) for (int k = 0; k < 2; k++) { hipEvent_t e; HIP_TRY(g, hipEventCreate(&e)); evs.push_back(e); }
  *e0 = evs[used]; *e1 = evs[used + 1]; used += 2;
  return PPS_OK;
}
// ... of a K1 sweep (resolve_k1_events sums them into t_linearize).  skip: not (yet) a linearisation that ran.  *pair: its index, -1 without profiling
static int take_k1_events(pps_graph* g, char skip, hipEvent_t* e0, hipEvent_t* e1, int* pair = nullptr) {
  const bool events = g->profiling == 1;
  const int rc = take_event_pair(g, events, g->k1_events, g->k1_used, e0, e1); if (rc != PPS_OK) return rc;
  if (pair) *pair = events ? g->k1_used / 2 - 1 : -1;
  if (!events) return PPS_OK;
  g->k1_skip.resize(g->k1_events.size() / 2, 0);
  g->k1_skip[g->k1_used / 2 - 1] = skip;
  return PPS_OK;
}

// linearise at `lin` (K1) and reduce the H blocks (K2)
// guard: the launches are speculative (dual LM loop) -- the caller counts them once it knows they ran
int do_linearize(pps_graph* g, const LinGuard* guard = nullptr) {
  if (g->profiling == 1) {
    hipEvent_t e0, e1;
    { const int rc = take_k1_events(g, 0, &e0, &e1); if (rc != PPS_OK) return rc; }
    HIP_TRY(g, lin_launch(g, g->props.jacobian_mode, false, guard, e0, e1));
  } else
  { PhaseTimer t(g, &g->stats.t_linearize); HIP_TRY(g, lin_launch(g, g->props.jacobian_mode, false, guard)); }
  { PhaseTimer t(g, &g->stats.t_assemble); HIP_TRY(g, launch_hblocks(g->dev, g->stream, guard, k1_products(g->dev, g->props.jacobian_mode))); }
  if (!guard) g->stats.n_linearize++;
  return PPS_OK;
}

// delta = (J'J + lambda diag(J'J))^-1 J'b  (Optimizer::compute_gauss_newton_step, Optimizer.cpp:49-67)
// Factor stages leaves -> root, back-substitution stages root -> leaves, for one damping value (alt == nullptr) or two.  The root stage
// is one launch for both directions where its fronts allow it (K3Plan::root).  events: the factor launches carry their own start /
// stop events (profiling level 1: resolve_k1_events sums the pairs into t_factor; the fused root launch's pair spans its back-substitution as well).
// first_launched: called once, behind the first launch (the dual LM loop does there what it kept off the stretch in front of that launch)
struct NoHook { void operator()() const {} };
template <class Hook = NoHook>
static int enqueue_factor_solve(pps_graph* g, const DevGraph& dv, const DualAlt* alt, double lambda, hipStream_t st_, bool events, Hook first_launched = Hook()) {
  const K3Plan& P = g->plan;
  hipEvent_t e0, e1;
  if (P.form == K3Form::BandAll) {                                 // the whole tree: two launches (pps_k3.hip, XGroup)
    { const int rc = take_event_pair(g, events, g->fk_events, g->fk_used, &e0, &e1); if (rc != PPS_OK) return rc; }
    g->k3_epoch = g->k3_epoch >= (1 << 30) ? 1 : g->k3_epoch + 1;
    HIP_TRY(g, launch_band_all_factor(dv, alt, P, lambda, g->k3_epoch, st_, e0, e1));
    first_launched();
    HIP_TRY(g, launch_band_all_solve(dv, alt, P, g->k3_epoch, st_));
    return PPS_OK;
  }
  const int top = (int)P.stages.size() - 1;
  const bool fuse = P.root.fusable;
  for (int st = 0; st <= top; st++) {
    { const int rc = take_event_pair(g, events, g->fk_events, g->fk_used, &e0, &e1); if (rc != PPS_OK) return rc; }
    if (fuse && st == top) HIP_TRY(g, launch_band_root(dv, alt, P, lambda, st_, e0, e1));
    else HIP_TRY(g, launch_band_factor(dv, alt, P.stages[st], lambda, st_, e0, e1));
    if (st == 0) first_launched();
  }
  for (int st = fuse ? top - 1 : top; st >= 0; st--) HIP_TRY(g, launch_band_solve(dv, alt, P.stages[st], st_));
  return PPS_OK;
}

// the second factorisation of a handle (its spec_* buffers, pps_upload.cpp), for the damping value lambda2
static DualAlt dual_alt(const pps_graph* g, double lambda2) {
  return DualAlt{g->spec_L, g->spec_U, g->spec_delta, g->spec_result, g->spec_chi2_partials, g->spec_dn_partials, g->spec_ticket, lambda2};
}

int do_solve_on(pps_graph* g, const DevGraph& dv, double lambda, hipStream_t st_) { return enqueue_factor_solve(g, dv, nullptr, lambda, st_, false); }

// The factorisation alone, every launch a plain one on g->stream: one launch per band stage, or -- dense fronts -- L zeroed, the H blocks
// pushed, one launch per level, or one launch per level of the workgroup-per-front kernels.  The profiled forms of do_solve and the
// covariance recovery (pps_cov.cpp: lambda = 0, band and dense fronts only) factor with it.
int enqueue_plain_factor(pps_graph* g, double lambda) {
  const Analysis& A = g->an;
  const DevGraph& d = g->dev;
  if (g->use_band()) {
    for (const K3StagePlan& sp : g->plan.stages) HIP_TRY(g, launch_band_factor(d, nullptr, sp, lambda, g->stream, nullptr, nullptr, false));
    return PPS_OK;
  }
  if (g->use_dense()) {
    HIP_TRY(g, hipMemsetAsync(d.L, 0, (size_t)A.L_size * 8, g->stream));
    HIP_TRY(g, launch_dense_hpush(d, g->plan.max_el_per_front, lambda, g->stream));
  }
  for (int l = 0; l < A.n_levels; l++) {
    const int base = A.level_off[l] + l, cnt = A.level_off[l + 1] - A.level_off[l];
    if (g->use_dense()) HIP_TRY(g, launch_dense_factor_level(d, A.level_off[l], cnt, g->d_dw_asm + base, g->plan.dw_asm[base + cnt], g->d_dw_pan + base, g->plan.dw_pan[base + cnt],
                                                             g->d_dw_trl + base, g->plan.dw_trl[base + cnt], g->stream));
    else HIP_TRY(g, launch_factor_level(d, A.level_off[l], cnt, g->plan.level_max_front[l], lambda, g->stream));
  }
  return PPS_OK;
}

// ... and its back-substitution: the stages, or the levels, from the root down
static int enqueue_plain_backsolve(pps_graph* g) {
  const Analysis& A = g->an;
  const DevGraph& d = g->dev;
  if (g->use_band()) {
    for (int st = A.n_stages - 1; st >= 0; st--) HIP_TRY(g, launch_band_solve(d, nullptr, g->plan.stages[st], g->stream));
    return PPS_OK;
  }
  for (int l = A.n_levels - 1; l >= 0; l--) {
    const int cnt = A.level_off[l + 1] - A.level_off[l];
    if (g->use_dense()) HIP_TRY(g, launch_dense_solve_level(d, A.level_off[l], cnt, g->plan.level_max_b[l], g->stream));
    else HIP_TRY(g, launch_backsolve_level(d, A.level_off[l], cnt, g->stream));
  }
  return PPS_OK;
}

int do_solve(pps_graph* g, double lambda) {
  if (g->use_band() && g->profiling < 2) {            // no per-phase timing: the fused launches
    const int rc = do_solve_on(g, g->dev, lambda, g->stream); if (rc != PPS_OK) return rc;
  } else {
    { PhaseTimer t(g, &g->stats.t_factor); const int rc = enqueue_plain_factor(g, lambda); if (rc != PPS_OK) return rc; }
    { PhaseTimer t(g, &g->stats.t_backsolve); const int rc = enqueue_plain_backsolve(g); if (rc != PPS_OK) return rc; }
  }
  g->stats.n_factorize++;
  return PPS_OK;
}

// the status word of a record that has arrived (kHandoverMessage, pps_graph.h)
static int check_handover(pps_graph* g, const double* rec) { return handover_timed_out(rec) ? fail(g, PPS_EHIP, kHandoverMessage) : PPS_OK; }

// Wait for the result record with sequence number `seq`: spin on the pinned word the chi2 kernel writes
// last (a few microseconds), falling back to a stream sync if it does not show up (launch failure).
int wait_result(pps_graph* g, volatile double* slot, double seq, hipStream_t producer = nullptr) {
  const double t0 = now_s();
  unsigned spins = 0;
  while (slot[3] != seq) {
    if ((++spins & 0x3ff) == 0 && now_s() - t0 > 0.5) {
      HIP_TRY(g, hipStreamSynchronize(producer ? producer : g->stream));
      if (slot[3] != seq) return fail(g, PPS_EHIP, "result record did not arrive");
      break;
    }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  return check_handover(g, const_cast<const double*>(slot));
}

// est <-> lin by pointer: a rejected LM trial (estimate_to_linpoint, Optimizer.cpp:454) and the final
// linpoint_to_estimate (:466) need no data movement because the other copy is dead afterwards
void swap_state(pps_graph* g) {
  std::swap(g->dev.pose_est, g->dev.pose_lin);
  std::swap(g->dev.plane_est, g->dev.plane_lin);
}

// est_to_lin (estimate_to_linpoint): every caller goes on to overwrite the whole estimate -- a Gauss-Newton step retracts into it,
// an LM solve uses it as the target of its first trial -- before anything reads it, and puts it back from lin when the step
// fails: the two copies trade places by pointer, no data moves.  lin -> est (that putting back) is a real copy.
int copy_state(pps_graph* g, bool est_to_lin) {
  const DevGraph& d = g->dev;
  if (est_to_lin) { swap_state(g); return PPS_OK; }
  HIP_TRY(g, hipMemcpyAsync(d.pose_est, d.pose_lin, ((size_t)7 * d.pose_ld + (size_t)4 * d.plane_ld) * 8, hipMemcpyDeviceToDevice, g->stream));
  return PPS_OK;
}

// est -> lin as data (the diagnostic entry points that linearise outside a solve and leave the estimate in place)
int linpoint_from_estimate(pps_graph* g) {
  const DevGraph& d = g->dev;
  HIP_TRY(g, hipMemcpyAsync(d.pose_lin, d.pose_est, ((size_t)7 * d.pose_ld + (size_t)4 * d.plane_ld) * 8, hipMemcpyDeviceToDevice, g->stream));
  return PPS_OK;
}

// chi2 (and |delta|^2, not-PD flag) -> host
int read_result(pps_graph* g, bool at_estimate, double* chi2, double* dnorm, bool* notpd) {
  if (g->n_live_factors == 0) { *chi2 = 0.0; if (dnorm) *dnorm = 0.0; if (notpd) *notpd = false; return PPS_OK; }
  {
    PhaseTimer t(g, &g->stats.t_retract_chi2);
    HIP_TRY(g, chi2_launch(g, at_estimate, g->host_result, 0.0));
  }
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  *chi2 = g->host_result[0];
  if (dnorm) *dnorm = std::sqrt(g->host_result[1]);
  if (notpd) *notpd = g->host_result[2] != 0.0;
  return check_handover(g, g->host_result);
}

// after the final stream sync of a solve: fold the K1 event pairs into stats.t_linearize
void resolve_k1_events(pps_graph* g) {
  for (int k = 0; k + 1 < g->k1_used; k += 2) {
    float ms = 0;
    if ((size_t)(k / 2) < g->k1_skip.size() && g->k1_skip[k / 2]) continue;       // a speculative K1 that left at its guard
    if (hipEventElapsedTime(&ms, g->k1_events[k], g->k1_events[k + 1]) == hipSuccess) g->stats.t_linearize += 1e-3 * ms;
  }
  g->k1_used = 0;
  for (int k = 0; k + 1 < g->fk_used; k += 2) {                // factor launches of the dual loop (two factorisations per launch)
    float ms = 0;
    if (hipEventElapsedTime(&ms, g->fk_events[k], g->fk_events[k + 1]) == hipSuccess) g->stats.t_factor += 1e-3 * ms;
  }
  g->fk_used = 0;
}

static void reset_solve_stats(pps_graph* g) {
  pps_stats& s = g->stats;
  s.t_linearize = s.t_assemble = s.t_factor = s.t_backsolve = s.t_retract_chi2 = 0;
  s.n_linearize = s.n_factorize = 0;
  s.lm_iterations = s.lm_trials_accepted = s.lm_trials_rejected = s.lm_trials_notpd = 0;
  s.t_analysis = s.t_upload = 0;
  s.n_launches = 0;
  g->launches0 = launch_count();
}

// a solve call ends: its wall time and the launches it issued
static void end_solve_stats(pps_graph* g, double t0) { g->stats.t_total = now_s() - t0; g->stats.n_launches = (int)(launch_count() - g->launches0); }

void begin_solve(pps_graph* g) {
  reset_solve_stats(g);
  g->tr_lambda.clear(); g->tr_chi2.clear(); g->tr_acc.clear();
}

// the device copy of a handle is given up after a failed solve: streams drained, nothing on the device is trusted any more --
// the next upload sends the whole arena (UploadMirror::unknown: the mirror says nothing about the device, measurements included) and the
// estimate falls back to the host's node values
// status_clean: both records' status words are zero since the upload, or the last call's chi2 kernels took them along.  The flag stands for BOTH
// records: a one-step LM solve may have left a not-PD flag of a speculative factorisation that was never evaluated in the second one, and the
// caller sets status_clean again at its end
int clear_stale_status(pps_graph* g) {
  if (!g->status_clean) {
    HIP_TRY(g, launch_clear_status(g->dev, g->stream));
    if (g->spec_result) HIP_TRY(g, hipMemsetAsync(g->spec_result, 0, 4 * sizeof(double), g->stream));
  }
  g->status_clean = false;
  return PPS_OK;
}

void abandon_device_copy(pps_graph* g) {
  if (!g->dev_ready) return;
  (void)hipStreamSynchronize(g->stream);
  g->topo_dirty = true; g->dev_values_newer = false; g->dev_meas_newer = false;
  g->mirror.forget_device(); g->mirror.forget_measurements(); g->pk_meas_ok = false; g->status_clean = false;
}

// A failure in the middle of a solve (a HIP error: lost device, out of memory) leaves est / lin possibly exchanged and
// speculative work in flight.  Both streams are drained and the device copy is abandoned: the next call uploads again from
// the host's node values -- the estimate falls back to the last state the host has seen -- instead of reading half-updated
// buffers.  (PPS_ENOTPD is not such a failure: the solve ran to its end.)
}  // namespace pps_impl

extern "C" {

static int update_impl(pps_graph* g);
// estimate_to_linpoint is a pointer trade (copy_state): a HIP failure behind it would leave est / lin exchanged with est holding
// dead data -- like the LM drivers, a failed update abandons the device copy, and the next call uploads from the host's values.
int pps_update(pps_graph* g) {
  if (!g) return PPS_EINVAL;
  cov_invalidate(g);
  const int rc = update_impl(g);
  if (rc != PPS_OK && rc != PPS_ENOTPD) abandon_device_copy(g);
  return rc;
}
static int update_impl(pps_graph* g) {
  const double t0 = now_s();
  reset_solve_stats(g);
  if (g->n_live_nodes > 0 && g->n_live_factors == 0) return PPS_OK;   // no factor, no step
  int rc = prepare_solve(g);
  if (rc != PPS_OK) return rc;
  rc = clear_stale_status(g); if (rc != PPS_OK) return rc;
  rc = copy_state(g, true); if (rc != PPS_OK) return rc;          // estimate_to_linpoint (Optimizer.cpp:116)
  rc = do_linearize(g); if (rc != PPS_OK) return rc;              // jacobian() (:119)
  rc = do_solve(g, 0.0); if (rc != PPS_OK) return rc;             // compute_gauss_newton_step, lambda = 0 (:122)
  // apply_exmap (:183) and chi2 at the new estimate in ONE launch (round 6: the trial kernel of the LM loop with one trial -- the retraction
  // blocks write est <- lin (+) delta, the chi2 blocks evaluate at lin (+) delta on the fly, same bits; it was k_retract + k_chi2)
  double chi2 = 0.0, dn = 0.0; bool notpd = false;
  if (g->n_live_factors > 0 && g->dev.n_pose + g->dev.n_plane > 0 && !robust(g)) {      // (a cost function: retraction, then the robust chi2 sweep -- the branch below)
    const DevGraph& d = g->dev;
    { PhaseTimer t(g, &g->stats.t_retract_chi2);
      HIP_TRY(g, launch_trial_dual(d, DualAlt{}, d.pose_lin, d.plane_lin, d.pose_est, d.plane_est, nullptr, nullptr, g->host_result, 0.0, nullptr, 0.0, g->stream, 1)); }
    rc = enqueue_state_download(g); if (rc != PPS_OK) return rc;   // (arrives with the synchronisation below)
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    chi2 = g->host_result[0]; dn = std::sqrt(g->host_result[1]); notpd = g->host_result[2] != 0.0;
    rc = check_handover(g, g->host_result); if (rc != PPS_OK) return rc;
  } else {
    { PhaseTimer t(g, &g->stats.t_retract_chi2); HIP_TRY(g, launch_retract_apply(g->dev, g->stream)); }
    rc = enqueue_state_download(g); if (rc != PPS_OK) return rc;
    rc = read_result(g, true, &chi2, &dn, &notpd); if (rc != PPS_OK) return rc;
  }
  resolve_k1_events(g);
  if (notpd) {
    // the step is garbage: put the estimate back (lin still holds it) instead of handing NaNs to the caller
    rc = copy_state(g, false); if (rc != PPS_OK) return rc;
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    end_solve_stats(g, t0);
    return fail(g, PPS_ENOTPD, "normal equations not positive definite");
  }
  g->dev_values_newer = true;
  state_download_arrived(g);
  g->status_clean = true;                                         // the chi2 kernel took the flag with it
  g->stats.chi2_final = chi2; g->stats.last_delta_norm = dn; g->stats.lambda_final = 0;
  end_solve_stats(g, t0);
  return PPS_OK;
}

static int lm_solve(pps_graph* g, int* iterations);

int pps_batch_optimize(pps_graph* g, int* iterations) {
  if (!g) return PPS_EINVAL;
  cov_invalidate(g);
  if (g->n_live_nodes > 0 && g->n_live_factors == 0) {          // nothing to optimise: chi2 = 0 ends LM before its first trial
    begin_solve(g);
    if (iterations) *iterations = 0;
    return PPS_OK;
  }
  const int rc = lm_solve(g, iterations);
  if (rc != PPS_OK && rc != PPS_ENOTPD) abandon_device_copy(g);
  return rc;
}

// The common end of the two single-graph loops, entered with est / lin in their final places: the state comes down, the stream
// drains, and the controller's figures go into the stats.
static int end_lm_solve(pps_graph* g, const LmControl& lm, const LmSink& sink, int* iterations, double t0) {
  { const int rc2 = enqueue_state_download(g); if (rc2 != PPS_OK) return rc2; }
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  g->dev_values_newer = true;
  state_download_arrived(g);
  g->status_clean = true;                // every solve was followed by its chi2 kernel (the dual loop: by both)
  resolve_k1_events(g);
  end_solve_stats(g, t0);
  if (g->dev.trace) report_front_trace(g);
  if (lm.finish(sink, iterations) != PPS_OK) return fail(g, PPS_ENOTPD, kLmNotPdMessage);
  return PPS_OK;
}

// Optimizer::levenberg_marquardt (Optimizer.cpp:371-467) with both candidate steps of a linearisation in the same launches.
// A rejected trial only changes lambda (same J, same H), so every solve factors H for lambda AND for lambda * factor
// (blockIdx.y of the band kernels, second L / U / delta set), applies both steps to two spare copies of the state and reduces
// both chi2 values into two pinned records.  One stream, no events: 10 launches per linearisation instead of 21 on two streams.
// The host walks the reference's lambda schedule over the records (LmDualWalk, pps_lm.h): an accepted step rotates its copy in as the
// new linearisation point, a first rejection finds the next trial's verdict already on the host.  Arithmetic, lambda schedule and
// LM trace are exactly those of the one-step-at-a-time loop below.  This function owns what surrounds the walk: the launches, when a
// record is on the host, whether the next set carries one trial or two, the two kinds of speculative linearisation and the profiling.
static int lm_solve_dual(pps_graph* g, int* iterations, double t0) {
  const pps_props& prop = g->props;
  const Analysis& A = g->an;
  int rc = clear_stale_status(g); if (rc != PPS_OK) return rc;
  LmDualWalk walk(prop);
  LmControl& lm = walk.lm;
  const LmSink sink = lm_sink(g, prop.verbose != 0);
  double* slot0 = g->host_result;                                   // chi2 at the linearisation point
  double* slot[2] = {g->host_result + 4, g->host_result + 8};       // trial for lambda / for lambda * factor
  DevGraph& d = g->dev;
  rc = copy_state(g, true); if (rc != PPS_OK) return rc;           // estimate_to_linpoint (Optimizer.cpp:376): est is dead from here on
  // three state copies: walk.x = the linearisation point (d.pose_lin), trial k = x (+) delta of the k-th damping value -> copy walk.trial(k)
  double* const c_pose[3] = {d.pose_lin, d.pose_est, g->spec_pose};
  double* const c_plane[3] = {d.plane_lin, d.plane_est, g->spec_plane};
  auto t_pose = [&](int k) { return c_pose[walk.trial(k)]; };
  auto t_plane = [&](int k) { return c_plane[walk.trial(k)]; };
  double seqs[2] = {0, 0};
  // Speculation costs what it computes: on a graph whose lower tree levels fill the GPU by themselves (C3: 5 359 fronts) the second
  // factorisation + back-substitution of a launch set are extra time, not idle lanes -- and LM accepts most steps there.  Such a
  // graph factors the second damping value only while LM zig-zags (after a rejection); the trace is the same either way.
  const bool adaptive = A.n_fronts >= 2048;
  bool use_alt = !adaptive;
  // Round 6: the linearisation at the trial point LM is expected to accept rides in the trial launch, and K2 follows at once (SpecLin,
  // pps_device.h): when the host has seen the verdict and the prediction held, that point's J / H exist and become the current ones by
  // pointer; a wrong prediction launches the linearisation the plain way.  Graphs whose K1 is not the lane form over plain plane
  // observations keep the linearisation queued behind a device-side guard (LinGuard).
  // ... as do graphs whose sweep does not fit the chip's wave slots beside the trial blocks (k_trial_lin holds three waves per SIMD: 3 072
  // slots; C2 needs 2 700): a second round of waves costs more than the launch boundary saved (C3, same box: 384 against 365 us per iteration).
  const bool fuse_lin = !g->sw.no_spec_lin && g->spec_J != nullptr && trial_lin_ok(d, prop.jacobian_mode) && trial_lin_waves(d) <= 3072;
  int fused_pair = -1;                   // K1 event pair of the last fused launch (profiling level 1)
  int pred = 0, pred_launched = 0;       // the trial predicted to be accepted: the one that was accepted last | the one the last launch linearised
  // trials + the predicted linearisation + its H blocks: what ends every launch set in this mode
  bool error_known = false;              // lm.error holds chi2 at the linearisation point (not yet while the first launch set is queued)
  auto enqueue_trial_lin = [&](const DualAlt& alt, double s0, double s1) -> int {
    pred_launched = use_alt ? pred : 0;
    const SpecLin sl{g->spec_J, g->spec_P, g->spec_H, g->spec_Hf, pred_launched};
    hipEvent_t e0, e1;                     // (skipped until the predicted trial is accepted: then its sweep was a linearisation the solve asked for)
    { const int rc2 = take_k1_events(g, 1, &e0, &e1, &fused_pair); if (rc2 != PPS_OK) return rc2; }
    HIP_TRY(g, launch_trial_lin(d, alt, sl, d.pose_lin, d.plane_lin, t_pose(0), t_plane(0), t_pose(1), t_plane(1), slot[0], s0, slot[1], s1, g->stream, e0, e1));
    // (K2 of that linearisation leaves at once where the records say the prediction failed: 2 us instead of 7 in front of the plain sweep)
    const LinGuard gd{{d.result_dev, g->spec_result}, {nullptr, nullptr}, {nullptr, nullptr}, lm.error, error_known ? 1 : 0, use_alt ? 0 : 1, pred_launched};
    HIP_TRY(g, launch_hblocks_spec(d, sl, g->stream, &gd));
    return PPS_OK;
  };
  // The stretch between a trial record's arrival and the factor launch it triggers is on the solve's critical path -- the device has nothing
  // queued behind K2 until that launch arrives -- so the host does there only what depends on the verdict: the rule and the rotation
  // (LmDualWalk::judge), the launch.  The launch geometry of every form is worked out once per analysis (K3Plan), and what the trial leaves
  // in the trace and the counters (LmControl::note) is written behind the launch.  PPS_LM_PLAIN_HOST: everything in its old place.
  const bool plain_host = g->sw.lm_plain_host;
  struct PendingNote {                   // the judged trial whose bookkeeping is still owed (written at the latest when the loop is left, however)
    const LmSink& s; LmControl::Trial t{}; bool owed = false;
    void flush() { if (owed) { LmControl::note(s, t); owed = false; } }
    ~PendingNote() { flush(); }
  } pending{sink};
  // PPS_TIMING & 16: host seconds from the record's arrival to the factor launch call | inside that call (it returns when the doorbell has rung)
  const bool lm_timing = g->sw.lm_timing;
  // (launch sets whose prediction failed relinearise in between -- two launches more --: counted apart)
  double t_rec = 0.0, rt_pre = 0.0, rt_call = 0.0, rt_relin = 0.0; int rt_n = 0, rt_n_relin = 0; bool relin = false;
  auto rt_note = [&](double t_pre) {
    if (!lm_timing || t_rec <= 0.0) return;
    const double t = now_s();
    if (relin) { rt_relin += t - t_rec; rt_n_relin++; } else { rt_pre += t_pre - t_rec; rt_call += t - t_pre; rt_n++; }
    t_rec = 0.0; relin = false;
  };
  auto enqueue_dual = [&](double lam) -> int {
    const DualAlt alt = dual_alt(g, lam * prop.lm_lambda_factor);
    walk.begin_set(use_alt);
    // one damping value (!use_alt): the single-lambda launches, and the trial kernel with ONE trial (round 6: it used to walk both copies, the
    // second one with a stale delta that nothing read -- twice the retraction and chi2 work of a launch that C3 pays 22 us for; the walk never
    // asks for the second record)
    const int n_trials = use_alt ? 2 : 1;
    const double t_pre = lm_timing ? now_s() : 0.0;
    {
      // (timed: the host's work up to the first launch call | that call; the rest of the launch set is queued behind the bookkeeping)
      const int rc2 = enqueue_factor_solve(g, d, use_alt ? &alt : nullptr, lam, g->stream, g->profiling == 1, [&] { rt_note(t_pre); pending.flush(); });
      if (rc2 != PPS_OK) return rc2;
    }
    g->stats.n_factorize += n_trials;
    g->seq += 1.0; seqs[0] = g->seq;
    g->seq2 += 1.0; seqs[1] = g->seq2;
    if (fuse_lin) return enqueue_trial_lin(alt, seqs[0], seqs[1]);
    HIP_TRY(g, launch_trial_dual(d, alt, d.pose_lin, d.plane_lin, t_pose(0), t_plane(0), t_pose(1), t_plane(1), slot[0], seqs[0], slot[1], seqs[1],
                                 g->stream, n_trials));
    return PPS_OK;
  };
  rc = do_linearize(g); if (rc != PPS_OK) return rc;               // jacobian() (:379)
  g->seq += 1.0;
  const double seq0 = g->seq;
  HIP_TRY(g, launch_chi2(d, false, slot0, seq0, g->stream));       // r = weighted_errors(LINPOINT); error = |r|^2 (:382-385)
  // Accept-branch speculation: the relinearisation that follows an accepted step is queued behind the trials before their
  // verdict is known; its kernels apply the accept test themselves (LinGuard) and pick the accepted copy, so the device does
  // not idle for the host round trip between chi2 and K1.
  // (not on a graph that fills the GPU by itself -- `adaptive` --: there the queued launches cost more than the host round trip they hide; C3, same
  // box, three runs each: 358-361 us per LM iteration with them, 352-354 without)
  const bool spec_lin = !g->sw.no_spec_lin && !fuse_lin && !adaptive;
  int spec_pair = -1;                    // K1 event pair of the queued speculative linearisation
  auto enqueue_spec_lin = [&](double err) -> int {
    if (!spec_lin) return PPS_OK;
    LinGuard gd{{d.result_dev, g->spec_result}, {t_pose(0), t_pose(1)}, {t_plane(0), t_plane(1)}, err, 1, walk.have_next ? 0 : 1};
    spec_pair = g->profiling == 1 ? g->k1_used / 2 : -1;
    return do_linearize(g, &gd);
  };
  auto drop_spec_lin = [&]() { if (spec_pair >= 0 && (size_t)spec_pair < g->k1_skip.size()) g->k1_skip[spec_pair] = 1; spec_pair = -1; };
  rc = enqueue_dual(lm.lambda); if (rc != PPS_OK) return rc;
  rc = wait_result(g, slot0, seq0); if (rc != PPS_OK) return rc;
  lm.error = slot0[0]; error_known = true;
  g->stats.chi2_initial = lm.error;
  rc = enqueue_spec_lin(lm.error); if (rc != PPS_OK) return rc;
  rc = wait_result(g, slot[0], seqs[0]); if (rc != PPS_OK) return rc;
  lm.take_step(slot[0]);
  while (lm.running(prop)) {
    if (lm_timing) t_rec = now_s();
    const LmNext next = walk.judge(prop, slot[walk.cur][0], &pending.t);
    if (plain_host) LmControl::note(sink, pending.t); else pending.owed = true;      // (its note: behind the launch, in enqueue_dual)
    if (next == LmNext::Done) break;
    if (next == LmNext::Second) {                                  // computed alongside: nothing to launch
      t_rec = 0.0;
      pending.flush();
    } else {
      if (next == LmNext::Relinearise) {                           // the accepted copy is the linearisation point; the old one is a trial's target now
        const int acc = walk.cur;
        if (adaptive) use_alt = acc != 0;                          // (accepted at once: no speculation next time; after a rejection: keep it)
        pred = acc;
        d.pose_lin = c_pose[walk.x]; d.plane_lin = c_plane[walk.x];
        if (fuse_lin && acc == pred_launched) {                    // relinearise (:444): done beside the trials, at this very point
          std::swap(d.J, g->spec_J); std::swap(d.P, g->spec_P); std::swap(d.H, g->spec_H); std::swap(d.Hf, g->spec_Hf);
          g->stats.n_linearize++;
          if (fused_pair >= 0 && (size_t)fused_pair < g->k1_skip.size()) g->k1_skip[fused_pair] = 0;
        }
        else if (fuse_lin) { relin = true; rc = do_linearize(g); if (rc != PPS_OK) return rc; }      // (the other trial was accepted: the plain way)
        else if (spec_lin) { g->stats.n_linearize++; spec_pair = -1; }    // ... queued already, at this very copy
        else { rc = do_linearize(g); if (rc != PPS_OK) return rc; }
      } else {                                                     // estimate_to_linpoint (:454): x was never overwritten; same J and H
        drop_spec_lin();                                           // both trials rejected: its kernels left J and H alone
        if (adaptive) use_alt = true;                              // LM is zig-zagging: the next rejection should be free again
      }
      rc = enqueue_dual(lm.lambda); if (rc != PPS_OK) return rc;   // (:458)
      rc = enqueue_spec_lin(lm.error); if (rc != PPS_OK) return rc;
    }
    rc = wait_result(g, slot[walk.cur], seqs[walk.cur]); if (rc != PPS_OK) return rc;
    lm.take_step(slot[walk.cur]);
  }
  // linpoint_to_estimate (:466): the estimate is the accepted trial, or the linearisation point when the pending step is dropped
  drop_spec_lin();                       // (a linearisation queued behind the last trials is not one the solve asked for)
  pending.flush();
  if (lm_timing && rt_n > 0)
    fprintf(stderr, "[lm] record -> factor launch: %d launch sets, mean %.2f us before the launch call + %.2f us inside it; %d sets that relinearised first, mean %.2f us\n",
            rt_n, 1e6 * rt_pre / rt_n, 1e6 * rt_call / rt_n, rt_n_relin, rt_n_relin ? 1e6 * rt_relin / rt_n_relin : 0.0);
  place_state_copies(g, c_pose, c_plane, walk.final_copy());
  return end_lm_solve(g, lm, sink, iterations, t0);
}

static int lm_solve(pps_graph* g, int* iterations) {
  const double t0 = now_s();
  begin_solve(g);
  int rc = prepare_solve(g);
  if (rc != PPS_OK) return rc;
  if (g->use_band() && g->profiling < 2 && !g->dev.trace && !g->sw.no_dual && !robust(g)) return lm_solve_dual(g, iterations, t0);      // (PPS_NO_DUAL: the loop-forms parity test; a cost function: the robust kernels exist for this loop only)
  const pps_props& prop = g->props;
  rc = clear_stale_status(g); if (rc != PPS_OK) return rc;
  LmControl lm(prop);
  const LmSink sink = lm_sink(g, prop.verbose != 0);
  double* slot0 = g->host_result;       // chi2 at the linearisation point
  double* slot1 = g->host_result + 4;   // the trial: |delta|^2 of the step and chi2 after it
  // One stream, one result record per LM trial.  After every solve the trial step is applied at once (est <- lin,
  // lin <- lin (+) delta) and its chi2 is reduced, so a single record carries everything the loop condition and the accept
  // test need; a rejected trial is undone by exchanging the two copies (pointers), and if the loop ends on |delta| <= eps2
  // the pending step is undone the same way.  This is the reference's loop one step at a time: the form the profiling levels,
  // the phase trace and the graphs beyond the band kernels (dense fronts, level-per-launch fallback) run; band graphs take
  // lm_solve_dual.
  auto enqueue_trial = [&](double lam) -> int {
    int r = do_solve(g, lam); if (r != PPS_OK) return r;                       // compute_gauss_newton_step (:395,458)
    PhaseTimer t(g, &g->stats.t_retract_chi2);
    HIP_TRY(g, launch_retract_trial(g->dev, g->stream));                       // linpoint_to_estimate + self_exmap (:414-416)
    g->seq += 1.0;
    HIP_TRY(g, chi2_trial_launch(g, slot1, g->seq));                           // weighted_errors(LINPOINT) (:417)
    return PPS_OK;
  };
  rc = copy_state(g, true); if (rc != PPS_OK) return rc;          // estimate_to_linpoint (Optimizer.cpp:376)
  rc = do_linearize(g); if (rc != PPS_OK) return rc;              // jacobian() (:379)
  g->seq += 1.0;
  const double seq0 = g->seq;
  HIP_TRY(g, chi2_launch(g, false, slot0, seq0));                 // r = weighted_errors(LINPOINT); error = |r|^2 (:382-385)
  rc = enqueue_trial(lm.lambda); if (rc != PPS_OK) return rc;
  rc = wait_result(g, slot0, seq0); if (rc != PPS_OK) return rc;
  rc = wait_result(g, slot1, g->seq); if (rc != PPS_OK) return rc;
  lm.error = slot0[0];
  g->stats.chi2_initial = lm.error;
  lm.take_step(slot1);
  bool trial_pending = true;
  while (lm.running(prop)) {
    const LmVerdict v = lm.judge(sink, slot1[0]);
    if (v == LmVerdict::Converged) { trial_pending = false; break; }
    if (v == LmVerdict::Accepted) { rc = do_linearize(g); if (rc != PPS_OK) return rc; }   // relinearise around the accepted point (:444)
    else swap_state(g);                                           // estimate_to_linpoint: restore (:454)
    rc = enqueue_trial(lm.lambda); if (rc != PPS_OK) return rc;   // (:458)
    rc = wait_result(g, slot1, g->seq); if (rc != PPS_OK) return rc;
    lm.take_step(slot1);
  }
  if (trial_pending) swap_state(g);                               // undo the pending step
  swap_state(g);                                                  // linpoint_to_estimate (:466)
  return end_lm_solve(g, lm, sink, iterations, t0);
}

int pps_chi2(pps_graph* g, double* chi2) {
  if (!g || !chi2) return PPS_EINVAL;
  int rc = prepare_solve(g);
  if (rc != PPS_OK) return rc;
  double dn; bool np;
  return read_result(g, true, chi2, &dn, &np);
}

// The step of the shipped solve, outside any solve: K1 / K2 at the estimate (est -> lin as data, the estimate stays), then do_solve --
// or, for two damping values, enqueue_factor_solve with the DualAlt of lm_solve_dual -- and delta comes home instead of being applied.
// No retraction and no chi2 kernel follow, so nothing consumes the status words: they are read here and cleared again.
static int debug_solve_impl(pps_graph* g, double lambda, double lambda2, double* delta, double* delta2, int* form, double* not_pd) {
  int rc = prepare_solve(g);
  if (rc != PPS_OK) return rc;
  const bool dual = lambda2 >= 0.0;
  if (dual && !(g->use_band() && g->spec_L && g->spec_U && g->spec_delta && g->spec_result))
    return fail(g, PPS_ESTATE, "debug_solve: two damping values in one launch need the band kernels and their second L / U / delta set (this graph runs in another K3 form)");
  if (form) *form = g->use_band() ? (g->plan.form == K3Form::BandAll ? 1 : 0) : (g->use_dense() ? 2 : 3);
  const DevGraph& d = g->dev;
  rc = clear_stale_status(g); if (rc != PPS_OK) return rc;
  rc = linpoint_from_estimate(g); if (rc != PPS_OK) return rc;
  rc = do_linearize(g); if (rc != PPS_OK) return rc;
  if (dual) {
    const DualAlt alt = dual_alt(g, lambda2);
    rc = enqueue_factor_solve(g, d, &alt, lambda, g->stream, false); if (rc != PPS_OK) return rc;
  } else {
    rc = do_solve(g, lambda); if (rc != PPS_OK) return rc;
  }
  double status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const size_t n = (size_t)std::max(0, d.n_scalars);
  if (n) HIP_TRY(g, hipMemcpyAsync(delta, d.delta, n * 8, hipMemcpyDeviceToHost, g->stream));
  if (n && dual) HIP_TRY(g, hipMemcpyAsync(delta2, g->spec_delta, n * 8, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipMemcpyAsync(status, d.result_dev, 4 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  if (dual) HIP_TRY(g, hipMemcpyAsync(status + 4, g->spec_result, 4 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  if (status[2] != 0.0 || status[6] != 0.0) {                  // (status_clean is false since the clear above)
    rc = clear_stale_status(g); if (rc != PPS_OK) return rc;
    HIP_TRY(g, hipStreamSynchronize(g->stream));
  }
  g->status_clean = true;
  if (not_pd) *not_pd = std::max(status[2], status[6]);
  return PPS_OK;
}

int pps_debug_solve(pps_graph* g, double lambda, double lambda2, double* delta, double* delta2, int* form, double* not_pd) {
  if (!g) return PPS_EINVAL;
  if (!delta) return fail(g, PPS_EINVAL, "debug_solve: null delta");
  if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(g, PPS_EINVAL, "debug_solve: lambda must be a finite number >= 0");
  if (std::isnan(lambda2) || std::isinf(lambda2)) return fail(g, PPS_EINVAL, "debug_solve: lambda2 must be a finite number (negative: one damping value)");
  if (lambda2 >= 0.0 && !delta2) return fail(g, PPS_EINVAL, "debug_solve: lambda2 >= 0 needs delta2");
  if (g->n_live_nodes == 0) return fail(g, PPS_ESTATE, "empty graph");
  if (g->n_live_factors == 0) return fail(g, PPS_ESTATE, "debug_solve: the graph has no factor");
  cov_invalidate(g);                   // (dev.L is about to be overwritten)
  int rc;
  { NoSolveScope scope(g); rc = debug_solve_impl(g, lambda, lambda2, delta, delta2, form, not_pd); }      // (no solve: the figures of the last one stay)
  if (rc != PPS_OK && rc != PPS_EINVAL && rc != PPS_ESTATE) abandon_device_copy(g);
  return rc;
}

}  // extern "C"

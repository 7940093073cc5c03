// pps_graph.h -- the graph handle behind the C-ABI (include/pps.h) and what the implementation files share.
//
//   pps_api.cpp      graph bookkeeping: handles, nodes / factors, values, state snapshots, introspection, K1 micro-benchmarks
//   pps_upload.cpp   compaction + symbolic analysis, device arenas, difference upload, state / measurement transfers
//   pps_solve.cpp    pps_update (Optimizer::relinearize), pps_batch_optimize (Optimizer::levenberg_marquardt), chi2
//   pps_multi.cpp    pps_multi: G graphs per launch, lockstep LM rounds
//   pps_k3_plan.h    how K3 is launched on an analysis (plan_k3 -> K3Plan: form, waves, LDS of every launch): host only, no HIP
//   pps_lm.h         the LM rule the loops of pps_solve.cpp and pps_multi.cpp share (accept / reject / stop, lambda schedule, trace, counters) and the dual-trial walk with the rotation of the three state copies: host only, no HIP
//   pps_upmirror.h   the bookkeeping of the difference upload (UploadMirror: slots, owners, what differs, what a flush sends): host only, no HIP
//   pps_frames.cpp   registered frames (measurement refresh on the device), data association, point re-projection
//   pps_io.cpp       graph text format (Slam::save / Graph::write)
//   pps_cov.cpp      marginal covariances from the factor (isam::Covariances): the recovery pipeline and the reads of the selected inverse; kernels in pps_cov*.hip
//   pps_query.cpp    the protocol of the five calls that question the factor a recovery leaves (pps_query.h: QueryState below, CovQuery, begin / end,
//                    _last / _records), and the plainest of them, pps_cov_block
//   pps_gate.cpp     pps_assoc_gate (measurement against landmark); pps_merge.cpp: pps_merge_gate (landmark against landmark): queries on the factor
//   pps_loop.cpp     pps_loop_gate (a candidate loop closure between two poses): a query on the factor
//   pps_fgate.cpp    pps_factor_gate (every factor of the graph against the rest of it): a query on the selected inverse
//   pps_map.cpp      the dense map (pps_map: per-plane clouds of every frame, re-projected on the device); kernels in pps_map.hip
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/pps.h"
#include "pps_cov.h"
#include "pps_device.h"
#include "pps_geom.h"
#include "pps_lm.h"
#include "pps_popup_dev.h"
#include "pps_symbolic.h"
#include "pps_upmirror.h"

namespace pps_impl {

struct HostNode {
  int type;
  double v[7];
  bool deleted;
  int compact;   // index among live nodes (SymNode id)
  int slot;      // index in the pose / plane device array
};
struct HostFactor {
  int type;
  int a, b;
  double meas[6];
  double w[21];
  bool deleted;
  int slot;      // index in its type's device arrays
  int repop;     // plane observation that re-pops its measurement from `ray` (Pose3d_Plane3d_Factor2)
  double ray[6]; // K^-1 (u,v,1) of the two ground-edge end points
};

// what plan_k3 / band_group_fits_pre read of an analysis (pps_k3_plan.h)
inline pps::BandTreeView k3_tree_view(const pps::Analysis& A) {
  pps::BandTreeView v;
  v.n_stages = A.n_stages; v.n_groups = A.n_groups; v.n_levels = A.n_levels; v.n_fronts = A.n_fronts; v.band_levels = A.band_levels;
  v.stage_grp_off = A.stage_grp_off.data(); v.grp_lvl_off = A.grp_lvl_off.data(); v.glvl_front_off = A.glvl_front_off.data(); v.glvl_fronts = A.glvl_fronts.data();
  v.stage_max_front = A.stage_max_front.data(); v.stage_max_width = A.stage_max_width.data(); v.f_p = A.f_p.data(); v.f_b = A.f_b.data(); v.f_level = A.f_level.data();
  v.level_off = A.level_off.data(); v.level_fronts = A.level_fronts.data(); v.f_el_off = A.f_el_off.data();
  return v;
}

inline double now_s() {
  using namespace std::chrono;
  return duration_cast<duration<double>>(steady_clock::now().time_since_epoch()).count();
}

// a device buffer of one of the covariance calls (reserve / release: below, with the handle they take)
template <class T>
struct DevBuf {
  T* p = nullptr; size_t cap = 0;      // cap in elements
  int reserve(pps_graph* g, size_t count, const char* who = nullptr, const std::string& what = std::string(), const char* advice = "");
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// what one of the five query calls keeps on the handle between calls (the protocol that fills it: pps_query.h)
struct QueryState {
  DevBuf<char> out;                    // the result of a call on the device; where it has a status word, that comes first and is zero between calls
  DevBuf<unsigned int> ticket;         // ... and its tickets, zero between calls
  DevBuf<double> rec;                  // the records of the last call (pps_debug_*_records)
  size_t rec_n = 0;                    // ... how many it kept (0: the call failed, or had more entries than records are kept for)
  bool clean = false;                  // the status word and the tickets are zero
  bool done = false;                   // the last call on this handle succeeded
  double sec = 0; int launches = 0;    // its kernels: device seconds, launches
  int count = 0;                       // its entries without an answer (S not positive definite / d2 = NaN)
  void release() { out.release(); ticket.release(); rec.release(); rec_n = 0; clean = done = false; }
};

}  // namespace pps_impl

struct pps_graph {
  pps_props props;
  std::string err;
  std::vector<pps_impl::HostNode> nodes;
  std::vector<pps_impl::HostFactor> factors;
  int n_live_nodes = 0, n_live_factors = 0, dim_nodes = 0, dim_measure = 0;
  int n_live_type[4] = {0, 0, 0, 0}, n_live_repop = 0;      // live factors per type / live re-popping plane observations
  bool topo_dirty = true;       // structure changed since the last upload
  bool analysis_stale = true;   // structure changed since the last analysis
  bool host_values_newer = true;   // host node values must be pushed before the next solve
  bool dev_values_newer = false;   // device estimate is newer than the host copy
  bool meas_dirty = false;
  bool analyzed = false;
  int n_analyses = 0;              // analyses so far; with `grown_only` it selects the frame-loop form of the analysis
  // compacted node / factor tables of the last analysis (run_analysis appends to them while the graph only grows)
  std::vector<pps::SymNode> sym_nodes; std::vector<pps::SymFactor> sym_factors;
  size_t cmp_nodes = 0, cmp_factors = 0; int64_t cmp_base[4] = {0, 0, 0, 0}; bool cmp_valid = false, cmp_has_repop = false;
  bool grown_only = true;          // nothing has been removed since the last analysis (nodes / factors were only appended)
  bool grown_only_upload = false;  // ... since the last upload (false until there has been one)
  pps::Analysis an;
  pps::AnalysisParams aprm;
  pps::Switches sw;                // the PPS_* environment switches as they were when the handle was created
  // robust cost function (pps_set_cost_function; pps_cost.h).  COST_NONE: every call takes the launches it always took.  Otherwise K1 and the
  // chi2 sweeps go through the kernels of pps_robust.hip (lin_launch / chi2_launch / chi2_trial_launch below) and LM runs one step at a time.
  pps::CostFn cost;
  pps::AnalysisCache* acache = nullptr;   // what the last analysis left for the next one (frame loops)
  std::vector<int> pose_ids, plane_ids;   // slot -> node id
  std::vector<int> fslot_ids[4];          // per type: slot -> factor id
  // how K3 is launched on this analysis (pps_k3_plan.h): the form, the geometry of every launch, the dense-front work lists
  pps::K3Plan plan;
  bool use_band() const { return plan.band(); }                           // wave-per-front band kernels (fronts <= 127 rows)
  bool use_dense() const { return plan.form == pps::K3Form::Dense; }      // dense-front kernels (pps_dense.hip) when the band kernels do not apply
  int *d_dw_asm = nullptr, *d_dw_pan = nullptr, *d_dw_trl = nullptr;      // device copies of plan.dw_*
  // device
  bool dev_ready = false;
  hipStream_t stream = nullptr;
  pps::DevGraph dev;
  std::vector<void*> allocs;        // fallback allocations (arena full), freed at the next full upload
  // Device memory comes from two growable arenas that are re-used across uploads (a SLAM front end changes
  // the topology every frame; hipMalloc/hipFree per array per frame would dominate): `up` holds the arrays
  // that are uploaded (mirrored in a pinned host buffer; a flush sends what differs), `scr` the scratch arrays.
  struct Arena { char* base = nullptr; size_t cap = 0, off = 0, spill = 0; };
  Arena up, scr;
  // the pinned host mirror of `up` (UploadMirror::mir: allocated and freed by free_device / release_arenas), what it knows about the device,
  // where every upload of a layout goes, and which bytes the next flush sends (pps_upmirror.h)
  pps_impl::UploadMirror mirror;
  // Which analysis the upload mirror holds: `an` (sequence number an_seq) was built upon the analysis an_base_seq; when that is the
  // one whose arrays were uploaded last (up_an_seq), the leading entries `an.kept` names are in the mirror already and are not
  // compared again.  PPS_DEBUG_VERIFY_UPLOAD=1 checks every such claim (UploadMirror::hint_violation -> PPS_ESTATE).
  long an_seq = 0, an_base_seq = -1, up_an_seq = -1;
  // packed factor arrays of the last upload, per side (plane observations, odometry): an upload that only appends fills in the new slots
  // instead of packing every factor again (n = slots that are current; pk_meas_ok: the measurement rows of both sides still match the host factors)
  struct PackedSide {
    int type, km, kw;                  // factor type; rows of the measurement and of the weight array
    std::vector<int> ids, a, b;        // slot -> factor id as packed; slot -> slot of the first / second node
    std::vector<double> m, w;          // SoA with leading dimension ld
    size_t n = 0, ld = 0;
  };
  PackedSide pk_obs{pps::F_PLANE_OBS, 4, 6}, pk_odo{pps::F_ODOMETRY, 6, 21};
  bool pk_meas_ok = false;
  bool status_clean = false;     // result_dev / spec_result are zero: upload_all zeroed them, or the last solve's chi2 kernels consumed the flags
  bool up_inflight = false;      // upload_all left copies from the pinned buffers in flight on `stream`
  double* state_pin = nullptr; size_t state_pin_cap = 0;     // pinned staging of upload_state / download_state
  bool pin_holds_est = false;                                // state_pin holds the device estimate as it is now (enqueue_state_download)
  std::unordered_map<std::string, double> up_laps;         // PPS_TIMING=2: seconds per phase of upload_all, summed; printed at destroy
  char* patch_host = nullptr; size_t patch_cap = 0;    // pinned: the table of k_scatter_patches (the pieces are read from the pinned mirror)
  double* host_result = nullptr;   // pinned, 12 doubles: chi2 at the linearisation point | trial | speculative trial
  double seq = 0.0;                // sequence number the chi2 kernel publishes last (host polls it)
  // the second damping value of a dual solve (lambda * factor): its own L / U / delta, a third copy of the state, its own
  // reduction scratch and result record
  double *spec_pose = nullptr, *spec_plane = nullptr, *spec_chi2_partials = nullptr, *spec_dn_partials = nullptr;
  unsigned int* spec_ticket = nullptr;
  double seq2 = 0.0;
  double *spec_L = nullptr, *spec_U = nullptr, *spec_delta = nullptr;
  double* spec_result = nullptr;   // result_dev of the speculative set: its own not-PD flag
  // the spare set of J / P / H / Hf that the fused trial + linearisation launch writes (SpecLin, pps_device.h); when LM accepts the trial it was
  // made for, the set trades places with dev.J / P / H / Hf by pointer.  Null where the dual LM loop does not apply (no band schedule).
  double *spec_J = nullptr, *spec_P = nullptr, *spec_H = nullptr, *spec_Hf = nullptr;
  int k3_epoch = 0;                // number of the last whole-tree launch pair (its hand-over flags carry it: DevGraph::k3_flag)
  double *snap_pose = nullptr, *snap_plane = nullptr;   // pps_save_state
  int snap_version = -1, upload_version = 0;
  int k2t_version = -1;              // upload_version the class lists of K2's throughput form (dev.k2t) were built for
  int profiling = 0;               // 0 off, 1 = K1 event pairs without host syncs, 2 = every phase (adds syncs)
  hipEvent_t ev[2] = {nullptr, nullptr};
  unsigned long long launches0 = 0;   // launch_count() at the start of the solve call
  std::vector<char> k1_skip;          // per K1 event pair: not a linearisation that ran
  std::vector<hipEvent_t> k1_events;   // pairs (start, stop) recorded around the sweep
  std::vector<hipEvent_t> fk_events;   // profiling level 1: start / stop of every factor launch of the dual loop (dispatch timestamps)
  int fk_used = 0;
  int k1_used = 0;
  // registered frames (pps_frames_add): 2-D ground segments that re-derive edge measurements on the device
  float frames_invK[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  std::vector<int> fr_pose;          // frame -> pose node id
  std::vector<int> fr_seg_off{0};    // frame -> first segment
  std::vector<float> fr_seg;         // 4 floats per segment
  std::vector<int> fr_item_frame, fr_item_plane, fr_item_fid;
  bool frames_dirty = true;          // device tables must be rebuilt
  // the slot tables of the registered frames only grow while nothing is removed (n_removals): cached, and the first upload of the
  // tables after an upload_all lands on the slots of the previous layout's -- whose leading entries (fr_hint_*) are not compared again
  std::vector<int> fr_slot, fr_pslot;
  long n_removals = 0, fr_cache_removals = -1;
  int fr_hint_version = -2; size_t fr_hint_cursor = 0, fr_hint_items = 0, fr_hint_frames = 0;
  int frames_version = -1;
  int *d_item_frame = nullptr, *d_item_plane = nullptr, *d_item_slot = nullptr, *d_frame_pose_slot = nullptr, *d_frame_seg_off = nullptr;
  float* d_fr_seg = nullptr;
  bool dev_meas_newer = false;       // device edge measurements are newer than the host copies
  int n_obs_fixed = 0;               // plane observations with a stored measurement (slots below this)
  // landmark records for data association (pps_landmark_update / pps_find_closest_planes)
  struct Landmark { int plane_id, fpi, seq, deleted; float seg2d[4], seg3d[4]; };
  std::vector<Landmark> lms;
  std::unordered_map<int, int> lm_of_plane;
  bool lms_dirty = true;
  int lms_upload_version = -1;       // upload_version the slots of d_lms were resolved against
  pps::AssocLandmark* d_lms = nullptr; size_t d_lms_cap = 0;
  pps::AssocLandmark* h_lms = nullptr;                        // pinned staging of d_lms (same capacity): the copy is not waited for on its own
  pps::AssocQuery* d_queries = nullptr; pps::AssocResult* d_results = nullptr; size_t d_q_cap = 0;   // PINNED host memory: k_assoc reads the queries and writes the results over the bus
  double* d_lm_planes = nullptr; size_t d_lm_planes_cap = 0;   // [4][n] landmark planes when the solver state is not current
  char* rp_pin = nullptr; size_t rp_cap = 0;                  // pinned block of pps_reproject_points: [slots | points in | points out], read and written by the kernel
  // marginal covariances (pps_cov.cpp): the selected inverse of the last recovery pass, in the panel layout of L ([Sigma_AA; Sigma_BA] per
  // front at f_Loff; a front's Sigma_BB sits in its -- then dead -- update matrix in dev.U).  Buffers of their own, allocated on the first
  // recovery; cov_valid falls with every call that moves the estimate, the measurements or the topology (cov_invalidate)
  bool cov_valid = false;
  // a valid lambda = 0 factor is held in dev.L (all pps_cov_block and the gates read): set by a recovery pass together with cov_valid, by
  // pps_cov_factor alone; falls with cov_valid
  bool cov_factor_valid = false;
  int cov_version = -1;              // upload_version the recovery belongs to
  // what of the recovery's preparation is current: everything in `have` was built, checked or uploaded for the analysis of upload_version
  // `version` (cov_run forgets it all when the versions differ)
  enum : unsigned { kCovTables = 1,  // node -> front tables (cov_epos .. cov_max_rows) built, the tree checked for the path walks
                    kCovLevelShapes = 2,   // ... and for k_cov_level (its LDS)
                    kCovParent = 4,        // cov_parent holds f_parent
                    kCovDense = 8 };       // the tree checked for the dense-front pass; cov_dtab, cov_dpre_items and cov_dlevel hold its work lists
  struct CovCache { int version = -1; unsigned have = 0; } cov_cache;
  pps_impl::DevBuf<double> cov_S;
  pps_impl::DevBuf<int> cov_parent;
  pps_impl::DevBuf<char> cov_req;    // gather requests of a read call (device)
  pps_impl::DevBuf<double> cov_out;  // ... and the blocks they collect
  std::vector<int> cov_epos, cov_front_of;               // delta index -> elimination-ordered scalar; that scalar -> front
  hipEvent_t cov_ev[3] = {nullptr, nullptr, nullptr};
  double cov_sec[2] = {0, 0};        // device seconds of the last recovery: whole call | root -> leaves pass alone
  // the queries on the factor (CovQuery, pps_query.h: pps_cov_block, pps_assoc_gate, pps_merge_gate, pps_loop_gate): per front the pivots of the front and all its
  // ancestors; the request blob, the strips and the event pair of the query in flight (every query ends with a synchronisation)
  std::vector<int> cov_rootlen; int cov_max_p = 0, cov_max_rows = 0;
  pps_impl::DevBuf<char> cov_breq;
  pps_impl::DevBuf<double> cov_strip;
  hipEvent_t cov_qev[2] = {nullptr, nullptr};
  // the path walk for wide fronts (k_cov_path_wide): the right-hand sides of the walks of one query, sized by the widest front on its paths
  pps_impl::DevBuf<double> cov_zscr;
  int cov_path_form = 0;             // pps_debug_cov_path_form: 0 = k_cov_path where its LDS fits, 1 = always the wide kernel
  // the dense-front pass (pps_cov_dense.hip): G = L_B L_A^-1 of every front in the panel layout of L, and the work-item prefix sums of its
  // launches -- [all fronts: G slabs | per level: gather pieces, Sigma_BA strips] -- on the device (cov_dtab) with their places
  pps_impl::DevBuf<double> cov_G;
  pps_impl::DevBuf<int> cov_dtab;
  int cov_dpre_items = 0;
  std::vector<int> cov_dlevel;       // per level, 4 ints: place of the gather sums in cov_dtab, their total, place of the strip sums, their total
  int cov_select_form = 0;           // pps_debug_cov_select_form: 1 = pps_cov_select takes the dense-front pass on a band graph too
  // the five calls that question the factor (pps_query.h), one state each.  Result layouts: pps_cov_block [status | block] doubles; pps_assoc_gate
  // [status | d2 | best] doubles, one ticket per measurement; pps_merge_gate [status (16 bytes) | best | flags | d2 n x n], one ticket per plane;
  // pps_loop_gate [status (16 bytes) | flags | d2 n | S n x 36]; pps_factor_gate [d2 n | lev n | status: n ints], no status word
  pps_impl::QueryState q_block, q_assoc, q_merge, q_loop, q_factor;
  // pps_factor_gate (pps_fgate.cpp): one FgateFactor per factor id on the device -- where the blocks of its joint marginal sit in cov_S --, built
  // for the analysis of upload_version fgate_tab_version (like cov_cache); the fid list of the last call
  pps_impl::DevBuf<char> fgate_tab; int fgate_tab_version = -1, fgate_tab_n = 0;
  pps_impl::DevBuf<int> fgate_list;
  // stats / trace
  pps_stats stats{};
  std::vector<double> tr_lambda, tr_chi2;
  std::vector<int> tr_acc;
};

namespace pps_impl {
using namespace pps;

inline int fail(pps_graph* g, int code, const std::string& msg) {
  if (g) g->err = msg;
  return code;
}
inline int hip_fail(pps_graph* g, hipError_t e, const char* what) {
  return fail(g, PPS_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(g, expr)                                   \
  do {                                                     \
    hipError_t _e = (expr);                                \
    if (_e != hipSuccess) return hip_fail(g, _e, #expr);   \
  } while (0)

inline bool live_node(const pps_graph* g, int id, int type) {
  return id >= 0 && id < (int)g->nodes.size() && !g->nodes[id].deleted && g->nodes[id].type == type;
}

// ---- pps_upload.cpp ----
void free_device(pps_graph* g);
void release_arenas(pps_graph* g);
int flush_uploads(pps_graph* g);
int verify_uploads(pps_graph* g, const char* where);
int verify_frame_tables(pps_graph* g);         // PPS_DEBUG_VERIFY_UPLOAD: the frame tables against the factor / node records, host and device
int ensure_device(pps_graph* g);
int64_t j_capacity(int64_t n);
void slab_bases(const pps_graph* g, const int size[4], int64_t base[4], int64_t* total);
inline void j_bases(const pps_graph* g, int64_t base[4], int64_t* total) { slab_bases(g, pps::kJSize, base, total); }
inline void p_bases(const pps_graph* g, int64_t base[4], int64_t* total) { slab_bases(g, pps::kPSize, base, total); }      // product records, same slab capacities
int run_analysis(pps_graph* g);
int state_pin_reserve(pps_graph* g, size_t doubles);
int linpoint_from_estimate(pps_graph* g);
int download_state(pps_graph* g);
int enqueue_state_download(pps_graph* g);      // ... before the synchronisation a solve ends with,
void state_download_arrived(pps_graph* g);     // ... and this after it
int upload_state(pps_graph* g, bool sync = true);
int download_measurements(pps_graph* g);
int upload_measurements(pps_graph* g);
int upload_all(pps_graph* g);
int prepare_solve(pps_graph* g);
// ---- pps_solve.cpp ----
int read_result(pps_graph* g, bool at_estimate, double* chi2, double* dnorm, bool* notpd);
void begin_solve(pps_graph* g);                // an LM solve starts: the last one's stats and trace go
void abandon_device_copy(pps_graph* g);
int clear_stale_status(pps_graph* g);          // result_dev / spec_result zeroed unless they are (status_clean), which then no longer holds
int enqueue_plain_factor(pps_graph* g, double lambda);      // the factorisation alone, plain launches: the band stages, or memset + hpush + dense levels
// "this call is no solve": the figures of the last solve, the profiling level and launches0 come back when the scope ends; only the fields
// that describe the analysis follow the analysis
struct NoSolveScope {
  pps_graph* g; pps_stats saved; int profiling; unsigned long long launches0;
  explicit NoSolveScope(pps_graph* g_) : g(g_), saved(g_->stats), profiling(g_->profiling), launches0(g_->launches0) { g->profiling = 0; }
  ~NoSolveScope() {
    g->profiling = profiling;
    g->launches0 = launches0;
    pps_stats s = saved;
    s.n_fronts = g->stats.n_fronts; s.n_levels = g->stats.n_levels; s.max_front = g->stats.max_front; s.nnz_L = g->stats.nnz_L;
    g->stats = s;
  }
};
inline LmSink lm_sink(pps_graph* g, bool verbose) { return LmSink{&g->props, &g->tr_lambda, &g->tr_chi2, &g->tr_acc, &g->stats, verbose}; }
// the end of a dual-trial solve (LmDualWalk, pps_lm.h): of the three state copies, `fin` (LmDualWalk::final_copy) is the estimate; the other two,
// dead now, are the linearisation point and the spare of the next solve
inline void place_state_copies(pps_graph* g, double* const pose[3], double* const plane[3], int fin) {
  g->dev.pose_est = pose[fin]; g->dev.plane_est = plane[fin];
  g->dev.pose_lin = pose[(fin + 1) % 3]; g->dev.plane_lin = plane[(fin + 1) % 3];
  g->spec_pose = pose[(fin + 2) % 3]; g->spec_plane = plane[(fin + 2) % 3];
}
// status word of a result record (rec[2]): 0 ok | 1 not positive definite | >= kStatusInternal an internal hand-over of a K3 launch timed out
// (flow_wait, pps_k3.hip) -- the numbers of that record are not a solution, the call answers PPS_EHIP with this text
constexpr const char* kHandoverMessage = "internal error: a hand-over flag between the waves or workgroups of a K3 launch never arrived (the step was discarded)";
inline bool handover_timed_out(const double* rec) { return rec[2] >= pps::kStatusInternal; }
// the one place where a handle's cost function chooses the kernels: K1 and the two chi2 sweeps (everything else consumes J, r and delta)
inline bool robust(const pps_graph* g) { return g->cost.kind != COST_NONE; }
inline hipError_t lin_launch(pps_graph* g, int mode, bool at_estimate, const LinGuard* guard = nullptr, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  if (robust(g)) return launch_linearize_robust(g->dev, g->cost, mode, at_estimate, g->stream, ev0, ev1);      // (no guard: the one-step loop does not speculate)
  return launch_linearize(g->dev, mode, at_estimate, g->stream, guard, ev0, ev1);
}
inline hipError_t chi2_launch(pps_graph* g, bool at_estimate, double* host_result, double seq) {
  if (robust(g)) return launch_chi2_robust(g->dev, g->cost, at_estimate, host_result, seq, g->stream);
  return launch_chi2(g->dev, at_estimate, host_result, seq, g->stream);
}
inline hipError_t chi2_trial_launch(pps_graph* g, double* host_result, double seq) {
  if (robust(g)) return launch_chi2_trial_robust(g->dev, g->cost, host_result, seq, g->stream);
  return launch_chi2_trial(g->dev, host_result, seq, g->stream);
}
// ---- pps_cov.cpp ----
inline void cov_invalidate(pps_graph* g) { g->cov_valid = g->cov_factor_valid = false; }   // estimate, measurements or topology are about to change
void cov_release(pps_graph* g);                // pps_graph_destroy: the recovery's own device buffers
bool cov_current(const pps_graph* g);          // is there a recovery that belongs to the estimate, the measurements and the topology as they are?
bool cov_factor_current(const pps_graph* g);   // ... or at least its factor (pps_cov_factor)?
extern const char* const kNoRecovery;          // the text of the PPS_ESTATE answer when there is none
extern const char* const kFactorOnly;          // ... and when there is a factor, asked for the selected inverse
// where a node's scalars sit in the elimination order: its front and the local index of its first pivot
struct CovNode { int front, local, dim, epos, voff; };
int cov_node(pps_graph* g, int id, CovNode* out);      // id check (PPS_EINVAL) + dim; the rest by cov_locate, with a current recovery only
int cov_locate(pps_graph* g, int id, CovNode* n);
// the block Sigma(rows r, columns c) of the selected inverse as a gather request (pps_cov.h: source offset, leading dimension, transpose flag;
// dst as given); false: the pair is outside the pattern of L
bool cov_request(const pps_graph* g, const CovNode& r, const CovNode& c, long long dst, pps::CovReq* q);
// a device buffer of one of the covariance calls, grown by a quarter when it is too small.  Without `who` a failure answers as HIP_TRY does; with
// it, PPS_ENOMEM and "<who>no device memory for <what> (<n> bytes)<advice>"
template <class T>
int DevBuf<T>::reserve(pps_graph* g, size_t count, const char* who, const std::string& what, const char* advice) {
  if (count <= cap && p) return PPS_OK;
  const auto grow = [&]() -> int {
    HIP_TRY(g, hipStreamSynchronize(g->stream));          // (nothing in flight reads the old buffer)
    release();
    const size_t want = std::max<size_t>(64, count + count / 4);
    HIP_TRY(g, hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T)));
    cap = want;
    return PPS_OK;
  };
  const int rc = grow();
  if (rc == PPS_OK || !who) return rc;
  (void)hipGetLastError();
  return fail(g, PPS_ENOMEM, std::string(who) + "no device memory for " + what + " (" + std::to_string(count * sizeof(T)) + " bytes)" + advice);
}
// ---- pps_api.cpp ----
void report_front_trace(pps_graph* g);        // PPS_TRACE: the per-front cycle counters of the last solve -> stderr

// `count` elements of scratch from the arena `scr`; when it is full (it is re-sized at the next upload), a plain allocation
template <class T>
int dev_alloc(pps_graph* g, T** out, size_t count) {
  pps_graph::Arena& a = g->scr;
  *out = nullptr;
  if (count == 0) count = 1;
  const size_t bytes = count * sizeof(T);
  const size_t o = (a.off + 255) & ~size_t(255);
  if (a.base && o + bytes <= a.cap) { a.off = o + bytes; *out = reinterpret_cast<T*>(a.base + o); return PPS_OK; }
  a.spill += bytes + 256;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return hip_fail(g, e, "hipMalloc");
  g->allocs.push_back(p);
  *out = static_cast<T*>(p);
  return PPS_OK;
}

// The next upload of the layout: the mirror places it (pps_upmirror.h) and records what differs; a flush sends that.  An array the arena has no
// room for gets an allocation of its own and is copied at once (upload_spilled).
// same: leading ELEMENTS (of the array, or of every row) that the caller knows to be what this slot received last time; exact_from: kNoExact
int upload_spilled(pps_graph* g, void** out, const void* src, size_t n, size_t bytes);
template <class T>
int dev_upload_rows(pps_graph* g, T** out, const std::vector<T>& v, size_t rows, size_t ld, size_t used, bool force, size_t exact_from = kNoExact,
                    size_t same = 0) {
  constexpr size_t E = sizeof(T);
  const size_t n = v.size() * E, bytes = std::max<size_t>(1, v.size()) * E;
  const char* src = reinterpret_cast<const char*>(v.data());
  UploadMirror& m = g->mirror;
  const UploadMirror::Place p = m.place(out, bytes);
  if (!p.fits) return upload_spilled(g, reinterpret_cast<void**>(out), src, n, bytes);
  *out = reinterpret_cast<T*>(g->up.base + p.off);
  g->up.off = std::max(g->up.off, p.off + bytes);
  if (rows == 0) m.put_array(p, src, n, same * E);
  else m.put_rows(p, src, n, rows, ld * E, used * E, force, same * E, (exact_from != kNoExact && E == 8) ? exact_from * E : kNoExact);
  return PPS_OK;
}
template <class T>
int dev_upload(pps_graph* g, T** out, const std::vector<T>& v, size_t same = 0) { return dev_upload_rows(g, out, v, 0, 0, 0, false, kNoExact, same); }

}  // namespace pps_impl

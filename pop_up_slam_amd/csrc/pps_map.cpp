// pps_map.cpp -- host side of the dense map (include/pps.h: pps_map_*): the chunk table, the thinning of main_3d.cpp:544-562, the
// selection record both builds and both grids start from (MapSelection, pps_map_host.h), and the calls that drive the kernels of
// pps_map.hip.
//
// Streams.  A pop-up context runs on its own stream, the map's kernels on the stream of the graph it belongs to.  pps_map_add_frame first
// waits -- on the host -- for the run of the pop-up context (popup_last_run), so the cloud and the plane-id map are complete before the
// count kernel is enqueued on the graph's stream; it returns after a synchronisation of that stream, so the context's next run cannot
// overwrite a cloud that is still being read.  pps_map_build follows prepare_solve on the same stream: the solver's estimate, the store's
// last writes and the build are ordered by the stream itself.
#include "pps_map_host.h"
#include "pps_map_move.h"
#include "pps_popup_host.h"

using namespace pps;
using namespace pps_impl;

static_assert(sizeof(MapPt) == sizeof(pps_point), "MapPt is pps_point");

namespace {

bool select_valid(const pps_map_select* s) { return !s || (s->old_every > 0 && s->new_every > 0); }

// main_3d.cpp:544-562
void select_chunks(const pps_map_chunk* c, int n, const pps_map_select* s, int32_t* keep) {
  std::unordered_map<int, int> tracked;                // being_tracked_times: chunks that belong to the landmark now
  for (int i = 0; i < n; i++) tracked[c[i].plane_id]++;
  for (int i = 0; i < n; i++) {
    keep[i] = 1;
    if (!s) continue;
    const int seq = c[i].frame_seq_id, times = tracked[c[i].plane_id];
    if (!s->every_frame) {
      if (seq <= s->counter - s->old_age) { if (c[i].frame % s->old_every != 0) keep[i] = 0; }
      else if (c[i].frame % s->new_every != 0) keep[i] = 0;
    }
    for (int a = 0; a < 3; a++)
      if (seq <= s->counter - s->age[a] && times < s->min_tracked[a]) keep[i] = 0;
  }
}

}  // namespace

namespace pps_impl {
bool map_select_valid(const pps_map_select* s) { return select_valid(s); }

int map_use_device(pps_map* m) {
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  m->on_device = true;
  return PPS_OK;
}

void MapSelection::select(const pps_map* m, const pps_map_select* sel) {
  const int nc = (int)m->chunks.size();
  keep.resize((size_t)nc);
  select_chunks(m->chunks.data(), nc, sel, keep.data());
  src.clear(); total = 0;
  for (int i = 0; i < nc; i++) {
    if (!keep[i]) continue;
    if (m->chunks[i].count > 0) src.push_back(i);
    total += m->chunks[i].count;
  }
}

int MapSelection::upload(pps_map* m, bool posed, const std::map<int, int>* row_of, MapBuf<char>* buf, size_t over, MapSpan* span) {
  const pps_graph* g = m->g;
  const size_t ns = src.size();
  if (posed) map_motion_plan(m, src, &plan);
  at.src_off = (ns + 1) * sizeof(long long);
  at.slot = at.src_off + ns * sizeof(long long);
  at.lm = at.slot + ns * sizeof(int);
  at.fidx = at.lm + (row_of ? ns * sizeof(int) : 0);
  at.recs = (at.fidx + ns * sizeof(int) + 7) / 8 * 8;
  at.bytes = posed ? at.recs + plan.recs.size() * sizeof(MapFrameDev) : at.fidx;
  host.assign(at.bytes, 0);
  long long* h_out = reinterpret_cast<long long*>(host.data());
  long long* h_src = reinterpret_cast<long long*>(host.data() + at.src_off);
  int* h_slot = reinterpret_cast<int*>(host.data() + at.slot);
  int* h_lm = reinterpret_cast<int*>(host.data() + at.lm);
  long long o = 0;
  for (size_t j = 0; j < ns; j++) {
    const pps_map_chunk& c = m->chunks[src[j]];
    h_out[j] = o; o += c.count;
    h_src[j] = c.offset;
    const bool live = live_node(g, c.plane_id, NODE_PLANE);
    h_slot[j] = live ? g->nodes[c.plane_id].slot : -1;
    if (row_of) h_lm[j] = live ? row_of->at(c.plane_id) : -1;
  }
  h_out[ns] = o;
  if (posed) {
    memcpy(host.data() + at.fidx, plan.fidx.data(), ns * sizeof(int));
    memcpy(host.data() + at.recs, plan.recs.data(), plan.recs.size() * sizeof(MapFrameDev));
  }
  MAP_TRY(m, buf->reserve(at.bytes, g->stream, over));
  if (span) MAP_TRY(m, span->begin(g->stream));
  MAP_TRY(m, hipMemcpyAsync(buf->p, host.data(), at.bytes, hipMemcpyHostToDevice, g->stream));
  dev = buf->p;
  return PPS_OK;
}

void map_motion_plan(const pps_map* m, const std::vector<int>& src, MapMotionPlan* p) {
  const pps_graph* g = m->g;
  p->fidx.resize(src.size()); p->recs.clear(); p->n_unposed = 0;
  int last = -1;                                         // (chunks are in insertion order: the frames of src ascend)
  for (size_t j = 0; j < src.size(); j++) {
    const int f = m->chunks[src[j]].frame;
    if (f != last) {
      const MapFrameRec& r = m->frames[f];
      MapFrameDev d{};
      d.pose_slot = r.pose_id >= 0 && live_node(g, r.pose_id, NODE_POSE) ? g->nodes[r.pose_id].slot : -1;
      if (d.pose_slot >= 0) memcpy(d.T, r.T, sizeof d.T); else p->n_unposed++;
      p->recs.push_back(d);
      last = f;
    }
    p->fidx[j] = (int)p->recs.size() - 1;
  }
}

int map_motion_launch(pps_map* m, const MapSelection& s, MapMotionTable* t) {
  pps_graph* g = m->g;
  const size_t nf = s.plan.recs.size();
  MAP_TRY(m, m->d_motion.reserve(nf * (12 * sizeof(double) + sizeof(int)), g->stream, 2));
  MapMotionArgs a{};
  a.n_frames = (int)nf; a.recs = s.recs();
  a.pose_est = g->dev.pose_est; a.pose_ld = g->dev.pose_ld;
  a.motion = reinterpret_cast<double*>(m->d_motion.p);
  a.moved = reinterpret_cast<int*>(m->d_motion.p + nf * 12 * sizeof(double));
  MAP_TRY(m, m->t_motion.begin(g->stream));
  MAP_TRY(m, launch_map_motion(a, g->stream));
  MAP_TRY(m, m->t_motion.end(g->stream));
  m->n_motion = (int)nf; m->n_unposed = s.plan.n_unposed;
  t->fidx = s.fidx(); t->motion = a.motion; t->moved = a.moved;
  return PPS_OK;
}
}  // namespace pps_impl

extern "C" {

void pps_map_default_select(pps_map_select* s, int counter) {
  if (!s) return;
  s->counter = counter; s->every_frame = 0;
  s->old_age = 10; s->old_every = 3; s->new_every = 2;                          // main_3d.cpp:545-551
  s->age[0] = 15; s->min_tracked[0] = 10;                                       // :554-556
  s->age[1] = 8; s->min_tracked[1] = 5;                                         // :557-559
  s->age[2] = 4; s->min_tracked[2] = 2;                                         // :560-562
}

int pps_map_create(pps_graph* g, int64_t capacity_points, pps_map** out) {
  if (!g || !out || capacity_points < 0) return PPS_EINVAL;
  pps_map* m = new (std::nothrow) pps_map();
  if (!m) return PPS_ENOMEM;
  m->g = g; m->cap = capacity_points;
  *out = m;
  return PPS_OK;
}

int pps_map_destroy(pps_map* m) {
  if (!m) return PPS_EINVAL;
  if (m->on_device) {
    (void)hipSetDevice(m->g->props.device);
    if (m->g->stream) (void)hipStreamSynchronize(m->g->stream);
  }
  m->d_store.release(); m->d_built.release(); m->d_table.release(); m->d_sel.release(); m->d_dbg_cloud.release(); m->d_dbg_pid.release();
  m->d_motion.release();
  if (m->h_totals) (void)hipHostFree(m->h_totals);
  for (MapSpan* t : {&m->t_count, &m->t_scatter, &m->t_build, &m->t_motion, &m->t_posed}) t->release();
  map_grid_release(m);
  delete m;
  return PPS_OK;
}

const char* pps_map_last_error(const pps_map* m) { return m ? m->err.c_str() : "null handle"; }

}  // extern "C"

namespace {

// what both entry points of a frame ask of its plane list, answered on the host
int frame_planes_valid(pps_map* m, const char* who, int nplanes, const int* plane_node_ids) {
  if (nplanes < 0 || nplanes > kMapPlanes || (nplanes > 0 && !plane_node_ids)) return mfail(m, PPS_EINVAL, std::string(who) + ": nplanes outside 0 .. 65, or no ids");
  for (int k = 0; k < nplanes; k++)
    if (plane_node_ids[k] != -1 && !live_node(m->g, plane_node_ids[k], NODE_PLANE))
      return mfail(m, PPS_EINVAL, std::string(who) + ": plane_node_ids[" + std::to_string(k) + "] is not a live plane node");
  return PPS_OK;
}

// A frame from the point where its pixels are on the device (cloud, plane_id: npx records each, complete for the graph's stream): tiling,
// table growth, count + scan, the totals read back, the capacity check, scatter, the chunk table, counts and sec[0].
int add_points(pps_map* m, const char* who, const MapPt* cloud, const int* plane_id, int npx, int frame_seq_id, int nplanes,
               const int* plane_node_ids, int* counts, const float* run_T) {
  pps_graph* g = m->g;
  std::vector<int> cnt((size_t)nplanes, 0);
  int64_t kept = 0;
  MapScatterBase base;
  for (int k = 0; k < kMapPlanes; k++) base.base[k] = -1;
  m->sec[0] = 0;
  if (nplanes > 0) {
    int rc = ensure_device(g);
    if (rc != PPS_OK) return mfail(m, rc, g->err);
    rc = map_use_device(m);
    if (rc != PPS_OK) return rc;
    const MapTiling t = map_tiling(npx);
    MAP_TRY(m, m->d_table.reserve((size_t)kMapPlanes * t.nT + kMapPlanes, g->stream));
    if (!m->h_totals) MAP_TRY(m, hipHostMalloc(reinterpret_cast<void**>(&m->h_totals), kMapPlanes * sizeof(int), hipHostMallocDefault));
    MAP_TRY(m, m->d_store.reserve((size_t)m->cap, g->stream));
    int* d_totals = m->d_table.p + (size_t)kMapPlanes * t.nT;
    MAP_TRY(m, m->t_count.begin(g->stream));
    MAP_TRY(m, launch_map_count(cloud, plane_id, npx, nplanes, m->d_table.p, d_totals, g->stream));
    MAP_TRY(m, m->t_count.end(g->stream));
    MAP_TRY(m, hipMemcpyAsync(m->h_totals, d_totals, (size_t)nplanes * sizeof(int), hipMemcpyDeviceToHost, g->stream));
    MAP_TRY(m, hipStreamSynchronize(g->stream));
    for (int k = 0; k < nplanes; k++)
      if (plane_node_ids[k] >= 0) { cnt[k] = m->h_totals[k]; base.base[k] = m->used + kept; kept += cnt[k]; }
    if (kept > m->cap - m->used)
      return mfail(m, PPS_ENOMEM, std::string(who) + ": the frame keeps " + std::to_string(kept) + " points, the store has room for " + std::to_string(m->cap - m->used));
    m->sec[0] = m->t_count.seconds();
    if (kept > 0) {
      MAP_TRY(m, m->t_scatter.begin(g->stream));
      MAP_TRY(m, launch_map_scatter(cloud, plane_id, npx, nplanes, m->d_table.p, base, m->d_store.p, g->stream));
      MAP_TRY(m, m->t_scatter.end(g->stream));
      MAP_TRY(m, hipStreamSynchronize(g->stream));
      m->sec[0] += m->t_scatter.seconds();
    }
  }
  for (int k = 0; k < nplanes; k++) {
    if (plane_node_ids[k] < 0) continue;
    m->chunks.push_back(pps_map_chunk{m->n_frames, frame_seq_id, k, plane_node_ids[k], base.base[k], cnt[k]});
  }
  m->used += kept;
  MapFrameRec rec;                                       // (what pps_map_set_frame_pose with T_wc == NULL will use)
  rec.frame_seq_id = frame_seq_id;
  if (run_T) { rec.has_run_T = true; memcpy(rec.run_T, run_T, sizeof rec.run_T); }
  m->frames.push_back(rec);
  m->n_frames++;
  if (counts) for (int k = 0; k < nplanes; k++) counts[k] = cnt[k];
  return PPS_OK;
}

}  // namespace

extern "C" {

int pps_map_add_frame(pps_map* m, pps_popup* p, int frame_seq_id, int nplanes, const int* plane_node_ids, int* counts) {
  if (!m || !p) return mfail(m, PPS_EINVAL, "add_frame: null handle");
  int rc = frame_planes_valid(m, "add_frame", nplanes, plane_node_ids);
  if (rc != PPS_OK) return rc;
  PopupRunView v{};
  rc = popup_last_run(p, &v);
  if (rc != PPS_OK) return mfail(m, rc, std::string("add_frame: ") + pps_popup_last_error(p));
  if (v.device != m->g->props.device) return mfail(m, PPS_EINVAL, "add_frame: the pop-up context lives on another device than the graph");
  return add_points(m, "add_frame", reinterpret_cast<const MapPt*>(v.cloud), v.plane_id, v.width * v.height, frame_seq_id, nplanes,
                    plane_node_ids, counts, v.T_wc);
}

int pps_debug_map_add_points(pps_map* m, const pps_point* cloud, const int* plane_id, int64_t npx, int frame_seq_id, int nplanes,
                             const int* plane_node_ids, int* counts) {
  if (!m || !cloud || !plane_id) return mfail(m, PPS_EINVAL, "debug_add_points: null pointer");
  if (npx < 1 || npx > kMapMaxPixels) return mfail(m, PPS_EINVAL, "debug_add_points: npx outside 1 .. 2^30");
  int rc = frame_planes_valid(m, "debug_add_points", nplanes, plane_node_ids);
  if (rc != PPS_OK) return rc;
  if (nplanes > 0) {                                     // (a frame without planes reads no pixel, like add_frame)
    pps_graph* g = m->g;
    rc = ensure_device(g);
    if (rc != PPS_OK) return mfail(m, rc, g->err);
    rc = map_use_device(m);
    if (rc != PPS_OK) return rc;
    MAP_TRY(m, m->d_dbg_cloud.reserve((size_t)npx, g->stream));
    MAP_TRY(m, m->d_dbg_pid.reserve((size_t)npx, g->stream));
    MAP_TRY(m, hipMemcpyAsync(m->d_dbg_cloud.p, cloud, (size_t)npx * sizeof(MapPt), hipMemcpyHostToDevice, g->stream));
    MAP_TRY(m, hipMemcpyAsync(m->d_dbg_pid.p, plane_id, (size_t)npx * sizeof(int), hipMemcpyHostToDevice, g->stream));
  }
  return add_points(m, "debug_add_points", m->d_dbg_cloud.p, m->d_dbg_pid.p, (int)npx, frame_seq_id, nplanes, plane_node_ids, counts, nullptr);
}

int pps_map_redirect(pps_map* m, int from_plane, int to_plane) {
  if (!m) return PPS_EINVAL;
  const pps_graph* g = m->g;
  if (from_plane < 0 || from_plane >= (int)g->nodes.size() || g->nodes[from_plane].type != NODE_PLANE)
    return mfail(m, PPS_EINVAL, "redirect: from_plane is not a plane node of the graph");
  if (!live_node(g, to_plane, NODE_PLANE)) return mfail(m, PPS_EINVAL, "redirect: to_plane is not a live plane node");
  for (pps_map_chunk& c : m->chunks)
    if (c.plane_id == from_plane) c.plane_id = to_plane;
  return PPS_OK;
}

int pps_map_info(const pps_map* m, pps_map_totals* out) {
  if (!m || !out) return PPS_EINVAL;
  out->capacity = m->cap; out->n_points = m->used; out->built_points = m->built_points;
  out->n_frames = m->n_frames; out->n_chunks = (int)m->chunks.size(); out->built_chunks = (int)m->built.size(); out->reserved = 0;
  return PPS_OK;
}

int pps_map_chunks(const pps_map* m, int cap, pps_map_chunk* out, int* n) {
  return m ? map_table_copy(m->chunks.data(), m->chunks.size(), cap, out, n) : PPS_EINVAL;
}
int pps_map_built_chunks(const pps_map* m, int cap, pps_map_chunk* out, int* n) {
  return m ? map_table_copy(m->built.data(), m->built.size(), cap, out, n) : PPS_EINVAL;
}

int pps_map_select_host(const pps_map_chunk* chunks, int n, const pps_map_select* sel, int32_t* keep, int* n_keep) {
  if (n < 0 || (n > 0 && (!chunks || !keep)) || !select_valid(sel)) return PPS_EINVAL;
  select_chunks(chunks, n, sel, keep);
  if (n_keep) { int k = 0; for (int i = 0; i < n; i++) k += keep[i]; *n_keep = k; }
  return PPS_OK;
}

// pps_map_build and pps_map_build_posed: the selection and its one upload are the same; the posed build adds the per-chunk frame rows and
// the frame records to that upload, runs k_map_motion and the posed sibling of k_map_build.
static int build_common(pps_map* m, const pps_map_select* sel, bool posed, int64_t* n_points, int* n_chunks) {
  if (!m) return PPS_EINVAL;
  const char* who = posed ? "build_posed" : "build";
  if (!select_valid(sel)) return mfail(m, PPS_EINVAL, std::string(who) + ": old_every and new_every must be positive");
  pps_graph* g = m->g;
  MapSelection s;
  s.select(m, sel);
  std::vector<pps_map_chunk> built;
  int64_t total = 0;
  for (size_t i = 0; i < m->chunks.size(); i++) {
    if (!s.keep[i]) continue;
    pps_map_chunk c = m->chunks[i];
    c.offset = total; total += c.count;
    built.push_back(c);
  }
  if (posed) map_posed_reset(m);
  else m->sec[1] = 0;
  if (total > 0) {
    int rc = prepare_solve(g);
    if (rc != PPS_OK) return mfail(m, rc, g->err);
    rc = map_use_device(m);
    if (rc != PPS_OK) return rc;
    MAP_TRY(m, m->d_built.reserve((size_t)m->cap, g->stream));
    rc = s.upload(m, posed, nullptr, &m->d_sel, 2);
    if (rc != PPS_OK) return rc;
    MapBuildArgs a{};
    a.n_out = total; a.n_sel = s.n();
    a.out_off = s.out_off(); a.src_off = s.src_off(); a.slot = s.slot();
    a.plane_est = g->dev.plane_est; a.plane_ld = g->dev.plane_ld;
    a.store = m->d_store.p; a.built = m->d_built.p;
    if (posed) {
      MapMotionTable t{};
      rc = map_motion_launch(m, s, &t);
      if (rc != PPS_OK) return rc;
      MAP_TRY(m, m->t_posed.begin(g->stream));
      MAP_TRY(m, launch_map_build_posed(a, t, g->stream));
      MAP_TRY(m, m->t_posed.end(g->stream));
      MAP_TRY(m, hipStreamSynchronize(g->stream));
      m->posed_sec[0] = m->t_motion.seconds(); m->posed_sec[1] = m->t_posed.seconds();
      m->posed_launches = 2;
    } else {
      MAP_TRY(m, m->t_build.begin(g->stream));
      MAP_TRY(m, launch_map_build(a, g->stream));
      MAP_TRY(m, m->t_build.end(g->stream));
      MAP_TRY(m, hipStreamSynchronize(g->stream));            // (the selection leaves scope; the result is complete on return)
      m->sec[1] = m->t_build.seconds();
    }
  }
  m->built.swap(built);
  m->built_points = total;
  if (n_points) *n_points = total;
  if (n_chunks) *n_chunks = (int)m->built.size();
  return PPS_OK;
}

int pps_map_build(pps_map* m, const pps_map_select* sel, int64_t* n_points, int* n_chunks) { return build_common(m, sel, false, n_points, n_chunks); }
int pps_map_build_posed(pps_map* m, const pps_map_select* sel, int64_t* n_points, int* n_chunks) { return build_common(m, sel, true, n_points, n_chunks); }

int pps_map_set_frame_pose(pps_map* m, int frame, int pose_node_id, const float T_wc[16]) {
  if (!m) return PPS_EINVAL;
  if (frame < 0 || frame >= (int)m->frames.size()) return mfail(m, PPS_EINVAL, "set_frame_pose: unknown frame");
  MapFrameRec& r = m->frames[frame];
  if (pose_node_id == -1) { r.pose_id = -1; memset(r.T, 0, sizeof r.T); return PPS_OK; }
  if (!live_node(m->g, pose_node_id, NODE_POSE)) return mfail(m, PPS_EINVAL, "set_frame_pose: pose_node_id is not a live pose node");
  if (!T_wc && !r.has_run_T) return mfail(m, PPS_EINVAL, "set_frame_pose: the frame was not added from a pop-up run, T_wc must be given");
  const float* T = T_wc ? T_wc : r.run_T;
  if (!map_rigid(T)) return mfail(m, PPS_EINVAL, "set_frame_pose: T_wc is not a rigid transform (finite, last row 0 0 0 1, R^T R = I to 1e-4)");
  r.pose_id = pose_node_id;
  memcpy(r.T, T, sizeof r.T);
  return PPS_OK;
}

int pps_map_frames(const pps_map* m, int cap, pps_map_frame* out, int* n) {
  if (!m || !map_table_args(cap, out, n)) return PPS_EINVAL;
  *n = (int)m->frames.size();
  const size_t k = std::min<size_t>((size_t)cap, m->frames.size());
  for (size_t f = 0; f < k; f++) {
    const MapFrameRec& r = m->frames[f];
    out[f].frame = (int32_t)f; out[f].frame_seq_id = r.frame_seq_id; out[f].pose_id = r.pose_id; out[f].reserved = 0;
    memcpy(out[f].T_wc, r.T, sizeof r.T);
  }
  return PPS_OK;
}

int pps_map_frame_motions(pps_map* m, int cap, double* D, int32_t* moved, int* n) {
  if (!m || !n || cap < 0) return PPS_EINVAL;
  *n = m->n_motion;
  const size_t k = std::min<size_t>((size_t)cap, (size_t)m->n_motion);
  if (k == 0 || (!D && !moved)) return PPS_OK;
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  static_assert(sizeof(int32_t) == sizeof(int), "moved flags are int32");
  if (D) MAP_TRY(m, hipMemcpyAsync(D, m->d_motion.p, k * 12 * sizeof(double), hipMemcpyDeviceToHost, m->g->stream));
  if (moved) MAP_TRY(m, hipMemcpyAsync(moved, m->d_motion.p + (size_t)m->n_motion * 12 * sizeof(double), k * sizeof(int), hipMemcpyDeviceToHost, m->g->stream));
  MAP_TRY(m, hipStreamSynchronize(m->g->stream));
  return PPS_OK;
}

int pps_map_posed_last(const pps_map* m, double sec[2], int* launches, int* n_unposed_frames) {
  if (!m) return PPS_EINVAL;
  if (sec) { sec[0] = m->posed_sec[0]; sec[1] = m->posed_sec[1]; }
  if (launches) *launches = m->posed_launches;
  if (n_unposed_frames) *n_unposed_frames = m->n_unposed;
  return PPS_OK;
}

int pps_map_motion_host(const float T_wc[16], const double tq[7], double D[12]) {
  if (!T_wc || !tq || !D) return PPS_EINVAL;
  if (!map_rigid(T_wc)) return PPS_EINVAL;
  map_motion(T_wc, tq, D);
  return PPS_OK;
}

int pps_map_move_point_host(const double* D, const double* abcd, const float xyz[3], float out[3]) {
  if (!xyz || !out) return PPS_EINVAL;
  map_move_point(D, abcd, xyz[0], xyz[1], xyz[2], &out[0], &out[1], &out[2]);
  return PPS_OK;
}

int pps_map_download(pps_map* m, int which, int64_t first, int64_t n, pps_point* out) {
  if (!m) return PPS_EINVAL;
  if (which != 0 && which != 1) return mfail(m, PPS_EINVAL, "download: which is 0 (store) or 1 (built map)");
  const int64_t have = which == 0 ? m->used : m->built_points;
  if (first < 0 || n < 0 || first > have || n > have - first || (n > 0 && !out)) return mfail(m, PPS_EINVAL, "download: range outside the buffer");
  if (n == 0) return PPS_OK;
  MAP_TRY(m, hipSetDevice(m->g->props.device));
  const MapPt* src = (which == 0 ? m->d_store.p : m->d_built.p) + first;
  MAP_TRY(m, hipMemcpyAsync(out, src, (size_t)n * sizeof(MapPt), hipMemcpyDeviceToHost, m->g->stream));
  MAP_TRY(m, hipStreamSynchronize(m->g->stream));
  return PPS_OK;
}

int pps_map_last_times(const pps_map* m, double sec[2]) {
  if (!m || !sec) return PPS_EINVAL;
  sec[0] = m->sec[0]; sec[1] = m->sec[1];
  return PPS_OK;
}

}  // extern "C"

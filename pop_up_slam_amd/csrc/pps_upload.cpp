// pps_upload.cpp -- from the host tables to HBM: compaction + symbolic analysis (once per topology; incremental for frame
// loops), the two device arenas, the difference upload (pinned mirror: pps_upmirror.h; scatter kernel), state and measurement
// transfers.  pps_graph.h lists the other implementation files.
#include "pps_graph.h"

using namespace pps;
using namespace pps_impl;

namespace pps_impl {

#define TRY(x) do { const int rc_ = (x); if (rc_ != PPS_OK) return rc_; } while (0)      // (in the functions of this file that answer with a PPS_* code)

void free_device(pps_graph* g) {
  for (void* p : g->allocs) (void)hipFree(p);
  g->allocs.clear();
  UploadMirror& m = g->mirror;
  // arenas are kept; grow them when the last layout spilled into fallback allocations
  for (pps_graph::Arena* a : {&g->up, &g->scr}) {
    const size_t want = (a == &g->up ? std::max(a->off, m.high) : a->off) + a->spill;
    if (a->spill > 0 || a->base == nullptr) {
      if (a->base) (void)hipFree(a->base);
      a->cap = UploadMirror::grown_capacity(want);
      if (hipMalloc(reinterpret_cast<void**>(&a->base), a->cap) != hipSuccess) { a->base = nullptr; a->cap = 0; }
      if (a == &g->up) m.set_arena(a->cap);
    }
    a->off = 0; a->spill = 0;
  }
  m.begin_layout();
  if (m.mir_cap < g->up.cap) {                       // the pinned mirror: as large as the arena it describes
    if (m.mir) (void)hipHostFree(m.mir);
    char* p = nullptr;
    const bool ok = hipHostMalloc(reinterpret_cast<void**>(&p), g->up.cap, hipHostMallocDefault) == hipSuccess;
    m.set_mirror(ok ? p : nullptr, ok ? g->up.cap : 0);
  }
  g->dev = DevGraph();
}

void release_arenas(pps_graph* g) {
  for (pps_graph::Arena* a : {&g->up, &g->scr}) { if (a->base) (void)hipFree(a->base); a->base = nullptr; a->cap = a->off = a->spill = 0; }
  if (g->mirror.mir) (void)hipHostFree(g->mirror.mir);
  if (g->patch_host) (void)hipHostFree(g->patch_host);
  if (g->state_pin) (void)hipHostFree(g->state_pin);
  g->state_pin = nullptr; g->state_pin_cap = 0; g->pin_holds_est = false;
  g->patch_host = nullptr; g->patch_cap = 0;
  g->mirror.set_arena(0); g->mirror.set_mirror(nullptr, 0);
}

// an upload the arena has no room for (it is re-sized at the next upload): a plain allocation, copied at once
int upload_spilled(pps_graph* g, void** out, const void* src, size_t n, size_t bytes) {
  *out = nullptr;
  g->up.spill += bytes + bytes / 2 + 512;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return hip_fail(g, e, "hipMalloc");
  g->allocs.push_back(p);
  *out = p;
  if (n) HIP_TRY(g, hipMemcpy(p, src, n, hipMemcpyHostToDevice));
  return PPS_OK;
}

// send what the mirror recorded: everything in one copy when the device content is unknown, else the pieces
int flush_uploads(pps_graph* g) {
  // callers: upload_all (after its opening stream sync) and the frame tables of pps_refresh_measurements (which settles
  // up_inflight first) -- the pinned mirror and the patch table are never rewritten under a copy that still reads them
  UploadMirror& m = g->mirror;
  if (m.patches.empty()) return PPS_OK;
  if (m.unknown) HIP_TRY(g, hipMemcpyAsync(g->up.base, m.mir, m.whole_span(), hipMemcpyHostToDevice, g->stream));
  else {
    // the table in pinned host memory; k_scatter_patches reads the table AND the pieces -- straight from the pinned mirror -- over the bus
    // (round 6: no patch buffer, no host copy of the pieces into it, no copy launch in front of the kernel: 1.7 copies of 63 KB per frame of
    // the frame loop)
    const size_t need = m.patches.size() * 4 * sizeof(long long);
    if (need > g->patch_cap) {
      if (g->patch_host) (void)hipHostFree(g->patch_host);
      g->patch_host = nullptr; g->patch_cap = 0;
      const size_t cap = std::max<size_t>(1 << 12, 2 * need);
      HIP_TRY(g, hipHostMalloc(reinterpret_cast<void**>(&g->patch_host), cap, hipHostMallocDefault));
      g->patch_cap = cap;
    }
    m.write_table(reinterpret_cast<long long*>(g->patch_host));
    HIP_TRY(g, launch_scatter_patches(g->patch_host, m.mir, (int)m.patches.size(), g->up.base, g->stream));
    // (table and mirror are written again by the next upload_all / refresh, which wait for the stream first: up_inflight)
  }
  m.mark_flushed();
  return PPS_OK;
}

// PPS_DEBUG_VERIFY_UPLOAD=1: after a flush, the arena on the device must equal the pinned mirror (except the observation
// measurements, which kernels refresh behind the mirror's back) -- PPS_ESTATE if not.  tests/test_gpu_pipeline.py runs a frame
// loop under it.  verify_packed / verify_expanded / verify_frame_tables below check the mirror's content itself.
int verify_uploads(pps_graph* g, const char* where) {
  const UploadMirror& m = g->mirror;
  if (g->mirror.take_violation()) return fail(g, PPS_ESTATE, std::string("upload verification (") + where + "): an array differs from the mirror inside the part the analysis reported as kept");
  if (!g->sw.verify_upload || m.high == 0 || g->up.spill) return PPS_OK;
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  std::vector<char> dev(m.high);
  HIP_TRY(g, hipMemcpy(dev.data(), g->up.base, m.high, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < m.slots.size() && k < m.cursor; k++) {
    const UploadMirror::Slot& sl = m.slots[k];
    if (sl.owner == &g->dev.obs_meas || sl.owner == &g->dev.lp_meas || sl.off >= m.high) continue;
    const size_t o = sl.off, n = std::min(sl.cap, m.high - o);
    if (memcmp(dev.data() + o, m.mir + o, n) != 0) {
      size_t b = 0; while (b < n && dev[o + b] == m.mir[o + b]) b++;
      return fail(g, PPS_ESTATE, std::string("upload verification (") + where + "): slot " + std::to_string(k) + " (offset " + std::to_string(o) + ", capacity " +
                                     std::to_string(sl.cap) + ") differs from the mirror at byte " + std::to_string(b));
    }
  }
  return PPS_OK;
}

// ---- PPS_DEBUG_VERIFY_UPLOAD=1, beyond the mirror: what the device holds against what the host records say it should hold ----
// The mirror check above passes when a shortcut (incr_pack, pk_meas_ok, a kept prefix) has packed the mirror wrongly: these start
// from the host factor records and from the Analysis again.  tests/test_gpu_upload_states.py runs every upload path under them.
static int verify_fail(pps_graph* g, const char* where, const char* array, const char* against, size_t index) {
  return fail(g, PPS_ESTATE, std::string("upload verification (") + where + "): " + array + " differs from " + against + " at index " + std::to_string(index));
}
// rows x [exempt, used) of an SoA array with leading dimension ld (rows == 1, ld == used: a plain array): `have` against `want`
template <class T>
static int verify_rows(pps_graph* g, const char* where, const char* array, const char* against, const T* have, const T* want, size_t rows, size_t ld,
                       size_t used, size_t exempt = 0) {
  for (size_t r = 0; r < rows; r++)
    for (size_t s = exempt; s < used; s++)
      if (memcmp(&have[r * ld + s], &want[r * ld + s], sizeof(T)) != 0) return verify_fail(g, where, array, against, r * ld + s);
  return PPS_OK;
}
// ... the same with `have` on the device
template <class T>
static int verify_dev_rows(pps_graph* g, const char* where, const char* array, const char* against, const T* dev, const T* want, size_t rows, size_t ld,
                           size_t used, size_t exempt = 0) {
  if (rows * ld == 0 || used == 0) return PPS_OK;
  std::vector<T> have(rows * ld);
  HIP_TRY(g, hipMemcpy(have.data(), dev, have.size() * sizeof(T), hipMemcpyDeviceToHost));
  return verify_rows(g, where, array, against, have.data(), want, rows, ld, used, exempt);
}

// a. The arrays upload_all maintains incrementally (pk_*: plane observations and odometry) packed again from the host factor records:
// what was staged and what the device holds must both equal them.  kept_meas_rows: the leading rows of obs_meas that keep_meas left to the
// device, where a refresh has written values the host does not have -- exactly those are exempt, and only on the device side.
struct SideOnDevice { size_t ld; const int *a, *b; const double *m, *w; const char* names[4]; size_t exempt; };
static int verify_side(pps_graph* g, const pps_graph::PackedSide& S, const SideOnDevice& D) {
  const char* where = "upload_all";
  const char* scratch = "a pack from the host factor records";
  const std::vector<int>& ids = g->fslot_ids[S.type];
  const size_t n = ids.size(), ld = D.ld, km = (size_t)S.km, kw = (size_t)S.kw;
  if (n == 0) return PPS_OK;
  if (S.a.size() < n || S.b.size() < n || S.m.size() < km * ld || S.w.size() < kw * ld) return verify_fail(g, where, D.names[0], "the slot count (staged arrays too short)", n);
  std::vector<int> ia(n), ib(n);
  std::vector<double> pm(km * ld, 0.0), pw(kw * ld, 0.0);
  for (size_t s = 0; s < n; s++) {
    const HostFactor& f = g->factors[ids[s]];
    if (f.deleted || f.slot != (int)s) return verify_fail(g, where, D.names[0], "the slot table (deleted factor or wrong slot)", s);
    ia[s] = g->nodes[f.a].slot; ib[s] = g->nodes[f.b].slot;
    for (size_t k = 0; k < km; k++) pm[k * ld + s] = f.meas[k];
    for (size_t k = 0; k < kw; k++) pw[k * ld + s] = f.w[k];
  }
  TRY(verify_rows(g, where, D.names[0], scratch, S.a.data(), ia.data(), 1, n, n));
  TRY(verify_rows(g, where, D.names[1], scratch, S.b.data(), ib.data(), 1, n, n));
  TRY(verify_rows(g, where, D.names[2], scratch, S.m.data(), pm.data(), km, ld, n));
  TRY(verify_rows(g, where, D.names[3], scratch, S.w.data(), pw.data(), kw, ld, n));
  const char* scratch_dev = "a pack from the host factor records (device side)";
  TRY(verify_dev_rows(g, where, D.names[0], scratch_dev, D.a, ia.data(), 1, n, n));
  TRY(verify_dev_rows(g, where, D.names[1], scratch_dev, D.b, ib.data(), 1, n, n));
  TRY(verify_dev_rows(g, where, D.names[2], scratch_dev, D.m, pm.data(), km, ld, n, std::min(n, D.exempt)));
  return verify_dev_rows(g, where, D.names[3], scratch_dev, D.w, pw.data(), kw, ld, n);
}
static int verify_packed(pps_graph* g, size_t kept_meas_rows) {
  if (!g->sw.verify_upload) return PPS_OK;
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  const DevGraph& d = g->dev;
  const int rc = verify_side(g, g->pk_obs, {(size_t)d.obs_ld, d.obs_pose, d.obs_plane, d.obs_meas, d.obs_w, {"obs_pose", "obs_plane", "obs_meas", "obs_w"}, kept_meas_rows});
  return rc != PPS_OK ? rc : verify_side(g, g->pk_odo, {(size_t)d.odo_ld, d.odo_a, d.odo_b, d.odo_meas, d.odo_w, {"odo_a", "odo_b", "odo_meas", "odo_w"}, 0});
}

// b. ea_tgt, el_tgt and blk_dst as the expansion launch left them (k_expand_lists, or k_expand_ea + fills + k_expand_el) against
// expand_ea_tgt / expand_el_lists on a copy of the Analysis; blk_dst entries that no front gathers are -1 on both sides.
// c. The block behind delta (dn partials, tickets, result records, both deltas, hand-over flags) reads back as zeros.
// The zeroed block behind delta, in doubles from its start: [dn_partials | ticket | spec ticket | result record | the second factorisation's
// result record | delta | the second delta | the hand-over flags of the whole-tree launches: 4 ints per front].  Cleared by the expansion
// launch of upload_all (or by a memset when that launch has nothing to expand).
struct ZeroBlock {
  size_t n_dn, dn_partials = 0, ticket, spec_ticket, result, spec_result, delta, spec_delta, flags, total;
  ZeroBlock(int n_nodes, int n_scalars, int n_fronts) : n_dn((size_t)(n_nodes + 255) / 256 + 1) {
    const size_t delta_doubles = (size_t)std::max(1, n_scalars);
    ticket = n_dn; spec_ticket = ticket + 1; result = spec_ticket + 1; spec_result = result + 4; delta = spec_result + 4;
    spec_delta = delta + delta_doubles; flags = spec_delta + delta_doubles; total = flags + 2 * (size_t)std::max(1, n_fronts) + 1;
  }
};
static int verify_expanded(pps_graph* g, const double* zero_block, const ZeroBlock& Z) {
  if (!g->sw.verify_upload) return PPS_OK;
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  const DevGraph& d = g->dev;
  const char* where = "upload_all";
  Analysis A = g->an;
  expand_ea_tgt(A);
  expand_el_lists(A);
  TRY(verify_dev_rows(g, where, "ea_tgt", "expand_ea_tgt on the host", d.ea_tgt, A.ea_tgt.data(), 1, A.ea_tgt.size(), A.ea_tgt.size()));
  if (!A.el_tgt.empty()) {
    // (entry by entry of every assembled block: an element no block claims is written by nobody, on either side)
    std::vector<int> have(A.el_tgt.size());
    HIP_TRY(g, hipMemcpy(have.data(), d.el_tgt, have.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (size_t a = 0; a < A.asm_blk.size(); a++) {
      const int blk = A.asm_blk[a], rows = A.blk_rows[blk], cols = A.blk_cols[blk];
      const size_t cnt = A.blk_size[blk] != rows * cols ? (size_t)rows * (rows + 1) / 2 + rows : (size_t)rows * cols, e0 = (size_t)A.asm_el0[a];
      if (e0 + cnt > have.size()) return verify_fail(g, where, "asm_el0", "the length of el_tgt", a);
      for (size_t e = e0; e < e0 + cnt; e++)
        if (have[e] != A.el_tgt[e]) return verify_fail(g, where, "el_tgt", "expand_el_lists on the host", e);
    }
  }
  TRY(verify_dev_rows(g, where, "blk_dst", "expand_el_lists on the host", d.blk_dst, A.blk_dst.data(), 1, A.blk_dst.size(), A.blk_dst.size()));
  const std::vector<double> zeros(Z.total, 0.0);
  return verify_dev_rows(g, where, "the zeroed block behind delta", "zero", zero_block, zeros.data(), 1, Z.total, Z.total);
}

// The frame tables of pps_refresh_measurements after their flush: the cached slot tables (extended, not rebuilt, while nothing is removed)
// against tables built from the factor and node records, and all six tables on the device against the host's.  The slot rule itself (a live,
// fixed observation of a live pose, else -1) is restated from pps_frames.cpp, not checked: this pins the cache and the transfer, the rule is
// pinned by the measurements the refresh then writes (tests/test_gpu_upload_states.py holds every one of them to the pop-up's statement).
int verify_frame_tables(pps_graph* g) {
  if (!g->sw.verify_upload) return PPS_OK;
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  const char* where = "frames";
  std::vector<int> slot(g->fr_item_fid.size()), pslot(g->fr_pose.size());
  for (size_t i = 0; i < slot.size(); i++) {
    const int fid = g->fr_item_fid[i];
    slot[i] = (fid >= 0 && !g->factors[fid].deleted && !g->factors[fid].repop) ? g->factors[fid].slot : -1;
    if (slot[i] >= 0 && g->nodes[g->fr_pose[g->fr_item_frame[i]]].deleted) slot[i] = -1;
  }
  for (size_t f = 0; f < pslot.size(); f++) pslot[f] = g->nodes[g->fr_pose[f]].deleted ? 0 : g->nodes[g->fr_pose[f]].slot;
  if (g->fr_slot.size() != slot.size()) return verify_fail(g, where, "item_slot", "the number of registered items", std::min(slot.size(), g->fr_slot.size()));
  if (g->fr_pslot.size() != pslot.size()) return verify_fail(g, where, "frame_pose_slot", "the number of registered frames", std::min(pslot.size(), g->fr_pslot.size()));
  const char* scratch = "tables built from the factor and node records";
  const char* host = "the host tables (device side)";
  TRY(verify_rows(g, where, "item_slot", scratch, g->fr_slot.data(), slot.data(), 1, slot.size(), slot.size()));
  TRY(verify_rows(g, where, "frame_pose_slot", scratch, g->fr_pslot.data(), pslot.data(), 1, pslot.size(), pslot.size()));
  TRY(verify_dev_rows(g, where, "item_frame", host, g->d_item_frame, g->fr_item_frame.data(), 1, g->fr_item_frame.size(), g->fr_item_frame.size()));
  TRY(verify_dev_rows(g, where, "item_plane", host, g->d_item_plane, g->fr_item_plane.data(), 1, g->fr_item_plane.size(), g->fr_item_plane.size()));
  TRY(verify_dev_rows(g, where, "item_slot", host, g->d_item_slot, slot.data(), 1, slot.size(), slot.size()));
  TRY(verify_dev_rows(g, where, "frame_pose_slot", host, g->d_frame_pose_slot, pslot.data(), 1, pslot.size(), pslot.size()));
  TRY(verify_dev_rows(g, where, "frame_seg_off", host, g->d_frame_seg_off, g->fr_seg_off.data(), 1, g->fr_seg_off.size(), g->fr_seg_off.size()));
  TRY(verify_dev_rows(g, where, "fr_seg", host, g->d_fr_seg, g->fr_seg.data(), 1, g->fr_seg.size(), g->fr_seg.size()));
  return PPS_OK;
}

int ensure_device(pps_graph* g) {
  if (g->dev_ready) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  HIP_TRY(g, hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
  HIP_TRY(g, hipHostMalloc(reinterpret_cast<void**>(&g->host_result), 12 * sizeof(double), hipHostMallocDefault));
  HIP_TRY(g, hipEventCreate(&g->ev[0]));
  HIP_TRY(g, hipEventCreate(&g->ev[1]));
  g->dev_ready = true;
  return PPS_OK;
}

// Offsets of the four per-type slabs of the J buffer: [plane obs | odometry | pose priors | plane priors].  Every slab is
// sized for a capacity that grows in powers of two, so that a graph that gains a few factors per frame keeps all of its J
// offsets -- and with them the whole contribution list of the H-block kernel -- from one frame to the next.
int64_t j_capacity(int64_t n) { int64_t c = 16; while (c < n) c <<= 1; return c; }
// (size: kJSize, or kPSize for the product records, in slabs of the same capacities: a product offset moves exactly when the J offset does)
void slab_bases(const pps_graph* g, const int size[4], int64_t base[4], int64_t* total) {
  int64_t off = 0;
  for (int t : {F_PLANE_OBS, F_ODOMETRY, F_POSE_PRIOR, F_PLANE_PRIOR}) { base[t] = off; off += j_capacity((int64_t)g->fslot_ids[t].size()) * size[t]; }
  if (total) *total = off;
}

// ---- compaction + symbolic analysis (host only) -------------------------------------------
static int run_analysis_impl(pps_graph* g);
// A failed analysis may have rewritten g->an in place (the incremental path) before it gave up: the handle is marked as not
// analysed, so that no later upload sends a half-rewritten Analysis to the device -- the next solve runs the analysis again.
int run_analysis(pps_graph* g) {
  const int rc = run_analysis_impl(g);
  if (rc != PPS_OK) { g->analyzed = false; g->analysis_stale = true; g->topo_dirty = true; g->cmp_valid = false; g->an_seq++; g->an_base_seq = -1; }
  return rc;
}
// host node i joins the compacted tables: the next compact id and the next slot of its type
static void compact_node(pps_graph* g, size_t i) {
  HostNode& n = g->nodes[i];
  n.compact = (int)g->sym_nodes.size();
  if (n.type == NODE_POSE) { n.slot = (int)g->pose_ids.size(); g->pose_ids.push_back((int)i); g->sym_nodes.push_back({NODE_POSE, 6, n.slot}); }
  else { n.slot = (int)g->plane_ids.size(); g->plane_ids.push_back((int)i); g->sym_nodes.push_back({NODE_PLANE, 3, -1}); }
}
// the analysis' view of a live factor whose slot is assigned (base / pbase: j_bases / p_bases)
static SymFactor sym_factor_of(const pps_graph* g, const HostFactor& f, const int64_t base[4], const int64_t pbase[4]) {
  SymFactor q;
  q.type = f.type;
  q.a = g->nodes[f.a].compact;
  q.b = f.b >= 0 ? g->nodes[f.b].compact : -1;
  q.joff = (int)(base[f.type] + (int64_t)f.slot * kJSize[f.type]);
  q.poff = (int)(pbase[f.type] + (int64_t)f.slot * kPSize[f.type]);
  q.direct_ok = (f.type == F_PLANE_OBS && !f.repop) ? 1 : 0;
  return q;
}
static int run_analysis_impl(pps_graph* g) {
  const double t0 = now_s();
  std::vector<SymNode>& sn = g->sym_nodes;
  std::vector<SymFactor>& sf = g->sym_factors;
  // A graph that only grew since the last analysis (the frame loop) appends to the compacted tables instead of walking
  // every node and factor again; re-popping edges are ordered behind the fixed ones, which moves slots: they take the full path.
  bool append = g->cmp_valid && g->grown_only && g->n_analyses > 0 && !g->cmp_has_repop && g->cmp_nodes <= g->nodes.size() &&
                g->cmp_factors <= g->factors.size() && !g->sw.no_incr_compact;
  for (size_t i = g->cmp_factors; append && i < g->factors.size(); i++)
    append = !g->factors[i].deleted && !(g->factors[i].type == F_PLANE_OBS && g->factors[i].repop);
  for (size_t i = g->cmp_nodes; append && i < g->nodes.size(); i++) append = !g->nodes[i].deleted;
  if (append) {
    for (size_t i = g->cmp_nodes; i < g->nodes.size(); i++) compact_node(g, i);
    for (size_t i = g->cmp_factors; i < g->factors.size(); i++) {
      HostFactor& f = g->factors[i];
      f.slot = (int)g->fslot_ids[f.type].size();
      g->fslot_ids[f.type].push_back((int)i);
    }
    g->n_obs_fixed = (int)g->fslot_ids[F_PLANE_OBS].size();
  } else {
    g->pose_ids.clear(); g->plane_ids.clear();
    for (int t = 0; t < 4; t++) g->fslot_ids[t].clear();
    sn.clear(); sf.clear();
    for (size_t i = 0; i < g->nodes.size(); i++) {
      if (g->nodes[i].deleted) g->nodes[i].compact = g->nodes[i].slot = -1;
      else compact_node(g, i);
    }
    // plane observations with a fixed measurement first, the re-popping ones (Factor2) behind them
    g->cmp_has_repop = false;
    for (int pass = 0; pass < 2; pass++)
      for (size_t i = 0; i < g->factors.size(); i++) {
        HostFactor& f = g->factors[i];
        if (f.deleted) { f.slot = -1; continue; }
        if ((f.type == F_PLANE_OBS && f.repop) != (pass == 1)) continue;
        if (pass == 1) g->cmp_has_repop = true;
        f.slot = (int)g->fslot_ids[f.type].size();
        g->fslot_ids[f.type].push_back((int)i);
      }
    g->n_obs_fixed = 0;
    for (int id : g->fslot_ids[F_PLANE_OBS]) g->n_obs_fixed += g->factors[id].repop ? 0 : 1;
    sf.reserve(g->factors.size());
  }
  int64_t base[4], j_total = 0, pbase[4], p_total = 0;
  j_bases(g, base, &j_total);
  p_bases(g, pbase, &p_total);
  if (j_total > 0x7fffffffLL || p_total > 0x7fffffffLL) return fail(g, PPS_ENOMEM, "graph too large for int32 J offsets");
  if (append && memcmp(base, g->cmp_base, sizeof(base)) != 0) {          // a J slab outgrew its capacity: every offset moves
    int cnt[4] = {0, 0, 0, 0};
    for (SymFactor& q : sf) { const int k = cnt[q.type]++; q.joff = (int)(base[q.type] + (int64_t)k * kJSize[q.type]); q.poff = (int)(pbase[q.type] + (int64_t)k * kPSize[q.type]); }
  }
  memcpy(g->cmp_base, base, sizeof(base));
  bool any_deleted = false;
  for (size_t i = append ? g->cmp_factors : 0; i < g->factors.size(); i++) {
    if (g->factors[i].deleted) any_deleted = true;
    else sf.push_back(sym_factor_of(g, g->factors[i], base, pbase));
  }
  // the append path relies on: table index == host index order with nothing skipped
  if (!append) g->cmp_valid = !any_deleted && sn.size() == g->nodes.size();
  g->cmp_nodes = g->nodes.size(); g->cmp_factors = g->factors.size();
  // band depth: 3 levels per launch when the solve is latency bound, 2 when the lower levels are throughput bound (C3: 5 360 fronts;
  // 637 vs 710 us).  (Up to round 4: 4 levels, 113.3 vs 115.0 us per C2 LM iteration with 3.  Round 5: a group of 4 + 2 + 1 fronts on
  // eight waves has a wave for every front, so every separator front is assembled ahead of its level while the leaves are eliminated,
  // and the top group -- levels 6 .. 8 of C2's nine -- is factored and solved by one launch with the data-flow back-substitution:
  // 60.9 against 63.7 us per C2 LM iteration with 4, same box.)
  g->aprm.band_levels = 0;        // chosen by the analysis from the tree: three levels per band below 2 400 poses, four above -- two where a front needs the fifteen-tile kernel (pps_symbolic.cpp)
  // H-block segments (contributions reduced by one wave of K2): short on small graphs, where the few long segments
  // (ground plane, 32 contributions = 16 dependent load rounds) are K2's critical path; long on large ones, where the
  // number of waves is (C2: 23.3 -> 18.7 us with 8; C3: 82 -> 102 us)
  // (round 4: a plane observation reaches K2 as ONE coalesced load per lane -- its product record -- so a wave sums up to 64
  // contributions per segment: every landmark but the ground plane is one segment, and no second reduction pass)
  g->aprm.seg_len = 64;
  // a graph that is re-analysed after pure appends is a frame loop: absolute cut positions keep the left part of its tree
  g->aprm.aligned_cuts = (g->n_analyses > 0 && g->grown_only) ? 1 : 0;
  // ... whose groups of 4 leaves (3 levels per launch) keep every front of a level on its own wave (C5: 1 580 vs 1 500 frames/s; up to round 5
  // its aligned cuts also left fronts of 65 .. 80 rows: AnalysisParams::front_rows / cut_shift now keep every front of the loop within 63)
  if (g->aprm.aligned_cuts && g->pose_ids.size() < 4000) g->aprm.band_levels = 3;
  g->aprm.band_rows = band_front_limit();
  const char* msg = "";
  try {
  if (g->sw.analysis_timing) fprintf(stderr, "[analysis] %-22s %8.3f ms\n", "compaction (api)", 1e3 * (now_s() - t0));
  if (!g->acache) g->acache = analysis_cache_new();
  if (!analyze(sn, sf, g->aprm, g->an, &msg, g->sw.no_incremental ? nullptr : g->acache))
    return fail(g, PPS_EINVAL, std::string("analysis failed: ") + msg);
  // fronts beyond the wave-per-front kernels (loop-closure separators) run in the dense-front form, whose cost is
  // per tree level: split their supernodes into 64-pivot chunks instead of 48 (a quarter fewer levels)
  if (g->an.max_front > band_front_limit() && g->aprm.max_pivots < dense_front_max_pivots()) {
    AnalysisParams wide = g->aprm;
    wide.max_pivots = dense_front_max_pivots();
    if (!analyze(sn, sf, wide, g->an, &msg, g->sw.no_incremental ? nullptr : g->acache))
      return fail(g, PPS_EINVAL, std::string("analysis failed: ") + msg);
  }
  } catch (const std::bad_alloc&) {
    g->an = Analysis();
    return fail(g, PPS_ENOMEM, "symbolic analysis ran out of host memory (fronts too wide for this ordering)");
  }
  // how K3 runs on this tree -- band kernels per stage or whole tree, dense fronts, or a launch per level -- and the geometry of every launch
  g->plan = plan_k3(k3_tree_view(g->an), K3Switches{g->sw.no_preassemble, g->sw.no_solve_flow, g->sw.no_root_fuse, g->sw.no_strip, g->sw.trace});
  if (!g->use_band() && !g->use_dense() && g->an.max_front > 4096)
    return fail(g, PPS_ENOMEM, "fronts too wide for this ordering (max front " + std::to_string(g->an.max_front) +
                               " scalars): the pose chain is not a good dissection backbone for this graph");
  if (g->sw.analysis_timing) fprintf(stderr, "[analysis] %-22s %8.3f ms\n", "total incl. api", 1e3 * (now_s() - t0));
  g->analyzed = true; g->analysis_stale = false;
  g->n_analyses++; g->grown_only = true;
  g->an_base_seq = g->an_seq; g->an_seq++;                // (an.kept is relative to the analysis this one replaced)
  g->stats.n_fronts = g->an.n_fronts; g->stats.n_levels = g->an.n_levels; g->stats.max_front = g->an.max_front;
  g->stats.nnz_L = g->an.L_size;
  g->stats.t_analysis = now_s() - t0;
  return PPS_OK;
}

// pinned staging for the estimate (pose rows, then plane rows): copies to and from pageable memory are staged by the runtime
// and cost a synchronisation each
int state_pin_reserve(pps_graph* g, size_t doubles) {
  if (doubles <= g->state_pin_cap) return PPS_OK;
  if (g->up_inflight) { HIP_TRY(g, hipStreamSynchronize(g->stream)); g->up_inflight = false; }
  if (g->state_pin) (void)hipHostFree(g->state_pin);
  g->state_pin = nullptr; g->state_pin_cap = 0; g->pin_holds_est = false;
  const size_t cap = std::max<size_t>(4096, 2 * doubles);
  HIP_TRY(g, hipHostMalloc(reinterpret_cast<void**>(&g->state_pin), cap * sizeof(double), hipHostMallocDefault));
  g->state_pin_cap = cap;
  return PPS_OK;
}

// pull the device estimate back into the host node table
// The solves end with this: the estimate travels to the pinned buffer behind their last kernels and arrives with the
// synchronisation they end with anyway -- whoever reads a value next (a frame loop does, every frame) finds it on the host
// instead of paying a copy and a synchronisation of its own.  Call before that synchronisation, state_download_arrived() after it.
int enqueue_state_download(pps_graph* g) {
  const DevGraph& d = g->dev;
  const size_t np = (size_t)7 * d.pose_ld, nl = (size_t)4 * d.plane_ld;
  g->pin_holds_est = false;
  int rc = state_pin_reserve(g, np + nl);
  if (rc != PPS_OK) return rc;
  HIP_TRY(g, hipMemcpyAsync(g->state_pin, d.pose_est, (np + nl) * 8, hipMemcpyDeviceToHost, g->stream));   // [poses | planes], one block
  return PPS_OK;
}
void state_download_arrived(pps_graph* g) { g->pin_holds_est = true; }

int download_state(pps_graph* g) {
  if (!g->dev_values_newer) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  const DevGraph& d = g->dev;
  if (!g->pin_holds_est) {
    int rc = enqueue_state_download(g);
    if (rc != PPS_OK) return rc;
    HIP_TRY(g, hipStreamSynchronize(g->stream));
  }
  g->pin_holds_est = false;
  double* bp = g->state_pin; double* bl = g->state_pin + (size_t)7 * d.pose_ld;
  for (int s = 0; s < d.n_pose; s++) for (int k = 0; k < 7; k++) g->nodes[g->pose_ids[s]].v[k] = bp[(size_t)k * d.pose_ld + s];
  for (int s = 0; s < d.n_plane; s++) for (int k = 0; k < 4; k++) g->nodes[g->plane_ids[s]].v[k] = bl[(size_t)k * d.plane_ld + s];
  g->dev_values_newer = false;
  return PPS_OK;
}

int upload_state(pps_graph* g, bool sync) {
  DevGraph& d = g->dev;
  if (g->up_inflight) { HIP_TRY(g, hipStreamSynchronize(g->stream)); g->up_inflight = false; }   // the staging buffer is still being read
  const size_t np = (size_t)7 * d.pose_ld, nl = (size_t)4 * d.plane_ld;
  int rc = state_pin_reserve(g, np + nl);
  if (rc != PPS_OK) return rc;
  double* bp = g->state_pin; double* bl = g->state_pin + np;
  g->pin_holds_est = false;
  for (int k = 0; k < 7; k++) for (int s = d.n_pose; s < d.pose_ld; s++) bp[(size_t)k * d.pose_ld + s] = 0.0;
  for (int k = 0; k < 4; k++) for (int s = d.n_plane; s < d.plane_ld; s++) bl[(size_t)k * d.plane_ld + s] = 0.0;
  for (int s = 0; s < d.n_pose; s++) for (int k = 0; k < 7; k++) bp[(size_t)k * d.pose_ld + s] = g->nodes[g->pose_ids[s]].v[k];
  for (int s = 0; s < d.n_plane; s++) for (int k = 0; k < 4; k++) bl[(size_t)k * d.plane_ld + s] = g->nodes[g->plane_ids[s]].v[k];
  HIP_TRY(g, hipMemcpyAsync(d.pose_est, bp, (np + nl) * 8, hipMemcpyHostToDevice, g->stream));
  // (the linearisation point is set by whoever linearises next: copy_state / linpoint_from_estimate)
  if (sync) HIP_TRY(g, hipStreamSynchronize(g->stream));
  else g->up_inflight = true;
  g->host_values_newer = false;
  return PPS_OK;
}

// SoA with leading dimension ld (>= count): value k of slot s at [k * ld + s]
template <int K>
void pack_soa(const pps_graph* g, int type, bool weights, std::vector<double>& out, size_t ld) {
  const std::vector<int>& ids = g->fslot_ids[type];
  const size_t n = ids.size();
  out.assign((size_t)K * ld, 0.0);
  for (size_t s = 0; s < n; s++) {
    const HostFactor& f = g->factors[ids[s]];
    const double* src = weights ? f.w : f.meas;
    for (int k = 0; k < K; k++) out[(size_t)k * ld + s] = src[k];
  }
}

// pull device-refreshed plane-observation measurements back into the host factor table
int download_measurements(pps_graph* g) {
  if (!g->dev_meas_newer) return PPS_OK;
  HIP_TRY(g, hipSetDevice(g->props.device));
  const DevGraph& d = g->dev;
  const size_t n = g->fslot_ids[F_PLANE_OBS].size(), ld = (size_t)d.obs_ld;
  std::vector<double> m((size_t)4 * ld);
  if (n) HIP_TRY(g, hipMemcpyAsync(m.data(), d.obs_meas, m.size() * 8, hipMemcpyDeviceToHost, g->stream));
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  for (size_t s2 = 0; s2 < n && s2 < (size_t)d.n_obs; s2++) {
    HostFactor& f = g->factors[g->fslot_ids[F_PLANE_OBS][s2]];
    for (int k = 0; k < 4; k++) f.meas[k] = m[(size_t)k * ld + s2];
  }
  g->dev_meas_newer = false;
  g->pk_meas_ok = false;
  return PPS_OK;
}

int upload_measurements(pps_graph* g) {
  DevGraph& d = g->dev;
  std::vector<double> m;
  pack_soa<4>(g, F_PLANE_OBS, false, m, (size_t)d.obs_ld);
  if (d.n_obs) HIP_TRY(g, hipMemcpyAsync(d.obs_meas, m.data(), m.size() * 8, hipMemcpyHostToDevice, g->stream));
  std::vector<double> m2;
  pack_soa<4>(g, F_PLANE_PRIOR, false, m2, (size_t)d.lp_ld);
  if (d.n_lp) HIP_TRY(g, hipMemcpyAsync(d.lp_meas, m2.data(), m2.size() * 8, hipMemcpyHostToDevice, g->stream));
  // (the upload mirror no longer describes these arrays: the next topology upload sends them whole)
  g->mirror.forget_measurements();
  HIP_TRY(g, hipStreamSynchronize(g->stream));
  g->meas_dirty = false;
  return PPS_OK;
}

// the appended slots of one packed side (every slot unless the id list of the last pack is a prefix of today's and the leading dimension is
// unchanged); repack_meas: the host's measurements changed since, the rows of the old slots again.  Returns the first slot it packed.
// (One pass over the factors: a HostFactor is 300 bytes, a pass per array was four times the memory traffic.)
static size_t pack_side(const pps_graph* g, pps_graph::PackedSide& S, size_t ld, bool incr, bool repack_meas) {
  const std::vector<int>& ids = g->fslot_ids[S.type];
  const size_t n = ids.size(), km = (size_t)S.km, kw = (size_t)S.kw;
  size_t s_begin = 0;
  if (incr && S.ld == ld && S.n <= n && S.m.size() == km * ld && S.ids.size() == S.n && std::equal(S.ids.begin(), S.ids.end(), ids.begin()))
    s_begin = S.n;                                     // (re-popping edges sit behind the fixed ones: their slots move)
  S.a.resize(n); S.b.resize(n); S.m.resize(km * ld); S.w.resize(kw * ld);
  for (size_t s = s_begin; s < n; s++) {
    const HostFactor& f = g->factors[ids[s]];
    S.a[s] = g->nodes[f.a].slot; S.b[s] = g->nodes[f.b].slot;
    for (size_t k = 0; k < km; k++) S.m[k * ld + s] = f.meas[k];
    for (size_t k = 0; k < kw; k++) S.w[k * ld + s] = f.w[k];
  }
  for (size_t s = 0; repack_meas && s < s_begin; s++) { const HostFactor& f = g->factors[ids[s]]; for (size_t k = 0; k < km; k++) S.m[k * ld + s] = f.meas[k]; }
  S.n = n; S.ld = ld; S.ids.resize(s_begin); S.ids.insert(S.ids.end(), ids.begin() + (std::ptrdiff_t)s_begin, ids.end());
  return s_begin;
}

// One topology upload: the phases of upload_all in the order it runs them, and what one hands to the next.  The sequence of dev_upload* calls
// is the layout of the upload arena (slots go by call order, hints hold per owner): it does not change from one upload to the next.
struct UploadPass {
  pps_graph* const g;
  const Analysis& A = g->an;
  DevGraph& d = g->dev;
  const double t0 = now_s();
  double tl = t0;
  // Refreshed measurements may stay on the device across an upload that only appends (see the obs_meas upload): same arena, same slot with
  // room for the new rows, same leading dimension, no re-popping edges (their slots sit behind the fixed ones and would move).
  bool keep_meas = false;
  const size_t n_obs_on_device = (size_t)g->dev.n_obs;         // (reset() clears g->dev)
  bool hints = false;                  // the mirror holds the arrays of the analysis this one was built upon: its kept parts are not compared again
  Analysis::Kept K;
  ZeroBlock Z{0, 0, 0};
  double* zero_block = nullptr;

  void lap(const char* what) { if (!g->sw.upload_timing) return; const double t = now_s(); g->up_laps[what] += t - tl; tl = t; }
  size_t state_doubles() const { return (size_t)7 * g->dev.pose_ld + (size_t)4 * g->dev.plane_ld; }

  // what only the device has: the estimate, and the refreshed measurements unless they can stay there
  int bring_home() {
    if (g->dev_values_newer) TRY(download_state(g));
    lap("1a state download");
    if (g->dev_meas_newer) {
      // (live counts kept by the add / remove calls: a walk over the 300-byte factor records here was 30 us per frame at 7 600 factors)
      keep_meas = g->grown_only_upload && !g->mirror.unknown && !g->mirror.unknown_meas && g->up.spill == 0 && g->n_live_repop == 0 && d.n_obs == d.n_obs_fixed &&
                  j_capacity(g->n_live_type[F_PLANE_OBS]) == d.obs_ld && j_capacity(g->n_live_type[F_PLANE_PRIOR]) == d.lp_ld &&
                  g->mirror.slot_of(&d.obs_meas) != UploadMirror::npos;
      if (!keep_meas) {
        if (g->sw.upload_timing) g->up_laps["(measurement downloads, count)"] += 1e-3;      // (printed as ms: the count)
        TRY(download_measurements(g));
      }
    }
    lap("1b measurements");
    return PPS_OK;
  }
  // the stream drained, the last layout given up, every pointer into it forgotten
  int reset() {
    HIP_TRY(g, hipStreamSynchronize(g->stream));
    g->up_inflight = false;
    lap("1c opening stream sync");
    free_device(g);
    g->spec_L = g->spec_U = g->spec_delta = nullptr; g->spec_result = nullptr;
    g->spec_pose = g->spec_plane = g->spec_chi2_partials = g->spec_dn_partials = nullptr; g->spec_ticket = nullptr;
    g->spec_J = g->spec_P = g->spec_H = g->spec_Hf = nullptr;
    g->d_item_frame = g->d_item_plane = g->d_item_slot = g->d_frame_pose_slot = g->d_frame_seg_off = nullptr; g->d_fr_seg = nullptr;
    g->frames_dirty = true;
    g->snap_pose = g->snap_plane = nullptr; g->upload_version++;
    lap("2 free_device");
    hints = g->grown_only_upload && !g->mirror.unknown && g->up_an_seq >= 0 && g->an_base_seq == g->up_an_seq;
    if (hints) K = g->an.kept;
    return PPS_OK;
  }
  // One packed side, packed (pack_side; the previous upload's arrays are still right for the old factors when nothing was removed since: slots
  // only append) and uploaded: [first index | second index | measurements | weights].  same: rows packed and sent by the previous upload
  int put_side(pps_graph::PackedSide& S, int** da, int** db, double** dm, double** dw, size_t n, size_t ld, bool repack_meas, bool force_meas, size_t exact_from) {
    const size_t s_begin = pack_side(g, S, ld, g->grown_only_upload, repack_meas);
    const size_t same_idx = hints ? s_begin : 0, same_meas = (hints && g->pk_meas_ok) ? s_begin : 0;
    TRY(dev_upload(g, da, S.a, same_idx)); TRY(dev_upload(g, db, S.b, same_idx));
    TRY(dev_upload_rows(g, dm, S.m, (size_t)S.km, ld, n, force_meas, exact_from, same_meas));
    return dev_upload_rows(g, dw, S.w, (size_t)S.kw, ld, n, false, kNoExact, same_idx);
  }
  // the state copies, the value offsets and the arrays of the four factor types
  int factor_arrays() {
    d.n_pose = (int)g->pose_ids.size(); d.n_plane = (int)g->plane_ids.size();
    d.no_strip = g->sw.no_strip ? 1 : 0;
    d.sw = g->sw.dev_bits();
    HIP_TRY(g, step_constants(d.step_ac));
    d.pose_ld = std::max(1, (d.n_pose + 63) / 64 * 64); d.plane_ld = std::max(1, (d.n_plane + 63) / 64 * 64);
    // every copy of the state is one block [poses | planes]: one transfer moves it (copies rotate by pointer pairs, so a
    // plane array always sits behind its pose array)
    TRY(dev_alloc(g, &d.pose_est, state_doubles())); d.plane_est = d.pose_est + (size_t)7 * d.pose_ld;
    TRY(dev_alloc(g, &d.pose_lin, state_doubles())); d.plane_lin = d.pose_lin + (size_t)7 * d.pose_ld;
    std::vector<int> pv(d.n_pose), lv(d.n_plane);
    for (int s = 0; s < d.n_pose; s++) pv[s] = A.node_voff[g->nodes[g->pose_ids[s]].compact];
    for (int s = 0; s < d.n_plane; s++) lv[s] = A.node_voff[g->nodes[g->plane_ids[s]].compact];
    TRY(dev_upload(g, &d.pose_voff, pv)); TRY(dev_upload(g, &d.plane_voff, lv));
    d.n_obs = (int)g->fslot_ids[F_PLANE_OBS].size(); d.n_odo = (int)g->fslot_ids[F_ODOMETRY].size();
    d.n_pp = (int)g->fslot_ids[F_POSE_PRIOR].size(); d.n_lp = (int)g->fslot_ids[F_PLANE_PRIOR].size();
    { int64_t base[4]; j_bases(g, base, nullptr); d.joff_obs = base[F_PLANE_OBS]; d.joff_odo = base[F_ODOMETRY]; d.joff_pp = base[F_POSE_PRIOR]; d.joff_lp = base[F_PLANE_PRIOR]; }
    auto idx_of = [&](int type) {
      std::vector<int> v(g->fslot_ids[type].size());
      for (size_t s = 0; s < v.size(); s++) v[s] = g->nodes[g->factors[g->fslot_ids[type][s]].a].slot;
      return v;
    };
    std::vector<double> tmp;
    d.obs_ld = (int)j_capacity(d.n_obs); d.odo_ld = (int)j_capacity(d.n_odo); d.pp_ld = (int)j_capacity(d.n_pp); d.lp_ld = (int)j_capacity(d.n_lp);
    UploadMirror& m = g->mirror;
    // Measurements that a device-side refresh has rewritten (pps_refresh_measurements) stay where they are when this upload
    // only appends: the host packs its (older) copies, the mirror holds the same bytes, so nothing is sent for them and the
    // device keeps the refreshed values; only the new observations travel.  dev_meas_newer stays set.
    TRY(put_side(g->pk_obs, &d.obs_pose, &d.obs_plane, &d.obs_meas, &d.obs_w, (size_t)d.n_obs, (size_t)d.obs_ld, !g->pk_meas_ok, m.unknown_meas,
                 keep_meas ? std::min((size_t)d.n_obs, n_obs_on_device) : kNoExact));
    d.n_obs_fixed = g->n_obs_fixed;
    if (const size_t n2 = (size_t)(d.n_obs - d.n_obs_fixed)) {      // the re-popping observations' rays
      tmp.assign(6 * n2, 0.0);
      for (size_t k = 0; k < n2; k++)
        for (int c = 0; c < 6; c++) tmp[(size_t)c * n2 + k] = g->factors[g->fslot_ids[F_PLANE_OBS][d.n_obs_fixed + k]].ray[c];
      TRY(dev_upload(g, &d.obs_ray, tmp));
    }
    TRY(put_side(g->pk_odo, &d.odo_a, &d.odo_b, &d.odo_meas, &d.odo_w, (size_t)d.n_odo, (size_t)d.odo_ld, false, false, kNoExact));      // (only the observations re-pack old measurement rows)
    TRY(dev_upload(g, &d.pp_pose, idx_of(F_POSE_PRIOR)));
    pack_soa<6>(g, F_POSE_PRIOR, false, tmp, (size_t)d.pp_ld); TRY(dev_upload_rows(g, &d.pp_meas, tmp, 6, (size_t)d.pp_ld, (size_t)d.n_pp, false));
    pack_soa<21>(g, F_POSE_PRIOR, true, tmp, (size_t)d.pp_ld); TRY(dev_upload_rows(g, &d.pp_w, tmp, 21, (size_t)d.pp_ld, (size_t)d.n_pp, false));
    TRY(dev_upload(g, &d.lp_plane, idx_of(F_PLANE_PRIOR)));
    pack_soa<4>(g, F_PLANE_PRIOR, false, tmp, (size_t)d.lp_ld); TRY(dev_upload_rows(g, &d.lp_meas, tmp, 4, (size_t)d.lp_ld, (size_t)d.n_lp, m.unknown_meas));
    pack_soa<6>(g, F_PLANE_PRIOR, true, tmp, (size_t)d.lp_ld); TRY(dev_upload_rows(g, &d.lp_w, tmp, 6, (size_t)d.lp_ld, (size_t)d.n_lp, false));
    m.unknown_meas = false;
    g->pk_meas_ok = true;
    lap("4 factor packing + diff");
    return PPS_OK;
  }
  // the linear system's storage, the analysis' index arrays, the scratch of the solves
  int index_arrays() {
    const size_t kF = (size_t)K.fronts, kFl = (size_t)K.fronts_lists, kB = (size_t)K.blocks, kS = (size_t)K.segs;
    // (the device array of the analysis array of the same name)
#define UPA(name, same) TRY(dev_upload(g, &d.name, A.name, same))
    auto at = [](const auto& v, size_t i) -> size_t { return i < v.size() ? (size_t)v[i] : 0; };     // (0 = no claim)
    TRY(dev_alloc(g, &d.J, (size_t)A.J_size)); TRY(dev_alloc(g, &d.H, (size_t)A.H_size));
    TRY(dev_alloc(g, &d.P, (size_t)std::max<int64_t>(1, A.P_size)));
    { int64_t pb[4]; p_bases(g, pb, nullptr); d.poff_obs = pb[F_PLANE_OBS]; }
    TRY(dev_alloc(g, &d.L, (size_t)A.L_size)); TRY(dev_alloc(g, &d.U, (size_t)A.U_size));
    TRY(dev_alloc(g, &g->spec_L, (size_t)A.L_size)); TRY(dev_alloc(g, &g->spec_U, (size_t)A.U_size));
    d.n_scalars = A.n_scalars;
    d.n_fronts = A.n_fronts; d.n_levels = A.n_levels; d.max_front = A.max_front; d.n_segs = A.n_segs; d.n_blocks = A.n_blocks;
    UPA(f_p, kF); UPA(f_b, kF); UPA(f_poff, kF); UPA(pidx, kF ? at(A.f_poff, kF) : 0); UPA(f_Loff, kF); UPA(f_Uoff, kF);
    UPA(f_bidx_off, kF ? kF + 1 : 0); UPA(bidx, kF ? at(A.f_bidx_off, kF) : 0); UPA(f_child_off, kF ? kF + 1 : 0); UPA(child, kF ? at(A.f_child_off, kF) : 0);
    UPA(f_cmap_off, kF ? kF + 1 : 0); UPA(cmap, 0); UPA(level_fronts, 0);      // (cmap: kept fronts below a redone parent are rewritten)
    const size_t kA = kFl ? at(A.f_asm_off, kFl) : 0;
    UPA(f_asm_off, kFl ? kFl + 1 : 0); UPA(asm_blk, kA); UPA(asm_lrow, kA); UPA(asm_lcol, kA);
    UPA(blk_rows, kB); UPA(blk_cols, kB); UPA(blk_size, kB); UPA(blk_nseg, kB); UPA(blk_hoff, kB);
    UPA(seg_blk, kS); UPA(seg_c0, kS); UPA(seg_cnt, kS); UPA(seg_hoff, kS); UPA(contrib, 4 * (size_t)K.contribs);
    {
      std::vector<int> mseg;
      for (int bk = 0; bk < A.n_blocks; bk++) if (A.blk_nseg[bk] > 1) mseg.push_back(bk);
      d.n_mseg = (int)mseg.size();
      TRY(dev_upload(g, &d.mseg_blk, mseg));
      // K2's two work lists: segments of single-segment blocks that K1 does not write itself; first segment of every other block
      std::vector<int> k2s, k2m, k2f;
      for (int sg : A.nd_segs) if (A.blk_nseg[A.seg_blk[sg]] == 1) k2s.push_back(sg);
      for (int sg = 0; sg < A.n_segs; sg++) {
        const int ns = A.blk_nseg[A.seg_blk[sg]];
        if (ns <= 1 || (sg > 0 && A.seg_blk[sg - 1] == A.seg_blk[sg])) continue;      // (first segment of a block of several)
        for (int c0 = 0; c0 < ns; c0 += 16) { k2m.push_back(sg + c0); k2m.push_back(std::min(16, ns - c0) | (ns <= 16 ? 1 << 16 : 0)); }
        if (ns > 16) k2f.push_back(sg);
      }
      d.n_k2_single = (int)k2s.size(); d.n_k2_multi = (int)k2m.size() / 2; d.n_k2_finish = (int)k2f.size();
      TRY(dev_upload(g, &d.k2_single, k2s)); TRY(dev_upload(g, &d.k2_multi, k2m)); TRY(dev_upload(g, &d.k2_finish, k2f));
    }
    UPA(f_el_off, kFl ? kFl + 1 : 0); TRY(dev_alloc(g, &d.el_tgt, (size_t)std::max<int64_t>(1, A.el_total)));   // filled by k_expand_el (expand)
    UPA(asm_el0, kA); UPA(asm_fsz, kA);
    UPA(f_ea_off, kF ? kF + 1 : 0); TRY(dev_alloc(g, &d.ea_tgt, (size_t)std::max<int64_t>(1, A.ea_total)));   // filled by k_expand_ea (expand)
    UPA(blk_doff, kB ? kB + 1 : 0); TRY(dev_alloc(g, &d.blk_dst, (size_t)std::max(1, A.blk_doff[A.n_blocks])));
    TRY(dev_alloc(g, &d.Hf, (size_t)A.el_total));
    if (g->use_band() && !g->sw.no_spec_lin) {                        // the spare set of the fused trial + linearisation launch (lm_solve_dual)
      TRY(dev_alloc(g, &g->spec_J, (size_t)A.J_size)); TRY(dev_alloc(g, &g->spec_P, (size_t)std::max<int64_t>(1, A.P_size)));
      TRY(dev_alloc(g, &g->spec_H, (size_t)A.H_size)); TRY(dev_alloc(g, &g->spec_Hf, (size_t)A.el_total));
    }
    UPA(grp_lvl_off, 0); UPA(glvl_front_off, 0);
    {
      // per group, one 32-byte record: first position, fronts, local levels, first position of local levels 1 .. 4 (the last one
      // repeated), 0 -- what the band kernels would otherwise fetch with two dependent look-ups (levels of the group, their offsets)
      std::vector<int> span(8 * (size_t)std::max(1, A.n_groups), 0);
      for (int gi = 0; gi < A.n_groups; gi++) {
        const int l0 = A.grp_lvl_off[gi], nl = A.grp_lvl_off[gi + 1] - l0;
        int* r = &span[8 * (size_t)gi];
        r[0] = A.glvl_front_off[l0]; r[1] = A.glvl_front_off[l0 + nl] - r[0]; r[2] = nl;
        for (int k = 1; k <= 4; k++) r[2 + k] = A.glvl_front_off[l0 + std::min(k, nl)];
      }
      TRY(dev_upload(g, &d.grp_span, span));
    }
    UPA(glvl_fronts, 0); UPA(frec, 0); UPA(crec, 0); UPA(srec, 8 * kS);
    UPA(obs_dir, 0); UPA(nd_segs, (size_t)K.nd_segs); d.n_nd_segs = (int)A.nd_segs.size();
    UPA(cls_off, 0); UPA(cls_fronts, 0);
    if (g->use_dense()) { TRY(dev_upload(g, &g->d_dw_asm, g->plan.dw_asm)); TRY(dev_upload(g, &g->d_dw_pan, g->plan.dw_pan)); TRY(dev_upload(g, &g->d_dw_trl, g->plan.dw_trl)); }
    d.chi2_blocks = (d.n_obs + 255) / 256 + (d.n_odo + 255) / 256 + (d.n_pp + 255) / 256 + (d.n_lp + 255) / 256;
    TRY(dev_alloc(g, &d.chi2_partials, (size_t)std::max(1, d.chi2_blocks)));

    Z = ZeroBlock(d.n_pose + d.n_plane, A.n_scalars, A.n_fronts);
    TRY(dev_alloc(g, &zero_block, Z.total));
    double* const zb = zero_block;
    d.dn_partials = zb + Z.dn_partials;
    d.ticket = reinterpret_cast<unsigned int*>(zb + Z.ticket); g->spec_ticket = reinterpret_cast<unsigned int*>(zb + Z.spec_ticket);
    d.result_dev = zb + Z.result; g->spec_result = zb + Z.spec_result;
    d.delta = zb + Z.delta; g->spec_delta = zb + Z.spec_delta;
    d.k3_flag = reinterpret_cast<int*>(zb + Z.flags);
    g->k3_epoch = 0;
    g->status_clean = true;
    // the local solutions that cross a band group in the whole-tree back-substitution (XGroup::hand, pps_k3.hip): every value is written in the
    // launch that reads it, behind its flag -- not zeroed
    if (g->plan.form == K3Form::BandAll) TRY(dev_alloc(g, &d.k3_xhand, 2 * (size_t)A.n_fronts * kBandMaxRows));
    TRY(dev_alloc(g, &g->spec_pose, state_doubles() + 1)); g->spec_plane = g->spec_pose + (size_t)7 * d.pose_ld;
    TRY(dev_alloc(g, &g->spec_chi2_partials, (size_t)std::max(1, d.chi2_blocks)));
    TRY(dev_alloc(g, &g->spec_dn_partials, Z.n_dn));
    d.trace_solve = g->sw.trace >= 2 ? 1 : 0;
    if (g->sw.trace) { TRY(dev_alloc(g, &d.trace, (size_t)A.n_fronts * 8)); HIP_TRY(g, hipMemset(d.trace, 0, (size_t)A.n_fronts * 64)); }
    // fronts that exceed the LDS limit run from a global workspace (one slab per front of the widest level)
    if (!g->use_band() && !g->use_dense() && A.max_front > lds_front_limit()) {
      const int fa = A.max_front + 1;
      d.gwork_stride = (int64_t)fa * (fa | 1);
      int widest = 0;
      for (int l = 0; l < A.n_levels; l++)
        if (g->plan.level_max_front[l] > lds_front_limit()) widest = std::max(widest, A.level_off[l + 1] - A.level_off[l]);
      TRY(dev_alloc(g, &d.gwork, (size_t)d.gwork_stride * std::max(1, widest)));
    }
#undef UPA
    lap("5 index arrays + diff");
    return PPS_OK;
  }
  int flush_and_verify() {
    TRY(flush_uploads(g));
    TRY(verify_uploads(g, "upload_all"));
    TRY(verify_packed(g, keep_meas ? n_obs_on_device : 0));
    lap("6 flush");
    return PPS_OK;
  }
  // ea_tgt, el_tgt and blk_dst filled on the device, the zeroed block cleared
  int expand() {
    // one launch for both expansions when every H block is assembled by exactly one front (always, unless an analysis ever lists a block
    // twice or not at all: then the fill of blk_dst has to run first, in a launch of its own)
    const bool one_launch = A.ea_total > 0 && Z.total < (size_t)1 << 30 && (int)A.asm_blk.size() == A.n_blocks && A.n_fronts > 0 &&
                            !g->sw.split_expand;
    if (one_launch) HIP_TRY(g, launch_expand_lists(d, A.n_fronts, (int)A.asm_blk.size(), zero_block, Z.total, g->stream));
    else {
      const size_t n_dst = (size_t)std::max(1, A.blk_doff[A.n_blocks]);
      if (A.ea_total > 0 && Z.total < (size_t)1 << 30 && n_dst < (size_t)1 << 30)
        HIP_TRY(g, launch_expand_ea(d, A.n_fronts, zero_block, Z.total, d.blk_dst, n_dst, g->stream));
      else {
        if (A.ea_total > 0) HIP_TRY(g, launch_expand_ea(d, A.n_fronts, nullptr, 0, nullptr, 0, g->stream));
        HIP_TRY(g, hipMemsetAsync(zero_block, 0, Z.total * 8, g->stream));
        HIP_TRY(g, hipMemsetAsync(d.blk_dst, 0xff, sizeof(int) * n_dst, g->stream));
      }
      HIP_TRY(g, launch_expand_el(d, (int)A.asm_blk.size(), g->stream));
    }
    TRY(verify_expanded(g, zero_block, Z));
    g->topo_dirty = false;
    g->meas_dirty = false;
    g->grown_only_upload = true;
    g->up_an_seq = g->an_seq;
    lap("7 expand kernels + sync");
    return PPS_OK;
  }
};

int upload_all(pps_graph* g) {
  UploadPass P{g};
  g->mirror.verify_hints = g->sw.verify_upload;
  TRY(ensure_device(g));
  P.lap("0 ensure_device");
  TRY(P.bring_home());
  // the analysis is host work on host tables: it runs while the device finishes what the last frame left on the stream (the measurement
  // refresh of a frame loop: the opening sync of reset() waited 10 us per frame for it)
  if (!g->analyzed || g->analysis_stale) TRY(run_analysis(g));
  P.lap("3 analysis");
  TRY(P.reset());
  TRY(P.factor_arrays());
  TRY(P.index_arrays());
  TRY(P.flush_and_verify());
  TRY(P.expand());
  // no sync: the solve that follows runs on the same stream (and ends with one); whatever writes the pinned buffers
  // again checks up_inflight or follows upload_all's opening sync
  const int rc = upload_state(g, false);
  P.lap("8 upload_state");
  g->stats.t_upload = now_s() - P.t0 - g->stats.t_analysis;
  return rc;
}

int prepare_solve(pps_graph* g) {
  int rc;
  if (g->n_live_nodes == 0) return fail(g, PPS_ESTATE, "empty graph");
  if (g->dev_ready) HIP_TRY(g, hipSetDevice(g->props.device));   // handles may be driven from any host thread
  if (g->topo_dirty || !g->dev_ready || g->dev.n_scalars == 0) { rc = upload_all(g); if (rc != PPS_OK) return rc; }
  if (g->host_values_newer) { rc = upload_state(g); if (rc != PPS_OK) return rc; }
  if (g->meas_dirty) { rc = upload_measurements(g); if (rc != PPS_OK) return rc; }
  HIP_TRY(g, ensure_k3_attrs());                                  // (once per device; the K3 launchers themselves check nothing)
  return PPS_OK;
}

#undef TRY
}  // namespace pps_impl

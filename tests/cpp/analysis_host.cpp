// analysis_host.cpp -- the symbolic analysis (csrc/pps_symbolic.cpp, the only file this links against) driven without the C ABI, so that
// the parameter sets the ABI never passes are covered and the whole thing can run under the host sanitizers as a plain program:
//   g++ -O2 -std=c++17 -Wall -Werror -I pop_up_slam_amd/csrc tests/cpp/analysis_host.cpp pop_up_slam_amd/csrc/pps_symbolic.cpp -o analysis_host
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined ... (same files)
//
// Graphs are built here: a pose chain with a ground plane seen from every pose, walls seen from runs of consecutive poses (lengths and
// starts from a fixed LCG), optionally a loop-closure edge every few dozen poses.  Jacobian / product offsets are laid out as the
// uploader lays them out (one slab per factor type, capacities in powers of two), so the offsets of every old factor move whenever a
// slab outgrows its capacity -- the `offsets_changed` arm of the incremental analysis.  A graph grows by `stride` poses per step; after
// every step dump_analysis() of analyze(..., cache) into the Analysis of the step before must equal, word for word, dump_analysis() of
// analyze(..., nullptr) into a fresh Analysis, and every Analysis::Kept count must name a leading part that the previous step's
// arrays held.  One line per set; the first difference ends the program with status 1.
//
// The aligned-cut chain sets (no closures, ordering 2 and 0) also pin HOW MANY steps build on the previous analysis: the counts in
// kSets[].expect_reusing were measured with this program linked against pps_symbolic.cpp as it stood before the analysis was split into
// phases (Pass / KeptPrefix): 290 of 300 (ordering 2), 290 of 300 (ordering 0), 291 of 300 (leaf_poses 1), 290 of 300 (front_rows 0), 94 of 100
// (three poses per step) and 332 of 342 (every seventh graph analysed twice) -- 94 to 97 % of the steps.
#include "pps_symbolic.h"

#include <cstdio>
#include <cstring>
#include <string>

using namespace pps;

namespace {

struct Lcg { uint32_t s; uint32_t next() { s = s * 1664525u + 1013904223u; return s >> 8; } };

struct Set {
  const char* name;
  int poses, stride, closure_every, twice_every;   // poses per step; a loop closure every so many poses (0: none); every so many steps the graph is analysed twice (0: never)
  int ordering, aligned_cuts, arity, leaf_poses, front_rows, band_rows;
  int expect_reusing;                                // steps that must build on the previous analysis (-1: only reported)
};
const Set kSets[] = {
    {"chain aligned ord2", 300, 1, 0, 0, 2, 1, 2, 4, 63, 127, 290},
    {"chain aligned ord0", 300, 1, 0, 0, 0, 1, 2, 4, 63, 127, 290},
    {"chain aligned leaf1", 300, 1, 0, 0, 2, 1, 2, 1, 63, 127, 291},
    {"chain aligned rows0", 300, 1, 0, 0, 2, 1, 2, 4, 0, 127, 290},
    {"chain aligned stride3", 300, 3, 0, 0, 2, 1, 2, 4, 63, 127, 94},
    {"chain aligned twice", 300, 1, 0, 7, 2, 1, 2, 4, 63, 127, 332},
    {"closures aligned ord0", 300, 1, 37, 0, 0, 1, 2, 4, 63, 127, -1},
    {"closures aligned ord2", 300, 1, 37, 5, 2, 1, 2, 4, 63, 127, -1},
    {"closures band_rows 31", 260, 1, 29, 0, 0, 1, 2, 4, 63, 31, -1},
    {"closures mindeg ord1", 160, 1, 29, 0, 1, 0, 2, 4, 63, 127, -1},
    {"chain quantile", 200, 1, 0, 0, 2, 0, 2, 4, 63, 127, -1},
    {"chain quantile leaf1", 120, 2, 0, 0, 0, 0, 2, 1, 63, 127, -1},
    {"closures arity 4", 200, 1, 41, 0, 2, 0, 4, 4, 63, 127, -1},
    {"closures arity 4 rows0", 200, 1, 41, 0, 0, 1, 4, 4, 0, 127, -1},
};

struct Graph {
  std::vector<SymNode> nodes;
  std::vector<SymFactor> factors;
  int n_type[4] = {0, 0, 0, 0};
  void add(int type, int a, int b) { SymFactor f; f.type = type; f.a = a; f.b = b; f.joff = n_type[type]++; f.direct_ok = type == F_PLANE_OBS; factors.push_back(f); }
  // offsets as the uploader lays them out: [plane obs | odometry | pose priors | plane priors], capacities in powers of two
  void lay_out() {
    const int order[4] = {F_PLANE_OBS, F_ODOMETRY, F_POSE_PRIOR, F_PLANE_PRIOR};
    int64_t jb[4], pb[4], j = 0, p = 0;
    for (int t : order) { int64_t cap = 16; while (cap < n_type[t]) cap <<= 1; jb[t] = j; pb[t] = p; j += cap * kJSize[t]; p += cap * kPSize[t]; }
    int cnt[4] = {0, 0, 0, 0};
    for (SymFactor& f : factors) { const int k = cnt[f.type]++; f.joff = (int)(jb[f.type] + (int64_t)k * kJSize[f.type]); f.poff = (int)(pb[f.type] + (int64_t)k * kPSize[f.type]); }
  }
};

// one more pose: its prior or odometry edge, the ground plane, the walls in sight (a wall is seen from a run of consecutive poses)
struct Scene {
  Lcg rng{12345u};
  int prev = -1, ground = -1, n_poses = 0;
  std::vector<int> pose_ids;
  struct Wall { int node, until; };
  std::vector<Wall> walls;
  void grow(Graph& g, int closure_every) {
    const int p = (int)g.nodes.size();
    g.nodes.push_back({NODE_POSE, 6, n_poses});
    if (prev < 0) g.add(F_POSE_PRIOR, p, -1); else g.add(F_ODOMETRY, prev, p);
    if (ground < 0) { ground = (int)g.nodes.size(); g.nodes.push_back({NODE_PLANE, 3, -1}); g.add(F_PLANE_PRIOR, ground, -1); }
    g.add(F_PLANE_OBS, p, ground);
    size_t live = 0;
    for (const Wall& w : walls) if (w.until > n_poses) walls[live++] = w;
    walls.resize(live);
    while (walls.size() < 2 || (walls.size() < 5 && rng.next() % 4 == 0)) {
      walls.push_back({(int)g.nodes.size(), n_poses + 2 + (int)(rng.next() % 24)});
      g.nodes.push_back({NODE_PLANE, 3, -1});
    }
    for (const Wall& w : walls) g.add(F_PLANE_OBS, p, w.node);
    if (closure_every > 0 && n_poses > 20 && n_poses % closure_every == 0) g.add(F_ODOMETRY, pose_ids[rng.next() % (n_poses - 10)], p);
    pose_ids.push_back(p); prev = p; n_poses++;
  }
};

template <class T>
bool same_head(const std::vector<T>& now, const std::vector<T>& before, int64_t count, const char* what, std::string& err) {
  if (count < 0 || count > (int64_t)now.size() || count > (int64_t)before.size() || (count > 0 && memcmp(now.data(), before.data(), (size_t)count * sizeof(T)) != 0)) {
    err = std::string("kept prefix does not hold for ") + what;
    return false;
  }
  return true;
}

// every Analysis::Kept count names leading entries that the analysis before held (the layout in pps_symbolic.h)
bool kept_holds(const Analysis& a, const Analysis& b, std::string& err) {
  const Analysis::Kept k = a.kept;
  const int F = k.fronts, Fl = k.fronts_lists;
  if (Fl > F) { err = "fronts_lists > fronts"; return false; }
  if (F == 0) { if (Fl || k.blocks || k.segs || k.contribs || k.nd_segs) { err = "claims without kept fronts"; return false; } return true; }
  bool ok = same_head(a.f_p, b.f_p, F, "f_p", err) && same_head(a.f_b, b.f_b, F, "f_b", err) && same_head(a.f_poff, b.f_poff, F, "f_poff", err) &&
            same_head(a.f_Loff, b.f_Loff, F, "f_Loff", err) && same_head(a.f_Uoff, b.f_Uoff, F, "f_Uoff", err) &&
            same_head(a.f_bidx_off, b.f_bidx_off, F + 1, "f_bidx_off", err) && same_head(a.f_child_off, b.f_child_off, F + 1, "f_child_off", err) &&
            same_head(a.f_cmap_off, b.f_cmap_off, F + 1, "f_cmap_off", err) && same_head(a.f_ea_off, b.f_ea_off, F + 1, "f_ea_off", err);
  if (!ok) return false;
  ok = same_head(a.pidx, b.pidx, F < a.n_fronts ? a.f_poff[F] : a.n_scalars, "pidx", err) && same_head(a.bidx, b.bidx, a.f_bidx_off[F], "bidx", err) &&
       same_head(a.child, b.child, a.f_child_off[F], "child", err);
  if (ok && Fl > 0) {
    const int n = a.f_asm_off[Fl];
    ok = same_head(a.f_asm_off, b.f_asm_off, Fl + 1, "f_asm_off", err) && same_head(a.f_el_off, b.f_el_off, Fl + 1, "f_el_off", err) &&
         same_head(a.asm_blk, b.asm_blk, n, "asm_blk", err) && same_head(a.asm_lrow, b.asm_lrow, n, "asm_lrow", err) && same_head(a.asm_lcol, b.asm_lcol, n, "asm_lcol", err) &&
         same_head(a.asm_el0, b.asm_el0, n, "asm_el0", err) && same_head(a.asm_fsz, b.asm_fsz, n, "asm_fsz", err);
  }
  ok = ok && same_head(a.blk_rows, b.blk_rows, k.blocks, "blk_rows", err) && same_head(a.blk_cols, b.blk_cols, k.blocks, "blk_cols", err) &&
       same_head(a.blk_size, b.blk_size, k.blocks, "blk_size", err) && same_head(a.blk_nseg, b.blk_nseg, k.blocks, "blk_nseg", err) &&
       same_head(a.blk_hoff, b.blk_hoff, k.blocks, "blk_hoff", err) && (k.blocks == 0 || same_head(a.blk_doff, b.blk_doff, k.blocks + 1, "blk_doff", err)) &&
       same_head(a.seg_blk, b.seg_blk, k.segs, "seg_blk", err) && same_head(a.seg_c0, b.seg_c0, k.segs, "seg_c0", err) && same_head(a.seg_cnt, b.seg_cnt, k.segs, "seg_cnt", err) &&
       same_head(a.seg_hoff, b.seg_hoff, k.segs, "seg_hoff", err) && same_head(a.srec, b.srec, 8 * (int64_t)k.segs, "srec", err) &&
       same_head(a.contrib, b.contrib, 4 * (int64_t)k.contribs, "contrib", err) && same_head(a.nd_segs, b.nd_segs, k.nd_segs, "nd_segs", err);
  return ok;
}

bool run(const Set& s) {
  AnalysisParams prm;
  prm.ordering = s.ordering; prm.aligned_cuts = s.aligned_cuts; prm.arity = s.arity; prm.leaf_poses = s.leaf_poses;
  prm.front_rows = s.front_rows; prm.band_rows = s.band_rows; prm.seg_len = 64;
  Graph g; Scene scene;
  Analysis inc, before;
  AnalysisCache* cache = analysis_cache_new();
  std::vector<int32_t> d_inc, d_ref;
  int compared = 0, reusing = 0, moved = 0, mindeg = 0, chain_shaped = 0, step = 0;
  std::string err;
  while (scene.n_poses < s.poses && err.empty()) {
    for (int k = 0; k < s.stride && scene.n_poses < s.poses; k++) scene.grow(g, s.closure_every);
    g.lay_out();
    step++;
    const int reps = (s.twice_every > 0 && step % s.twice_every == 0) ? 2 : 1;   // (the second time: an unchanged graph)
    for (int rep = 0; rep < reps && err.empty(); rep++) {
      const char* msg = "";
      before = inc;
      if (!analyze(g.nodes, g.factors, prm, inc, &msg, cache)) { err = std::string("analysis failed: ") + msg; break; }
      Analysis ref;
      if (!analyze(g.nodes, g.factors, prm, ref, &msg, nullptr)) { err = std::string("analysis from scratch failed: ") + msg; break; }
      dump_analysis(inc, d_inc); dump_analysis(ref, d_ref);
      if (d_inc != d_ref) {
        size_t w = 0;
        while (w < d_inc.size() && w < d_ref.size() && d_inc[w] == d_ref[w]) w++;
        err = "dump differs from the analysis from scratch at word " + std::to_string(w);
        break;
      }
      // (kept is all 0 where the minimum-degree ordering replaced the dissection's result, whatever the cache took over on the way)
      int reused = 0, total = 0;
      analysis_cache_stats(cache, &reused, &total);
      if (inc.kept.fronts > reused) { err = "kept.fronts exceeds the cache's count of reused fronts"; break; }
      if (!kept_holds(inc, before, err)) break;
      compared++; reusing += inc.kept.fronts > 0; moved += inc.kept.fronts > 0 && inc.kept.fronts_lists == 0;
      if (prm.ordering == 0) {                          // did the dissection leave a front beyond band_rows, i.e. was minimum degree analysed as well?
        AnalysisParams chain_only = prm;
        chain_only.ordering = 2;
        Analysis dis;
        if (!analyze(g.nodes, g.factors, chain_only, dis, &msg, nullptr)) { err = std::string("chain-only analysis failed: ") + msg; break; }
        mindeg += dis.max_front > prm.band_rows;
      }
      bool chain = ref.n_fronts >= 8;
      for (int f = 0; chain && f + 1 < ref.n_fronts; f++) chain = ref.f_parent[f] == f + 1;
      chain_shaped += chain;
    }
  }
  analysis_cache_free(cache);
  if (err.empty() && s.expect_reusing >= 0 && reusing != s.expect_reusing) err = "steps building on the previous analysis: " + std::to_string(reusing) + ", expected " + std::to_string(s.expect_reusing);
  if (err.empty() && s.band_rows < 63 && mindeg == 0) err = "no step took the minimum-degree comparison";
  printf("%-24s poses %3d  compared %3d  reusing %3d  with moved offsets %2d  min-degree compared %3d  chain-shaped trees %d  %s\n", s.name, scene.n_poses, compared, reusing, moved, mindeg, chain_shaped,
         err.empty() ? "ok" : ("FAILED at step " + std::to_string(step) + ": " + err).c_str());
  return err.empty();
}

}  // namespace

int main() {
  for (const Set& s : kSets)
    if (!run(s)) return 1;
  return 0;
}

// pps_map_host.h -- the map handle and what the host files of the dense map share (pps_map.cpp: store and build; pps_map_grid.cpp: grid map).
#pragma once
#include "pps_graph.h"
#include "pps_map.h"

namespace pps_impl {
struct MapGrid;
// what the posed build knows of a frame (pps_map_set_frame_pose); run_T: the T_wc of the pop-up run pps_map_add_frame took the frame from
struct MapFrameRec {
  int frame_seq_id = 0;
  int pose_id = -1;
  bool has_run_T = false;
  float T[16] = {0}, run_T[16] = {0};
};
}  // namespace pps_impl

struct pps_map {
  pps_graph* g = nullptr;
  std::string err;
  int64_t cap = 0, used = 0;
  int n_frames = 0;
  std::vector<pps_map_chunk> chunks, built;
  int64_t built_points = 0;
  pps::MapPt *d_store = nullptr, *d_built = nullptr;
  int* d_table = nullptr; size_t table_cap = 0;       // planes x wave tiles of the last frame, then kMapPlanes totals
  int* h_totals = nullptr;                            // pinned, kMapPlanes
  char* d_sel = nullptr; size_t sel_cap = 0;          // offset table of a build: [out_off | src_off | slot]
  pps::MapPt* d_dbg_cloud = nullptr; int* d_dbg_pid = nullptr; size_t dbg_cap = 0;   // pixels uploaded by pps_debug_map_add_points
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  double sec[2] = {0, 0};
  // the posed build (pps_map_build_posed / pps_map_build_grid_posed)
  std::vector<pps_impl::MapFrameRec> frames;          // one per frame, in insertion order
  char* d_motion = nullptr; size_t motion_cap = 0;    // motion table of the last posed call: [12 doubles per frame | moved flag per frame]
  int n_motion = 0, n_unposed = 0, posed_launches = 0;
  hipEvent_t ev_posed[4] = {nullptr, nullptr, nullptr, nullptr};
  double posed_sec[2] = {0, 0};
  pps_impl::MapGrid* grid = nullptr;                  // the last grid map and its buffers (pps_map_grid.cpp), made by the first pps_map_build_grid
};

namespace pps_impl {

inline int mfail(pps_map* m, int code, const std::string& msg) { if (m) m->err = msg; return code; }
#define MAP_TRY(m, expr)                                                                                        \
  do {                                                                                                          \
    hipError_t _e = (expr);                                                                                     \
    if (_e != hipSuccess) return mfail(m, _e == hipErrorOutOfMemory ? PPS_ENOMEM : PPS_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// pps_map.cpp
bool map_select_valid(const pps_map_select* s);
void map_select_chunks(const pps_map_chunk* c, int n, const pps_map_select* s, int32_t* keep);      // main_3d.cpp:544-562
// The motion table of a posed call over the chunks `src` (rows of m->chunks: selected and not empty), after prepare_solve.  plan: the
// frames of those chunks in order, one record each (recs), and per chunk the row of its frame (fidx); both go into the caller's one
// upload.  launch: k_map_motion into m->d_motion on the graph's stream (the caller synchronises; map_motion_done then reads the time).
struct MapMotionPlan { std::vector<int> fidx; std::vector<pps::MapFrameDev> recs; int n_unposed = 0; };
void map_motion_plan(const pps_map* m, const std::vector<int>& src, MapMotionPlan* p);
int map_motion_launch(pps_map* m, const MapMotionPlan& p, const pps::MapFrameDev* d_recs, const int* d_fidx, pps::MapMotionTable* t);
void map_motion_done(pps_map* m);
// pps_map_grid.cpp: frees the grid's device buffers (the caller has set the device and drained the stream) and the record itself
void map_grid_release(pps_map* m);

}  // namespace pps_impl

// pps_map_host.h -- the map handle and what the host files of the dense map share (pps_map.cpp: store and build; pps_map_grid.cpp: grid map).
#pragma once
#include "pps_graph.h"
#include "pps_map.h"

namespace pps_impl { struct MapGrid; }

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
// pps_map_grid.cpp: frees the grid's device buffers (the caller has set the device and drained the stream) and the record itself
void map_grid_release(pps_map* m);

}  // namespace pps_impl

// pps_map_grid_host.h -- the record of the last grid map, of the last view rendered from it and of the last comparison with that view,
// shared by pps_map_grid.cpp (which builds the grid), pps_map_render.cpp and pps_map_compare.cpp (which only read it).
#pragma once
#include "pps_compare.h"
#include "pps_grid.h"
#include "pps_map_host.h"
#include "pps_render.h"

namespace pps_impl {

// The last pps_map_compare, of THIS view: whatever ends the view ends it (MapRender::clear, a new render).  tables: the plane rows and
// their ids are on the device for this grid.
struct MapCompare {
  bool valid = false, tables = false;
  pps_map_compare_totals tot{};
  MapBuf<unsigned long long> table;
  MapBuf<pps::ComparePlane> planes; MapBuf<int> ids;
  MapBuf<pps::CompareBlock> block;
  MapBuf<pps_map_compare_row> rows; MapBuf<pps_map_compare_pair> pairs;
  MapSpan t_kernels;
  void clear() { valid = tables = false; tot = pps_map_compare_totals{}; }
  void release() { table.release(); planes.release(); ids.release(); block.release(); rows.release(); pairs.release(); t_kernels.release(); }
};

// The last pps_map_render.  tables: the slot table, the landmark rows and their ids are on the device for THIS grid (made by the first
// render after a grid call, kept until the next one).  on_host: the grid had no cell, the view is empty and no buffer holds it.
struct MapRender {
  bool valid = false, tables = false, on_host = false;
  pps_map_render_totals tot{};
  int n_rows = 0;
  MapBuf<int> slot;
  MapBuf<pps::RenderPlane> rows; MapBuf<int> ids;
  MapBuf<pps::MapPt> cloud; MapBuf<float> depth; MapBuf<int> plane_id; MapBuf<long long> cell;
  MapBuf<unsigned long long> n_hit;
  MapSpan t_kernels;
  MapCompare compare;
  void clear() { valid = tables = on_host = false; tot = pps_map_render_totals{}; n_rows = 0; compare.clear(); }
  void release() {
    slot.release(); rows.release(); ids.release(); cloud.release(); depth.release(); plane_id.release(); cell.release(); n_hit.release();
    t_kernels.release(); compare.release();
  }
};

struct MapGrid {
  // the last grid (valid: the last call succeeded)
  bool valid = false;
  std::vector<pps_map_grid_plane> planes;
  std::vector<double> plane_eq;                       // four doubles per row of `planes`: the estimate grid_frame was given
  pps_map_grid_totals tot{};
  int64_t n_box_cells = 0;                            // cells of all boxes: the length of key[] and cnt[]
  int min_count = 1;
  // device
  MapBuf<char> sel;                                   // tables of the selection, with the lm column (MapSelection)
  MapBuf<pps::GridPlaneDev> d_planes;
  MapBuf<char> small;                                 // GridExtent per landmark, then the dropped counter
  MapBuf<long long> plane_tab;                        // plane_base[n + 1], plane_off[n + 1]
  MapBuf<unsigned long long> key;
  MapBuf<unsigned int> cnt;
  MapBuf<int> tile_count;
  MapBuf<long long> tile_prefix;
  MapBuf<pps::MapPt> out_pts; MapBuf<unsigned int> out_cnt; MapBuf<int> out_ij; MapBuf<long long> out_src;
  // tot.sec: [0] the extent pass, [1] zeroing and votes, [2] count + scan + plane_off and the emission, [3] first upload to last kernel
  MapSpan t_extent, t_vote, t_count, t_emit, t_call;
  MapRender render;                                   // a view of THIS grid: every grid call ends it
  void clear() {                                      // a call that fails leaves no grid
    valid = false; planes.clear(); plane_eq.clear(); tot = pps_map_grid_totals{}; n_box_cells = 0; min_count = 1;
    render.clear();
  }
};

}  // namespace pps_impl

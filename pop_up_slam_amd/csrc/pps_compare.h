// pps_compare.h -- argument blocks and launch functions of the compare kernels (pps_compare.hip), shared with the host side (pps_map_compare.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/pps.h"
#include "pps_compare_px.h"
#include "pps_map.h"

namespace pps {

constexpr int kComparePlanes = 65;               // frame planes of a run at most (kMapPlanes)
constexpr int kComparePasses = 4;                // a workgroup owns 4 x 256 consecutive pixels, one per thread and pass
constexpr int kCompareSlotBits = 6, kCompareSlots = 1 << kCompareSlotBits;       // entries of a workgroup's table in LDS
constexpr int kCompareProbes = 8;                // slots a key may try before its wave adds to memory itself

// The table: (nplanes + 1) x (n_rows + 1) records of four 64-bit counters {n, n_agree, sum_q, sum_q2}, entry (k, r) at k * (n_rows + 1) + r.
// Column n_rows: no view; row nplanes: no frame; so the margins take the path of the pairs.  One more counter behind the last record:
// n_bad_id.
PPS_GRID_HD size_t compare_entries(int nplanes, int n_rows) { return (size_t)(nplanes + 1) * (size_t)(n_rows + 1); }
PPS_GRID_HD size_t compare_table_words(int nplanes, int n_rows) { return 4 * compare_entries(nplanes, n_rows) + 1; }

struct CompareArgs {
  int npx, nplanes, n_rows;
  double tol;
  const MapPt* cloud;                  // [npx] the frame's points
  const int* frame_id;                 // [npx] the frame's plane ids
  const int* view_id;                  // [npx] the render's plane ids; NULL: a view without a hit anywhere
  const int* ids;                      // [n_rows] node ids of the plane table, ascending
  const ComparePlane* planes;          // [n_rows]
  unsigned long long* table;           // compare_table_words(nplanes, n_rows), zeroed
};
hipError_t launch_compare(const CompareArgs& a, hipStream_t st);

// What the finish kernels leave in one block: the host reads the head and the first nplanes plane records with one copy.
struct CompareHead { long long n_both, n_frame_only, n_view_only, n_neither, n_bad_id, n_pairs; };
struct CompareBlock {
  CompareHead head;
  pps_map_compare_plane planes[kComparePlanes];
  long long pair_cnt[kComparePlanes + 1];      // entries with n >= 1 of every table row (k_compare_scan -> k_compare_emit)
  long long view_only;
};
struct CompareFinishArgs {
  int nplanes, n_rows;
  const int* ids;
  const unsigned long long* table;
  CompareBlock* block;
  pps_map_compare_row* rows;           // [n_rows]
  pps_map_compare_pair* pairs;         // room for every entry with n >= 1: min(nplanes * n_rows, pixels)
};
// two launches: k_compare_scan (per table row: the best landmark, the margins, the count of pairs), then k_compare_emit (the pair list in
// order, the per-row records, the totals)
hipError_t launch_compare_finish(const CompareFinishArgs& a, hipStream_t st);

}  // namespace pps

// pps_map_host.h -- the map handle and what the host files of the dense map share (pps_map.cpp: store and build; pps_map_grid.cpp: grid map):
// the device buffer (MapBuf), the timed span (MapSpan), the selection of a build call with its tables on the device (MapSelection), the
// motion table of a posed call.
#pragma once
#include <map>

#include "pps_graph.h"
#include "pps_map.h"

struct pps_map;

namespace pps_impl {
struct MapGrid;
// what the posed build knows of a frame (pps_map_set_frame_pose); run_T: the T_wc of the pop-up run pps_map_add_frame took the frame from
struct MapFrameRec {
  int frame_seq_id = 0;
  int pose_id = -1;
  bool has_run_T = false;
  float T[16] = {0}, run_T[16] = {0};
};

// A device buffer that only grows.  reserve(n): room for n elements; when it has to grow, `over` times n are allocated (1: exactly; the
// tables of a build, uploaded anew by every call, take 2) and the stream is drained before the old block is freed.
template <class T>
struct MapBuf {
  T* p = nullptr; size_t cap = 0;                     // elements
  hipError_t reserve(size_t n, hipStream_t st, size_t over = 1) {
    if (n <= cap) return hipSuccess;
    if (p) { const hipError_t e = hipStreamSynchronize(st); if (e != hipSuccess) return e; }
    release();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), over * n * sizeof(T));
    if (e == hipSuccess) cap = over * n; else p = nullptr;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// A timed span of a stream: an event pair, created on first use.  seconds(): after the stream was synchronised behind end().
struct MapSpan {
  hipEvent_t a = nullptr, b = nullptr;
  hipError_t begin(hipStream_t st) {
    for (hipEvent_t* e : {&a, &b})
      if (!*e) { const hipError_t rc = hipEventCreate(e); if (rc != hipSuccess) return rc; }
    return hipEventRecord(a, st);
  }
  hipError_t end(hipStream_t st) { return hipEventRecord(b, st); }
  double seconds() const { float ms = 0; (void)hipEventElapsedTime(&ms, a, b); return 1e-3 * ms; }
  void release() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); a = b = nullptr; }
};

// The selection of a build call and its tables on the device.  select (host only): the keep flag of every chunk, the kept chunks that
// are not empty (src: rows of m->chunks, the rows of the device tables) and the points of all kept chunks.  upload, after prepare_solve:
//   [out_off (n + 1 long long) | src_off (n long long) | slot | (lm) | (fidx) | pad to 8 bytes | (recs)]
// lm: the row of the chunk's landmark in row_of (the grid; -1 with slot); fidx and recs: frame row per chunk and frame records of a posed
// call (map_motion_plan).  One copy into `buf` on the graph's stream (span: a span that begins at that copy, behind the buffer's growth);
// the caller synchronises before the record goes out of scope.
struct MapMotionPlan { std::vector<int> fidx; std::vector<pps::MapFrameDev> recs; int n_unposed = 0; };
struct MapSelection {
  std::vector<int32_t> keep;
  std::vector<int> src;
  int64_t total = 0;
  MapMotionPlan plan;
  struct { size_t src_off, slot, lm, fidx, recs, bytes; } at{};       // byte offsets of the columns in the image (out_off: 0)
  std::vector<char> host;
  const char* dev = nullptr;
  void select(const pps_map* m, const pps_map_select* sel);
  int upload(pps_map* m, bool posed, const std::map<int, int>* row_of, MapBuf<char>* buf, size_t over, MapSpan* span = nullptr);
  int n() const { return (int)src.size(); }
  template <class T> const T* col(size_t off) const { return reinterpret_cast<const T*>(dev + off); }
  const long long* out_off() const { return col<long long>(0); }
  const long long* src_off() const { return col<long long>(at.src_off); }
  const int* slot() const { return col<int>(at.slot); }
  const int* lm() const { return col<int>(at.lm); }
  const int* fidx() const { return col<int>(at.fidx); }
  const pps::MapFrameDev* recs() const { return col<pps::MapFrameDev>(at.recs); }
};
}  // namespace pps_impl

struct pps_map {
  pps_graph* g = nullptr;
  std::string err;
  int64_t cap = 0, used = 0;
  int n_frames = 0;
  std::vector<pps_map_chunk> chunks, built;
  int64_t built_points = 0;
  bool on_device = false;                             // a call has set the device (map_use_device): destroy drains the stream
  pps_impl::MapBuf<pps::MapPt> d_store, d_built;      // `cap` points each, from the first frame / the first build on
  pps_impl::MapBuf<int> d_table;                      // planes x wave tiles of the last frame, then kMapPlanes totals
  int* h_totals = nullptr;                            // pinned, kMapPlanes
  pps_impl::MapBuf<char> d_sel;                       // tables of a build (MapSelection)
  pps_impl::MapBuf<pps::MapPt> d_dbg_cloud; pps_impl::MapBuf<int> d_dbg_pid;       // pixels uploaded by pps_debug_map_add_points
  pps_impl::MapSpan t_count, t_scatter, t_build;      // sec[0]: count + scan and scatter of the last frame; sec[1]: k_map_build
  double sec[2] = {0, 0};
  // the posed build (pps_map_build_posed / pps_map_build_grid_posed)
  std::vector<pps_impl::MapFrameRec> frames;          // one per frame, in insertion order
  pps_impl::MapBuf<char> d_motion;                    // motion table of the last posed call: [12 doubles per frame | moved flag per frame]
  int n_motion = 0, n_unposed = 0, posed_launches = 0;
  pps_impl::MapSpan t_motion, t_posed;                // posed_sec[0]: k_map_motion; posed_sec[1]: k_map_build_posed
  double posed_sec[2] = {0, 0};
  pps_impl::MapGrid* grid = nullptr;                  // the last grid map, its buffers and its rendered view (pps_map_grid_host.h), made by the first pps_map_build_grid
};

namespace pps_impl {

inline int mfail(pps_map* m, int code, const std::string& msg) { if (m) m->err = msg; return code; }
#define MAP_TRY(m, expr)                                                                                        \
  do {                                                                                                          \
    hipError_t _e = (expr);                                                                                     \
    if (_e != hipSuccess) return mfail(m, _e == hipErrorOutOfMemory ? PPS_ENOMEM : PPS_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// what a posed call starts from: nothing of the call before
inline void map_posed_reset(pps_map* m) { m->posed_sec[0] = m->posed_sec[1] = 0; m->n_motion = 0; m->n_unposed = 0; m->posed_launches = 0; }

// the read-back of a table: *n = the rows there are, the first min(cap, rows) of them copied to out
inline bool map_table_args(int cap, const void* out, const int* n) { return n && cap >= 0 && (cap == 0 || out); }
template <class T>
int map_table_copy(const T* rows, size_t have, int cap, T* out, int* n) {
  if (!map_table_args(cap, out, n)) return PPS_EINVAL;
  *n = (int)have;
  const size_t k = std::min<size_t>((size_t)cap, have);
  if (k) memcpy(out, rows, k * sizeof(T));
  return PPS_OK;
}

// pps_map.cpp
int map_use_device(pps_map* m);                                                                    // hipSetDevice of the graph's device
bool map_select_valid(const pps_map_select* s);
// The motion table of a posed call over the chunks `src` (rows of m->chunks: selected and not empty), after prepare_solve.  plan: the
// frames of those chunks in order, one record each (recs), and per chunk the row of its frame (fidx); both go into the selection's one
// upload.  launch: k_map_motion into m->d_motion on the graph's stream, timed by m->t_motion (the caller synchronises, then reads it).
void map_motion_plan(const pps_map* m, const std::vector<int>& src, MapMotionPlan* p);
int map_motion_launch(pps_map* m, const MapSelection& s, pps::MapMotionTable* t);
// pps_map_grid.cpp: frees the grid's device buffers (the caller has set the device and drained the stream) and the record itself
void map_grid_release(pps_map* m);

}  // namespace pps_impl

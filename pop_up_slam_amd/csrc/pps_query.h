// pps_query.h -- the protocol of the five calls that question what a covariance recovery leaves on the device: pps_cov_block, pps_assoc_gate,
// pps_merge_gate, pps_loop_gate (the lambda = 0 factor in dev.L, by walks up the elimination tree) and pps_factor_gate (the selected inverse in
// cov_S, no walk).  Each keeps one QueryState on the handle (pps_graph.h).  The order of a call: its argument checks -> CovQuery: build -> add
// (its own sections) -> reserve -> query_begin (its state's buffers) -> walk -> its own launch -> finish -> its status word read as zero ->
// query_end -> the decoding of its result; the whole in a function-try-block that ends in query_no_memory.  DESIGN.md describes it once.
#pragma once
#include "pps_graph.h"

namespace pps_impl {

inline size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }      // sections of a request or a result sit at multiples of 16 bytes

// The timed half of a query: start() after the call's upload (the launch count, event 0), the launches, then stop() (event 1, the copy back, the
// synchronisation every query ends with, the figures of _last).  The event pair is the handle's (cov_qev): query_device makes it.
int query_device(pps_graph* g);      // the handle's device is current, its query events exist
struct QueryTimer {
  pps_graph* g; unsigned long long launches0;
  int start();
  int stop(void* host, size_t bytes, QueryState* st);      // the first `bytes` of st->out come home
};

// A query on the factor: walks up the tree for a list of distinct, checked nodes (k_cov_path / k_cov_path_wide, pps_cov.h), then the caller's
// own kernel over the strips the walks leave.
struct CovQuery {
  pps_graph* g;
  std::vector<CovNode> nd;                       // the nodes, located
  std::vector<pps::CovWalk> walks; std::vector<pps::CovStep> steps; std::vector<int> step_end;
  int K = 0;                                     // the longest path of the query in pivots
  long long n_strip = 0;
  int max_rows = 1;                              // the widest front (p + b) on the paths of this query
  std::vector<char> req;                         // [walks | steps | the caller's sections ...], every section at a multiple of 16 bytes
  size_t o_steps = 0;
  QueryTimer timer;
  explicit CovQuery(pps_graph* g_) : g(g_), timer{g_, 0} {}
  int build(const std::vector<int>& ids);                      // id check (cov_node), cov_locate, paths leaf -> root; starts the request
  int common_pivots(int a, int b) const;                       // walks a, b: pivots of their common ancestors
  size_t add(const void* data, size_t bytes);                  // a section of the caller's; its offset in the request
  // the tree as the pair kernels walk it: sections [f_parent | cov_rootlen], n_fronts ints each, after the check that both tables have them
  int add_tree(const char* who, size_t* o_parent, size_t* o_rootlen);
  template <class T> const T* dev(size_t off) const { return reinterpret_cast<const T*>(g->cov_breq.p + off); }   // (after reserve)
  int reserve(const char* who = nullptr, const char* advice = "");   // device, events, cov_breq, cov_strip, the wide scratch (that one always PPS_ENOMEM)
  int walk(double* status);                                    // upload -> event -> the walk launch; the caller's launch comes next
  int finish(void* host, size_t bytes, QueryState* st) { return timer.stop(host, bytes, st); }
};

// What a call asks of its state: out_bytes of result, of which the first status_bytes are its status word (0: it has none), its tickets (0: none) and
// its records in doubles (kNoRecords: none are kept for this call).  The result, the tickets and the records are reserved in this order, the last
// call's records and success forgotten in between -- without `who` a buffer that cannot be had answers as HIP_TRY does, with it PPS_ENOMEM and
// "<who>no device memory for <name> (<n> bytes)<advice>" (DevBuf::reserve).  The status word and the tickets are zero between calls: zeroed here
// after a call that failed (!st->clean) or when one of the two buffers is new; st->clean is false from here until query_end.
constexpr size_t kNoRecords = (size_t)-1;
int query_begin(pps_graph* g, QueryState* st, size_t out_bytes, size_t status_bytes, size_t tickets, size_t rec_doubles, const char* who = nullptr,
                const char* advice = "", const char* out_name = "the result", const char* ticket_name = "the tickets");
// after the status word was read as zero: the call has succeeded, with rec_n records kept and `count` entries without an answer
inline void query_end(QueryState* st, size_t rec_n, int count) { st->clean = st->done = true; st->rec_n = rec_n; st->count = count; }

// the pps_*_last entry points, whole (g may be NULL: PPS_EINVAL, hence the state by member; count NULL: pps_cov_block_last and pps_assoc_gate_last have none)
int query_last(const pps_graph* g, QueryState pps_graph::*which, double* kernel_sec, int* launches, int* count);
// the pps_debug_*_records entry points, whole: `unit` doubles per record of the last call of `name` ("merge gate"); max_entries > 0: records are kept for
// calls of at most that many `entries` ("pairs")
int query_records(pps_graph* g, QueryState pps_graph::*which, int unit, const char* name, long long max_entries, const char* entries, int64_t cap, double* rec,
                  int64_t* needed);

// "<list> and n_<list> go together (<list> may be NULL with cap_<list> 0: the count alone)"
int list_with_count(pps_graph* g, const char* who, const char* list_name, const void* list, const void* count, int cap);
// the default list (ids == NULL: all live planes) and the check of a given one: live planes, none listed twice
int plane_list(pps_graph* g, const char* prefix, const int** ids, int* n, std::vector<int>* all);

// the flag bytes of a pair kernel (2: S not positive definite, 1: d2 under the threshold): under(i) for every index flagged 1, in order; *not_pd counts the 2s
template <class F>
long long decode_flags(const unsigned char* flag, long long n, int* not_pd, F under) {
  long long n_under = 0;
  *not_pd = 0;
  for (long long i = 0; i < n; i++) {
    if (flag[i] == 2) ++*not_pd;
    else if (flag[i] == 1) { under(i, n_under); n_under++; }
  }
  return n_under;
}

// the handler of the function-try-block around each of the five calls: no std::bad_alloc crosses the C boundary
inline int query_no_memory(pps_graph* g, const char* who) { return fail(g, PPS_ENOMEM, std::string(who) + "no host memory for the request or the result"); }

}  // namespace pps_impl

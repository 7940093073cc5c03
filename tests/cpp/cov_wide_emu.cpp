// cov_wide_emu.cpp -- k_cov_path_wide and k_cov_pivots of csrc/pps_cov_wide.hip next to k_cov_path / k_cov_gram of csrc/pps_cov.hip, compiled for
// the host like tests/cpp/cov_block_emu.cpp compiles the latter two (block_emu/hip/hip_runtime.h: one std::thread per thread of a workgroup,
// std::barrier as __syncthreads).  tests/test_host_cov_factor.py feeds them the factor panels of a dense Cholesky factor in the device layout
// (what is unspecified on the device is NaN here) and the request tables of a query; it compares the blocks with np.linalg.inv and the
// strips of the two walk kernels bit for bit.
//
// With -DCOV_WIDE_EMU_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): it builds a chain of fronts with random
// panels -- boundaries of up to 700 rows, so that a thread of the wide kernel takes several rows --, walks it from several nodes with
// both kernels and compares the strips with a sequential restatement of the walk, bit for bit.  Exit code 0: all equal, status words zero.
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
std::barrier<>* g_barrier = nullptr;
std::mutex g_mu;
namespace pps { namespace { alignas(16) double cov_lds[32768]; } }
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a) {
  for (unsigned b = 0; b < grid.x; b++) {
    std::barrier<> bar(block.x); g_barrier = &bar;
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++) th.emplace_back([&, t]() { threadIdx = dim3(t); blockIdx = dim3(b); k(a...); g_barrier->arrive_and_drop(); });
    for (auto& x : th) x.join();
  }
}
#include "pps_cov.hip"
#include "pps_cov_wide.hip"
namespace pps { unsigned long long launch_count() { return 0; } void count_launch() {} }
using namespace pps;

static DevGraph emu_graph(int n_fronts, int* f_p, int* f_b, int64_t* f_Loff, int* f_cmap_off, int* cmap, double* L) {
  DevGraph d; d.n_fronts = n_fronts; d.f_p = f_p; d.f_b = f_b; d.f_Loff = f_Loff; d.f_cmap_off = f_cmap_off; d.cmap = cmap; d.L = L;
  return d;
}

// wide != 0: k_cov_path_wide with the scratch Z (n_scratch doubles, max_front = the widest front of the query); else k_cov_path (max_p,
// max_front = the widest of the graph).  status = one double, raised; Y = the strip buffer
extern "C" int emu_cov_walks(int wide, int n_fronts, int* f_p, int* f_b, int64_t* f_Loff, int* f_cmap_off, int* cmap, double* L, const void* walks, int n_walks,
                             const void* steps, int n_steps, int K, int max_p, int max_front, double* Z, long long n_scratch, double* Y, long long n_strip,
                             double* status) {
  const DevGraph d = emu_graph(n_fronts, f_p, f_b, f_Loff, f_cmap_off, cmap, L);
  if (wide) return launch_cov_path_wide(d, (const CovWalk*)walks, n_walks, (const CovStep*)steps, n_steps, K, max_front, Z, n_scratch, Y, n_strip, status, nullptr);
  if (cov_path_lds_bytes(max_p, max_front) > sizeof(cov_lds)) return -1;
  return launch_cov_path(d, (const CovWalk*)walks, n_walks, (const CovStep*)steps, n_steps, K, max_p, max_front, Y, n_strip, status, nullptr);
}

extern "C" int emu_cov_gram(const void* pairs, int n_pairs, const double* Y, long long n_strip, double* out, long long n_out) {
  return launch_cov_gram((const CovPair*)pairs, n_pairs, Y, n_strip, out, n_out, nullptr);
}

// result4: the status record of the device (entry 2 is raised)
extern "C" int emu_cov_pivots(int n_fronts, int* f_p, int64_t* f_Loff, double* L, double* result4) {
  DevGraph d; d.n_fronts = n_fronts; d.f_p = f_p; d.f_Loff = f_Loff; d.L = L; d.result_dev = result4;
  return launch_cov_pivots(d, n_fronts, nullptr);
}

#ifdef COV_WIDE_EMU_MAIN
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>

namespace {

struct Chain {
  std::vector<int> f_p, f_b, f_cmap_off, cmap;
  std::vector<int64_t> f_Loff;
  std::vector<double> L;
  int n() const { return (int)f_p.size(); }
};

// front s has parent s + 1; its boundary rows map to an increasing subset of the parent's rows
Chain make_chain(const std::vector<int>& p, const std::vector<int>& b, unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  Chain c; c.f_p = p; c.f_b = b; c.f_cmap_off.push_back(0);
  for (int s = 0; s < c.n(); s++) {
    c.f_Loff.push_back((int64_t)c.L.size());
    for (int i = 0; i < p[s] + b[s] + 1; i++)
      for (int j = 0; j < p[s]; j++) {
        double v = 0.3 * u(rng);
        if (i < p[s]) v = j < i ? v : j == i ? 2.0 + u(rng) : nan;      // above the diagonal of L_A: unspecified
        if (i == p[s] + b[s]) v = nan;                                   // the rhs row
        c.L.push_back(v);
      }
    if (b[s] > 0) {
      const int nq = p[s + 1] + b[s + 1];
      std::vector<int> rows(nq);
      for (int k = 0; k < nq; k++) rows[k] = k;
      std::shuffle(rows.begin(), rows.end(), rng);
      rows.resize(b[s]);
      std::sort(rows.begin(), rows.end());
      c.cmap.insert(c.cmap.end(), rows.begin(), rows.end());
    }
    c.cmap.push_back(s + 1 < c.n() ? p[s + 1] + b[s + 1] : 0);           // (the rhs row's target)
    c.f_cmap_off.push_back((int)c.cmap.size());
  }
  return c;
}

// the walk, one operation after the other in the order of cov_walk
void ref_walk(const Chain& c, int s0, int local, int D, int K, const std::vector<int>& rootlen, double* Y) {
  std::vector<double> z((size_t)(c.f_p[s0] + c.f_b[s0]) * D, 0.0);
  for (int a = 0; a < D; a++) z[(size_t)(local + a) * D + a] = 1.0;
  int m0 = local;
  for (int s = s0; s < c.n(); s++) {
    const int p = c.f_p[s], b = c.f_b[s];
    const double* Lp = c.L.data() + c.f_Loff[s];
    std::vector<double> y((size_t)p * D, 0.0), zr(z.begin(), z.begin() + (size_t)p * D);
    for (int m = m0; m < p; m++) {
      for (int a = 0; a < D; a++) y[(size_t)m * D + a] = zr[(size_t)m * D + a] / Lp[(size_t)m * p + m];
      for (int i = m + 1; i < p; i++)
        for (int a = 0; a < D; a++) zr[(size_t)i * D + a] -= Lp[(size_t)i * p + m] * y[(size_t)m * D + a];
    }
    for (int i = 0; i < p * D; i++) Y[(size_t)(K - rootlen[s]) * D + i] = i < m0 * D ? 0.0 : y[i];
    if (b == 0) break;
    std::vector<double> zq((size_t)(c.f_p[s + 1] + c.f_b[s + 1]) * D, 0.0);
    for (int r = 0; r < b; r++)
      for (int a = 0; a < D; a++) {
        double acc = 0.0;
        for (int m = m0; m < p; m++) acc += Lp[(size_t)(p + r) * p + m] * y[(size_t)m * D + a];
        zq[(size_t)c.cmap[c.f_cmap_off[s] + r] * D + a] = z[(size_t)(p + r) * D + a] - acc;
      }
    z.swap(zq);
    m0 = 0;
  }
}

int run_chain(const char* label, const std::vector<int>& p, const std::vector<int>& b, bool narrow_too, unsigned seed) {
  Chain c = make_chain(p, b, seed);
  const int F = c.n();
  std::vector<int> rootlen(F, 0);
  for (int s = F - 1; s >= 0; s--) rootlen[s] = p[s] + (s + 1 < F ? rootlen[s + 1] : 0);
  // walks: a pose at the first pivot of front 0, a plane at its last three pivots, a pose in the middle of the chain, a plane in the root
  struct Q { int front, local, dim; };
  const std::vector<Q> qs = {{0, 0, 6}, {0, p[0] - 3, 3}, {F / 2, p[F / 2] - 6, 6}, {F - 1, 1, 3}};
  const int K = rootlen[0];
  std::vector<CovWalk> walks; std::vector<CovStep> steps;
  long long n_strip = 0;
  int max_rows = 1, max_p = 1, max_all = 1;
  for (int s = 0; s < F; s++) { max_p = std::max(max_p, p[s]); max_all = std::max(max_all, p[s] + b[s]); }
  for (const Q& q : qs) {
    walks.push_back(CovWalk{n_strip, (int)steps.size(), F - q.front, q.local, q.dim});
    for (int s = q.front; s < F; s++) { steps.push_back(CovStep{s, K - rootlen[s]}); max_rows = std::max(max_rows, p[s] + b[s]); }
    n_strip += (long long)K * q.dim;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> ref((size_t)n_strip, nan), wide((size_t)n_strip, nan), narrow((size_t)n_strip, nan);
  for (size_t w = 0; w < qs.size(); w++) ref_walk(c, qs[w].front, qs[w].local, qs[w].dim, K, rootlen, ref.data() + walks[w].strip);
  std::vector<double> Z(walks.size() * cov_wide_scratch(max_rows), nan);
  double status = 0.0;
  int rc = emu_cov_walks(1, F, c.f_p.data(), c.f_b.data(), c.f_Loff.data(), c.f_cmap_off.data(), c.cmap.data(), c.L.data(), walks.data(), (int)walks.size(),
                         steps.data(), (int)steps.size(), K, max_p, max_rows, Z.data(), (long long)Z.size(), wide.data(), n_strip, &status);
  if (rc != 0 || status != 0.0) { printf("%s: wide kernel rc %d status %g\n", label, rc, status); return 1; }
  int bad = 0;
  for (size_t w = 0; w < qs.size(); w++) {
    const size_t lo = (size_t)walks[w].strip + (size_t)(K - rootlen[qs[w].front]) * qs[w].dim, hi = (size_t)walks[w].strip + (size_t)K * qs[w].dim;
    for (size_t i = lo; i < hi; i++) bad += memcmp(&ref[i], &wide[i], 8) != 0 || !std::isfinite(wide[i]);
    for (size_t i = (size_t)walks[w].strip; i < lo; i++) bad += !std::isnan(wide[i]);          // (ahead of the path: never written)
  }
  if (narrow_too) {
    rc = emu_cov_walks(0, F, c.f_p.data(), c.f_b.data(), c.f_Loff.data(), c.f_cmap_off.data(), c.cmap.data(), c.L.data(), walks.data(), (int)walks.size(),
                       steps.data(), (int)steps.size(), K, max_p, max_all, nullptr, 0, narrow.data(), n_strip, &status);
    if (rc != 0 || status != 0.0) { printf("%s: k_cov_path rc %d status %g\n", label, rc, status); return 1; }
    bad += memcmp(narrow.data(), wide.data(), (size_t)n_strip * 8) != 0;
  }
  // a scratch buffer one double too short, and a step outside the tree: the status word, nothing written
  std::vector<double> Y2((size_t)n_strip, 7.0);
  status = 0.0;
  const DevGraph d = emu_graph(F, c.f_p.data(), c.f_b.data(), c.f_Loff.data(), c.f_cmap_off.data(), c.cmap.data(), c.L.data());
  hipLaunchKernelGGL(k_cov_path_wide, dim3((unsigned)walks.size()), dim3(256), 0, nullptr, d, walks.data(), (int)walks.size(), steps.data(), (int)steps.size(), K, max_rows,
                     Z.data(), (long long)Z.size() - 1, Y2.data(), n_strip, &status);
  bad += status != 64.0;
  for (size_t i = (size_t)walks.back().strip; i < (size_t)n_strip; i++) bad += Y2[i] != 7.0;   // (the last walk is the one whose scratch is short)
  steps.back().front = F + 5; status = 0.0;
  rc = emu_cov_walks(1, F, c.f_p.data(), c.f_b.data(), c.f_Loff.data(), c.f_cmap_off.data(), c.cmap.data(), c.L.data(), walks.data(), (int)walks.size(),
                     steps.data(), (int)steps.size(), K, max_p, max_rows, Z.data(), (long long)Z.size(), Y2.data(), n_strip, &status);
  bad += rc != 0 || status != 64.0;
  // the pivot criterion: clean, then one collapsed pivot, then a NaN
  double res[4] = {0, 0, 0, 0};
  emu_cov_pivots(F, c.f_p.data(), c.f_Loff.data(), c.L.data(), res); bad += res[2] != 0.0;
  const size_t piv = (size_t)c.f_Loff[F / 2] + (size_t)2 * p[F / 2] + 2;
  const double keep = c.L[piv];
  c.L[piv] = 1e-8; emu_cov_pivots(F, c.f_p.data(), c.f_Loff.data(), c.L.data(), res); bad += res[2] != 1.0; res[2] = 0.0;
  c.L[piv] = nan; emu_cov_pivots(F, c.f_p.data(), c.f_Loff.data(), c.L.data(), res); bad += res[2] != 1.0;
  c.L[piv] = keep;
  printf("%s: fronts %d K %d widest front of the query %d rows, %s\n", label, F, K, max_rows, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += run_chain("narrow chain", {12, 9, 17, 6, 30, 8}, {50, 45, 40, 36, 8, 0}, true, 1);
  // a front's boundary is at most its parent's rows and a front has at most 64 pivots: 700 rows take a dozen levels
  const std::vector<int> p = {12, 64, 9, 33, 63, 64, 64, 17, 64, 64, 60, 64, 64, 64, 7};
  std::vector<int> b(p.size(), 0);
  for (int s = (int)p.size() - 2; s >= 0; s--) b[s] = p[s + 1] + b[s + 1] - s % 3;      // (some rows of a parent have no child row)
  bad += run_chain("wide chain", p, b, false, 2);
  return bad ? 1 : 0;
}
#endif

// cov_dense_emu.cpp -- the kernels of csrc/pps_cov_dense.hip (the selected inverse on dense fronts) and k_cov_pivots of csrc/pps_cov_wide.hip compiled
// for the host: block_emu/hip/hip_runtime.h gives one std::thread per thread of a workgroup and std::barrier as __syncthreads; the static
// __shared__ arrays of the file become function statics (the workgroups run one after the other).  v_mfma_f64_16x16x4_f64 is the emulation of
// tests/cpp/wave_emu.h restated for threads instead of coroutines: the 64 threads of a wave publish their operands, meet at a barrier of
// their wave, and each computes its four accumulator entries with the same fused multiply-adds in the same order (lane l supplies
// A[l % 16][l / 16] and B[l / 16][l % 16]; register r is row (l / 16) + 4 r, column l % 16).  The operand buffers alternate between two
// sets, so that one barrier per MFMA is enough: a lane can be at most one MFMA ahead of the slowest lane of its wave.
//
// tests/test_host_cov_select.py feeds emu_cov_dense the panels of a dense Cholesky factor in the device layout, NaN wherever the device
// leaves memory unspecified, and compares the blocks of S with np.linalg.inv.
//
// With -DCOV_DENSE_EMU_MAIN the file is a stand-alone program (for -fsanitize=address,undefined): a chain of fronts with random panels in
// shapes that are no multiples of 16 or 64 -- and chains at the tile edges no graph reaches (p = 64 with b = 256 and 257, p around 16 and 32 with
// b around 32 and 64, p = 1 with b = 1) --, against a sequential restatement of the recursion.  Exit code 0: all within 1e-10 of the largest
// entry, status word zero, and the three refusals (collapsed pivot, corrupted child map, short update-matrix array) raise what they should.
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>
#include <hip/hip_runtime.h>
thread_local dim3 threadIdx, blockIdx;
std::barrier<>* g_barrier = nullptr;
std::mutex g_mu;
#define PPS_COV_DENSE_EMU
namespace pps { namespace {
alignas(16) double cov_lds[64];
typedef double double4_t __attribute__((vector_size(32)));
struct EmuWave { double a[2][64], b[2][64]; std::barrier<>* bar; };
EmuWave emu_wave[4];
thread_local int emu_parity = 0;
inline double4_t emu_mfma(double a, double b, double4_t c) {
  const int l = (int)threadIdx.x & 63;
  EmuWave& w = emu_wave[threadIdx.x >> 6];
  const int par = emu_parity; emu_parity ^= 1;
  w.a[par][l] = a; w.b[par][l] = b;
  w.bar->arrive_and_wait();
  const int col = l & 15, lq = l >> 4;
  for (int r = 0; r < 4; r++) {
    const int row = lq + 4 * r;
    double acc = c[r];
    for (int k = 0; k < 4; k++) acc = std::fma(w.a[par][row + 16 * k], w.b[par][col + 16 * k], acc);
    c[r] = acc;
  }
  return c;
}
} }
#define __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, x, y, z) emu_mfma((a), (b), (c))
template <class K, class... A> void emu_launch(K k, dim3 grid, dim3 block, A... a) {
  for (unsigned b = 0; b < grid.x; b++) {
    std::barrier<> bar(block.x); g_barrier = &bar;
    std::vector<std::barrier<>*> wb;
    for (unsigned w = 0; w * 64 < block.x; w++) { wb.push_back(new std::barrier<>(std::min(64u, block.x - 64 * w))); pps::emu_wave[w].bar = wb.back(); }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < block.x; t++) th.emplace_back([&, t]() { threadIdx = dim3(t); blockIdx = dim3(b); pps::emu_parity = 0; k(a...); g_barrier->arrive_and_drop(); });
    for (auto& x : th) x.join();
    for (auto* x : wb) delete x;
  }
}
#include "pps_cov_wide.hip"
#undef __shared__
#define __shared__ static
#include "pps_cov_dense.hip"
namespace pps { unsigned long long launch_count() { return 0; } void count_launch() {} }
using namespace pps;

// the launches of pps_cov_select's pass (pps_cov.cpp: cov_run, the dense-front pass) after the pivot criterion; result4: the status record of the device
extern "C" int emu_cov_dense(int n_fronts, int n_levels, int* f_p, int* f_b, int64_t* f_Loff, int64_t* f_Uoff, int* f_cmap_off, int* cmap, int* parent, int* level_off,
                             int* level_fronts, double* L, double* U, long long n_U, double* S, double* G, long long n_panel, double* result4) {
  DevGraph d; d.n_fronts = n_fronts; d.n_levels = n_levels; d.f_p = f_p; d.f_b = f_b; d.f_Loff = f_Loff; d.f_Uoff = f_Uoff; d.f_cmap_off = f_cmap_off; d.cmap = cmap;
  d.level_fronts = level_fronts; d.L = L; d.U = U; d.result_dev = result4;
  int rc = launch_cov_pivots(d, n_fronts, nullptr); if (rc != 0) return rc;
  const CovDenseExtents ext{n_panel, n_U};
  std::vector<int> off(1, 0);
  for (int s = 0; s < n_fronts; s++) off.push_back(off.back() + cov_dense_pre_items(f_b[s]));
  rc = launch_cov_dense_pre(d, S, G, ext, off.data(), off.back(), n_fronts, nullptr); if (rc != 0) return rc;
  for (int l = n_levels - 1; l >= 0; l--) {
    std::vector<int> og(1, 0), os(1, 0);
    for (int k = level_off[l]; k < level_off[l + 1]; k++) {
      og.push_back(og.back() + cov_dense_gather_items(f_b[level_fronts[k]])); os.push_back(os.back() + cov_dense_strip_items(f_b[level_fronts[k]]));
    }
    rc = launch_cov_dense_level(d, S, G, ext, parent, level_off[l], level_off[l + 1] - level_off[l], og.data(), og.back(), os.data(), os.back(), nullptr);
    if (rc != 0) return rc;
  }
  return 0;
}

#ifdef COV_DENSE_EMU_MAIN
#include <algorithm>
#include <cstdio>
#include <limits>
#include <random>

namespace {

struct Chain {
  std::vector<int> f_p, f_b, f_cmap_off, cmap, parent, level_off, level_fronts;
  std::vector<int64_t> f_Loff, f_Uoff;
  std::vector<double> L;
  long long n_U = 0;
  int n() const { return (int)f_p.size(); }
};

// front s has parent s + 1 and sits alone on level s; its boundary rows map to an increasing subset of the parent's rows
Chain make_chain(const std::vector<int>& p, const std::vector<int>& b, unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  Chain c; c.f_p = p; c.f_b = b; c.f_cmap_off.push_back(0); c.level_off.push_back(0);
  for (int s = 0; s < c.n(); s++) {
    c.f_Loff.push_back((int64_t)c.L.size()); c.f_Uoff.push_back(c.n_U); c.n_U += (long long)(b[s] + 1) * (b[s] + 1);
    c.parent.push_back(s + 1 < c.n() ? s + 1 : -1); c.level_fronts.push_back(s); c.level_off.push_back(s + 1);
    for (int i = 0; i < p[s] + b[s] + 1; i++)
      for (int j = 0; j < p[s]; j++) {
        double v = 0.3 * u(rng) / std::sqrt((double)p[s]);
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

// the recursion of pps_cov.h, front by front from the root, in plain loops; full[s] = [S_AA S_BA'; S_BA S_BB] of (p + b)^2 doubles
std::vector<std::vector<double>> reference(const Chain& c) {
  std::vector<std::vector<double>> full(c.n());
  for (int s = c.n() - 1; s >= 0; s--) {
    const int p = c.f_p[s], b = c.f_b[s], f = p + b;
    const double* Lp = c.L.data() + c.f_Loff[s];
    std::vector<double> X((size_t)p * p, 0.0), G((size_t)b * p, 0.0), F((size_t)f * f, 0.0);
    for (int j = 0; j < p; j++)
      for (int i = j; i < p; i++) {
        double acc = i == j ? 1.0 : 0.0;
        for (int m = j; m < i; m++) acc -= Lp[(size_t)i * p + m] * X[(size_t)m * p + j];
        X[(size_t)i * p + j] = acc / Lp[(size_t)i * p + i];
      }
    for (int i = 0; i < b; i++)
      for (int k = 0; k < p; k++) { double acc = 0.0; for (int m = k; m < p; m++) acc += Lp[(size_t)(p + i) * p + m] * X[(size_t)m * p + k]; G[(size_t)i * p + k] = acc; }
    const int* cm = c.cmap.data() + c.f_cmap_off[s];
    const int fq = b ? c.f_p[s + 1] + c.f_b[s + 1] : 0;
    for (int i = 0; i < b; i++) for (int j = 0; j < b; j++) F[(size_t)(p + i) * f + p + j] = full[s + 1][(size_t)cm[i] * fq + cm[j]];
    for (int i = 0; i < b; i++)
      for (int l = 0; l < p; l++) {
        double acc = 0.0;
        for (int j = 0; j < b; j++) acc += F[(size_t)(p + i) * f + p + j] * G[(size_t)j * p + l];
        F[(size_t)(p + i) * f + l] = -acc; F[(size_t)l * f + p + i] = -acc;
      }
    for (int k = 0; k < p; k++)
      for (int l = 0; l < p; l++) {
        double acc = 0.0;
        for (int m = 0; m < p; m++) acc += X[(size_t)m * p + k] * X[(size_t)m * p + l];
        for (int i = 0; i < b; i++) acc -= G[(size_t)i * p + k] * F[(size_t)(p + i) * f + l];
        F[(size_t)k * f + l] = acc;
      }
    full[s] = F;
  }
  return full;
}

int run(const Chain& c, long long n_U, std::vector<double>* S, std::vector<double>* U, double* status) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  Chain m = c;
  S->assign(c.L.size(), nan); U->assign((size_t)c.n_U, nan);
  std::vector<double> G(c.L.size(), nan);
  double res[4] = {0, 0, 0, 0};
  const int rc = emu_cov_dense(m.n(), m.n(), m.f_p.data(), m.f_b.data(), m.f_Loff.data(), m.f_Uoff.data(), m.f_cmap_off.data(), m.cmap.data(), m.parent.data(),
                               m.level_off.data(), m.level_fronts.data(), m.L.data(), U->data(), n_U, S->data(), G.data(), (long long)m.L.size(), res);
  *status = res[2];
  return rc;
}

int run_chain(const char* label, const std::vector<int>& p, const std::vector<int>& b, unsigned seed) {
  Chain c = make_chain(p, b, seed);
  const std::vector<std::vector<double>> ref = reference(c);
  std::vector<double> S, U;
  double status = 0.0;
  int rc = run(c, c.n_U, &S, &U, &status);
  if (rc != 0 || status != 0.0) { printf("%s: rc %d status %g\n", label, rc, status); return 1; }
  double worst = 0.0, scale = 0.0;
  int bad = 0;
  for (int s = 0; s < c.n(); s++) {
    const int ps = p[s], bs = b[s], f = ps + bs;
    for (int i = 0; i < f; i++)
      for (int j = 0; j < f; j++) {
        if (j >= ps && i < ps) continue;
        const double got = j < ps ? S[(size_t)c.f_Loff[s] + (size_t)i * ps + j] : U[(size_t)c.f_Uoff[s] + (size_t)(i - ps) * bs + (j - ps)];
        const double want = ref[s][(size_t)i * f + j];
        if (!std::isfinite(got)) bad++;
        worst = std::max(worst, std::fabs(got - want)); scale = std::max(scale, std::fabs(want));
      }
    for (int i = 0; i < ps; i++) for (int j = 0; j < i; j++)          // the diagonal block: symmetric bit for bit
      bad += S[(size_t)c.f_Loff[s] + (size_t)i * ps + j] != S[(size_t)c.f_Loff[s] + (size_t)j * ps + i];
  }
  bad += !(worst <= 1e-10 * scale);
  // a collapsed pivot; a child map entry outside the parent; an update-matrix array one double short of the last front's Sigma_BB
  const int mid = c.n() / 2;
  Chain c2 = c; c2.L[(size_t)c.f_Loff[mid] + (size_t)2 * p[mid] + 2] = 1e-9;
  rc = run(c2, c2.n_U, &S, &U, &status); bad += rc != 0 || status != 1.0;
  Chain c3 = c; c3.cmap[c.f_cmap_off[mid] + 1] = p[mid + 1] + b[mid + 1] + 4;
  rc = run(c3, c3.n_U, &S, &U, &status); bad += rc != 0 || status != 64.0;
  for (int i = 0; i < b[mid] * b[mid]; i++) bad += !std::isnan(U[(size_t)c.f_Uoff[mid] + i]);          // nothing of that front was written
  int lastb = c.n() - 1; while (lastb > 0 && b[lastb] == 0) lastb--;
  const long long shortU = c.f_Uoff[lastb] + (long long)b[lastb] * b[lastb] - 1;
  rc = run(c, shortU, &S, &U, &status); bad += rc != 0 || status != 64.0;
  printf("%s: fronts %d, largest difference %.3e of %.3e, %s\n", label, c.n(), worst, scale, bad ? "MISMATCH" : "ok");
  return bad ? 1 : 0;
}

}  // namespace

int main() {
  int bad = 0;
  bad += run_chain("band shapes", {15, 9, 17, 6, 30, 8}, {33, 30, 27, 25, 8, 0}, 1);
  bad += run_chain("wide fronts", {12, 64, 33, 63, 64, 64, 64, 30}, {300, 257, 230, 170, 108, 46, 29, 0}, 2);
  // the tile edges no graph reaches (every shape of a graph is a multiple of 3): four full column tiles at the end of the first and one row
  // into the second 256-row slab of G; p one below / at / one beyond a tile against b around the 32-row k-slab and the 64-row strip (b = 65 and
  // 80: the last strip leaves waves 1 .. 3 without a row); a front of one pivot and one row
  bad += run_chain("p 64, b 257 and 256", {64, 64, 64, 64, 64, 64}, {257, 256, 192, 128, 64, 0}, 3);
  for (int p : {16, 17, 32, 33}) {
    char label[64];
    snprintf(label, sizeof label, "p %d, b 80 65 64 33 32 31", p);
    bad += run_chain(label, {p, p, p, p, p, p, 40}, {80, 65, 64, 33, 32, 31, 0}, 4 + (unsigned)p);
  }
  bad += run_chain("p 1, b 1", {1, 3, 4}, {1, 3, 0}, 5);
  return bad ? 1 : 0;
}
#endif

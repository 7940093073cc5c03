// upmirror_host.cpp -- UploadMirror (csrc/pps_upmirror.h) against a simulated device, without HIP: tests/test_host_upmirror.py builds this
// twice (plain and with the address + undefined-behaviour sanitizers) and runs both.
//
// The device is a byte array that starts as junk.  Its only writers are transcriptions of what flush_uploads does -- one copy of [0, hi) of
// the mirror, or the scatter rule of k_scatter_patches over the table the mirror writes (16-byte units for plain pieces, 8-byte units for
// exact ones) -- and the "refresh" that scribbles over the leading entries of the exact rows behind the mirror's back.  Seeded sequences of
// layouts (appends, single changes, shrinks, arrays that outgrow their slot, an optional array that shifts every owner behind it, SoA rows
// that gain a column or double their leading dimension, exact rows, arena reallocations, abandoned device copies, truthful and -- under
// verification -- lying hints) are uploaded, flushed and read back.  One line per run on stdout: the branch counts the Python test sums.
//
//   upmirror_host            every seed, verification off and on; exit status 0 when every assertion held
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "pps_upmirror.h"

using pps_impl::kNoExact;
using pps_impl::UploadMirror;

namespace {

[[noreturn]] void die(const char* what, uint32_t seed, int step, long long a = 0, long long b = 0) {
  fprintf(stderr, "FAIL seed %u step %d: %s (%lld, %lld)\n", seed, step, what, a, b);
  exit(1);
}

struct Rng {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  size_t below(size_t n) { return n ? next() % n : 0; }
};

enum Kind { PLAIN, ROWS, EXACT_ROWS };
struct Arr {
  Kind kind;
  bool present = true;
  std::vector<char> host;                    // what the host uploads: ints (PLAIN) or rows x ld doubles
  size_t rows = 0, ld = 0, used = 0;         // in elements
  std::vector<char> prev;                    // what this owner uploaded in the previous layout (hints are claims about it)
  bool prev_valid = false; size_t prev_ld = 0, prev_used = 0;
  UploadMirror::Place place;
  std::vector<char> spilled;                 // the allocation of its own when the arena had no room
  size_t exact_from = 0;                     // EXACT_ROWS: what the layout in flight was put with
  size_t scribbled = 0;                      // EXACT_ROWS: entries [0, scribbled) of every row are newer on the device than on the host
  std::vector<double> dev_vals;              // ... their values
  size_t elem() const { return kind == PLAIN ? 4 : 8; }
};

enum Branch { FRESH, KEPT, MOVED, SHIFT, IDENTICAL, EXACT, WHOLE, HINT4K, SPILL, HINT_DROPPED, LIE_CAUGHT, LIE_DROPPED, N_BRANCH };
const char* const kBranchName[N_BRANCH] = {"fresh", "kept", "moved", "shift", "identical", "exact", "whole", "hint4k", "spill", "hint_dropped", "lie_caught", "lie_dropped"};

struct Sim {
  const uint32_t seed; const bool verify;
  Rng rng;
  Sim(uint32_t sd, bool v) : seed(sd), verify(v), rng{sd * 2654435761ull + (uint64_t)v} {}
  int step = 0;
  UploadMirror m;
  std::vector<char> dev, mir;
  size_t arena_off = 0, arena_spill = 0;     // what the caller keeps per arena (pps_graph::Arena)
  bool realloc_next = true;
  std::vector<Arr> arrs;
  void* owners[8] = {};                      // an array's owner is the address of its device pointer
  long long count[N_BRANCH] = {};
  int drawn = 0, skipped = 0;

  void put_int(Arr& a, size_t i, int32_t v) { memcpy(&a.host[4 * i], &v, 4); }
  void put_dbl(Arr& a, size_t i, double v) { memcpy(&a.host[8 * i], &v, 8); }
  double rnd_dbl() { return (double)rng.next() / 65536.0 + 1.0; }
  void grow_plain(Arr& a, size_t n_new) {
    const size_t n0 = a.host.size() / 4;
    a.host.resize(4 * n_new);
    for (size_t i = n0; i < n_new; i++) put_int(a, i, (int32_t)rng.next());
  }
  void init() {
    // order of upload: [big plain | exact rows | optional plain | plain | rows | plain]
    const Kind kinds[6] = {PLAIN, EXACT_ROWS, PLAIN, PLAIN, ROWS, PLAIN};
    const size_t n0[6] = {2500, 0, 40, 300, 0, 90};
    for (int i = 0; i < 6; i++) {
      Arr a; a.kind = kinds[i];
      if (a.kind == PLAIN) grow_plain(a, n0[i] + rng.below(50));
      else { a.rows = i == 1 ? 4 : 6; a.ld = 16; a.used = 3 + rng.below(4); a.host.assign(8 * a.rows * a.ld, 0); for (size_t r = 0; r < a.rows; r++) for (size_t s = 0; s < a.used; s++) put_dbl(a, r * a.ld + s, rnd_dbl()); }
      arrs.push_back(a);
    }
    arrs[2].present = rng.below(2) == 0;
    m.verify_hints = verify;
  }

  // ---- the caller's side of free_device: arenas grow when the last layout spilled; the first arena is small on purpose ----
  void begin_layout() {
    if (realloc_next || arena_spill > 0 || dev.empty()) {
      const size_t want = std::max(arena_off, m.high) + arena_spill;
      const size_t cap = dev.empty() ? 8192 : UploadMirror::grown_capacity(want);
      dev.assign(cap, (char)0xA5);
      m.set_arena(cap);
      mir.resize(cap);
      for (size_t i = 0; i < cap; i++) mir[i] = (char)(0x5A ^ (i * 7));
      m.set_mirror(mir.data(), cap);
      for (Arr& a : arrs) { a.prev_valid = false; settle_scribbles(a); }
      realloc_next = false;
    }
    arena_off = arena_spill = 0;
    m.begin_layout();
  }
  // the host takes the refreshed values home (download_measurements): nothing is newer on the device any more
  void settle_scribbles(Arr& a) {
    for (size_t r = 0; r < a.rows; r++) for (size_t s = 0; s < a.scribbled; s++) put_dbl(a, r * a.ld + s, a.dev_vals[r * a.ld + s]);
    a.scribbled = 0;
  }

  // ---- the device's side of flush_uploads ----
  const UploadMirror::Slot* slot_around(size_t off) const {
    for (const auto& sl : m.slots) if (off >= sl.off && off < sl.off + sl.cap) return &sl;
    return nullptr;
  }
  void flush() {
    if (m.patches.empty()) { m.mark_flushed(); return; }
    if (m.unknown) {
      const size_t hi = m.whole_span();
      if (hi > dev.size() || hi > mir.size()) die("the whole-arena copy leaves the arena", seed, step, (long long)hi);
      memcpy(dev.data(), mir.data(), hi);
      count[WHOLE]++;
    } else {
      std::vector<long long> tab(4 * m.patches.size(), -1);
      m.write_table(tab.data());
      for (size_t i = 0; i < m.patches.size(); i++) {
        const size_t dst = (size_t)tab[4 * i], src = (size_t)tab[4 * i + 1], len = (size_t)tab[4 * i + 2];
        const bool exact = tab[4 * i + 3] != 0;
        const UploadMirror::Slot* sl = slot_around(dst);
        if (!sl) die("a piece starts outside every slot", seed, step, (long long)dst);
        if (dst + len > sl->off + sl->cap) die("a piece ends beyond its slot's capacity", seed, step, (long long)dst, (long long)len);
        if (dst + len > m.high) die("a piece writes at or beyond the high-water mark", seed, step, (long long)dst, (long long)len);
        if (src != dst) die("a piece is read from another offset than it is written to", seed, step, (long long)src, (long long)dst);
        if (exact) {
          // nothing around an exact piece may be written: it lies inside the entries [exact_from, used) of one row of the exact array
          const Arr& a = arrs[1];
          if (sl->owner != &owners[1] || dst % 8 || len % 8) die("an exact piece outside the exact rows, or not in 8-byte units", seed, step, (long long)dst, (long long)len);
          const size_t rel = dst - a.place.off, row = rel / (8 * a.ld), e0 = rel % (8 * a.ld) / 8, e1 = e0 + len / 8;
          if (row >= a.rows || e0 < a.scribbled || e0 < a.exact_from || e1 > a.used) die("an exact piece touches entries outside [exact_from, used) of its row", seed, step, (long long)e0, (long long)e1);
          for (size_t u = 0; u < len / 8; u++) memcpy(&dev[dst + 8 * u], &mir[src + 8 * u], 8);
        } else {
          if (dst % 16) die("a plain piece does not start on a 16-byte boundary", seed, step, (long long)dst);
          for (size_t u = 0; u < len / 16; u++) memcpy(&dev[dst + 16 * u], &mir[src + 16 * u], 16);
          if (len % 16) die("a plain piece is not a whole number of 16-byte units", seed, step, (long long)len);
        }
      }
    }
    m.mark_flushed();
    if (!m.patches.empty() || m.unknown) die("a flush left patches or an unknown device behind", seed, step);
  }

  // ---- one layout: every present array in order, then the flush and the read-back ----
  struct Options { bool hints = false, exact = false, expect_nothing = false, lie = false; };
  static size_t common_prefix(const char* a, const char* b, size_t n, size_t elem) {
    size_t i = 0;
    while (i < n && memcmp(a + i * elem, b + i * elem, elem) == 0) i++;
    return i;
  }
  void layout(const Options& opt) {
    begin_layout();
    // under verification, at most one array of the layout makes a claim that is false
    int liar = -1;
    if (opt.lie) {
      std::vector<int> can;
      for (int i = 0; i < (int)arrs.size(); i++) {
        const Arr& a = arrs[i];
        if (!a.present || !a.prev_valid) continue;
        if (a.kind != PLAIN) { if (a.prev_ld == a.ld && a.used > a.prev_used) can.push_back(i); continue; }      // (the claim: the appended entries are there already)
        const size_t n = a.host.size() / 4, np = a.prev.size() / 4;
        if (common_prefix(a.host.data(), a.prev.data(), std::min(n, np), 4) < std::min(n, np)) can.push_back(i);
      }
      if (!can.empty()) liar = can[rng.below(can.size())];
    }
    bool lie_effective = false;
    for (int i = 0; i < (int)arrs.size(); i++) {
      Arr& a = arrs[i];
      if (!a.present) { a.prev_valid = false; continue; }
      const size_t E = a.elem(), n = a.host.size(), bytes = std::max<size_t>(E, n);
      const size_t k = m.cursor, n_slots = m.slots.size(), n_patches = m.patches.size(), high = m.high;
      const UploadMirror::Place p = m.place(&owners[i], bytes);
      // the slot rule: half as much again, in units of 256 bytes, behind everything placed so far
      if (p.fresh && (p.cap != ((std::max<size_t>(256, bytes + bytes / 2) + 255) & ~size_t(255)) || p.off != ((high + 255) & ~size_t(255)) || m.high != p.off + p.cap))
        die("a fresh slot does not follow the capacity rule", seed, step, (long long)p.off, (long long)p.cap);
      if (p.fits && !p.fresh && (k >= n_slots || m.high != high)) die("a kept slot moved the high-water mark", seed, step, (long long)k);
      a.place = p; a.spilled.clear();
      if (!p.fits) {                                                // the caller's spill: an allocation of its own, copied at once
        arena_spill += bytes + bytes / 2 + 512;
        a.spilled = a.host; a.spilled.push_back(0);                 // (never empty: what marks the array as spilled)
        count[SPILL]++;
        a.prev_valid = false;
        continue;
      }
      if (p.off % 256 || p.off + p.cap > dev.size() || p.cap < bytes) die("a slot is misaligned, too small or outside the arena", seed, step, (long long)p.off, (long long)p.cap);
      arena_off = std::max(arena_off, p.off + bytes);
      const bool was_unknown = m.unknown;
      count[p.fresh ? (k < n_slots ? MOVED : FRESH) : (p.same_owner ? KEPT : SHIFT)]++;
      if (a.kind == PLAIN) {
        size_t same = 0;
        if (a.prev_valid && (opt.hints || i == liar)) {
          const size_t lim = std::min(n, a.prev.size()) / 4;
          same = common_prefix(a.host.data(), a.prev.data(), lim, 4);
          if (i == liar) { same += 1 + rng.below(lim - same); lie_effective = !p.fresh && p.same_owner && !was_unknown; }
          else if (rng.below(3) == 0) same = rng.below(same + 1);
        }
        if (!p.fresh && p.same_owner && !was_unknown && i != liar && (same * 4 & ~size_t(63)) >= 4096) count[HINT4K]++;
        if (!p.fresh && !p.same_owner && !was_unknown && same * 4 >= 64) count[HINT_DROPPED]++;       // a claim about another slot: the mirror must not use it
        m.put_array(p, a.host.data(), n, same * 4);
        if (!p.fresh && !was_unknown && n > 0 && m.patches.size() == n_patches) count[IDENTICAL]++;
      } else {
        size_t same = 0;
        if (a.prev_valid && opt.hints && a.prev_ld == a.ld) {
          same = std::min(a.used, a.prev_used);
          for (size_t r = 0; r < a.rows; r++) same = std::min(same, common_prefix(&a.host[8 * r * a.ld], &a.prev[8 * r * a.ld], same, 8));
        }
        const bool exact = a.kind == EXACT_ROWS && opt.exact;
        const bool force = !exact && !opt.expect_nothing && rng.below(8) == 0;       // (unknown_meas: the whole rows again)
        if (i == liar) { same = a.used; lie_effective = !p.fresh && p.same_owner && !was_unknown && !force; }
        if (exact) {
          // the refresh wrote every entry the device had (a.prev_used per row); the host's copies of those are older and unchanged
          if (p.fresh || was_unknown || a.prev_ld != a.ld) die("the test drives exact rows into a slot that cannot keep them", seed, step);
          a.exact_from = a.prev_used;
          m.put_rows_exact(p, a.host.data(), n, a.rows, 8 * a.ld, 8 * a.used, 8 * a.exact_from, 8 * same);
          count[EXACT]++;
        } else {
          m.put_rows(p, a.host.data(), n, a.rows, 8 * a.ld, 8 * a.used, force, 8 * same);
        }
      }
      if (p.fresh && (m.patches.size() != n_patches + 1 || m.patches.back().off != p.off || m.patches.back().len != p.cap))
        die("a fresh slot is not sent over its whole capacity", seed, step, i);
      a.prev = a.host; a.prev_valid = true; a.prev_ld = a.ld; a.prev_used = a.used;
    }
    if (opt.expect_nothing && !m.patches.empty()) die("an unchanged layout sends something", seed, step, (long long)m.patches.size());
    const bool violation = m.take_violation();
    if (violation != lie_effective) die(violation ? "the violation flag was set without a lying hint" : "a lying hint did not set the violation flag", seed, step, liar);
    if (liar >= 0) count[lie_effective ? LIE_CAUGHT : LIE_DROPPED]++;
    flush();
    if (lie_effective) {
      // (the caller answers PPS_ESTATE; the bytes behind the false claim were skipped.)  The device copy is given up, as after any failure
      m.forget_device(); m.forget_measurements();
      for (Arr& a : arrs) settle_scribbles(a);
      Options again; layout(again);
      return;
    }
    read_back();
  }

  void read_back() {
    for (int i = 0; i < (int)arrs.size(); i++) {
      const Arr& a = arrs[i];
      if (!a.present) continue;
      const char* have = a.spilled.empty() ? dev.data() + a.place.off : a.spilled.data();
      if (a.kind == PLAIN) {
        if (memcmp(have, a.host.data(), a.host.size()) != 0) die("an array does not read back as its content", seed, step, i);
      } else {
        for (size_t r = 0; r < a.rows; r++)
          for (size_t s = 0; s < a.used; s++) {
            const void* want = s < a.scribbled ? (const void*)&a.dev_vals[r * a.ld + s] : (const void*)&a.host[8 * (r * a.ld + s)];
            if (memcmp(have + 8 * (r * a.ld + s), want, 8) != 0) die(s < a.scribbled ? "a refreshed entry of the exact rows was overwritten" : "a row does not read back as its content", seed, step, i, (long long)(r * a.ld + s));
          }
      }
      // a slot created by this layout is defined over its whole capacity: zeros behind the content
      if (a.spilled.empty() && a.place.fresh)
        for (size_t b = a.host.size(); b < a.place.cap; b++) if (dev[a.place.off + b] != 0) die("a fresh slot is not zero behind its content", seed, step, i, (long long)b);
    }
    // the mirror equals the device over every slot's whole capacity, except the refreshed entries
    const Arr& x = arrs[1];
    for (size_t k = 0; k < m.slots.size(); k++) {
      const auto& sl = m.slots[k];
      for (size_t b = 0; b < sl.cap; b++) {
        if (dev[sl.off + b] == mir[sl.off + b]) continue;
        const size_t e = b / 8 % x.ld;
        if (sl.owner == &owners[1] && x.spilled.empty() && b < 8 * x.rows * x.ld && e < x.scribbled) continue;
        die("the mirror differs from the device inside a slot", seed, step, (long long)k, (long long)b);
      }
    }
  }

  // ---- the drawn steps ----
  std::vector<int> plain_ids() const { std::vector<int> v; for (int i = 0; i < (int)arrs.size(); i++) if (arrs[i].kind == PLAIN && arrs[i].present) v.push_back(i); return v; }
  bool can_go_exact() const {
    const Arr& x = arrs[1];
    return !m.unknown && !realloc_next && arena_spill == 0 && x.spilled.empty() && x.prev_valid && x.prev_ld == x.ld && x.place.fits;
  }
  void one_step() {
    step++; drawn++;
    Options opt;
    opt.hints = rng.below(3) != 0;
    opt.lie = verify && rng.below(5) == 0;
    const std::vector<int> pl = plain_ids();
    Arr& pick = arrs[pl[rng.below(pl.size())]];
    const size_t np = pick.host.size() / 4;
    bool ok = true;
    switch (rng.below(11)) {
      case 0: for (int i : pl) grow_plain(arrs[i], arrs[i].host.size() / 4 + rng.below(i == 0 ? 64 : 8)); break;                     // append
      case 1: if (np == 0) ok = false; else put_int(pick, rng.below(np), (int32_t)rng.next()); break;                                   // one element changes
      case 2: if (np < 2) ok = false; else pick.host.resize(4 * (np - 1 - rng.below(np / 2))); break;                                   // shrink
      case 3: grow_plain(pick, np + np / 2 + 70 + rng.below(100)); break;                                                               // outgrows its slot
      case 4:                                                                                                                           // every later owner shifts (and one of them may change)
        arrs[2].present = !arrs[2].present;
        if (rng.below(2)) { Arr& a = arrs[rng.below(2) ? 3 : 5]; const size_t na = a.host.size() / 4; if (na) put_int(a, na / 2 + rng.below(na - na / 2), (int32_t)rng.next()); }
        break;
      case 5:                                                                                                                           // a column per row
        if (arrs[1].used == arrs[1].ld || arrs[4].used == arrs[4].ld) { ok = false; break; }
        for (Arr& a : arrs) if (a.kind != PLAIN) { for (size_t r = 0; r < a.rows; r++) put_dbl(a, r * a.ld + a.used, rnd_dbl()); a.used++; }
        break;
      case 6: {                                                                                                                         // leading dimension doubles
        Arr& a = arrs[rng.below(2) ? 1 : 4];
        settle_scribbles(a);
        std::vector<char> old = a.host;
        a.host.assign(8 * a.rows * 2 * a.ld, 0);
        for (size_t r = 0; r < a.rows; r++) memcpy(&a.host[8 * r * 2 * a.ld], &old[8 * r * a.ld], 8 * a.used);
        a.ld *= 2;
      } break;
      case 7: case 8: {                                                                                                                 // the device refreshes the exact rows; a few are appended
        Arr& a = arrs[1];
        if (!can_go_exact() || a.prev_used == 0) { ok = false; break; }
        a.dev_vals.resize(a.rows * a.ld);
        a.scribbled = a.prev_used;
        for (size_t r = 0; r < a.rows; r++)
          for (size_t s = 0; s < a.scribbled; s++) { const double v = rnd_dbl(); a.dev_vals[r * a.ld + s] = v; memcpy(&dev[a.place.off + 8 * (r * a.ld + s)], &v, 8); }
        for (size_t add = rng.below(4); add > 0 && a.used < a.ld; add--) { for (size_t r = 0; r < a.rows; r++) put_dbl(a, r * a.ld + a.used, rnd_dbl()); a.used++; }
        opt.exact = true;
      } break;
      case 9: if (rng.below(2)) realloc_next = true; else { m.forget_device(); m.forget_measurements(); for (Arr& a : arrs) settle_scribbles(a); } break;   // arena reallocated / device copy abandoned
      case 10: opt.expect_nothing = arena_spill == 0 && !m.unknown && !realloc_next; ok = opt.expect_nothing; opt.hints = rng.below(2); opt.lie = false; break;
    }
    if (!ok) { skipped++; return; }
    // refreshed entries stay on the device across layouts that can keep them (keep_meas), else they are taken home first
    if (!opt.exact && arrs[1].scribbled > 0) { if (can_go_exact()) opt.exact = true; else settle_scribbles(arrs[1]); }
    layout(opt);
  }
  void run(int steps) {
    init();
    Options first; layout(first);
    for (int s = 0; s < steps; s++) one_step();
    std::string line = "run seed " + std::to_string(seed) + " verify " + std::to_string((int)verify) + " drawn " + std::to_string(drawn) + " skipped " + std::to_string(skipped);
    for (int b = 0; b < N_BRANCH; b++) line += std::string(" ") + kBranchName[b] + " " + std::to_string(count[b]);
    line += " compared " + std::to_string(m.bytes_compared) + " sent " + std::to_string(m.bytes_sent) + " patches " + std::to_string(m.n_patches);
    puts(line.c_str());
  }
};

}  // namespace

int main() {
  // (chosen on the CPU so that every branch occurs at least three times over the set and no run skips more than a quarter of its steps)
  const uint32_t seeds[] = {1, 2, 3, 5, 8, 13, 21, 34};
  for (uint32_t seed : seeds)
    for (int verify = 0; verify < 2; verify++) {
      Sim* s = new Sim(seed, verify != 0);
      s->run(80);
      delete s;
    }
  return 0;
}

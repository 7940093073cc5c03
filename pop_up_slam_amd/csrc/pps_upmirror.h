// pps_upmirror.h -- the bookkeeping of the difference upload: which slot of the upload arena every array went to, what the device holds there,
// and which bytes have to travel.  Host only, no HIP: the pinned mirror and the arena are handed in as pointer / capacity, pps_upload.cpp keeps every
// allocation, copy and launch (dev_upload*, flush_uploads).  tests/cpp/upmirror_host.cpp drives it against a simulated device.
//
// Invariant: between two flushes that nobody invalidated (forget_device), the mirror equals the device over the whole capacity of every slot,
// except the entries [0, exact_from) of rows put with put_rows_exact -- kernels refresh those behind the mirror's back, and no piece touches them.
//
// Frame loops re-upload a topology that is the previous one plus a little: the k-th upload of a layout goes where the k-th upload of the previous
// layout went, as long as it fits the slot (capacity: half as much again), and only the bytes that differ from the mirror are sent -- as pieces
// that k_scatter_patches reads straight from the pinned mirror (whose offsets are the arena's), or in one copy of [0, high) when the device
// content is unknown.
// owner: which array (the address of its device pointer) the slot received last.  Slots go by call order, and an array that is uploaded only on
// some graphs (obs_ray: re-popping edges) shifts every array behind it by one slot when it appears or goes: a claim about "what this slot received
// last time" (kept-prefix hints, rows sent by the previous upload) holds only while the owner is the same.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

namespace pps_impl {

// exact_from (rows of 8-byte values only): entries [0, exact_from) of every row are newer on the device than anywhere on the host (measurements
// refreshed by k_refresh_measurements) -- exactly the entries [exact_from, used) are sent, byte for byte, and nothing around them (a piece rounded
// to the 64-byte compare stride or to the 16-byte copy unit would put the mirror's stale values over up to seven refreshed neighbours)
constexpr size_t kNoExact = (size_t)-1;

struct UploadMirror {
  static constexpr size_t npos = (size_t)-1;
  struct Slot { size_t off, cap; const void* owner; };
  struct Patch { size_t off, len; bool exact8; };      // exact8: 8-byte granularity, nothing around the piece may be written
  // where an upload goes.  !fits: neither its old slot nor the rest of the arena holds it (the caller spills into an allocation of its own).
  // fresh: a new slot, defined over its whole capacity by the put that follows.  same_owner: the slot received this array last time too.
  struct Place { bool fits = false, fresh = false, same_owner = false; size_t off = 0, cap = 0; };

  char* mir = nullptr;                 // the pinned mirror (at least arena_cap bytes) and the capacity of the device arena it describes
  size_t mir_cap = 0, arena_cap = 0;
  std::vector<Slot> slots;
  size_t cursor = 0, high = 0;         // uploads of the current layout so far; end of the last slot
  bool unknown = true;                 // the mirror says nothing about the device
  bool unknown_meas = false;           // ... only about the measurement arrays (written behind the mirror's back)
  bool verify_hints = false;           // check every `same` claim against the mirror (PPS_DEBUG_VERIFY_UPLOAD), read once per upload
  bool hint_violation = false;
  std::vector<Patch> patches;          // what the next flush sends
  size_t bytes_compared = 0, bytes_sent = 0, n_patches = 0;      // over the life of the handle (PPS_TIMING=2 prints them)

  // arenas grow to twice what the last layout needed (off + spill of the arena; for the upload arena at least `high`)
  static size_t grown_capacity(size_t want) { return std::max<size_t>(size_t(1) << 20, 2 * want); }
  void set_arena(size_t cap) { arena_cap = cap; slots.clear(); high = 0; unknown = true; }            // (re)allocated or released
  void set_mirror(char* p, size_t cap) { mir = p; mir_cap = cap; unknown = true; }
  void forget_device() { unknown = true; }
  void forget_measurements() { unknown_meas = true; }
  // (a slot the layout that ends here did not reach holds what an older layout sent: no claim about "last time" applies to it)
  void begin_layout() {
    for (size_t k = cursor; k < slots.size(); k++) slots[k].owner = nullptr;
    cursor = 0; patches.clear();
  }
  size_t slot_of(const void* owner) const {
    for (size_t k = 0; k < slots.size() && k < cursor; k++) if (slots[k].owner == owner) return k;
    return npos;
  }
  bool take_violation() { const bool v = hint_violation; hint_violation = false; return v; }

  // the next upload of the layout: `bytes` (>= 1) of the array `owner`
  Place place(const void* owner, size_t bytes) {
    const size_t k = cursor++;
    if (!mir || !arena_cap) return Place();
    if (k < slots.size() && bytes <= slots[k].cap) {
      const bool same_owner = slots[k].owner == owner;      // else the slot held another array: its bytes are compared like any others
      slots[k].owner = owner;
      return Place{true, false, same_owner, slots[k].off, slots[k].cap};
    }
    const size_t cap = (std::max<size_t>(256, bytes + bytes / 2) + 255) & ~size_t(255), o = (high + 255) & ~size_t(255);
    if (o + cap > arena_cap) return Place();                // arena exhausted (it is re-sized at the next layout)
    if (k < slots.size()) slots[k] = Slot{o, cap, owner}; else slots.push_back(Slot{o, cap, owner});
    high = o + cap;
    return Place{true, true, false, o, cap};
  }

  // n bytes of an array; same: leading bytes the caller knows to be what this slot received last time
  void put_array(const Place& p, const char* src, size_t n, size_t same) { put_rows(p, src, n, 1, n, n, false, same); }
  // an SoA array of `rows` rows with leading dimension ld of which the first `used` bytes per row are live (n = rows * ld): the rows are compared
  // one by one (appending a factor touches the end of every row, not the array from end to end).  same: leading bytes of every row, as above
  void put_rows(const Place& p, const char* src, size_t n, size_t rows, size_t ld, size_t used, bool force, size_t same, size_t exact_from = kNoExact) {
    if (p.fresh) return define(p, src, n);
    if (unknown || n == 0) return diff(p.off, src, n, force, 0);
    const size_t keep = p.same_owner ? std::min(same, used) : 0;
    for (size_t r = 0; r < rows; r++) {
      if (exact_from == kNoExact || force) { diff(p.off + r * ld, src + r * ld, used, force, keep); continue; }
      char* row = mir + p.off + r * ld;
      if (keep && verify_hints && memcmp(row, src + r * ld, keep) != 0) hint_violation = true;
      memcpy(row + keep, src + r * ld + keep, used - keep);      // the mirror keeps the host's view of the row
      bytes_compared += used;
      if (used > exact_from) patches.push_back(Patch{p.off + r * ld + exact_from, used - exact_from, true});
    }
  }
  // ... of 8-byte values whose entries [0, exact_from) per row the device may hold newer than the host: see kNoExact
  void put_rows_exact(const Place& p, const char* src, size_t n, size_t rows, size_t ld, size_t used, size_t exact_from, size_t same) { put_rows(p, src, n, rows, ld, used, false, same, exact_from); }

  // What a flush sends: [0, whole_span()) of the mirror in one copy when the device content is unknown.  Otherwise nothing but the changed pieces
  // may be written: the span between two pieces can hold what kernels have refreshed behind the mirror's back (the observation measurements that
  // stay on the device) -- a copy "from the first to the last change" would put stale values over them.
  size_t whole_span() const {
    size_t hi = high;
    for (const Patch& pt : patches) hi = std::max(hi, pt.off + pt.len);
    return std::min(hi, mir_cap);
  }
  // ... the pieces as the table k_scatter_patches reads: (destination, source, bytes, unit) per piece, four long long each.  Lengths are rounded
  // up to 16 bytes except where the bytes behind a piece may be newer on the device than in the mirror (exact pieces are multiples of 8; every
  // slot's capacity is a multiple of 16)
  void write_table(long long* tab) const {
    for (size_t i = 0; i < patches.size(); i++) {
      const Patch& pt = patches[i];
      tab[4 * i + 0] = tab[4 * i + 1] = (long long)pt.off;
      tab[4 * i + 2] = (long long)(pt.exact8 ? pt.len : ((pt.len + 15) & ~size_t(15)));
      tab[4 * i + 3] = pt.exact8 ? 1 : 0;
    }
  }
  void mark_flushed() {            // (a flush with nothing to send leaves everything as it is, `unknown` included)
    if (patches.empty()) return;
    n_patches += patches.size();
    if (unknown) bytes_sent += whole_span();
    else for (const Patch& pt : patches) bytes_sent += pt.len;
    unknown = false;
    patches.clear();
  }

 private:
  // A slot that has just been created (or moved behind the others because it outgrew its place) lies in a part of the arena the mirror says
  // nothing about: neither side has ever been written there, and a diff against it may find the new bytes "already there" (zeros against a
  // fresh pinned page, say) and leave the device with whatever it held.  Define the whole slot -- capacity, not just what is used today: later
  // uploads grow into it -- and send it once.
  void define(const Place& p, const char* src, size_t n) {
    memset(mir + p.off, 0, p.cap);
    if (n) memcpy(mir + p.off, src, n);
    bytes_compared += p.cap;
    patches.push_back(Patch{p.off, p.cap, false});
  }
  // bytes [0, n) of `src` against the mirror at offset o: record (and copy into the mirror) the range that differs.  same: leading bytes the
  // caller knows to be in the mirror already: the comparison starts behind them
  void diff(size_t o, const char* src, size_t n, bool force, size_t same) {
    if (n == 0) return;
    char* m = mir + o;
    bytes_compared += n;
    if (unknown || force) { memcpy(m, src, n); patches.push_back(Patch{o, n, false}); return; }
    if (same && verify_hints && memcmp(m, src, same) != 0) hint_violation = true;      // (the whole claim, not only the chunks it saves)
    same &= ~size_t(63);
    // first and last 64-byte chunk that differs from what the device holds (4 KB strides first: most arrays of a frame loop are unchanged from
    // end to end, or up to a short tail)
    size_t lo = same, hi = n;
    while (lo + 4096 <= hi && memcmp(m + lo, src + lo, 4096) == 0) lo += 4096;
    while (lo + 64 <= hi && memcmp(m + lo, src + lo, 64) == 0) lo += 64;
    if (lo + 64 > hi && memcmp(m + lo, src + lo, hi - lo) == 0) return;      // identical
    while (hi >= lo + 4096 && memcmp(m + hi - 4096, src + hi - 4096, 4096) == 0) hi -= 4096;
    while (hi >= lo + 64 && memcmp(m + hi - 64, src + hi - 64, 64) == 0) hi -= 64;
    lo &= ~size_t(15);
    memcpy(m + lo, src + lo, hi - lo);
    patches.push_back(Patch{o + lo, hi - lo, false});
  }
};

}  // namespace pps_impl

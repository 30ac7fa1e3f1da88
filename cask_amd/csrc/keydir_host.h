// The host keydir of the engine above the C ABI: the keydir fold Index::update + Stats
// (cask.rs:28-95; stats.rs:6-67) over hash-split open-addressing tables, the little-endian field
// accessors of the record formats, and the units of work of the fold on threads (keydir_host.cpp).
// Member functions are defined in-class: every user of the tables inlines them.
#pragma once
#include <sys/mman.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/cask_scan.h"
#include "host_ring.h"

// The engine's internal names (engine_*.cpp, keydir_host.cpp); none of them leaves the library.
#define CASK_ENGINE_NAMESPACE namespace cask_engine __attribute__((visibility("hidden")))

CASK_ENGINE_NAMESPACE {

inline uint16_t rd16(const uint8_t* p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
inline uint64_t rd64(const uint8_t* p) { return (uint64_t)rd32(p) | ((uint64_t)rd32(p + 4) << 32); }
inline void wr16(uint8_t* p, uint16_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
inline void wr32(uint8_t* p, uint32_t v) { for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i)); }
inline void wr64(uint8_t* p, uint64_t v) { for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i)); }

inline uint64_t hash_key(const uint8_t* k, uint32_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (n * 0xC2B2AE3D27D4EB4Full);
  uint32_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    memcpy(&w, k + i, 8);
    h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 31;
  }
  uint64_t t = 0;
  for (uint32_t j = 0; i + j < n; ++j) t |= (uint64_t)k[i + j] << (8 * j);
  h = (h ^ t) * 0x94D049BB133111EBull;
  return h ^ (h >> 29);
}

struct StatsEntry {  // stats.rs:7-11
  uint64_t entries = 0, dead_entries = 0, dead_bytes = 0;
};
using StatsMap = std::unordered_map<uint32_t, StatsEntry>;

// Stats::add_entry / remove_entry (stats.rs:23-48) into `st`. A fold on threads keeps per-table
// deltas: then `base` is the map entering the fold, and a remove of a file absent from the delta
// still counts when that file has a row there (remove_entry only skips files with no row at all).
// The rows a fold touches are few (the files of the replay) and each is touched by most records: a
// 16-entry cache of row pointers by file id (unordered_map elements never move) keeps the map
// lookups off the per-record path.
class StatsDelta {
 public:
  StatsDelta(StatsMap& st, const StatsMap* base) : st_(st), base_(base) {}
  void add(uint32_t file_id) { get(file_id, true)->entries += 1; }
  void remove(uint32_t file_id, uint64_t size) {
    StatsEntry* e = get(file_id, false);
    if (!e) return;  // "Tried to reclaim non-existant entry": warn only
    e->dead_entries += 1;
    e->dead_bytes += size;
  }

 private:
  StatsEntry* get(uint32_t fid, bool create) {
    const unsigned c = fid & 15u;
    if (ce_[c] && cf_[c] == fid) return ce_[c];
    auto it = st_.find(fid);
    if (it == st_.end()) {
      if (!create && !(base_ && base_->count(fid))) return nullptr;
      it = st_.emplace(fid, StatsEntry{}).first;
    }
    cf_[c] = fid;
    ce_[c] = &it->second;
    return ce_[c];
  }
  StatsMap& st_;
  const StatsMap* base_;
  uint32_t cf_[16] = {};
  StatsEntry* ce_[16] = {};
};

// Allocator for large tables: 2-MiB-aligned and advised as transparent huge pages (a keydir fold
// hits random slots of tables of tens of MB; with 4-KiB pages nearly every access also misses the
// TLB). Small allocations take the ordinary heap; up to kMap the heap's huge-aligned blocks (which a
// later table of the process reuses without new page faults: the host fold's 16-MB tables), above it
// fresh anonymous pages, zero until first written, so a table of empty slots costs no fill pass
// (KeyDir::reserve; configs[3]'s merge tables of ~90 MB, which the heap would map afresh anyway).
template <class T>
struct HugeAlloc {
  using value_type = T;
  HugeAlloc() = default;
  template <class U>
  HugeAlloc(const HugeAlloc<U>&) {}
  static constexpr size_t kHuge = 2ull << 20, kMap = 32ull << 20;
  static size_t rounded(size_t b) { return (b + kHuge - 1) & ~(kHuge - 1); }
  T* allocate(size_t n) {
    const size_t b = n * sizeof(T);
    if (b < kHuge) {
      void* p = ::operator new(b, std::align_val_t(alignof(T) < 64 ? 64 : alignof(T)));
      return static_cast<T*>(p);
    }
    const size_t r = rounded(b);
    if (b < kMap) {
      void* p = std::aligned_alloc(kHuge, r);
      if (!p) throw std::bad_alloc();
      (void)madvise(p, r, MADV_HUGEPAGE);
      return static_cast<T*>(p);
    }
    // (over-map by one huge page and trim to a 2-MiB-aligned range)
    void* m = mmap(nullptr, r + kHuge, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (m == MAP_FAILED) throw std::bad_alloc();
    const uintptr_t a = ((uintptr_t)m + kHuge - 1) & ~(uintptr_t)(kHuge - 1);
    if (a > (uintptr_t)m) munmap(m, a - (uintptr_t)m);
    const uintptr_t e = (uintptr_t)m + r + kHuge;
    if (e > a + r) munmap((void*)(a + r), e - (a + r));
    (void)madvise((void*)a, r, MADV_HUGEPAGE);
    return reinterpret_cast<T*>(a);
  }
  static bool zeroed(size_t n) { return n * sizeof(T) >= kMap; }  // allocate(n) hands out zero bytes
  template <class U>
  void construct(U* p) noexcept {  // resize/size-constructor leave trivial elements uninitialized
    ::new (static_cast<void*>(p)) U;
  }
  template <class U, class... A>
  void construct(U* p, A&&... a) {
    ::new (static_cast<void*>(p)) U(std::forward<A>(a)...);
  }
  void deallocate(T* p, size_t n) {
    const size_t b = n * sizeof(T);
    if (b < kHuge) ::operator delete(p, std::align_val_t(alignof(T) < 64 ? 64 : alignof(T)));
    else if (b < kMap) std::free(p);
    else munmap(p, rounded(b));
  }
  template <class U>
  bool operator==(const HugeAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const HugeAlloc<U>&) const { return false; }
};

// One table of HashMap<Vec<u8>, IndexEntry> (cask.rs:28-31). Open addressing over 64-B slots (one
// cache line each); a key of up to 16 bytes lives in its slot, a longer one in an append-only arena
// (the reference copies every key: hint.key.to_vec(), cask.rs:68). A fold touches one line per
// record for short keys: the slot holds hash, entry and key.
class KeyDir {
 public:
  static constexpr uint32_t kInline = 16;
  struct alignas(64) Slot {
    uint64_t hash;
    cask_index_entry e;
    uint32_t ksz;
    uint32_t state;  // 0 empty, 1 live, 2 deleted
    union {
      uint8_t kin[kInline];  // ksz <= kInline
      uint64_t key_off;      // else: the key's offset in the arena
    };
  };
  static_assert(sizeof(Slot) == 64, "a slot is one cache line");
  std::vector<Slot, HugeAlloc<Slot>> slots;
  std::vector<uint8_t> arena;
  uint64_t live = 0, used = 0;

  KeyDir() { slots.assign(256, Slot{}); }

  const uint8_t* key_of(const Slot& s) const { return s.ksz <= kInline ? s.kin : arena.data() + s.key_off; }
  // a key's home slot: the hash's bits below the table bits (Index::sub_of), scaled to the table —
  // any size, not only powers of two (a table sized to its keys: 4.5 instead of 8 GB of slots for
  // configs[3]'s 52 M keys, all of which are first-touch page faults in the merge)
  uint64_t home(uint64_t h) const { return (uint64_t)(((unsigned __int128)(h << 6) * slots.size()) >> 64); }
  void prefetch(uint64_t h) const { __builtin_prefetch(&slots[home(h)]); }
  // the arena bytes of a long key on the slot h lands on, once that slot is in cache (prefetch() a
  // few records before)
  void prefetch_key(uint64_t h) const {
    const Slot& s = slots[home(h)];
    if (s.state == 1 && s.hash == h && s.ksz > kInline) __builtin_prefetch(arena.data() + s.key_off);
  }

  bool key_eq(const Slot& s, const uint8_t* k, uint32_t n) const {
    if (n == kInline) {  // (the common fixed-size key: two word compares, no call)
      uint64_t a[2], b[2];
      memcpy(a, s.kin, 16);
      memcpy(b, k, 16);
      return a[0] == b[0] && a[1] == b[1];
    }
    return n == 0 || memcmp(key_of(s), k, n) == 0;
  }

  int64_t find(const uint8_t* k, uint32_t n, uint64_t h) const {
    const uint64_t c = slots.size();
    for (uint64_t i = home(h);; i = i + 1 == c ? 0 : i + 1) {
      const Slot& s = slots[i];
      if (s.state == 0) return -(int64_t)i - 1;
      if (s.state == 1 && s.hash == h && s.ksz == n && key_eq(s, k, n)) return (int64_t)i;
    }
  }

  // Room for n live keys without growing; a rebuild drops the slots of deleted keys.
  void reserve(uint64_t n) {
    // A table holds up to 3/4 of its slots; one that must grow is sized to 2/5 (a slot is a line:
    // each probe past the home slot is one more line, each slot a first-touch fault. configs[3]'s
    // 52 M-key merge: loads 0.39-0.6 within 15 % of each other, 0.39 the fastest,
    // profiles/r06h_merge_loadsweep.txt; its compaction's 42 M lookups: 0.70-0.74 s at 0.39 against
    // 0.86-0.87 at 0.6, profiles/r06k_compaction_ab.txt)
    const uint64_t m = std::max(n, live) + 1;
    const bool fits = slots.size() * 3 >= m * 4;
    if (fits && (used + 1) * 4 <= slots.size() * 3) return;
    constexpr uint64_t kG = HugeAlloc<Slot>::kHuge / sizeof(Slot);  // (whole huge pages when large)
    const uint64_t need = m * 5 / 2 + 1;
    const uint64_t cap = fits ? slots.size()  // (same size: the deleted slots dropped)
                         : need <= 256 ? 256 : need < kG ? (need + 63) & ~63ull : (need + kG - 1) / kG * kG;
    std::vector<Slot, HugeAlloc<Slot>> old;
    old.swap(slots);
    slots.resize(cap);  // (default-initialised: a huge allocation is zero already, see HugeAlloc)
    if (!HugeAlloc<Slot>::zeroed(cap)) memset((void*)slots.data(), 0, cap * sizeof(Slot));
    used = 0;
    for (const Slot& s : old) {
      if (s.state != 1) continue;
      uint64_t i = home(s.hash);
      while (slots[i].state) i = i + 1 == cap ? 0 : i + 1;
      slots[i] = s;
      ++used;
    }
  }

  // Index::update's effect on the keydir alone (cask.rs:60-90 without the Stats calls): the fold of
  // the sharded replay, whose stats come from per-file counts (cask_keydir_finish).
  void update_kd(const uint8_t* key, uint32_t ksz, uint32_t file_id, uint64_t pos, uint32_t vsz_raw, uint64_t seq,
                 uint64_t h) {
    const bool deleted = vsz_raw == CASK_ENTRY_TOMBSTONE;
    if ((used + 1) * 4 > slots.size() * 3) reserve(live + live / 2 + 1);
    const int64_t f = find(key, ksz, h);
    if (f >= 0) {
      Slot& s = slots[f];
      if (s.e.sequence <= seq) {
        if (deleted) {
          s.state = 2;
          --live;
        } else {
          s.e = cask_index_entry{file_id, 0, pos, 18ull + ksz + vsz_raw, seq};
        }
      }
      return;
    }
    if (deleted) return;
    insert_at((uint64_t)(-f - 1), key, ksz, h, cask_index_entry{file_id, 0, pos, 18ull + ksz + vsz_raw, seq});
  }

  // Index::update (cask.rs:60-90). vsz_raw is the hint's value_size field.
  void update(const uint8_t* key, uint32_t ksz, uint32_t file_id, uint64_t pos, uint32_t vsz_raw, uint64_t seq,
              uint64_t h, StatsDelta& sd) {
    const bool deleted = vsz_raw == CASK_ENTRY_TOMBSTONE;
    cask_index_entry ie{};
    ie.file_id = file_id;
    ie.entry_pos = pos;
    ie.entry_size = 18ull + ksz + (deleted ? 0ull : (uint64_t)vsz_raw);  // data.rs:238-240
    ie.sequence = seq;
    if ((used + 1) * 4 > slots.size() * 3) reserve(live + live / 2 + 1);
    int64_t f = find(key, ksz, h);
    if (f >= 0) {  // Occupied
      Slot& s = slots[f];
      if (s.e.sequence <= seq) {
        sd.remove(s.e.file_id, s.e.entry_size);
        if (deleted) {
          s.state = 2;
          --live;
        } else {
          sd.add(file_id);
          s.e = ie;
        }
      } else {
        sd.add(file_id);
        sd.remove(file_id, ie.entry_size);
      }
      return;
    }
    if (deleted) return;  // Vacant + tombstone: nothing
    sd.add(file_id);
    insert_at((uint64_t)(-f - 1), key, ksz, h, ie);
  }

 private:
  void insert_at(uint64_t i, const uint8_t* key, uint32_t ksz, uint64_t h, const cask_index_entry& e) {
    Slot& s = slots[i];
    s.hash = h;
    s.ksz = ksz;
    s.state = 1;
    s.e = e;
    if (ksz <= kInline) {
      if (ksz) memcpy(s.kin, key, ksz);
    } else {
      s.key_off = arena.size();
      arena.insert(arena.end(), key, key + ksz);
    }
    ++live;
    ++used;
  }
};

// The keydir (Index, cask.rs:28-95): kSub tables split by key hash, so a fold on threads writes each
// table from one thread with no merge pass afterwards; one Stats map.
class Index {
 public:
  static constexpr unsigned kSub = 64;
  KeyDir sub[kSub];
  StatsMap stats;

  static unsigned sub_of(uint64_t h) { return (unsigned)(h >> 58); }
  uint64_t live() const {
    uint64_t n = 0;
    for (const KeyDir& k : sub) n += k.live;
    return n;
  }
  const cask_index_entry* get(const uint8_t* k, uint32_t n) const {  // Index::get (cask.rs:41-43)
    return get_h(k, n, hash_key(k, n));
  }
  const cask_index_entry* get_h(const uint8_t* k, uint32_t n, uint64_t h) const {
    const KeyDir& t = sub[sub_of(h)];
    const int64_t f = t.find(k, n, h);
    return f >= 0 ? &t.slots[(uint64_t)f].e : nullptr;
  }
  void update(const uint8_t* key, uint32_t ksz, uint32_t file_id, uint64_t pos, uint32_t vsz_raw, uint64_t seq) {
    const uint64_t h = hash_key(key, ksz);
    StatsDelta sd(stats, nullptr);
    sub[sub_of(h)].update(key, ksz, file_id, pos, vsz_raw, seq, h, sd);
  }
  void update_kd(const uint8_t* key, uint32_t ksz, uint32_t file_id, uint64_t pos, uint32_t vsz_raw, uint64_t seq) {
    const uint64_t h = hash_key(key, ksz);
    sub[sub_of(h)].update_kd(key, ksz, file_id, pos, vsz_raw, seq, h);
  }
  void prefetch(uint64_t h) const { sub[sub_of(h)].prefetch(h); }
  void prefetch_key(uint64_t h) const { sub[sub_of(h)].prefetch_key(h); }
  template <class F>
  void for_each_live(F fn) const {
    for (const KeyDir& t : sub)
      for (const KeyDir::Slot& s : t.slots)
        if (s.state == 1) fn(t, s);
  }
};

constexpr uint64_t kFoldPiece = 1ull << 19;  // records per fold source (pass 1's unit of work)

// A stretch of a hint body (Hint::write_bytes records, data.rs:242-256: seq u64, ksz u16, vsz u32,
// pos u64, key) holding `cnt` whole records, all of one file: what the replay folds, in order.
struct FoldSrc {
  const uint8_t* b;
  uint64_t n, cnt;
  uint32_t file_id;
};

// One record on its way to its keydir table: everything Index::update reads, key bytes included
// when short, so the table's fold streams its list and touches only its own slots.
struct FoldItem {
  uint64_t hash, seq, pos;
  uint32_t file_id, vsz_raw, ksz, pad;
  union {
    uint8_t kin[KeyDir::kInline];
    const uint8_t* kp;  // ksz > kInline: the key in its hint body
  };
  const uint8_t* key() const { return ksz <= KeyDir::kInline ? kin : kp; }
};

// Pass 1's lists, kept across the batches of one open() so that later batches reuse their pages.
struct FoldScratch {
  std::vector<std::vector<FoldItem>> lists;
  std::vector<uint8_t> hll;
};

using cask_host::host_threads;
using cask_host::parallel_for;

// Threads for n independent pieces of work: the host's, at most one per piece, at least one.
inline unsigned host_lanes(uint64_t n) {
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(host_threads(), n));
}

// CASK_PAR_FOLD_MIN (tuning/test knob): the smallest replay folded, looked up or merged on threads
inline uint64_t par_fold_min() {
  const char* mv = cask_knobs::hook("CASK_PAR_FOLD_MIN");
  return mv ? strtoull(mv, nullptr, 10) : (1ull << 16);
}

// Index::update over the hint records of `src`, in order, on threads by keydir table (keydir_host.cpp)
void parallel_fold(const std::vector<FoldSrc>& src, Index& out, FoldScratch* keep = nullptr);

// Per file: (live entries, their bytes) over the whole keydir (keydir_host.cpp)
std::unordered_map<uint32_t, std::pair<uint64_t, uint64_t>> live_by_file(const Index& ix);

}  // namespace cask_engine

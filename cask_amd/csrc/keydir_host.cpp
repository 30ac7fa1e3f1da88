// The keydir's work on host threads: the fold of hint records into the tables (the open replay,
// cask.rs:346-382; compact_files' re-index, cask.rs:528-536) and the per-file live counts.
#include "keydir_host.h"

#include <atomic>
#include <cmath>

#include "knobs.h"

CASK_ENGINE_NAMESPACE {

// Per file: (live entries, their bytes) over the whole keydir, counted on threads by table (a dense
// array per thread for the usual small file ids; the Stats that a sharded replay completes from it,
// cask_keydir_finish, and an owner's terms).
std::unordered_map<uint32_t, std::pair<uint64_t, uint64_t>> live_by_file(const Index& ix) {
  using Acc = std::pair<uint64_t, uint64_t>;
  constexpr uint32_t kDense = 1u << 16;
  const unsigned nt = host_lanes(Index::kSub);
  std::vector<std::vector<Acc>> dense(nt);
  std::vector<std::unordered_map<uint32_t, Acc>> sparse(nt);
  parallel_for(nt, [&](unsigned t) {
    std::vector<Acc>& d = dense[t];
    for (unsigned q = t; q < Index::kSub; q += nt)
      for (const KeyDir::Slot& sl : ix.sub[q].slots) {
        if (sl.state != 1) continue;
        const uint32_t f = sl.e.file_id;
        Acc* a;
        if (f < kDense) {
          if (f >= d.size()) d.resize(std::min<size_t>(kDense, std::max<size_t>(f + 1, 2 * d.size())));
          a = &d[f];
        } else {
          a = &sparse[t][f];
        }
        a->first += 1;
        a->second += sl.e.entry_size;
      }
  });
  std::unordered_map<uint32_t, Acc> out;
  for (unsigned t = 0; t < nt; ++t) {
    for (uint32_t f = 0; f < dense[t].size(); ++f)
      if (dense[t][f].first) {
        Acc& a = out[f];
        a.first += dense[t][f].first;
        a.second += dense[t][f].second;
      }
    for (const auto& kv : sparse[t]) {
      Acc& a = out[kv.first];
      a.first += kv.second.first;
      a.second += kv.second.second;
    }
  }
  return out;
}

// Index::update over the hint records of `src` in order (the open replay, cask.rs:346-382;
// compact_files' re-index, cask.rs:528-536), on threads by key-hash table. Index::update's outcome
// for a key depends only on that key's records in order, and each table sees its keys' records in
// replay order. Pass 1 (threads by source) hashes every key and appends the record to its
// (source, table) list; pass 2 (threads by table) folds each table's lists in source order. Stats
// rows are per-file counters (order-free sums): each table keeps deltas, summed at the end; a remove
// counts when its file has a row in the delta or in the map entering the fold. The two differ from
// one serial fold only if a key's entry pointed at a file with no stats row, which cannot happen:
// every entry's file got its row when the entry was written, and compaction drops a file's row only
// after re-indexing all of its live entries elsewhere. Small replays fold on the calling thread.
void parallel_fold(const std::vector<FoldSrc>& src, Index& out, FoldScratch* keep) {
  uint64_t n = 0;
  for (const FoldSrc& f : src) n += f.cnt;
  const uint64_t min_par = par_fold_min();
  const unsigned nt = std::min(host_threads(), Index::kSub);
  if (n < min_par || nt == 1) {
    StatsDelta sd(out.stats, nullptr);
    for (const FoldSrc& f : src)
      for (uint64_t p = 0, j = 0; j < f.cnt; ++j) {
        const uint8_t* h = f.b + p;
        const uint16_t k = rd16(h + 8);
        const uint64_t hs = hash_key(h + 22, k);
        out.sub[Index::sub_of(hs)].update(h + 22, k, f.file_id, rd64(h + 14), rd32(h + 10), rd64(h), hs, sd);
        p += 22ull + k;
      }
    return;
  }
  constexpr unsigned S = Index::kSub;
  const size_t ns = src.size();
  // 1. per (source, table) lists, sources claimed by threads
  FoldScratch local;
  FoldScratch& fs = keep ? *keep : local;
  if (fs.lists.size() < ns * S) fs.lists.resize(ns * S);
  std::vector<std::vector<FoldItem>>& lists = fs.lists;
  // and per (source, table) a 256-register HyperLogLog sketch of the keys (hash bits below the
  // table's), so that each table is sized once for the keys it will hold: a table sized from the
  // record count instead (configs[3]: 5 records per key) costs pass 2 a third more in page faults
  // and cache misses, one sized too small a rehash per doubling.
  constexpr unsigned kReg = 256;
  std::vector<uint8_t>& hll = fs.hll;
  hll.assign(ns * S * kReg, 0);
  std::atomic<size_t> next{0};
  parallel_for(nt, [&](unsigned) {
    for (size_t k; (k = next.fetch_add(1)) < ns;) {
      const FoldSrc& f = src[k];
      std::vector<FoldItem>* L = &lists[k * S];
      for (unsigned q = 0; q < S; ++q) {
        L[q].clear();
        L[q].reserve(f.cnt / S + f.cnt / (4 * S) + 16);
      }
      for (uint64_t p = 0, j = 0; j < f.cnt; ++j) {
        const uint8_t* h = f.b + p;
        FoldItem it;
        it.ksz = rd16(h + 8);
        it.hash = hash_key(h + 22, it.ksz);
        it.seq = rd64(h);
        it.pos = rd64(h + 14);
        it.file_id = f.file_id;
        it.vsz_raw = rd32(h + 10);
        it.pad = 0;
        if (it.ksz <= KeyDir::kInline) {  // (16 bytes at once unless that would pass the body's end)
          if (p + 22 + KeyDir::kInline <= f.n) memcpy(it.kin, h + 22, KeyDir::kInline);
          else memcpy(it.kin, h + 22, it.ksz);
        } else {
          it.kp = h + 22;
        }
        const unsigned q = Index::sub_of(it.hash);
        L[q].push_back(it);
        uint8_t& reg = hll[(k * S + q) * kReg + ((it.hash >> 50) & (kReg - 1))];
        const uint8_t rank = (uint8_t)(__builtin_clzll((it.hash << 14) | (1ull << 13)) + 1);
        reg = rank > reg ? rank : reg;
        p += 22ull + it.ksz;
      }
    }
  });
  // 2. each table folds its lists in source order, stats into its own delta map
  std::vector<StatsMap> delta(S);
  parallel_for(nt, [&](unsigned t) {
    for (unsigned q = t; q < S; q += nt) {
      KeyDir& kd = out.sub[q];
      uint64_t cnt = 0;
      for (size_t k = 0; k < ns; ++k) cnt += lists[k * S + q].size();
      {  // the sketches of the table's lists merged: an estimate of its distinct keys (+-7 %)
        uint8_t m[kReg] = {};
        for (size_t k = 0; k < ns; ++k) {
          const uint8_t* r = &hll[(k * S + q) * kReg];
          for (unsigned j = 0; j < kReg; ++j) m[j] = r[j] > m[j] ? r[j] : m[j];
        }
        double z = 0;
        unsigned zeros = 0;
        for (unsigned j = 0; j < kReg; ++j) {
          z += std::ldexp(1.0, -(int)m[j]);
          zeros += m[j] == 0;
        }
        double est = 0.7213 / (1 + 1.079 / kReg) * kReg * kReg / z;
        if (est < 2.5 * kReg && zeros) est = kReg * std::log((double)kReg / zeros);
        const uint64_t want = std::min<uint64_t>(cnt, (uint64_t)(est * 1.15) + 64);
        // A fresh table is sized for its keys at once. A table holding keys grows when it fills
        // (update()): how many of the batch's keys it holds already is not known here, and sizing
        // for all of them as new rebuilt every table of compact_files' re-index, whose keys are all
        // in the keydir (0.36 -> 0.63-0.74 s on configs[3], profiles/r06k_compaction_ab.txt).
        if (!kd.live) kd.reserve(want);
      }
      StatsDelta sd(delta[q], &out.stats);
      for (size_t k = 0; k < ns; ++k) {
        const std::vector<FoldItem>& L = lists[k * S + q];
        const size_t m = L.size();
        for (size_t j = 0; j < m; ++j) {  // the slot of the record 8 ahead, a long key 4 ahead
          if (j + 16 < m) kd.prefetch(L[j + 16].hash);
          if (j + 4 < m) kd.prefetch_key(L[j + 4].hash);
          const FoldItem& r = L[j];
          kd.update(r.key(), r.ksz, r.file_id, r.pos, r.vsz_raw, r.seq, r.hash, sd);
        }
        if (!keep) std::vector<FoldItem>().swap(lists[k * S + q]);
      }
    }
  });
  // 3. stats deltas
  for (const StatsMap& d : delta)
    for (const auto& kv : d) {
      StatsEntry& e = out.stats[kv.first];
      e.entries += kv.second.entries;
      e.dead_entries += kv.second.dead_entries;
      e.dead_bytes += kv.second.dead_bytes;
    }
}

}  // namespace cask_engine

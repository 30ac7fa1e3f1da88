// ------------------------------------------------------------------------------------------
// Sharded replay: rank 0 folds the shards' keydir blocks (keydir_format.h) in
// rank order — the replay order, since shards are contiguous file-id ranges. The fold is
// Index::update + Stats (cask.rs:28-95; stats.rs:6-67) restated over the blocks' records.
// ------------------------------------------------------------------------------------------
#include <chrono>
#include <cstdio>
#include <map>

#include "engine_db.h"
#include "keydir_format.h"

using namespace cask_engine;

namespace {
using namespace cask_kd;

struct Blk {
  ShardHeader hd;
  const ShardRec* rec;
  const uint8_t* keys;
  const ShardFileStat* fs;
  uint64_t n, r0;  // records, the first record's index over all blocks
};

// One record on its way to its keydir table, with its key hash (and its key when short)
struct Item {
  uint64_t hash, seq, pos;
  uint32_t file_id, vsz;
  uint16_t ksz;
  uint8_t kind, pad0;
  uint32_t pad1;
  union {
    uint8_t kin[KeyDir::kInline];
    const uint8_t* kp;  // ksz > kInline: the key in its block
  };
  const uint8_t* key() const { return ksz <= KeyDir::kInline ? kin : kp; }
};

// The blocks of one merge cut into pieces for the threads: np pieces per block, P = b * np + g
struct MergePieces {
  std::vector<Blk> B;
  uint64_t n = 0;  // records over all blocks
  unsigned nt = 1, np = 1;
  size_t NP = 0;
  std::vector<uint64_t> pko;  // every piece's first key offset in its block
  void range(size_t P, uint64_t* lo, uint64_t* hi) const {
    const Blk& k = B[P / np];
    const uint64_t g = P % np;
    *lo = k.n * g / np;
    *hi = k.n * (g + 1) / np;
  }
};

// What pass 1 leaves for pass 2: the items in (table, block, piece, record) order
struct MergeItems {
  const Item* items = nullptr;
  std::vector<uint64_t> at;    // (table q, piece P) starts at at[q * NP + P]
  std::vector<char> has_cond;  // the blocks with conditional tombstones
};

// Every block checked before anything changes, and cut into pieces (every piece's first key offset
// in its block: the keys lie in record order).
int merge_pieces(const uint8_t* const* blks, const uint64_t* bytes, uint32_t nb, MergePieces& M) {
  std::vector<Blk>& B = M.B;
  B.resize(nb);
  uint64_t n = 0;
  for (uint32_t b = 0; b < nb; ++b) {
    const uint8_t* blk = blks[b];
    if ((bytes[b] && !blk) || bytes[b] < sizeof(ShardHeader)) return CASK_E_INVALID_ARG;
    ShardHeader& hd = B[b].hd;
    memcpy(&hd, blk, sizeof(hd));
    // counts bounded by the block's size before any offset is derived from them (no wrap-around)
    if (hd.nrec > (bytes[b] - sizeof(ShardHeader)) / sizeof(ShardRec) ||
        (uint64_t)hd.nfiles > (bytes[b] - sizeof(ShardHeader)) / sizeof(ShardFileStat))
      return CASK_E_INVALID_ARG;
    const uint64_t rec_at = sizeof(ShardHeader), fst_at = rec_at + sizeof(ShardRec) * hd.nrec,
                   key_at = fst_at + sizeof(ShardFileStat) * (uint64_t)hd.nfiles;
    if (hd.magic != kMagic || hd.version != kVersion || hd.bytes > bytes[b] || key_at + hd.key_bytes > hd.bytes)
      return CASK_E_INVALID_ARG;
    B[b].rec = (const ShardRec*)(blk + rec_at);
    B[b].keys = blk + key_at;
    B[b].fs = (const ShardFileStat*)(blk + fst_at);
    B[b].n = hd.nrec;
    B[b].r0 = n;
    n += hd.nrec;
  }
  M.n = n;
  M.nt = n < par_fold_min() ? 1u : std::min(host_threads(), Index::kSub);
  M.np = M.nt == 1 ? 1u : 4 * M.nt;
  M.NP = (size_t)nb * M.np;
  const unsigned nt = M.nt, np = M.np;
  const size_t NP = M.NP;
  std::vector<uint64_t>& pko = M.pko;
  pko.assign(NP + 1, 0);
  parallel_for(nt, [&](unsigned t) {
    for (size_t P = t; P < NP; P += nt) {
      uint64_t lo, hi, o = 0;
      M.range(P, &lo, &hi);
      const ShardRec* rec = B[P / np].rec;
      for (uint64_t i = lo; i < hi; ++i) o += rec[i].ksz;
      pko[P + 1] = o;
    }
  });
  for (uint32_t b = 0; b < nb; ++b) {  // (exclusive prefix within each block)
    uint64_t o = 0;
    for (unsigned g = 0; g < np; ++g) {
      const uint64_t k = pko[(size_t)b * np + g + 1];
      pko[(size_t)b * np + g + 1] = 0;
      pko[(size_t)b * np + g] = o;
      o += k;
    }
    if (o > B[b].hd.key_bytes) return CASK_E_INVALID_ARG;
  }
  return CASK_OK;
}

// (scratch in db: the next call reuses its pages; cask_keydir_finish gives it back)
uint8_t* merge_scratch(cask_db* db, HostBuf& hb, uint64_t nbytes) {
  if (hb.n >= nbytes) return hb.get();
  db->discard({&hb});
  if (!hb.alloc(nbytes + nbytes / 2)) throw std::bad_alloc();  // (headroom for a larger next call:
  return hb.get();                                              // untouched pages cost nothing)
}

// Pass 1, threads by piece of a block: each record with its key hash (and its key when short)
// written to its place in one array of items in (table, block, piece, record) order, so that
// pass 2 streams each table's items instead of reaching back into the blocks for every record.
// (a) every record's key hash, and per (piece, table) how many; (b) the items scattered to their
// places — written once, no list growing (a list per piece and table of freshly allocated small
// vectors cost the pass its page faults: 0.39 s per 20 M records on 8 threads, tools/merge_bench.py)
MergeItems merge_scatter(cask_db* db, const MergePieces& M, double* ms_hash) {
  constexpr unsigned S = Index::kSub;
  const std::vector<Blk>& B = M.B;
  const unsigned nt = M.nt, np = M.np;
  const size_t NP = M.NP;
  const auto tmA = std::chrono::steady_clock::now();
  uint64_t* hs = (uint64_t*)merge_scratch(db, db->mhash, std::max<uint64_t>(M.n, 1) * sizeof(uint64_t));
  std::vector<uint64_t> cnt(NP * S, 0);
  std::vector<uint64_t> nconds(NP, 0);
  parallel_for(nt, [&](unsigned t) {
    for (size_t P = t; P < NP; P += nt) {
      uint64_t lo, hi;
      M.range(P, &lo, &hi);
      const Blk& k = B[P / np];
      uint64_t* c = &cnt[P * S];
      uint64_t ko = M.pko[P];
      uint64_t lc[S] = {}, nc = 0;  // (locals: no stores to lines other threads write)
      for (uint64_t i = lo; i < hi; ++i) {
        const uint64_t h = hash_key(k.keys + ko, k.rec[i].ksz);
        hs[k.r0 + i] = h;
        ++lc[Index::sub_of(h)];
        nc += k.rec[i].kind == kCond;
        ko += k.rec[i].ksz;
      }
      for (unsigned q = 0; q < S; ++q) c[q] = lc[q];
      nconds[P] = nc;
    }
  });
  MergeItems out;
  std::vector<uint64_t>& at = out.at;
  at.assign(NP * S + 1, 0);
  for (size_t q = 0, k = 0; q < S; ++q)
    for (size_t P = 0; P < NP; ++P, ++k) at[k + 1] = at[k] + cnt[P * S + q];
  *ms_hash = ms_since(tmA);
  Item* items = (Item*)merge_scratch(db, db->mitems, std::max<uint64_t>(M.n, 1) * sizeof(Item));
  parallel_for(nt, [&](unsigned t) {
    for (size_t P = t; P < NP; P += nt) {
      uint64_t lo, hi;
      M.range(P, &lo, &hi);
      const Blk& k = B[P / np];
      uint64_t w[S];
      for (unsigned q = 0; q < S; ++q) w[q] = at[q * NP + P];
      uint64_t ko = M.pko[P];
      for (uint64_t i = lo; i < hi; ++i) {
        const ShardRec& r = k.rec[i];
        const uint64_t h = hs[k.r0 + i];
        Item& it = items[w[Index::sub_of(h)]++];
        it.hash = h;
        it.seq = r.seq;
        it.pos = r.pos;
        it.file_id = r.file_id;
        it.vsz = r.vsz;
        it.ksz = r.ksz;
        it.kind = r.kind;
        it.pad0 = 0;
        it.pad1 = 0;
        if (r.ksz <= KeyDir::kInline) memcpy(it.kin, k.keys + ko, r.ksz);
        else it.kp = k.keys + ko;
        ko += r.ksz;
      }
    }
  });
  out.items = items;
  out.has_cond.assign(B.size(), 0);
  for (size_t P = 0; P < NP; ++P)
    if (nconds[P]) out.has_cond[P / np] = 1;
  return out;
}

// Pass 2, threads by keydir table (parallel_fold's split): each table takes its records in block
// order — first the thresholds of the block's conditional tombstones against the keydir entering
// the block, then the updates. Stale terms are per-file sums, added to db->terms at the end.
void merge_fold_tables(cask_db* db, const MergePieces& M, const MergeItems& L) {
  constexpr unsigned S = Index::kSub;
  const unsigned nt = M.nt, np = M.np;
  const size_t NP = M.NP;
  const uint32_t nb = (uint32_t)M.B.size();
  const std::vector<uint64_t>& at = L.at;
  std::vector<std::unordered_map<uint32_t, cask_db::ShardTerms>> sterms(nt);
  parallel_for(nt, [&](unsigned t) {
    auto stale = [&](uint32_t fid, uint32_t ksz) {  // Stats add + remove of a stale tombstone
      cask_db::ShardTerms& x = sterms[t][fid];
      x.stale += 1;
      x.stale_bytes += 18ull + ksz;
    };
    for (unsigned q = t; q < S; q += nt) {
      KeyDir& kd = db->index.sub[q];
      // (a fresh table: room for every record's key — a block holds about one record per key; a
      // table holding keys grows when it fills, as in parallel_fold)
      if (!kd.live) kd.reserve(at[(q + 1) * NP] - at[q * NP]);
      for (uint32_t b = 0; b < nb; ++b) {
        const Item* Lq = L.items + at[q * NP + (size_t)b * np];
        const size_t m = at[q * NP + (size_t)(b + 1) * np] - at[q * NP + (size_t)b * np];  // block b's, in order
        // phase 0 (the thresholds) only for a block with conditional tombstones, against a table
        // that holds something (an empty one stales none of them)
        for (int phase = L.has_cond[b] && kd.live ? 0 : 1; phase < 2; ++phase) {
          for (size_t jj = 0; jj < m; ++jj) {
            if (jj + 16 < m) kd.prefetch(Lq[jj + 16].hash);
            if (jj + 4 < m) kd.prefetch_key(Lq[jj + 4].hash);
            const Item& r = Lq[jj];
            auto entry = [&]() -> const cask_index_entry* {
              const int64_t f = kd.find(r.key(), r.ksz, r.hash);
              return f >= 0 ? &kd.slots[(uint64_t)f].e : nullptr;
            };
            if (phase == 0) {  // 1. thresholds, against the keydir entering the block
              if (r.kind == kCond) {
                const cask_index_entry* e = entry();
                if ((e ? e->sequence + 1 : 0ull) > r.seq) stale(r.file_id, r.ksz);
              }
              continue;
            }
            // 2. the keydir: kept rows, and collided keys record by record, in the block's order
            if (r.kind == kCond) continue;
            if (r.kind == kRaw && r.vsz == CASK_ENTRY_TOMBSTONE) {
              const cask_index_entry* e = entry();
              if (e && e->sequence > r.seq) stale(r.file_id, r.ksz);
            }
            kd.update_kd(r.key(), r.ksz, r.file_id, r.pos, r.vsz, r.seq, r.hash);
          }
        }
      }
    }
  });
  for (const auto& m : sterms)
    for (const auto& kv : m) {
      cask_db::ShardTerms& x = db->terms[kv.first];
      x.stale += kv.second.stale;
      x.stale_bytes += kv.second.stale_bytes;
    }
}

// Blocks [0, nb) merged in order, in one pass: each keydir table takes its records block after
// block (for each, the thresholds of its conditional tombstones against the table as the block
// finds it, then the updates), which is what merging the blocks one by one does — a key's outcome
// depends on that key's records alone, in order — with one hashing and scatter pass over all the
// blocks and a fresh table sized once for all of them (one by one, every later block grew the
// tables: 8 blocks of 2 M records merged in 0.78-1.44 s against 0.46-0.83 s for one block of 16 M,
// tools/merge_bench.py's blocks on this container's 8 threads).
int keydir_merge_impl(cask_db* db, const uint8_t* const* blks, const uint64_t* bytes, uint32_t nb) {
  if (!db || !db->merging) return CASK_E_INVALID_ARG;
  const bool tracing = cask_knobs::hook("CASK_OPEN_TRACE") != nullptr;
  const auto tm0 = std::chrono::steady_clock::now();
  MergePieces M;
  const int st = merge_pieces(blks, bytes, nb, M);
  if (st != CASK_OK) return st;
  const double ms_pko = ms_since(tm0);
  double ms_hash = 0;
  const MergeItems L = merge_scatter(db, M, &ms_hash);
  if (tracing)
    fprintf(stderr, "keydir merge: %u blocks, %llu records, lists %.1f ms (pko %.1f, hash %.1f)\n", nb,
            (unsigned long long)M.n, ms_since(tm0), ms_pko, ms_hash);
  const auto tm1 = std::chrono::steady_clock::now();
  merge_fold_tables(db, M, L);
  if (tracing) fprintf(stderr, "keydir merge: tables %.1f ms\n", ms_since(tm1));
  for (const Blk& k : M.B) {  // the blocks' own per-file terms, their files and the highest sequence
    const ShardHeader& hd = k.hd;
    for (uint32_t f = 0; f < hd.nfiles; ++f) {
      const ShardFileStat& fs = k.fs[f];
      cask_db::ShardTerms& t = db->terms[fs.file_id];
      t.puts += fs.puts;
      t.put_bytes += fs.put_bytes;
      t.stale += fs.stale;
      t.stale_bytes += fs.stale_bytes;
      db->files.push_back(fs.file_id);
    }
    if (hd.max_seq_p1 && hd.max_seq_p1 - 1 > db->sequence) db->sequence = hd.max_seq_p1 - 1;
    ++db->shards;
  }
  return CASK_OK;
}

}  // namespace

extern "C" {

cask_db* cask_keydir_new(void) {
  cask_db* db = new (std::nothrow) cask_db();
  if (db) db->merging = true;
  return db;
}

int cask_keydir_merge(cask_db* db, const uint8_t* blk, uint64_t bytes) {
  try {  // the block comes from a peer rank: no exception crosses the C ABI
    return keydir_merge_impl(db, &blk, &bytes, 1);
  } catch (const std::bad_alloc&) {
    return CASK_E_NOMEM;
  } catch (...) {
    return CASK_E_INVALID_ARG;
  }
}

int cask_keydir_merge_many(cask_db* db, const uint8_t* const* blocks, const uint64_t* bytes, uint32_t n) {
  try {
    if (n && (!blocks || !bytes)) return CASK_E_INVALID_ARG;
    return keydir_merge_impl(db, blocks, bytes, n);
  } catch (const std::bad_alloc&) {
    return CASK_E_NOMEM;
  } catch (...) {
    return CASK_E_INVALID_ARG;
  }
}

// Stats after the last shard: per file, entries = puts + stale tombstones, dead = puts that are not
// the key's final entry + stale tombstones (stats.rs:23-48 summed over Index::update's cases).
int cask_keydir_finish(cask_db* db) {
  return cask_abi::guard([&]() -> int {
    if (!db || !db->merging) return CASK_E_INVALID_ARG;
    const auto live = live_by_file(db->index);  // file -> (entries, bytes)
    db->index.stats.clear();
    for (const auto& kv : db->terms) {
      const cask_db::ShardTerms& t = kv.second;
      if (!t.puts && !t.stale) continue;  // no Stats::add_entry for this file
      const auto it = live.find(kv.first);
      const uint64_t le = it == live.end() ? 0 : it->second.first, lb = it == live.end() ? 0 : it->second.second;
      StatsEntry& e = db->index.stats[kv.first];
      e.entries = t.puts + t.stale;
      e.dead_entries = t.puts - le + t.stale;
      e.dead_bytes = t.put_bytes - lb + t.stale_bytes;
    }
    std::sort(db->files.begin(), db->files.end());
    db->files.erase(std::unique(db->files.begin(), db->files.end()), db->files.end());
    db->file_seq = db->files.empty() ? 0u : db->files.back();
    db->merging = false;
    db->discard({&db->mhash, &db->mitems});
    return CASK_OK;
  });
}

// ------------------------------------------------------------------------------------------
// Key-hash partition of the sharded replay (keydir_format.h, SURVEY.md §8e's huge-keyspace case):
// every rank splits its block by key owner, owner o folds the parts it receives in rank order (the
// fold above: each key's records arrive in replay order, all in one part), and the owners' per-file
// terms summed are the Stats of one fold of every block.
// ------------------------------------------------------------------------------------------
uint32_t cask_keydir_owner(const uint8_t* key, uint64_t ksz, uint32_t nparts) {
  if (nparts < 1 || ksz > 0xFFFFu || (ksz && !key)) return 0;
  return cask_kd::key_owner(cask_kd::key_hash(key, (uint32_t)ksz), nparts);
}

static int partition_host_impl(const uint8_t* blk, uint64_t bytes, uint32_t nparts, uint8_t* out, uint64_t cap,
                               uint64_t* part_off) {
  using namespace cask_kd;
  if (!blk || !part_off || nparts < 1 || nparts > kMaxParts || bytes < sizeof(ShardHeader)) return CASK_E_INVALID_ARG;
  ShardHeader hd;
  memcpy(&hd, blk, sizeof(hd));
  if (hd.magic != kMagic || hd.version != kVersion || hd.bytes > bytes ||
      hd.nrec > (bytes - sizeof(ShardHeader)) / sizeof(ShardRec) ||
      (uint64_t)hd.nfiles > (bytes - sizeof(ShardHeader)) / sizeof(ShardFileStat))
    return CASK_E_INVALID_ARG;
  const uint64_t n = hd.nrec, fst_at = sizeof(ShardHeader) + sizeof(ShardRec) * n,
                 key_at = fst_at + sizeof(ShardFileStat) * (uint64_t)hd.nfiles;
  if (key_at + hd.key_bytes > hd.bytes) return CASK_E_INVALID_ARG;
  const ShardRec* rec = (const ShardRec*)(blk + sizeof(ShardHeader));
  const uint8_t* keys = blk + key_at;
  std::vector<uint64_t> ko(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) ko[i + 1] = ko[i] + rec[i].ksz;
  if (ko[n] != hd.key_bytes) return CASK_E_INVALID_ARG;
  std::vector<uint32_t> own(n);
  std::vector<uint64_t> cnt(nparts, 0), kb(nparts, 0);
  for (uint64_t i = 0; i < n; ++i) {
    own[i] = key_owner(key_hash(keys + ko[i], rec[i].ksz), nparts);
    ++cnt[own[i]];
    kb[own[i]] += rec[i].ksz;
  }
  part_off[0] = 0;
  for (uint32_t o = 0; o < nparts; ++o) part_off[o + 1] = part_off[o] + part_bytes(cnt[o], kb[o], hd.nfiles);
  if (!out || cap < part_off[nparts]) return CASK_E_CAPACITY;
  memset(out, 0, part_off[nparts]);
  std::vector<uint64_t> r(nparts, 0), k(nparts, 0);
  const ShardFileStat* fst = (const ShardFileStat*)(blk + fst_at);
  for (uint32_t o = 0; o < nparts; ++o) {
    uint8_t* base = out + part_off[o];
    ShardHeader h{};
    h.magic = kMagic;
    h.version = kVersion;
    h.nrec = cnt[o];
    h.key_bytes = kb[o];
    h.nfiles = hd.nfiles;
    h.max_seq_p1 = hd.max_seq_p1;
    h.rows_in = o == 0 ? hd.rows_in : 0;
    h.bytes = part_off[o + 1] - part_off[o];
    memcpy(base, &h, sizeof(h));
    ShardFileStat* fo = (ShardFileStat*)(base + sizeof(ShardHeader) + sizeof(ShardRec) * cnt[o]);
    for (uint32_t f = 0; f < hd.nfiles; ++f) {
      ShardFileStat st = fst[f];
      if (o) st.puts = st.put_bytes = st.stale = st.stale_bytes = 0;
      st.pad = 0;
      memcpy(fo + f, &st, sizeof(st));
    }
  }
  for (uint64_t i = 0; i < n; ++i) {  // records and keys in block order within each part
    const uint32_t o = own[i];
    uint8_t* base = out + part_off[o];
    memcpy(base + sizeof(ShardHeader) + sizeof(ShardRec) * r[o]++, rec + i, sizeof(ShardRec));
    const uint64_t ka = sizeof(ShardHeader) + sizeof(ShardRec) * cnt[o] + sizeof(ShardFileStat) * (uint64_t)hd.nfiles;
    memcpy(base + ka + k[o], keys + ko[i], rec[i].ksz);
    k[o] += rec[i].ksz;
  }
  return CASK_OK;
}

int cask_keydir_partition_host(const uint8_t* block, uint64_t bytes, uint32_t nparts, uint8_t* out, uint64_t cap,
                               uint64_t* part_off) {
  return abi_status([&] { return partition_host_impl(block, bytes, nparts, out, cap, part_off); });
}

// This owner's terms: per file the part-0 sums and stale tombstones folded here, and its live keys.
static int64_t keydir_terms_impl(const cask_db* db, uint8_t* out, uint64_t cap) {
  using namespace cask_kd;
  if (!db || !db->merging) return CASK_E_INVALID_ARG;
  std::map<uint32_t, KeydirTerm> t;
  for (const auto& kv : db->terms) {
    KeydirTerm& x = t[kv.first];
    x.file_id = kv.first;
    x.puts += kv.second.puts;
    x.put_bytes += kv.second.put_bytes;
    x.stale += kv.second.stale;
    x.stale_bytes += kv.second.stale_bytes;
  }
  for (uint32_t f : db->files) t[f].file_id = f;  // (files with no terms still travel)
  for (const auto& kv : live_by_file(db->index)) {
    KeydirTerm& x = t[kv.first];
    x.file_id = kv.first;
    x.live += kv.second.first;
    x.live_bytes += kv.second.second;
  }
  const uint64_t need = sizeof(KeydirTerm) * t.size();
  if (out && cap >= need) {
    uint64_t o = 0;
    for (const auto& kv : t) {
      memcpy(out + o, &kv.second, sizeof(KeydirTerm));
      o += sizeof(KeydirTerm);
    }
  }
  return (int64_t)need;
}

int64_t cask_keydir_terms(const cask_db* db, uint8_t* out, uint64_t cap) {
  return abi_status([&] { return keydir_terms_impl(db, out, cap); });
}

// Stats from every owner's terms (this one's included), as cask_keydir_finish computes them from one
// whole fold: entries = puts + stale, dead = puts - live + stale, dead_bytes likewise.
static int keydir_finish_terms_impl(cask_db* db, const uint8_t* terms, uint64_t bytes) {
  using namespace cask_kd;
  if (!db || !db->merging || (bytes && !terms) || bytes % sizeof(KeydirTerm)) return CASK_E_INVALID_ARG;
  std::map<uint32_t, KeydirTerm> sum;
  for (uint64_t o = 0; o < bytes; o += sizeof(KeydirTerm)) {
    KeydirTerm t;
    memcpy(&t, terms + o, sizeof(t));
    KeydirTerm& x = sum[t.file_id];
    x.file_id = t.file_id;
    x.puts += t.puts;
    x.put_bytes += t.put_bytes;
    x.stale += t.stale;
    x.stale_bytes += t.stale_bytes;
    x.live += t.live;
    x.live_bytes += t.live_bytes;
  }
  for (const auto& kv : sum)
    if (kv.second.live > kv.second.puts || kv.second.live_bytes > kv.second.put_bytes) return CASK_E_INVALID_ARG;
  db->index.stats.clear();
  for (const auto& kv : sum) {
    const KeydirTerm& t = kv.second;
    db->files.push_back(kv.first);
    if (!t.puts && !t.stale) continue;  // no Stats::add_entry for this file
    StatsEntry& e = db->index.stats[kv.first];
    e.entries = t.puts + t.stale;
    e.dead_entries = t.puts - t.live + t.stale;
    e.dead_bytes = t.put_bytes - t.live_bytes + t.stale_bytes;
  }
  std::sort(db->files.begin(), db->files.end());
  db->files.erase(std::unique(db->files.begin(), db->files.end()), db->files.end());
  db->file_seq = db->files.empty() ? 0u : db->files.back();
  db->merging = false;
  return CASK_OK;
}

int cask_keydir_finish_terms(cask_db* db, const uint8_t* terms, uint64_t bytes) {
  return abi_status([&] { return keydir_finish_terms_impl(db, terms, bytes); });
}

}  // extern "C"

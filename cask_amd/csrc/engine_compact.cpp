// The compaction merge (cask.rs:451-640): Cask::compact_files_aux + compact_files (cask.rs:451-560)
// and Cask::compact's choice of files (cask.rs:563-642). The hint pass and the liveness test run on
// the host against the keydir; the live records' checksums are verified by the device scan of their
// files (Log::read_entry -> Entry::from_read, log.rs:150-166) and their bytes are copied into the
// new data files by the device gather. LogWriter rollover (log.rs:282-306) and the
// EntryWriter/HintWriter output (log.rs:317-395) are restated on the host.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "engine_db.h"
#include "engine_dev.h"
#include "knobs.h"
#include "xxh32.h"

using namespace cask_engine;

namespace {

// (test hook CASK_COMPACT_TRACE: the sub-phases to stderr)
struct Trace {
  const bool on = cask_knobs::hook("CASK_COMPACT_TRACE") != nullptr;
  std::chrono::steady_clock::time_point tp = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    if (!on) return;
    fprintf(stderr, "compact hint pass: %s %.1f ms\n", what, ms_since(tp));
    tp = std::chrono::steady_clock::now();
  }
};

// ---- 1. the hint pass --------------------------------------------------------------------------

struct Ins {
  uint32_t src;  // index into `srcs`
  uint64_t pos;
};

// What the hint pass hands to the rest of the compaction.
struct HintPassResult {
  std::vector<uint32_t> compacted, srcs;  // srcs: compacted files with live records
  std::vector<Ins> ins;                   // the live records, in hint order
  std::vector<uint8_t> del_key_bytes;     // the tombstone tail, in first-seen order
  std::vector<uint64_t> del_key_off, del_seq;
  std::thread reaper;  // frees the hint pass's buffers beside the batches
  ~HintPassResult() {
    if (reaper.joinable()) reaper.join();
  }
};

struct HintFile {
  HostBuf hb;
  uint64_t hn = 0;  // the file's length
  bool ok = false;
  uint64_t bad = UINT64_MAX, base = 0, nlive = 0, ntomb = 0, ins0 = 0, tomb0 = 0;
  std::vector<uint64_t> offs;
  std::vector<uint8_t> kind;  // 1: live (cask.rs:500-502); 2: tombstone of an absent key (:487-499)
};

struct Tomb {
  const uint8_t* key;
  uint64_t seq;
  uint64_t hash;
  uint32_t ksz;
  uint32_t first;  // 1: the key's first tombstone (its place in the tail)
};

// Hints::next (log.rs:437-447) per file on threads: each valid hint file read, its record offsets.
void read_hint_files(const std::string& path, const std::vector<uint32_t>& files, std::vector<HintFile>& hf) {
  const size_t nh = files.size();
  const unsigned ntf = host_lanes(nh);
  parallel_for(ntf, [&](unsigned t) {
    for (size_t i = t; i < nh; i += ntf) {
      HintFile& H = hf[i];
      if (!load_valid_hint(hint_path(path, files[i]), H.hb, H.hn)) continue;
      H.ok = true;
      H.bad = walk_hint_body(H.hb.get(), H.hn - 4, [&](uint64_t p, uint16_t) { H.offs.push_back(p); });
    }
  });
}

// The keydir lookups (read-only) over all nrec records of the files hf[used[]], split evenly over
// nt threads: each record's kind.
void lookup_records(const Index& index, std::vector<HintFile>& hf, const std::vector<size_t>& used, uint64_t nrec,
                    unsigned nt) {
  parallel_for(nt, [&](unsigned t) {
    const uint64_t lo = nrec * t / nt, hi = nrec * (t + 1) / nt;
    size_t u = 0;
    while (u + 1 < used.size() && hf[used[u + 1]].base <= lo) ++u;
    for (uint64_t g = lo; g < hi;) {
      HintFile& H = hf[used[u]];
      const uint64_t e = std::min<uint64_t>(hi, H.base + H.offs.size());
      // lookups in flight: slots prefetched D records ahead, keys D/2 (test hook
      // CASK_COMPACT_LOOKAHEAD: a power of two up to 64)
      static const uint64_t D = [] {
        const char* v = cask_knobs::hook("CASK_COMPACT_LOOKAHEAD");
        const uint64_t d = v ? strtoull(v, nullptr, 10) : 16;
        return d >= 2 && d <= 64 && !(d & (d - 1)) ? d : 16ull;
      }();
      uint64_t hr[64];
      auto hash_at = [&](uint64_t i) {
        const uint8_t* h = H.hb.get() + H.offs[i];
        return hash_key(h + 22, rd16(h + 8));
      };
      const uint64_t i0 = g - H.base, i1 = e - H.base;
      for (uint64_t i = i0; i < std::min(i1, i0 + D); ++i) {
        hr[i & (D - 1)] = hash_at(i);
        index.prefetch(hr[i & (D - 1)]);
      }
      for (uint64_t i = i0; i < i1; ++i) {
        if (i + D / 2 < i1) index.prefetch_key(hr[(i + D / 2) & (D - 1)]);
        const uint8_t* h = H.hb.get() + H.offs[i];
        const cask_index_entry* ie = index.get_h(h + 22, rd16(h + 8), hr[i & (D - 1)]);
        H.kind[i] = rd32(h + 10) == CASK_ENTRY_TOMBSTONE ? (ie ? 0 : 2) : (ie && ie->sequence == rd64(h)) ? 1 : 0;
        if (i + D < i1) {
          hr[i & (D - 1)] = hash_at(i + D);
          index.prefetch(hr[i & (D - 1)]);
        }
      }
      g = e;
      ++u;
    }
  });
}

// the tail: each absent key once, at its first tombstone, with its highest sequence; keys
// deduplicated by hash-split tables on threads
void dedup_tombstones(std::vector<Tomb>& tombs, unsigned nt) {
  constexpr unsigned S = Index::kSub;
  const uint64_t ntomb = tombs.size();
  std::vector<std::vector<uint64_t>> tl(S);
  for (uint64_t i = 0; i < ntomb; ++i) tl[Index::sub_of(tombs[i].hash)].push_back(i);
  const unsigned ntt = ntomb < 4096 ? 1u : std::min(nt, S);
  parallel_for(ntt, [&](unsigned t) {
    for (unsigned q = t; q < S; q += ntt) {
      std::unordered_map<uint64_t, uint64_t> seen;  // hash -> the key's first tombstone
      std::vector<uint64_t> more;                     // first tombstones of keys whose hash was taken
      seen.reserve(tl[q].size());
      auto same = [&](const Tomb& A, const Tomb& B) {
        return A.hash == B.hash && A.ksz == B.ksz && (A.ksz == 0 || memcmp(A.key, B.key, A.ksz) == 0);
      };
      for (uint64_t i : tl[q]) {
        Tomb& T = tombs[i];
        auto ins_at = seen.emplace(T.hash, i);
        uint64_t f = UINT64_MAX;
        if (!ins_at.second) {
          if (same(tombs[ins_at.first->second], T)) f = ins_at.first->second;
          for (size_t m = 0; f == UINT64_MAX && m < more.size(); ++m)
            if (same(tombs[more[m]], T)) f = more[m];
          if (f == UINT64_MAX) more.push_back(i);
        }
        if (f == UINT64_MAX) {
          T.first = 1;
        } else if (tombs[f].seq < T.seq) {
          tombs[f].seq = T.seq;
        }
      }
    }
  });
}

// the tail's keys and sequences in first-seen order: counted per slice of `tombs` on threads,
// then each slice writes its part at its prefix
void emit_tail(const std::vector<Tomb>& tombs, unsigned nt, HintPassResult& out) {
  const uint64_t ntomb = tombs.size();
  const unsigned nts = ntomb < 65536 ? 1u : nt;
  std::vector<uint64_t> cnt(nts + 1, 0), kb(nts + 1, 0);
  parallel_for(nts, [&](unsigned t) {
    for (uint64_t i = ntomb * t / nts, e = ntomb * (t + 1) / nts; i < e; ++i)
      if (tombs[i].first) {
        ++cnt[t + 1];
        kb[t + 1] += tombs[i].ksz;
      }
  });
  for (unsigned t = 0; t < nts; ++t) {
    cnt[t + 1] += cnt[t];
    kb[t + 1] += kb[t];
  }
  out.del_key_off.resize(cnt[nts] + 1);
  out.del_seq.resize(cnt[nts]);
  out.del_key_bytes.resize(kb[nts]);
  parallel_for(nts, [&](unsigned t) {
    uint64_t j = cnt[t], o = kb[t];
    for (uint64_t i = ntomb * t / nts, e = ntomb * (t + 1) / nts; i < e; ++i) {
      const Tomb& T = tombs[i];
      if (!T.first) continue;
      out.del_key_off[j] = o;
      out.del_seq[j++] = T.seq;
      if (T.ksz) memcpy(out.del_key_bytes.data() + o, T.key, T.ksz);
      o += T.ksz;
    }
  });
  out.del_key_off[cnt[nts]] = kb[nts];
}

// 1. hints of each file with a valid hint file (files without one are skipped: cask.rs:456-468).
// Hints::next (log.rs:437-447) per file on threads: the record offsets (`hint?` aborts,
// cask.rs:483, the first bad file in order wins), then the keydir lookups (read-only), the live
// list and the tombstone tail in hint order.
int compact_hint_pass(cask_db* db, const std::vector<uint32_t>& files, cask_open_error* err, Trace& trace,
                      HintPassResult& out) {
  const size_t nh = files.size();
  std::vector<HintFile> hf(nh);
  read_hint_files(db->path, files, hf);
  trace("read+parse");
  uint64_t nrec = 0;
  std::vector<size_t> used;  // indices into hf of the compacted files, in order
  for (size_t i = 0; i < nh; ++i) {
    if (!hf[i].ok) continue;
    if (hf[i].bad != UINT64_MAX) {
      set_err(err, CASK_E_EOF, files[i], hf[i].bad);
      return CASK_E_EOF;
    }
    hf[i].base = nrec;
    nrec += hf[i].offs.size();
    hf[i].kind.resize(hf[i].offs.size());
    used.push_back(i);
  }
  const unsigned nt = nrec < par_fold_min() ? 1u : host_threads();  // the same knob as parallel_fold
  lookup_records(db->index, hf, used, nrec, nt);
  trace("lookups");
  const unsigned ntu = std::min(nt, host_lanes(used.size()));
  parallel_for(ntu, [&](unsigned t) {
    for (size_t j = t; j < used.size(); j += ntu) {
      HintFile& H = hf[used[j]];
      for (uint8_t k : H.kind) {
        H.nlive += k == 1;
        H.ntomb += k == 2;
      }
    }
  });
  uint64_t nins = 0, ntomb = 0;
  for (size_t u : used) {
    HintFile& H = hf[u];
    out.compacted.push_back(files[u]);
    H.ins0 = nins;
    H.tomb0 = ntomb;
    if (H.nlive) out.srcs.push_back(files[u]);
    nins += H.nlive;
    ntomb += H.ntomb;
  }
  // the live list (hint order) and the tombstones of absent keys (hint order), file by file
  out.ins.resize(nins);
  std::vector<Tomb> tombs(ntomb);
  parallel_for(ntu, [&](unsigned t) {
    for (size_t j = t; j < used.size(); j += ntu) {
      const HintFile& H = hf[used[j]];
      const uint32_t si =
          (uint32_t)(std::lower_bound(out.srcs.begin(), out.srcs.end(), files[used[j]]) - out.srcs.begin());
      uint64_t a = H.ins0, d = H.tomb0;
      for (uint64_t i = 0; i < H.kind.size(); ++i) {
        if (!H.kind[i]) continue;
        const uint8_t* h = H.hb.get() + H.offs[i];
        if (H.kind[i] == 1) {
          out.ins[a++] = Ins{si, rd64(h + 14)};
        } else {
          const uint16_t k = rd16(h + 8);
          tombs[d++] = Tomb{h + 22, rd64(h), hash_key(h + 22, k), k, 0};
        }
      }
    }
  });
  trace("lists");
  dedup_tombstones(tombs, nt);
  trace("tail-dedup");
  emit_tail(tombs, nt, out);
  trace("tail");
  // the hint files' buffers (GiB at configs[3] scale) are unmapped on a thread of their own while
  // the live records go through the device
  std::vector<HintFile>* dying = new std::vector<HintFile>(std::move(hf));
  try {
    out.reaper = std::thread([dying] { delete dying; });
  } catch (...) {  // (no thread: freed here)
    delete dying;
  }
  return CASK_OK;
}

// ---- the output side ---------------------------------------------------------------------------

struct OutFile {
  uint32_t fid;
  uint64_t len = 0;
  int fd = -1;
  std::vector<uint8_t> hints;
};

// One batch of live records on its way to the new data files.
struct WBatch {
  std::vector<HostBuf> regions;       // per source file of the batch: its live records' bytes, in order
  std::vector<const uint8_t*> at;     // per record: its bytes (in a region)
  std::vector<uint64_t> len, foff;    // per record: length, offset in its output file
  std::vector<OutFile*> op;           // per record: its output file
  // outs[done, complete) take no record after this batch: the writer finishes them. (The writer
  // never indexes `outs`: placement appends to it meanwhile, which may rewrite the deque's block
  // map; the elements themselves never move, so pointers resolved at placement stay valid.)
  std::vector<OutFile*> fin;
  size_t complete = 0;
};

// The files a compaction creates: placement by the LogWriter rollover (log.rs:282-306), and the
// live records' writes, one batch behind the device: a writer thread takes each batch's gathered
// bytes (in write order) while the caller reads, verifies and gathers the next batch on the device.
// Within a batch, the runs of records bound for one file (placement only moves forward: one run per
// file per batch) get their hints appended on a thread each, and their bytes written with pwrite
// in pieces of at most 64 MiB at their offsets in the file, all on threads.
// On an error, the files this call created are removed; an exception before the new files are
// complete (std::bad_alloc while gathering or placing) removes them too, on its way to
// cask_db_compact_files' handler: the destructor joins the writer thread first, then removes.
class CompactOutputs {
 public:
  explicit CompactOutputs(cask_db* db) : db_(db), path_(db->path) {}
  CompactOutputs(const CompactOutputs&) = delete;
  CompactOutputs& operator=(const CompactOutputs&) = delete;
  ~CompactOutputs() {
    stop_writer();
    if (armed_ && std::uncaught_exceptions()) remove();
  }

  // (a deque: the writer thread holds references into it while placement appends to it, and
  // push_back on a deque never moves the elements already there)
  std::deque<OutFile>& files() { return outs_; }
  const std::vector<uint32_t>& new_files() const { return new_files_; }
  const std::vector<uint32_t>& tomb_files() const { return tomb_files_; }
  uint64_t cur() const { return cur_; }  // the bytes placed in the last file
  double writer_ms() const { return ms_; }
  void disarm() { armed_ = false; }  // the new files are complete: they stay whatever happens next

  size_t place(uint64_t size, bool live) {  // LogWriter::write's rollover
    if (outs_.empty() || cur_ + size > db_->opts.max_file_size) {
      const uint32_t fid = ++db_->file_seq;  // Sequence::increment (util.rs:62-64)
      (live ? new_files_ : tomb_files_).push_back(fid);  // cask.rs:510-512, 518-520
      outs_.push_back(OutFile{fid});
      cur_ = 0;
    }
    cur_ += size;
    return outs_.size() - 1;
  }

  bool open_fd(OutFile& o) const {
    return o.fd >= 0 || (o.fd = open(data_path(path_, o.fid).c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644)) >= 0;
  }

  // placement (LogWriter::write's rollover, log.rs:282-306) of a batch's records, in write order
  void place_batch(WBatch& wb) {
    const uint64_t n = wb.len.size();
    wb.op.resize(n);
    wb.foff.resize(n);
    for (uint64_t k = 0; k < n; ++k) {
      wb.op[k] = &outs_[place(wb.len[k], true)];
      wb.foff[k] = cur_ - wb.len[k];  // (its offset in its file: placement just added it)
    }
    wb.complete = outs_.empty() ? 0 : outs_.size() - 1;  // (the last output file may take more)
    for (size_t i = fin_next_; i < wb.complete; ++i) wb.fin.push_back(&outs_[i]);
    fin_next_ = std::max(fin_next_, wb.complete);
  }

  // The batch to the writer once it has taken the previous one; the writer's status so far (a
  // failure: *fail_fid is its file, and the batch is not handed over).
  int hand_over(std::unique_ptr<WBatch> wb, uint32_t* fail_fid) {
    if (!th_.joinable()) th_ = std::thread([this] { writer_loop(); });
    wait_idle();
    if (status_ != CASK_OK) {
      *fail_fid = fail_fid_;
      return status_;
    }
    {
      std::lock_guard<std::mutex> g(m_);
      pending_ = std::move(wb);
    }
    cv_.notify_all();
    return CASK_OK;
  }

  // The last batch's writes waited for and the writer thread ended; its status.
  int drain(uint32_t* fail_fid) {
    wait_idle();
    stop_writer();
    *fail_fid = fail_fid_;
    return status_;
  }

  // the output files the writer thread has not finished (the last live one, the tombstone tail's)
  int finish_rest(uint32_t* fail_fid) {
    std::vector<OutFile*> rest;
    for (size_t i = hints_done_; i < outs_.size(); ++i) rest.push_back(&outs_[i]);
    return finish_outputs(rest, fail_fid);
  }

  // An error: the writer finishes (or skips) the batch it may hold and stops, then every file this
  // call created is removed, with any hint file already written.
  int abort(cask_open_error* err, int st, uint32_t fid = 0, uint64_t pos = 0, uint32_t e = 0, uint32_t f = 0) {
    stop_writer();
    remove();
    set_err(err, st, fid, pos, e, f);
    return st;
  }

 private:
  void remove() {
    for (OutFile& o : outs_) {
      if (o.fd >= 0) close(o.fd);
      o.fd = -1;
      (void)unlink(data_path(path_, o.fid).c_str());
      (void)unlink(hint_path(path_, o.fid).c_str());
    }
    db_->file_seq -= (uint32_t)outs_.size();
    outs_.clear();
  }
  void wait_idle() {
    std::unique_lock<std::mutex> lk(m_);
    cv_.wait(lk, [&] { return !busy_ && !pending_; });
  }
  void stop_writer() {
    if (!th_.joinable()) return;
    {
      std::lock_guard<std::mutex> g(m_);
      quit_ = true;
    }
    cv_.notify_all();
    th_.join();
  }

  // one record's bytes' place in its file, and its hint (Hint::new(entry, entry_pos), data.rs:218-226)
  static void append(OutFile& o, const uint8_t* rec, uint64_t n) {
    const uint16_t k = rd16(rec + 12);
    uint8_t h[22];
    wr_hint_header(h, rd64(rec + 4), k, rd32(rec + 14), o.len);
    o.hints.insert(o.hints.end(), h, h + 22);
    o.hints.insert(o.hints.end(), rec + 18, rec + 18 + k);
    o.len += n;
  }

  int write_batch(WBatch& B) {  // (on the writer thread)
    const uint64_t n = B.op.size();
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for (uint64_t k = 0; k < n;) {
      uint64_t e = k;
      while (e < n && B.op[e] == B.op[k]) ++e;
      runs.emplace_back(k, e);
      k = e;
    }
    for (const auto& r : runs) {  // (fds opened here, on one thread)
      OutFile& o = *B.op[r.first];
      if (!open_fd(o)) {
        fail_fid_ = o.fid;
        return CASK_E_IO;
      }
    }
    struct Piece {
      size_t run;
      const uint8_t* at;  // host bytes
      uint64_t n, foff;
    };
    std::vector<Piece> pieces;
    constexpr uint64_t kWPiece = 64ull << 20;
    for (size_t r = 0; r < runs.size(); ++r) {  // each run's records contiguous in memory (one source's region)
      for (uint64_t k = runs[r].first, e = runs[r].second; k < e;) {
        uint64_t j = k + 1;
        while (j < e && B.at[j] == B.at[j - 1] + B.len[j - 1]) ++j;
        const uint8_t* a = B.at[k];
        const uint64_t nb = (uint64_t)(B.at[j - 1] + B.len[j - 1] - a);
        for (uint64_t x = 0; x < nb; x += kWPiece) pieces.push_back(Piece{r, a + x, std::min(kWPiece, nb - x), B.foff[k] + x});
        k = j;
      }
    }
    std::vector<char> ok(runs.size(), 1);
    const size_t ntask = runs.size() + pieces.size();  // tasks [0, runs): hints; then the pieces
    const unsigned ntw = host_lanes(ntask);
    parallel_for(ntw, [&](unsigned t) {
      for (size_t x = t; x < ntask; x += ntw) {
        if (x < runs.size()) {
          for (uint64_t j = runs[x].first; j < runs[x].second; ++j) append(*B.op[j], B.at[j], B.len[j]);
        } else {
          const Piece& pc = pieces[x - runs.size()];
          if (!pwrite_all(B.op[runs[pc.run].first]->fd, pc.at, pc.n, pc.foff)) ok[pc.run] = 0;
        }
      }
    });
    for (size_t r = 0; r < runs.size(); ++r)
      if (!ok[r]) {
        fail_fid_ = B.op[runs[r].first]->fid;
        return CASK_E_IO;
      }
    return CASK_OK;
  }

  // Output files finished: hint file (HintWriter: body + XXH32 trailer) written and data file
  // closed, a file per thread (the first failure in file order is the error). The writer thread
  // finishes each output file once no later batch can add to it; the caller the rest at the end.
  int finish_outputs(const std::vector<OutFile*>& fo, uint32_t* fail) {
    if (fo.empty()) return CASK_OK;
    std::vector<char> okh(fo.size(), 1);
    const unsigned nth = host_lanes(fo.size());
    parallel_for(nth, [&](unsigned t) {
      for (size_t i = t; i < fo.size(); i += nth) {
        OutFile& o = *fo[i];
        if (!open_fd(o)) {
          okh[i] = 0;
          continue;
        }
        close(o.fd);
        o.fd = -1;
        okh[i] = write_hint_file(hint_path(path_, o.fid), o.hints.data(), o.hints.size());
      }
    });
    for (size_t i = 0; i < fo.size(); ++i)
      if (!okh[i]) {
        *fail = fo[i]->fid;
        return CASK_E_IO;
      }
    return CASK_OK;
  }

  void writer_loop() {
    for (;;) {
      std::unique_ptr<WBatch> B;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return quit_ || pending_; });
        if (!pending_) return;  // quit
        B = std::move(pending_);
        busy_ = true;
      }
      const auto tw0 = std::chrono::steady_clock::now();
      int st = status_ == CASK_OK ? abi_status([&] { return write_batch(*B); }) : status_;
      if (st == CASK_OK && B->complete > hints_done_) {  // (output files no later batch adds to)
        st = abi_status([&] { return finish_outputs(B->fin, &fail_fid_); });
        if (st == CASK_OK) hints_done_ = B->complete;
      }
      const double dt = ms_since(tw0);
      B.reset();  // (the batch's host bytes go before the next one is taken)
      {
        std::lock_guard<std::mutex> g(m_);
        if (status_ == CASK_OK) status_ = st;
        ms_ += dt;
        busy_ = false;
      }
      cv_.notify_all();
    }
  }

  cask_db* db_;
  const std::string path_;
  std::deque<OutFile> outs_;
  std::vector<uint32_t> new_files_, tomb_files_;
  uint64_t cur_ = 0;
  bool armed_ = true;
  size_t hints_done_ = 0;  // (the writer's; read by the caller only once it has stopped)
  size_t fin_next_ = 0;    // (the caller's: the output files already handed to the writer to finish)
  // the writer thread and what it shares with the caller
  std::thread th_;
  std::mutex m_;
  std::condition_variable cv_;
  std::unique_ptr<WBatch> pending_;
  bool busy_ = false, quit_ = false;
  uint32_t fail_fid_ = 0;
  int status_ = CASK_OK;
  double ms_ = 0;
};

// ---- 2-5. the live records ---------------------------------------------------------------------

struct LiveTimes {
  double verify = 0, gather = 0, write = 0, read = 0, h2d = 0;
};

// What pass 1 of a batch found, per source file of the batch.
struct BatchCopy {
  std::vector<uint64_t> used;  // bytes copied into each region
  std::vector<uint64_t> eof;   // per file: its first record cut short (batch index)
  std::vector<char> io_ok;
};

// Pass 1 of a batch on host threads, a source file each — the file mapped, each live record's
// header read at its hint position and its bytes copied, in write order, into the file's region of
// the batch (Log::read_entry's reads, log.rs:150-166; only the live records' lines are touched, not
// the dead 80 % of configs[3]); a record cut short by the file's end is its UnexpectedEof and ends
// that file's pass. The batch's files are srcs[0, nf), file f's records ins[fk[f], fk[f + 1]), and
// the batch's first record is ins[k0].
void copy_live_records(const std::string& path, const uint32_t* srcs, size_t nf, const std::vector<size_t>& fk,
                       const std::vector<Ins>& ins, size_t k0, WBatch& WB, BatchCopy& C) {
  C.used.assign(nf, 0);
  C.eof.assign(nf, UINT64_MAX);
  C.io_ok.assign(nf, 1);
  const unsigned ntf = host_lanes(nf);
  parallel_for(ntf, [&](unsigned t) {
    for (size_t f = t; f < nf; f += ntf) {
      if (fk[f] == fk[f + 1]) continue;
      const int fdsc = open(data_path(path, srcs[f]).c_str(), O_RDONLY);  // File::open: Io
      struct stat stt;
      if (fdsc < 0 || fstat(fdsc, &stt) != 0) {
        if (fdsc >= 0) close(fdsc);
        C.io_ok[f] = 0;
        continue;
      }
      const uint64_t flen = (uint64_t)stt.st_size;
      const uint8_t* m = nullptr;
      if (flen) {
        void* q = mmap(nullptr, flen, PROT_READ, MAP_PRIVATE, fdsc, 0);
        if (q == MAP_FAILED) {
          close(fdsc);
          C.io_ok[f] = 0;
          continue;
        }
        m = (const uint8_t*)q;
      }
      close(fdsc);
      HostBuf& rg = WB.regions[f];
      if (!rg.alloc(std::max<uint64_t>(flen, 1))) {
        if (m) munmap((void*)m, flen);
        throw std::bad_alloc();
      }
      uint64_t o = 0;
      for (size_t k = fk[f]; k < fk[f + 1]; ++k) {
        const uint64_t pos = ins[k].pos;
        if (pos > flen || flen - pos < 18) {  // header cut short (data.rs:163)
          C.eof[f] = k - k0;
          break;
        }
        const uint8_t* h = m + pos;
        const uint32_t vsz = rd32(h + 14);
        const uint64_t rl = 18ull + rd16(h + 12) + (vsz == CASK_ENTRY_TOMBSTONE ? 0ull : (uint64_t)vsz);
        if (flen - pos < rl) {  // key or value cut short (data.rs:172,181)
          C.eof[f] = k - k0;
          break;
        }
        memcpy(rg.get() + o, h, rl);
        WB.at[k - k0] = rg.get() + o;
        WB.len[k - k0] = rl;
        o += rl;
      }
      C.used[f] = o;
      if (m) munmap((void*)m, flen);
    }
  });
}

// 2-5. The live records, source file batch by batch (at most ~kBatch bytes of sources on the
// device at once): the sources read straight to the device, each live record read and verified
// where its hint says it is (Log::read_entry -> Entry::from_read, log.rs:150-166; the device
// hashes only the live bytes), placed by the LogWriter rollover (log.rs:282-306), its bytes
// gathered on the device in write order and appended to the new data files.
// Per batch: pass 1 (copy_live_records); then the regions' bytes go to the device through the
// pinned ring and the device verifies every copied record (cask_read_entries_device: the header's
// length again, XXH32 against the stored checksum, Entry::from_read, data.rs:161-206). The first
// failure in write order — an EOF from pass 1 or a checksum from the device — is the reference's
// error. The batch's bytes are already in write order on the host: placement, and the batch to the
// writer thread. On an error, the files this call created are removed and the reference's error
// returned.
int compact_live_records(cask_db* db, const HintPassResult& H, CompactOutputs& out, uint64_t* bytes_in,
                         cask_open_error* err, LiveTimes& T) {
  const std::vector<Ins>& ins = H.ins;
  const std::vector<uint32_t>& srcs = H.srcs;
  if (ins.empty()) return CASK_OK;
  const std::string& path = db->path;
  const size_t ns = srcs.size();
  std::vector<uint64_t> slen(ns, 0);
  for (size_t i = 0; i < ns; ++i) {
    struct stat stt;
    slen[i] = stat(data_path(path, srcs[i]).c_str(), &stt) == 0 ? (uint64_t)stt.st_size : 0;
  }
  EngineDev* ed = engine_dev(db->opts.device);
  if (!ed) return out.abort(err, CASK_E_DEVICE);
  std::lock_guard<std::mutex> g(ed->mu);
  int st = ed->prepare();
  if (st != CASK_OK) return out.abort(err, st);
  // (test hook CASK_COMPACT_BATCH: source bytes per batch, so small databases run several batches)
  const char* bh = cask_knobs::hook("CASK_COMPACT_BATCH");
  const uint64_t kBatch = bh && strtoull(bh, nullptr, 10) ? strtoull(bh, nullptr, 10) : (16ull << 30);
  size_t k0 = 0;
  for (size_t b0 = 0; b0 < ns;) {
    auto tv = std::chrono::steady_clock::now();
    size_t b1 = b0 + 1;
    uint64_t bytes = slen[b0];
    while (b1 < ns && bytes + slen[b1] <= kBatch) bytes += slen[b1++];
    *bytes_in += bytes;
    const size_t nf = b1 - b0;
    // the batch's records: ins[k0, k1), file f's from fk[f]
    std::vector<size_t> fk(nf + 1, k0);
    size_t k1 = k0;
    for (size_t f = 0; f < nf; ++f) {
      fk[f] = k1;
      while (k1 < ins.size() && ins[k1].src == b0 + f) ++k1;
    }
    fk[nf] = k1;
    const uint64_t n = k1 - k0;
    std::unique_ptr<WBatch> WB(new WBatch());
    WB->regions.resize(nf);
    WB->at.assign(n, nullptr);
    WB->len.assign(n, 0);
    BatchCopy C;
    auto ts = std::chrono::steady_clock::now();
    copy_live_records(path, srcs.data() + b0, nf, fk, ins, k0, *WB, C);
    T.read += ms_since(ts);
    // the first file that could not be opened ends the batch there (its records come first in
    // write order after the earlier files')
    size_t nv = n;  // records verified: those before the batch's first failure from pass 1
    for (size_t f = 0; f < nf; ++f) {
      if (!C.io_ok[f] && fk[f] != fk[f + 1]) {
        nv = std::min<size_t>(nv, fk[f] - k0);
        break;
      }
      if (C.eof[f] != UINT64_MAX) {
        nv = std::min<size_t>(nv, C.eof[f]);
        break;
      }
    }
    // the copied bytes to the device, contiguous; the device verifies records [0, nv)
    uint64_t total = 0;
    std::vector<uint64_t> doff(nf, 0);
    for (size_t f = 0; f < nf; ++f) {
      doff[f] = total;
      total += C.used[f];
    }
    std::vector<uint64_t> pos(nv), len(nv);
    std::vector<uint32_t> src(nv, 0u), ex(nv), fd(nv);
    std::vector<uint8_t> stv(nv);
    if (nv) {
      if (!ed->data.ensure(total + 256)) return out.abort(err, CASK_E_NOMEM);
      ts = std::chrono::steady_clock::now();
      std::vector<cask_host::PinnedRing::Piece> ps;
      for (size_t f = 0; f < nf; ++f)
        if (C.used[f]) cask_host::PinnedRing::split(WB->regions[f].get(), ed->data.p + doff[f], C.used[f], ps);
      if (!ed->ring.h2d(ps)) return out.abort(err, CASK_E_DEVICE);
      T.h2d += ms_since(ts);
      size_t f = 0;
      for (uint64_t k = 0; k < nv; ++k) {
        while (k0 + k >= fk[f + 1]) ++f;
        pos[k] = doff[f] + (uint64_t)(WB->at[k] - WB->regions[f].get());
      }
      const uint8_t* dsrc = ed->data.p;
      st = cask_read_entries_device(ed->ctx, &dsrc, &total, 1, src.data(), pos.data(), nv, len.data(), stv.data(),
                                    ex.data(), fd.data());
      if (st != CASK_OK) return out.abort(err, st);
    }
    for (uint64_t k = 0; k < nv; ++k)  // in write order: the first failure is the reference's
      if (stv[k] != CASK_ROW_OK || len[k] != WB->len[k])
        return stv[k] == CASK_ROW_CHECKSUM
                   ? out.abort(err, CASK_E_CHECKSUM, srcs[ins[k0 + k].src], ins[k0 + k].pos, ex[k], fd[k])
                   : out.abort(err, CASK_E_EOF, srcs[ins[k0 + k].src], ins[k0 + k].pos);
    if (nv < n) {  // pass 1's failure: File::open / read (Io) or a record cut short (UnexpectedEof)
      const uint32_t fid = srcs[ins[k0 + nv].src];
      const size_t f = ins[k0 + nv].src - b0;
      if (!C.io_ok[f]) return out.abort(err, CASK_E_IO, fid);
      return out.abort(err, CASK_E_EOF, fid, ins[k0 + nv].pos);
    }
    T.verify += ms_since(tv);
    auto tg = std::chrono::steady_clock::now();
    out.place_batch(*WB);
    T.gather += ms_since(tg);
    // hand the batch to the writer once it has taken the previous one
    auto tw = std::chrono::steady_clock::now();
    uint32_t wfid = 0;
    st = out.hand_over(std::move(WB), &wfid);
    if (st != CASK_OK) return out.abort(err, st, wfid);
    T.write += ms_since(tw);  // (the time this thread waited for the writer)
    k0 = k1;
    b0 = b1;
  }
  return CASK_OK;
}

// the tombstone tail: Entry::deleted(sequence, key).write_bytes (data.rs:90-121), in first-seen
// order. The placement (the rollover) runs in order; the records, their checksums and their hints
// are then laid out on threads, and each output file's run of them goes out in one pwrite.
// CASK_E_IO with *fail_fid on a failed write.
int write_tombstone_tail(const HintPassResult& H, CompactOutputs& out, uint32_t* fail_fid) {
  const std::vector<uint64_t>& del_key_off = H.del_key_off;
  const std::vector<uint64_t>& del_seq = H.del_seq;
  const size_t nt = del_seq.size();
  if (!nt) return CASK_OK;
  std::deque<OutFile>& outs = out.files();
  std::vector<uint32_t> to(nt);
  std::vector<uint64_t> at(nt), hat(nt);  // offset in its file; offset in its file's hints
  std::vector<uint64_t> hl;               // per output: hint bytes as placed
  for (size_t j = 0; j < nt; ++j) {
    const uint64_t kn = del_key_off[j + 1] - del_key_off[j];
    const size_t o = out.place(18 + kn, false);
    to[j] = (uint32_t)o;
    at[j] = out.cur() - (18 + kn);
    if (hl.size() <= o) hl.resize(o + 1, UINT64_MAX);
    if (hl[o] == UINT64_MAX) hl[o] = outs[o].hints.size();
    hat[j] = hl[o];
    hl[o] += 22 + kn;
  }
  struct TRun {
    size_t j0, j1;
    std::vector<uint8_t> bytes;
  };
  std::vector<TRun> runs;
  for (size_t j = 0; j < nt;) {
    size_t e = j + 1;
    while (e < nt && to[e] == to[j]) ++e;
    runs.push_back(TRun{j, e, {}});
    j = e;
  }
  std::vector<uint32_t> run_of(nt);
  for (size_t r = 0; r < runs.size(); ++r) {
    const TRun& R = runs[r];
    const uint64_t kl = del_key_off[R.j1] - del_key_off[R.j1 - 1];
    runs[r].bytes.resize(at[R.j1 - 1] + 18 + kl - at[R.j0]);
    OutFile& o = outs[to[R.j0]];
    o.hints.resize(hl[to[R.j0]]);
    o.len = at[R.j1 - 1] + 18 + kl;
    for (size_t j = R.j0; j < R.j1; ++j) run_of[j] = (uint32_t)r;
  }
  const unsigned ntt = nt < 65536 ? 1u : host_threads();
  parallel_for(ntt, [&](unsigned t) {
    for (size_t j = nt * t / ntt, e = nt * (t + 1) / ntt; j < e; ++j) {
      const TRun& R = runs[run_of[j]];
      const uint64_t ko = del_key_off[j], kn = del_key_off[j + 1] - ko;
      uint8_t* rec = (uint8_t*)R.bytes.data() + (at[j] - at[R.j0]);
      wr64(rec + 4, del_seq[j]);
      wr16(rec + 12, (uint16_t)kn);
      wr32(rec + 14, CASK_ENTRY_TOMBSTONE);
      if (kn) memcpy(rec + 18, H.del_key_bytes.data() + ko, kn);
      wr32(rec, cask_xxh::xxh32(rec + 4, 14 + kn, 0));
      uint8_t* h = outs[to[j]].hints.data() + hat[j];  // Hint::new(entry, entry_pos) (data.rs:218-226)
      wr_hint_header(h, del_seq[j], (uint16_t)kn, CASK_ENTRY_TOMBSTONE, at[j]);
      if (kn) memcpy(h + 22, H.del_key_bytes.data() + ko, kn);
    }
  });
  for (const TRun& R : runs) {
    OutFile& o = outs[to[R.j0]];
    if (!out.open_fd(o) || !pwrite_all(o.fd, R.bytes.data(), R.bytes.size(), at[R.j0])) {
      *fail_fid = o.fid;
      return CASK_E_IO;
    }
  }
  return CASK_OK;
}

// 6. compact_files (cask.rs:528-550): index the new files from their hints, drop the compacted
// files' stats, swap the file sets
int reindex_and_swap(cask_db* db, CompactOutputs& out, const std::vector<uint32_t>& compacted, cask_open_error* err,
                     Trace& trace) {
  const std::string& path = db->path;
  {
    const std::deque<OutFile>& outs = out.files();
    std::vector<FoldSrc> srcs;
    for (uint32_t fid : out.new_files()) {
      const OutFile& o = *std::find_if(outs.begin(), outs.end(), [&](const OutFile& x) { return x.fid == fid; });
      hint_fold_sources(o.hints.data(), o.hints.size(), fid, srcs);
    }
    parallel_fold(srcs, db->index);
  }
  trace("(swap) re-index of the new files");
  for (uint32_t fid : compacted) db->index.stats.erase(fid);  // Stats::remove_files (stats.rs:50-54)
  {  // Log::swap_files (log.rs:198-217): the compacted files leave the database here, on threads (the
     // first failure in file order is the error, as the reference's loop would return it): each
     // data file and its hint file renamed out of the names find_data_files matches (log.rs:473-510:
     // `...cask.data.gone` does not end in `.cask.data`), then unlinked by a thread of the db's own
     // while this call returns (unlinking configs[3]'s 64 GiB in place took 1.4 s on /dev/shm)
    std::vector<char> gone(compacted.size(), 1);
    std::vector<std::string> dead(2 * compacted.size());
    const unsigned ntu = host_lanes(compacted.size());
    parallel_for(ntu, [&](unsigned t) {
      for (size_t j = t; j < compacted.size(); j += ntu) {
        const std::string dp = data_path(path, compacted[j]), hp = hint_path(path, compacted[j]);
        gone[j] = rename(dp.c_str(), (dp + ".gone").c_str()) == 0;
        if (!gone[j]) continue;
        dead[2 * j] = dp + ".gone";
        if (rename(hp.c_str(), (hp + ".gone").c_str()) == 0) dead[2 * j + 1] = hp + ".gone";
      }
    });
    try {
      db->reclaim = std::thread([dead = std::move(dead)] {
        for (const std::string& f : dead)
          if (!f.empty()) (void)unlink(f.c_str());
      });
    } catch (...) {  // (no thread: unlinked here)
      for (const std::string& f : dead)
        if (!f.empty()) (void)unlink(f.c_str());
    }
    for (size_t j = 0; j < compacted.size(); ++j) {
      db->files.erase(std::lower_bound(db->files.begin(), db->files.end(), compacted[j]));
      if (!gone[j]) {
        set_err(err, CASK_E_IO, compacted[j]);
        return CASK_E_IO;
      }
    }
  }
  db->files.insert(db->files.end(), out.new_files().begin(), out.new_files().end());
  std::sort(db->files.begin(), db->files.end());
  trace("(swap) stats + unlink");
  return CASK_OK;
}

int compact_files_impl(cask_db* db, const uint32_t* files_in, uint64_t nfiles, cask_compact_result* res,
                       cask_open_error* err) {
  set_err(err, CASK_OK);
  if (!db || (nfiles && !files_in)) return CASK_E_INVALID_ARG;
  db->reclaim_join();  // (the previous compaction's files are gone before this one starts)
  cask_compact_result R{};
  auto t0 = std::chrono::steady_clock::now();
  // BTreeSet<u32> order (cask.rs:574, 639-640); only files of this Log
  std::vector<uint32_t> files(files_in, files_in + nfiles);
  std::sort(files.begin(), files.end());
  files.erase(std::unique(files.begin(), files.end()), files.end());
  files.erase(std::remove_if(files.begin(), files.end(),
                             [&](uint32_t f) { return !std::binary_search(db->files.begin(), db->files.end(), f); }),
              files.end());

  // 1. the hint pass: the compacted files, their live records and the tombstone tail
  HintPassResult H;  // (its reaper thread is joined after everything below)
  Trace trace;
  int st = compact_hint_pass(db, files, err, trace, H);
  if (st != CASK_OK) return st;
  trace("hint pass end");
  R.ms[0] = ms_since(t0);

  // 2-5. the live records through the device into the new data files, batch by batch
  CompactOutputs out(db);
  LiveTimes T;
  st = compact_live_records(db, H, out, &R.bytes_in, err, T);
  if (st != CASK_OK) return st;
  // the last batch's writes (R.ms[3] counts what this thread waited for the writer, not the writer's
  // time beside the device work)
  auto twl = std::chrono::steady_clock::now();
  uint32_t ff = 0;
  st = out.drain(&ff);
  T.write += ms_since(twl);
  if (st != CASK_OK) return out.abort(err, st, ff);
  R.ms[1] = T.verify;
  R.ms[2] = T.gather;
  if (trace.on)
    fprintf(stderr, "compact batches: live records copied from the mapped sources %.1f ms, to the device %.1f ms (of verify), writer busy %.1f ms\n",
            T.read, T.h2d, out.writer_ms());
  // then the tombstone tail, and the hint files of the output files the writer has not finished
  auto tw = std::chrono::steady_clock::now();
  if (write_tombstone_tail(H, out, &ff) != CASK_OK || out.finish_rest(&ff) != CASK_OK)
    return out.abort(err, CASK_E_IO, ff);
  T.write += ms_since(tw);
  trace.tp = tw;
  trace("(writes) tombstone tail + hint files");
  R.ms[3] = T.write;
  uint64_t bytes_out = 0;
  for (const OutFile& o : out.files()) bytes_out += o.len;

  // 6. re-index of the new files, and the swap of the file sets
  out.disarm();
  auto t4 = std::chrono::steady_clock::now();
  trace.tp = t4;
  st = reindex_and_swap(db, out, H.compacted, err, trace);
  if (st != CASK_OK) return st;
  R.ms[4] = ms_since(t4);

  R.n_compacted = (uint32_t)H.compacted.size();
  R.n_new = (uint32_t)out.new_files().size();
  R.n_tomb_only = (uint32_t)out.tomb_files().size();
  R.live_records = H.ins.size();
  R.tombstones = H.del_seq.size();
  R.bytes_out = bytes_out;
  R.ms_total = ms_since(t0);
  if (res) *res = R;
  return CASK_OK;
}

// Cask::compact (cask.rs:563-642): pick the files by the stats and their sizes; compact them if
// a trigger fired. Returns the number of files compacted (0: no trigger), or a negative status.
int64_t compact_impl(cask_db* db, const cask_compact_options* opts_in, cask_compact_result* res,
                     cask_open_error* err) {
  set_err(err, CASK_OK);
  if (!db) return CASK_E_INVALID_ARG;
  cask_compact_options o;
  if (opts_in) o = *opts_in; else cask_compact_options_default(&o);
  std::vector<uint32_t> sel;
  bool triggered = false;
  std::vector<uint32_t> ids;
  for (const auto& kv : db->index.stats) ids.push_back(kv.first);
  std::sort(ids.begin(), ids.end());  // the reference iterates a HashMap; the selected set is order-free
  for (uint32_t fid : ids) {
    const StatsEntry& se = db->index.stats[fid];
    const double frag = (double)se.dead_entries / (double)se.entries;  // stats.rs:56-67
    const uint64_t dead = se.dead_bytes;
    auto has = [&](uint32_t f) { return std::find(sel.begin(), sel.end(), f) != sel.end(); };
    if (!triggered) {
      if (frag >= o.fragmentation_trigger) {
        triggered = true;
        sel.push_back(fid);
      } else if (dead >= o.dead_bytes_trigger && !has(fid)) {
        triggered = true;
        sel.push_back(fid);
      }
    }
    if (frag >= o.fragmentation_threshold && !has(fid)) {
      sel.push_back(fid);
    } else if (dead >= o.dead_bytes_threshold && !has(fid)) {
      sel.push_back(fid);
    }
    if (!has(fid)) {
      struct stat st;
      if (stat(data_path(db->path, fid).c_str(), &st) == 0 && (uint64_t)st.st_size <= o.small_file_threshold)
        sel.push_back(fid);
    }
  }
  if (res) *res = cask_compact_result{};
  if (!triggered) return 0;
  const int st = cask_db_compact_files(db, sel.data(), sel.size(), res, err);
  return st == CASK_OK ? (int64_t)sel.size() : (int64_t)st;
}

}  // namespace

extern "C" {

void cask_compact_options_default(cask_compact_options* o) {  // cask.rs:229-234
  if (!o) return;
  o->fragmentation_trigger = 0.6;
  o->dead_bytes_trigger = 512ull * 1024 * 1024;
  o->fragmentation_threshold = 0.4;
  o->dead_bytes_threshold = 128ull * 1024 * 1024;
  o->small_file_threshold = 10ull * 1024 * 1024;
}

int cask_db_compact_files(cask_db* db, const uint32_t* files_in, uint64_t nfiles, cask_compact_result* res,
                          cask_open_error* err) {
  const int st = abi_status([&] { return compact_files_impl(db, files_in, nfiles, res, err); });
  if (st != CASK_OK && err && err->status == CASK_OK) set_err(err, st);  // (an exception's status)
  return st;
}

int64_t cask_db_compact(cask_db* db, const cask_compact_options* opts_in, cask_compact_result* res,
                        cask_open_error* err) {
  const int64_t st = abi_status([&] { return compact_impl(db, opts_in, res, err); });
  if (st < 0 && err && err->status == CASK_OK) set_err(err, (int)st);
  return st;
}

}  // extern "C"

// Cask::open above the C ABI: the replay (cask.rs:335-382) with the data-file scan on the GPU.
// Mirrors the hint-file fast path (log.rs:121-135, 432-447, 512-539; data.rs:258-276), hint
// recreation (log.rs:137-148, 367-395, 449-471) and the keydir fold Index::update + Stats
// (cask.rs:28-95; stats.rs:6-67) on one device (cask_db_open) and over several
// (cask_db_open_multi). The scan itself is cask_scan_host (scan_runtime.cpp); Log::open is
// open_log (engine_db.h).
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <memory>
#include <mutex>
#include <thread>

#include "engine_db.h"
#include "engine_dev.h"
#include "knobs.h"

using namespace cask_engine;

namespace {

// Which files have a valid hint file (is_valid_hint_file, log.rs:121-135, 512-539)? Read and
// checked on threads; the others are scanned. File i's body is buf[i][0, len[i] - 4): Take(size - 4)
// (log.rs:129).
struct HintFiles {
  std::vector<HostBuf> buf;
  std::vector<uint64_t> len;
  std::vector<char> use;
  const uint8_t* body(size_t i) const { return buf[i].get(); }
  uint64_t body_len(size_t i) const { return len[i] - 4; }
};
HintFiles load_hint_files(const std::string& path, const std::vector<uint32_t>& files) {
  const size_t nf = files.size();
  HintFiles h;
  h.buf.resize(nf);
  h.len.assign(nf, 0);
  h.use.assign(nf, 0);
  const unsigned nt = host_lanes(nf);
  parallel_for(nt, [&](unsigned t) {
    for (size_t i = t; i < nf; i += nt) h.use[i] = load_valid_hint(hint_path(path, files[i]), h.buf[i], h.len[i]);
  });
  return h;
}

// The bytes of the data files scanned at once: an eighth of all of them, at least 1 GiB (the scan's
// scratch stays bounded). The two opens cut their batches at this size by rules of their own.
uint64_t open_batch_bytes(uint64_t all) { return std::max<uint64_t>(1ull << 30, all / 8); }

// ---- cask_db_open --------------------------------------------------------------------------------

// The scanned files, in batches of consecutive files (an eighth of their bytes each, at least
// 1 GiB): a reader thread reads batch b + 1 from disk straight to the device (host threads,
// pinned buffers) while a device thread scans batch b and brings its hint bodies back (built on
// the device, cask_hints_device), and the opening thread replays the batches before it in file
// order — the fold and the hint files. The host never holds the data bytes, only the hint records
// it writes and folds.
// The destructor stops and joins the threads: an exception in the replay (std::bad_alloc in the
// fold) unwinds through it before anything the threads use goes away.
struct OpenPipeline {
  struct Batch {
    RawBytes hb;                // hint bodies of the batch's files
    std::vector<uint64_t> fo;   // view k of the batch: hb[fo[k], fo[k + 1])
    cask_scan_error se{};
    int st = CASK_OK;
    bool read_done = false, ready = false;
  };

  cask_db* const db;
  const bool write_hints;
  std::vector<char> data_ok;           // per file: its data file can be read
  std::vector<cask_file_view> views;   // the scanned files
  std::vector<uint32_t> view_file;     // per view: its file's index
  std::vector<int64_t> view_of;        // per file: its view, or -1
  std::vector<size_t> vcut{0};         // batch b: views [vcut[b], vcut[b + 1])
  std::vector<Batch> bat;
  // Every file scanned (no valid hint file): the keydir is reduced on the device — each batch's rows
  // kept, and after the last batch one block of the whole replay (cask_shard_keydir: per key only the
  // records that can decide the final keydir; configs[3]: a fifth of the records) that the opening
  // thread merges (cask_keydir_merge + cask_keydir_finish, as the multi-GPU open folds its ranges'
  // blocks) instead of folding every hint record. A replay that also has hint files folds on the host
  // (CASK_OPEN_DEVFOLD=0, a test hook, forces the host fold).
  bool dev_fold = false;
  std::vector<uint64_t> roff_all;  // (dev_fold) each view's first row
  EngineDev::AllRows all_rows;
  HostBuf dblock;               // (dev_fold) the block, on the host (huge pages: the copy faults 2-MiB pages)
  double t_blk[2] = {0, 0};     // (dev_fold) its build on the device, its copy to the host
  uint64_t dblock_n = 0;        // (dev_fold) its bytes
  int dblock_st = CASK_E_IO;    // (dev_fold) CASK_OK once the block is here
  bool dblock_done = false;
  double t_read = 0, t_dev = 0;
  EngineDev* ed = nullptr;
  std::unique_lock<std::mutex> edlock;
  int dst = CASK_OK;  // the device's preparation: every batch's status when it failed

  explicit OpenPipeline(cask_db* d) : db(d), write_hints(d->opts.write_hints != 0) {}
  ~OpenPipeline() { join_all(); }

  size_t nbat() const { return vcut.size() - 1; }

  // The views of the files without a valid hint file, their batches and their place on the device.
  int setup(const std::vector<char>& use_hint) {
    const std::string& path = db->path;
    const size_t nf = db->files.size();
    data_ok.assign(nf, 1);
    view_of.assign(nf, -1);
    size_t nscan = 0;
    for (size_t i = 0; i < nf; ++i) {
      if (use_hint[i]) continue;
      ++nscan;
      struct stat stt;
      if (stat(data_path(path, db->files[i]).c_str(), &stt) != 0) {
        data_ok[i] = 0;
        continue;
      }
      view_of[i] = (int64_t)views.size();
      views.push_back(cask_file_view{db->files[i], CASK_VIEW_DEVICE, nullptr, (uint64_t)stt.st_size});
      view_file.push_back((uint32_t)i);
    }
    {
      uint64_t all = 0, acc = 0;
      for (const auto& v : views) all += v.len;
      // CASK_OPEN_BATCH (test and tuning knob): bytes per batch (1: every file a batch of its own)
      const uint64_t bb_env = cask_knobs::hook("CASK_OPEN_BATCH") ? strtoull(cask_knobs::hook("CASK_OPEN_BATCH"), nullptr, 10) : 0ull;
      const uint64_t bb = bb_env ? bb_env : open_batch_bytes(all);
      for (size_t v = 0; v < views.size(); ++v) {  // (a batch ends with the file that fills it)
        acc += views[v].len;
        if (acc >= bb && v + 1 < views.size()) {
          vcut.push_back(v + 1);
          acc = 0;
        }
      }
      vcut.push_back(views.size());
    }
    bat.resize(nbat());
    const char* dfh = cask_knobs::hook("CASK_OPEN_DEVFOLD");
    dev_fold = !views.empty() && nscan == nf && !(dfh && !strcmp(dfh, "0"));
    roff_all.assign(views.size() + 1, 0);
    if (views.empty()) return CASK_OK;
    ed = engine_dev(db->opts.device);
    if (!ed) return CASK_E_DEVICE;
    edlock = std::unique_lock<std::mutex>(ed->mu);
    dst = ed->prepare();
    std::vector<uint64_t> doff(views.size() + 1, 0);
    for (size_t v = 0; v < views.size(); ++v) doff[v + 1] = doff[v] + align256(views[v].len);
    if (dst == CASK_OK && !ed->data.ensure(doff.back() + 256)) dst = CASK_E_NOMEM;
    if (dst == CASK_OK)
      for (size_t v = 0; v < views.size(); ++v) views[v].data = ed->data.p + doff[v];
    return CASK_OK;
  }

  // The reader and the device thread started; no threads to be had: the same steps, one after the
  // other.
  void start() {
    if (views.empty()) {
      for (Batch& bt : bat) bt.read_done = bt.ready = true;
      dblock_done = true;
      return;
    }
    bool threaded = false;
    try {
      th_read = std::thread([this] { reader(); });
      try {
        th_dev = std::thread([this] { device(); });
        threaded = true;
      } catch (...) {
        stop = true;  // (the reader marks every batch and ends)
        th_read.join();
      }
    } catch (...) {
    }
    if (!threaded) {
      stop = false;
      for (auto& bt : bat) bt = Batch();
      reader();
      device();
    }
  }

  void wait_ready(size_t b) {
    std::unique_lock<std::mutex> lk(bm);
    bcv.wait(lk, [&] { return bat[b].ready; });
  }
  void wait_block() {
    std::unique_lock<std::mutex> lk(bm);
    bcv.wait(lk, [&] { return dblock_done; });
  }
  void join_all() {
    stop = true;
    if (th_read.joinable()) th_read.join();
    if (th_dev.joinable()) th_dev.join();
  }
  // The threads joined, the device's large buffers given back and the device released.
  void finish() {
    join_all();
    if (ed) ed->trim();
    edlock = std::unique_lock<std::mutex>();
  }

 private:
  std::mutex bm;
  std::condition_variable bcv;
  std::atomic<bool> stop{false};
  std::thread th_read, th_dev;

  void mark(size_t b, int st, bool ready) {
    {
      std::lock_guard<std::mutex> g(bm);
      if (st != CASK_OK && bat[b].st == CASK_OK) bat[b].st = st;
      (ready ? bat[b].ready : bat[b].read_done) = true;
    }
    bcv.notify_all();
  }
  std::vector<cask_file_view> batch_views(size_t b) const {
    return std::vector<cask_file_view>(views.begin() + (ptrdiff_t)vcut[b], views.begin() + (ptrdiff_t)vcut[b + 1]);
  }

  // (the two pipeline threads catch their own exceptions: a batch that throws gets a status, and
  // every batch is still marked, so nobody waits forever and the threads can be joined)
  void reader() {
    const auto tr = std::chrono::steady_clock::now();
    for (size_t b = 0; b < nbat(); ++b) {
      int st = dst;
      if (st == CASK_OK && !stop.load() && vcut[b + 1] > vcut[b]) {
        st = abi_status([&] {
          std::vector<std::string> paths;
          std::vector<cask_file_view> vb = batch_views(b);
          for (size_t v = vcut[b]; v < vcut[b + 1]; ++v) paths.push_back(data_path(db->path, db->files[view_file[v]]));
          std::vector<char> ok(vb.size(), 1);
          const int rs = ed->read_to_device(paths, vb, ok);
          for (size_t k = 0; k < vb.size(); ++k)
            if (!ok[k]) {  // the file could not be read whole: Log::entries' Io error when its turn comes
              data_ok[view_file[vcut[b] + k]] = 0;
              views[vcut[b] + k].len = 0;
            }
          return rs;
        });
      }
      mark(b, st, false);
    }
    t_read = ms_since(tr);
  }

  void device() {
    for (size_t b = 0; b < nbat(); ++b) {
      {
        std::unique_lock<std::mutex> lk(bm);
        bcv.wait(lk, [&] { return bat[b].read_done; });
      }
      const auto td = std::chrono::steady_clock::now();
      int st = bat[b].st;
      if (st == CASK_OK && !stop.load() && vcut[b + 1] > vcut[b]) {
        st = abi_status([&] {
          std::vector<cask_file_view> vb = batch_views(b);
          std::vector<uint64_t> ro(vb.size() + 1);
          int ds = ed->scan(vb, ro, bat[b].se);
          // the hint bodies: for the hint files, and for the host fold (with the keydir reduced on
          // the device and no hint files to write, none)
          if (ds == CASK_OK && dev_fold && !write_hints) bat[b].fo.assign(vb.size() + 1, 0);
          else if (ds == CASK_OK) ds = ed->hints(vb, ro, bat[b].hb, bat[b].fo);
          if (ds == CASK_OK && dev_fold && !bat[b].se.kind) {  // the batch's rows, kept for the block
            for (size_t k = 0; k <= vb.size(); ++k) roff_all[vcut[b] + k] = all_rows.n + ro[k];
            ds = all_rows.append(ed->r, ro[vb.size()], (hipStream_t)cask_ctx_stream(ed->ctx));
          }
          return ds;
        });
      }
      t_dev += ms_since(td);
      mark(b, st, true);
    }
    // (dev_fold) every batch scanned clean: the replay's block, reduced on the device, to the host
    bool clean = dev_fold;
    for (size_t b = 0; b < nbat() && clean; ++b) clean = bat[b].st == CASK_OK && !bat[b].se.kind && !stop.load();
    int bs = CASK_E_IO;
    if (clean) {
      const auto td = std::chrono::steady_clock::now();
      bs = abi_status([&] {
        const cask_rows r = all_rows.view();
        return ed->block_to_host(
            false, views, r, roff_all,
            [&](uint64_t nb) { return dblock.alloc(std::max<uint64_t>(nb, 1)) ? dblock.get() : nullptr; }, &dblock_n,
            t_blk);
      });
      t_dev += ms_since(td);
    }
    {
      std::lock_guard<std::mutex> g(bm);
      dblock_st = bs;
      dblock_done = true;
    }
    bcv.notify_all();
  }
};

// What the replay carries from batch to batch.
struct Replay {
  size_t fi = 0;  // the next file to replay
  FoldScratch fscratch;
  double t_fold = 0, t_hint = 0;
};

// One batch replayed in ascending file order (cask.rs:348-369): the files up to the batch's last
// scanned one, the first Err aborts open() (`fail`). Hint files of the scanned files up to that
// point are written on threads: each is its body + XXH32 trailer (RecreateHints keeps draining after
// an error, so a failing file's hint file has every Ok row).
void replay_batch(cask_db* db, OpenPipeline& P, HintFiles& hints, size_t b, Replay& R, cask_open_error& fail) {
  const std::string& path = db->path;
  const size_t nf = db->files.size(), fi = R.fi;
  OpenPipeline::Batch& bt = P.bat[b];
  const size_t fe = b + 1 < P.nbat() ? (size_t)P.view_file[P.vcut[b + 1] - 1] + 1 : nf;
  uint32_t err_file = UINT32_MAX;  // the batch's first failing record is in this file
  if (bt.se.kind)
    for (size_t v = P.vcut[b]; v < P.vcut[b + 1]; ++v)
      if (P.views[v].file_id == bt.se.file_id) err_file = P.view_file[v];
  auto tf = std::chrono::steady_clock::now();
  // each file's hint body (a hint file's, or the one built for a scanned file), walked on threads:
  // its fold sources, highest sequence and first short read (Hints::next / Hint::from_read,
  // log.rs:437-447; data.rs:258-276)
  struct Body {
    const uint8_t* b = nullptr;
    uint64_t n = 0, max_seq = 0, bad = UINT64_MAX;
    std::vector<FoldSrc> src;  // pieces of kFoldPiece records: the fold's sources
  };
  std::vector<Body> bodies(fe - fi);
  for (size_t i = fi; i < fe; ++i) {
    Body& B = bodies[i - fi];
    if (hints.use[i]) {
      B.b = hints.body(i);
      B.n = hints.body_len(i);
    } else if (P.data_ok[i] && P.view_of[i] >= 0) {
      const size_t k = (size_t)P.view_of[i] - P.vcut[b];
      B.b = bt.hb.data() + bt.fo[k];
      B.n = bt.fo[k + 1] - bt.fo[k];
    }
  }
  // (dev_fold: the bodies were built on the device from the scan's rows — whole records, and the
  // block carries the highest sequence — so only their hint files are written below)
  const unsigned nt = host_lanes(fe - fi);
  if (!P.dev_fold) parallel_for(nt, [&](unsigned t) {
    for (size_t i = fi + t; i < fe; i += nt) {
      Body& B = bodies[i - fi];
      B.bad = hint_fold_sources(B.b, B.n, db->files[i], B.src, &B.max_seq);
    }
  });
  size_t nrep = fi;  // files of the batch replayed: [fi, nrep)
  std::vector<uint32_t> to_write;
  for (size_t i = fi; i < fe && fail.status == CASK_OK; ++i) {
    const uint32_t fid = db->files[i];
    if (!hints.use[i]) {
      if (!P.data_ok[i]) {
        // HintWriter::new truncated the hint file before Log::entries failed; its Drop then wrote
        // the trailer of an empty body (log.rs:141-142, 389-395).
        if (P.write_hints) write_hint_file(hint_path(path, fid), nullptr, 0);
        fail = cask_open_error{CASK_E_IO, fid, 0, 0, 0};
        break;
      }
      if (P.write_hints) to_write.push_back((uint32_t)i);
      if (err_file == i) {
        const cask_scan_error& se = bt.se;
        fail = cask_open_error{se.kind == CASK_ROW_CHECKSUM ? CASK_E_CHECKSUM : CASK_E_EOF, fid, se.pos, se.expected,
                               se.found};
        break;
      }
    }
    if (bodies[i - fi].bad != UINT64_MAX) {
      fail = cask_open_error{CASK_E_EOF, fid, bodies[i - fi].bad, 0, 0};
      break;
    }
    if (bodies[i - fi].max_seq > db->sequence) db->sequence = bodies[i - fi].max_seq;
    nrep = i + 1;
  }
  // the batch's fold sources, in order: the pieces of each replayed file's body
  std::vector<FoldSrc> srcs;
  if (fail.status == CASK_OK)
    for (size_t i = fi; i < nrep; ++i) srcs.insert(srcs.end(), bodies[i - fi].src.begin(), bodies[i - fi].src.end());
  R.t_fold += ms_since(tf);
  auto th = std::chrono::steady_clock::now();
  {
    std::vector<char> wok(to_write.size(), 1);
    const unsigned nw = host_lanes(to_write.size());
    parallel_for(nw, [&](unsigned t) {
      for (size_t j = t; j < to_write.size(); j += nw) {
        const Body& B = bodies[to_write[j] - fi];
        wok[j] = write_hint_file(hint_path(path, db->files[to_write[j]]), B.b, B.n);
      }
    });
    for (size_t j = 0; j < to_write.size() && fail.status == CASK_OK; ++j)
      if (!wok[j]) fail = cask_open_error{CASK_E_IO, db->files[to_write[j]], 0, 0, 0};
  }
  R.t_hint += ms_since(th);
  if (fail.status != CASK_OK) return;
  // Index::update + Stats over the batch's records (their keys stay in the hint files' buffers / the
  // batch's bodies until here)
  auto tf2 = std::chrono::steady_clock::now();
  if (!P.dev_fold) parallel_fold(srcs, db->index, &R.fscratch);
  R.t_fold += ms_since(tf2);
  RawBytes().p.swap(bt.hb.p);  // (the batch's bodies are no longer needed)
  for (size_t i = fi; i < fe; ++i)
    if (hints.use[i]) hints.buf[i].reset();
  R.fi = fe;
}

// (dev_fold) the whole replay's block, merged in one fold; its status
int merge_device_block(cask_db* db, OpenPipeline& P) {
  auto tf3 = std::chrono::steady_clock::now();
  P.wait_block();
  const double t_wait = ms_since(tf3);
  int st = P.dblock_st;
  double t_merge = 0;
  if (st == CASK_OK) {
    const auto tm = std::chrono::steady_clock::now();
    db->merging = true;
    st = cask_keydir_merge(db, P.dblock.get(), P.dblock_n);
    t_merge = ms_since(tm);
    if (st == CASK_OK) st = cask_keydir_finish(db);
  }
  if (cask_knobs::hook("CASK_OPEN_TRACE"))
    fprintf(stderr, "open (device-reduced keydir): block %.1f ms on the device, %.1f ms to the host (%llu B); "
                    "waited %.1f ms; merge %.1f ms, finish %.1f ms\n",
            P.t_blk[0], P.t_blk[1], (unsigned long long)P.dblock_n, t_wait, t_merge, ms_since(tf3) - t_wait - t_merge);
  db->discard({&P.dblock});
  return st;
}

cask_db* db_open_impl(const char* path_c, const cask_options* opts_in, cask_open_error* err) {
  auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<cask_db> own(open_log(path_c, opts_in, err));  // (deleted on every failure: the lock goes)
  cask_db* db = own.get();
  if (!db) return nullptr;
  // 1. which files have a valid hint file; the others go through the pipeline
  HintFiles hints = load_hint_files(db->path, db->files);
  OpenPipeline P(db);
  const int st0 = P.setup(hints.use);
  if (st0 != CASK_OK) {
    set_err(err, st0);
    return nullptr;
  }
  P.start();
  db->timings[0] = ms_since(t0);  // (until the replay starts; the reads' own span is added below)
  // 2. the replay, batch after batch; the first Err aborts open()
  Replay R;
  cask_open_error fail{};
  for (size_t b = 0; b < P.nbat() && fail.status == CASK_OK; ++b) {
    P.wait_ready(b);
    if (P.bat[b].st != CASK_OK) {
      fail.status = P.bat[b].st;
      break;
    }
    replay_batch(db, P, hints, b, R, fail);
  }
  // 3. (dev_fold) the keydir from the device's block
  if (P.dev_fold && fail.status == CASK_OK) {
    auto tf3 = std::chrono::steady_clock::now();
    const int st = merge_device_block(db, P);
    if (st != CASK_OK) fail = cask_open_error{st, 0, 0, 0, 0};
    R.t_fold += ms_since(tf3);
  }
  P.finish();
  db->timings[0] = P.t_read;
  db->timings[1] = P.t_dev;
  db->timings[2] = R.t_hint;
  db->timings[3] = R.t_fold;
  db->timings[4] = ms_since(t0);
  if (fail.status != CASK_OK) {
    if (err) *err = fail;
    return nullptr;
  }
  return own.release();
}

// ---- cask_db_open_multi --------------------------------------------------------------------------

// One range of files on its device.
struct Shard {
  size_t lo = 0, hi = 0;
  std::vector<RawBytes> blocks;
  std::vector<uint32_t> parts;  // hint files written under their temporary names, in order
  cask_open_error e{};
  double ms_read = 0, ms_scan = 0;
  bool fail(int st, uint32_t fid = 0, uint64_t pos = 0, uint32_t ex = 0, uint32_t f = 0) {
    e = cask_open_error{st, fid, pos, ex, f};
    return false;
  }
  // a keydir block's place on the host (EngineDev::block_to_host)
  uint8_t* new_block(uint64_t nb) {
    blocks.emplace_back();
    return blocks.back().resize(nb) ? blocks.back().data() : nullptr;
  }
};

// The files of a stretch side by side in one device allocation, freed when dropped.
struct StretchViews {
  uint8_t* dbuf = nullptr;
  uint64_t total = 0;
  std::vector<cask_file_view> views;
  ~StretchViews() {
    if (dbuf) (void)hipFree(dbuf);
  }
  int alloc(int dev, const uint32_t* file_ids, const std::vector<uint64_t>& blen) {
    for (uint64_t b : blen) total += align256(b);
    if (hipSetDevice(dev) != hipSuccess) return CASK_E_DEVICE;
    if (hipMalloc(&dbuf, total + 256) != hipSuccess) return CASK_E_NOMEM;
    views.resize(blen.size());
    uint64_t off = 0;
    for (size_t i = 0; i < blen.size(); ++i) {
      views[i] = cask_file_view{file_ids[i], CASK_VIEW_DEVICE, dbuf + off, blen[i]};
      off += align256(blen[i]);
    }
    return CASK_OK;
  }
};

// One stretch [lo, hi) of files with valid hint files on device `dev` through its EngineDev `ed`
// (locked by the caller; its context, pinned rings and buffers), reduced to one keydir block; false
// on failure (s.e set). The bodies are parsed on the device (cask_parse_hints_device).
bool run_hint_stretch(cask_db* db, const HintFiles& hints, Shard& s, int dev, EngineDev* ed, size_t lo, size_t hi) {
  auto tr = std::chrono::steady_clock::now();
  const size_t n = hi - lo;
  std::vector<uint64_t> blen(n);
  for (size_t i = 0; i < n; ++i) blen[i] = hints.body_len(lo + i);
  StretchViews sv;
  int st = sv.alloc(dev, db->files.data() + lo, blen);
  if (st != CASK_OK) return s.fail(st);
  const std::vector<cask_file_view>& views = sv.views;
  for (size_t i = 0; i < n; ++i)  // (the bodies are in host memory already)
    if (blen[i] && hipMemcpy((void*)views[i].data, hints.body(lo + i), blen[i], hipMemcpyHostToDevice) != hipSuccess)
      return s.fail(CASK_E_DEVICE);
  s.ms_read += ms_since(tr);
  auto ts = std::chrono::steady_clock::now();
  // rows sized from the body bytes (hint records are at least 22 B)
  const uint64_t cap = cask_rows_bound(views.data(), (uint32_t)n);
  if (!ed->rows.ensure(rows_bytes(cap))) return s.fail(CASK_E_NOMEM);
  cask_rows rows = carve_rows(ed->rows.p, cap);
  std::vector<uint64_t> roff(n + 1, 0);
  cask_scan_error se{};
  st = cask_parse_hints_device(ed->ctx, views.data(), (uint32_t)n, &rows, roff.data(), &se);
  if (st != CASK_OK) return s.fail(st);
  if (se.kind)  // a hint record cut short: Cask::open's `?` (cask.rs:360,365)
    return s.fail(CASK_E_EOF, se.file_id, se.pos, se.expected, se.found);
  uint64_t nb = 0;
  st = ed->block_to_host(true, views, rows, roff, [&](uint64_t b) { return s.new_block(b); }, &nb);
  if (st != CASK_OK) return s.fail(st);
  s.ms_scan += ms_since(ts);
  return true;
}

// One stretch [lo, hi) of data files without a valid hint file, as above: read straight to the
// device by the pinned ring's reader threads (the stretch's bytes stay resident: the block reads its
// keys there), scanned in batches of at most an eighth of the stretch (at least 1 GiB: the scan's
// scratch stays bounded), each batch's hint bodies written under their temporary names and its rows
// kept, then one block over every row of the stretch (as open() does).
bool run_data_stretch(cask_db* db, Shard& s, int dev, EngineDev* ed, size_t lo, size_t hi) {
  const std::string& path = db->path;
  const size_t n = hi - lo;
  std::vector<uint64_t> blen(n);
  std::vector<std::string> paths;
  for (size_t i = 0; i < n; ++i) {  // File::open + metadata (log.rs:190-196): a file that cannot be read is its Io error
    struct stat stt;
    paths.push_back(data_path(path, db->files[lo + i]));
    if (stat(paths.back().c_str(), &stt) != 0) return s.fail(CASK_E_IO, db->files[lo + i]);
    blen[i] = (uint64_t)stt.st_size;
  }
  StretchViews sv;
  int st = sv.alloc(dev, db->files.data() + lo, blen);
  if (st != CASK_OK) return s.fail(st);
  const std::vector<cask_file_view>& views = sv.views;
  hipStream_t cst = (hipStream_t)cask_ctx_stream(ed->ctx);
  std::vector<uint64_t> roff(n + 1, 0);
  EngineDev::AllRows all;
  // batches of consecutive files (a batch ends before the file that would overfill it)
  const uint64_t bb = open_batch_bytes(sv.total);
  for (size_t b0 = 0; b0 < n;) {
    size_t b1 = b0 + 1;
    uint64_t acc = blen[b0];
    while (b1 < n && acc + blen[b1] <= bb) acc += blen[b1++];
    const std::vector<cask_file_view> vb(views.begin() + (ptrdiff_t)b0, views.begin() + (ptrdiff_t)b1);
    const std::vector<std::string> pb(paths.begin() + (ptrdiff_t)b0, paths.begin() + (ptrdiff_t)b1);
    auto tb = std::chrono::steady_clock::now();
    std::vector<char> ok(vb.size(), 1);
    st = ed->read_to_device(pb, vb, ok);
    if (st != CASK_OK) return s.fail(st);
    for (size_t k = 0; k < vb.size(); ++k)
      if (!ok[k]) return s.fail(CASK_E_IO, vb[k].file_id);
    s.ms_read += ms_since(tb);
    tb = std::chrono::steady_clock::now();
    std::vector<uint64_t> ro(vb.size() + 1);
    cask_scan_error se{};
    st = ed->scan(vb, ro, se);
    if (st != CASK_OK) return s.fail(st);
    if (db->opts.write_hints) {  // RecreateHints (log.rs:137-148): every Ok row of each file, trailer
      RawBytes hb;
      std::vector<uint64_t> fo;
      st = ed->hints(vb, ro, hb, fo);
      if (st != CASK_OK) return s.fail(st);
      // files up to the first failing one (that one included: the drain on drop, log.rs:466-470)
      for (size_t k = 0; k < vb.size(); ++k) {
        s.parts.push_back(vb[k].file_id);
        if (!write_hint_file(part_path(hint_path(path, vb[k].file_id)), hb.data() + fo[k], fo[k + 1] - fo[k]))
          return s.fail(CASK_E_IO, vb[k].file_id);
        if (se.kind && se.file_id == vb[k].file_id) break;
      }
    }
    if (se.kind)  // the stretch's first failing record: Cask::open's `?` (cask.rs:360,365)
      return s.fail(se.kind == CASK_ROW_CHECKSUM ? CASK_E_CHECKSUM : CASK_E_EOF, se.file_id, se.pos, se.expected, se.found);
    for (size_t k = 0; k <= vb.size(); ++k) roff[b0 + k] = all.n + ro[k];
    st = all.append(ed->r, ro[vb.size()], cst);
    if (st != CASK_OK) return s.fail(st);
    s.ms_scan += ms_since(tb);
    b0 = b1;
  }
  auto ts = std::chrono::steady_clock::now();
  const cask_rows rows = all.view();
  uint64_t nb = 0;
  st = ed->block_to_host(false, views, rows, roff, [&](uint64_t b) { return s.new_block(b); }, &nb);
  if (st != CASK_OK) return s.fail(st);
  s.ms_scan += ms_since(ts);
  return true;
}

// A range on its device: maximal stretches of files of one kind, in order, a block each.
void run_shard(cask_db* db, const HintFiles& hints, Shard& s, int dev) {
  if (s.lo == s.hi) return;
  EngineDev* ed = engine_dev(dev);  // (its pinned ring, for the reads; one user at a time)
  if (!ed) {
    s.fail(CASK_E_DEVICE);
    return;
  }
  std::lock_guard<std::mutex> edg(ed->mu);
  const int st0 = ed->prepare();
  if (st0 != CASK_OK) {
    s.fail(st0);
    return;
  }
  for (size_t i = s.lo; i < s.hi;) {
    size_t j = i + 1;
    while (j < s.hi && hints.use[j] == hints.use[i]) ++j;
    // (an exception in a stretch is its failure)
    const int st = abi_status([&] {
      return (hints.use[i] ? run_hint_stretch(db, hints, s, dev, ed, i, j) : run_data_stretch(db, s, dev, ed, i, j))
                 ? CASK_OK
                 : 1;
    });
    if (st != CASK_OK) {
      if (st != 1) s.fail(st);
      break;
    }
    i = j;
  }
  ed->trim();
}

// The ranges run in parallel, but the reference's replay stops at the first Err: the hint files
// written under temporary names go into place up to the first failing range rf (in replay order; its
// own, which end at its failing file, included) and are removed after it. False when a rename
// failed (*ren_fail: its file).
bool place_part_files(const std::string& path, const std::vector<Shard>& sh, int rf, uint32_t* ren_fail) {
  bool ren_ok = true;
  for (int r = 0; r < (int)sh.size(); ++r)
    for (uint32_t fid : sh[r].parts) {
      const std::string hp = hint_path(path, fid);
      if (r <= rf) {
        if (ren_ok && rename(part_path(hp).c_str(), hp.c_str()) != 0) {
          ren_ok = false;
          *ren_fail = fid;
        }
        if (!ren_ok) (void)unlink(part_path(hp).c_str());
      } else {
        (void)unlink(part_path(hp).c_str());
      }
    }
  return ren_ok;
}

// Cask::open over several GPUs of this process: contiguous file-id ranges, one per devices[] entry;
// each range is reduced to keydir blocks on its device (one host thread per distinct device, its
// ranges one after another), and the blocks are folded here in range order. Within a range, files
// with a valid hint file take the fast path (log.rs:121-135): their bodies are parsed on the device
// (cask_parse_hints_device) and reduced (cask_shard_keydir_hints); the others are scanned
// (cask_scan_device, cask_shard_keydir) and, with write_hints, get their hint files from the device
// (cask_hints_device). Each maximal stretch of files of one kind gives one block.
// The ranges run in parallel, but the reference's replay stops at the first Err (cask.rs:357-368)
// and never reaches a later file: so every hint file is first written under a temporary name
// (`.part`), and only once all ranges are done are the ones up to the first failure (in replay order)
// renamed into place — the failing range's own, which end at its failing file, included — and the
// later ranges' removed.
cask_db* open_multi_impl(const char* path_c, const cask_options* opts_in, const int* devices, int ndev,
                         cask_open_error* err) {
  set_err(err, CASK_OK);
  if (!devices || ndev < 1) {
    set_err(err, CASK_E_INVALID_ARG);
    return nullptr;
  }
  auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<cask_db> own(open_log(path_c, opts_in, err));
  cask_db* db = own.get();
  if (!db) return nullptr;
  const size_t nf = db->files.size();
  HintFiles hints = load_hint_files(db->path, db->files);
  std::vector<Shard> sh((size_t)ndev);
  for (int r = 0; r < ndev; ++r) {
    sh[r].lo = nf * (size_t)r / (size_t)ndev;
    sh[r].hi = nf * (size_t)(r + 1) / (size_t)ndev;
  }
  // one thread per distinct device; a device's shards run in order on its thread
  std::vector<int> devs;
  for (int r = 0; r < ndev; ++r)
    if (std::find(devs.begin(), devs.end(), devices[r]) == devs.end()) devs.push_back(devices[r]);
  parallel_for((unsigned)devs.size(), [&](unsigned t) {
    for (int r = 0; r < ndev; ++r)
      if (devices[r] == devs[t]) run_shard(db, hints, sh[r], devices[r]);
  });
  int rf = ndev;  // the first range that failed, in replay order
  for (int r = 0; r < ndev && rf == ndev; ++r)
    if (sh[r].e.status != CASK_OK) rf = r;
  // hint files: into place up to the first failure, removed after it
  uint32_t ren_fail = 0;
  const bool ren_ok = place_part_files(db->path, sh, rf, &ren_fail);
  if (rf < ndev) {
    if (err) *err = sh[rf].e;
    return nullptr;
  }
  if (!ren_ok) {
    set_err(err, CASK_E_IO, ren_fail);
    return nullptr;
  }
  double rd = 0, sc = 0;
  for (const Shard& s : sh) {
    rd = std::max(rd, s.ms_read);
    sc = std::max(sc, s.ms_scan);
  }
  hints = HintFiles();
  auto tf = std::chrono::steady_clock::now();
  db->merging = true;
  {  // every range's blocks, in range order, in one pass
    std::vector<const uint8_t*> bp;
    std::vector<uint64_t> bl;
    for (int r = 0; r < ndev; ++r)
      for (const auto& b : sh[r].blocks) {
        bp.push_back(b.data());
        bl.push_back(b.size());
      }
    const int st = cask_keydir_merge_many(db, bp.data(), bl.data(), (uint32_t)bp.size());
    if (st != CASK_OK) {
      set_err(err, st);
      return nullptr;
    }
  }
  cask_keydir_finish(db);
  db->timings[0] = rd;
  db->timings[1] = sc;
  db->timings[2] = 0;
  db->timings[3] = ms_since(tf);
  db->timings[4] = ms_since(t0);
  return own.release();
}

}  // namespace

extern "C" {

void cask_options_default(cask_options* o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->create = 1;
  o->write_hints = 1;
  o->max_file_size = 2ull * 1024 * 1024 * 1024;  // cask.rs:225
  o->device = 0;
}

cask_db* cask_db_open(const char* path_c, const cask_options* opts_in, cask_open_error* err) {
  return abi_db(err, [&] { return db_open_impl(path_c, opts_in, err); });
}

cask_db* cask_db_open_multi(const char* path_c, const cask_options* opts_in, const int* devices, int ndev,
                            cask_open_error* err) {
  return abi_db(err, [&] { return open_multi_impl(path_c, opts_in, devices, ndev, err); });
}

}  // extern "C"

// The database handle behind the C ABI (Cask, cask.rs:97-110: the Log's files and lock, the keydir,
// the sequence), Log::open (log.rs:36-85), and what every entry point shares: the error record and
// the guards that keep C++ exceptions inside the library.
#pragma once
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <chrono>
#include <initializer_list>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/cask_scan.h"
#include "abi_guard.h"
#include "engine_io.h"
#include "keydir_host.h"

// (the C ABI's opaque handle: a global name, but none of its members leaves the library)
struct __attribute__((visibility("hidden"))) cask_db {
  using HostBuf = cask_engine::HostBuf;
  std::string path;
  cask_options opts{};
  int lock_fd = -1;
  std::vector<uint32_t> files;
  cask_engine::Index index;
  uint64_t sequence = 0;
  uint32_t file_seq = 0;  // Log::file_id_seq: the last data file id at open (log.rs:63-69)
  double timings[5] = {0, 0, 0, 0, 0};
  // sharded replay (cask_keydir_merge): per-file order-free stats terms, summed over shards
  struct ShardTerms {
    uint64_t puts = 0, put_bytes = 0, stale = 0, stale_bytes = 0;
  };
  std::unordered_map<uint32_t, ShardTerms> terms;
  bool merging = false;
  uint32_t shards = 0;
  // the merge's scratch (key hashes, items), kept from block to block and given back after the
  // last one (cask_keydir_finish), off the calling thread
  HostBuf mhash, mitems;
  // Host buffers of GiBs given back on threads of the db's own (unmapping them takes a while and
  // nothing waits for it: a thread per discard, each owning what it unmaps), all joined at close;
  // here when no thread can be had.
  std::vector<std::thread> gone_th;
  void discard(std::initializer_list<HostBuf*> bs) {
    std::vector<HostBuf> g;
    for (HostBuf* b : bs)
      if (b->p) g.push_back(std::move(*b));
    if (g.empty()) return;
    try {
      gone_th.emplace_back([v = std::move(g)]() mutable { v.clear(); });
    } catch (...) {
    }  // (g, if not moved into a thread, is unmapped here)
  }
  // the bytes of files a compaction took out of the database, released on a thread of their own
  // (joined before the next compaction and at close)
  std::thread reclaim;
  void reclaim_join() {
    if (reclaim.joinable()) reclaim.join();
  }
  ~cask_db() {
    reclaim_join();
    for (std::thread& t : gone_th)
      if (t.joinable()) t.join();
    if (lock_fd >= 0) {
      flock(lock_fd, LOCK_UN);  // Drop for Log (log.rs:225-229)
      close(lock_fd);
    }
  }
};

CASK_ENGINE_NAMESPACE {

inline double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

inline void set_err(cask_open_error* err, int status, uint32_t fid = 0, uint64_t pos = 0, uint32_t e = 0,
                    uint32_t f = 0) {
  if (!err) return;
  err->status = status;
  err->file_id = fid;
  err->pos = pos;
  err->expected = e;
  err->found = f;
}

// No C++ exception crosses the C ABI (cask_scan.h): the entry points that allocate or start threads
// run their bodies under these guards — std::bad_alloc (host memory pressure: a huge hint file, a
// keydir at cfg5 scale) is CASK_E_NOMEM, anything else (std::system_error from a thread or a mutex)
// CASK_E_IO. parallel_for (host_ring.h) carries a worker's exception back to its caller, and the open
// pipeline's threads turn theirs into a batch status, so every exception ends up here.
template <class F>
inline auto abi_status(F&& f) noexcept -> decltype(f()) {
  return cask_abi::guard(static_cast<F&&>(f));
}
template <class F>
inline cask_db* abi_db(cask_open_error* err, F&& f) noexcept {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    set_err(err, CASK_E_NOMEM);
  } catch (...) {
    set_err(err, CASK_E_IO);
  }
  return nullptr;
}

// Log::open (log.rs:36-85): path checks, the lock file, the data files in id order. Returns the
// handle (no keydir yet) or NULL with *err set.
inline cask_db* open_log(const char* path_c, const cask_options* opts_in, cask_open_error* err) {
  set_err(err, CASK_OK);
  if (!path_c) {
    set_err(err, CASK_E_INVALID_ARG);
    return nullptr;
  }
  cask_options opts;
  if (opts_in) opts = *opts_in; else cask_options_default(&opts);
  std::string path = path_c;
  // Log::open path checks (log.rs:46-56)
  if (opts.create) {
    if (exists(path) && !is_dir(path)) {
      set_err(err, CASK_E_INVALID_PATH);
      return nullptr;
    }
    if (!exists(path) && mkdir(path.c_str(), 0755) != 0) {
      set_err(err, CASK_E_IO);
      return nullptr;
    }
  } else if (!exists(path) || !is_dir(path)) {
    set_err(err, CASK_E_INVALID_PATH);
    return nullptr;
  }
  cask_db* db = new (std::nothrow) cask_db();
  if (!db) {
    set_err(err, CASK_E_NOMEM);
    return nullptr;
  }
  db->path = path;
  db->opts = opts;
  // File::create("cask.lock") + try_lock_exclusive (log.rs:58-59)
  db->lock_fd = open((path + "/cask.lock").c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (db->lock_fd < 0) {
    delete db;
    set_err(err, CASK_E_IO);
    return nullptr;
  }
  if (flock(db->lock_fd, LOCK_EX | LOCK_NB) != 0) {
    close(db->lock_fd);
    db->lock_fd = -1;
    delete db;
    set_err(err, CASK_E_LOCKED);
    return nullptr;
  }
  remove_gone_files(path);
  if (!find_data_files(path, db->files)) {
    delete db;
    set_err(err, CASK_E_IO);
    return nullptr;
  }
  db->file_seq = db->files.empty() ? 0u : db->files.back();
  return db;
}

}  // namespace cask_engine

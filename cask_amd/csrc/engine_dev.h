// The device side of the engine: one EngineDev per GPU, kept for the life of the process, with the
// scan of Cask::open's data files (Log::entries, log.rs:150-166, as cask_scan_device), the hint
// bodies built on the device (RecreateHints, log.rs:137-148) and the keydir block of a replay.
#pragma once
#include <hip/hip_runtime_api.h>

#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cask_scan.h"
#include "engine_io.h"
#include "host_ring.h"

CASK_ENGINE_NAMESPACE {

// The SoA rows of a scan carved out of one device buffer: pos, seq (u64), vsz (u32), ksz (u16) and
// status (u8) columns of `cap` rows, each starting on a 256-byte boundary. rows_bytes(cap) bounds
// the buffer: 23 bytes per row, the padding of four columns (under 256 bytes each) and 256 bytes to
// spare after the last one.
inline uint64_t rows_bytes(uint64_t cap) { return cap * 23 + 5 * 256; }
inline cask_rows carve_rows(uint8_t* p, uint64_t cap) {
  cask_rows r{};
  r.capacity = cap;
  r.pos = (uint64_t*)p;
  r.seq = (uint64_t*)(p + align256(cap * 8));
  r.vsz = (uint32_t*)(p + 2 * align256(cap * 8));
  r.ksz = (uint16_t*)(p + 2 * align256(cap * 8) + align256(cap * 4));
  r.status = p + 2 * align256(cap * 8) + align256(cap * 4) + align256(cap * 2);
  return r;
}

// The scan side of Cask::open on one GPU, kept per device for the life of the process (a context,
// its buffers and a ring of pinned staging buffers are created once, not per open): data files
// read by host threads into pinned buffers and copied to the device as they arrive, the device
// scan, and the hint bodies built on the device (cask_hints_device) and copied back.
struct EngineDev {
  int device = 0;
  std::mutex mu;  // one open() at a time per device
  cask_ctx* ctx = nullptr;
  struct Buf {
    uint8_t* p = nullptr;
    size_t cap = 0;
    bool ensure(size_t b) {
      if (b <= cap) return true;
      if (p) (void)hipFree(p);
      p = nullptr;
      cap = 0;
      if (hipMalloc(&p, b + b / 8 + 4096) != hipSuccess) {
        p = nullptr;
        return false;
      }
      cap = b + b / 8 + 4096;
      return true;
    }
  } data, rows, hint;
  // pinned staging: reads of data files to the device, copies of results back to the host
  cask_host::PinnedRing ring;
  // open(): hint bodies back to the host while `ring` reads files in. Hint bodies are ~1/8 of the data
  // at most (22 + key bytes per record), so 4 threads' slots (256 MiB) are made, and only when the
  // first hint copy is large enough to be staged; if they cannot be made, cask_copy carries it.
  cask_host::PinnedRing ring_out;
  bool ring_out_tried = false, ring_out_ok = false;
  static constexpr int kOutThreads = 4;
  static constexpr int kReaders = cask_host::PinnedRing::kThreads;
  static constexpr size_t kSlotBytes = cask_host::PinnedRing::kBytes;
  cask_rows r{};

  // After a large open: the data, row and hint buffers go back to the device (they are sized for
  // the largest batch or stretch seen; kept only while small, for the next open or compaction).
  void trim();
  int prepare();

  // Reader thread t takes every kReaders-th 32-MiB piece of the files, alternating between its two
  // pinned slots: pread into one while the other's copy to the device is in flight.
  int read_to_device(const std::vector<std::string>& paths, const std::vector<cask_file_view>& v, std::vector<char>& ok);

  // Device -> pageable host copy, staged through the pinned slots when large (engine_dev.cpp)
  static bool staged(uint64_t n);
  int to_host(uint8_t* dst, const uint8_t* src, uint64_t n, cask_host::PinnedRing* rg = nullptr);

  // open() with the keydir built on the device: every batch's rows, appended in file order (the
  // block needs the rows of all the scanned files at once; the data files stay resident anyway)
  struct AllRows {
    uint8_t* p = nullptr;
    uint64_t cap = 0, n = 0;
    ~AllRows() {
      if (p) (void)hipFree(p);
    }
    cask_rows view() const {
      cask_rows r = carve_rows(p, cap);
      r.count = n;
      return r;
    }
    // rows [0, m) of `src` after the n already here (the buffer grows by half again when short)
    int append(const cask_rows& src, uint64_t m, hipStream_t st);
  };

  // Device rows sized from a guess (average record >= 48 B), once more at the exact count if short.
  int scan(const std::vector<cask_file_view>& v, std::vector<uint64_t>& row_off, cask_scan_error& se);

  // The hint bodies of the scanned files v (rows of the last scan) into hbuf, file k's at
  // [fo[k], fo[k + 1]); copied back through ring_out (open() reads the next files through `ring`).
  int hints(const std::vector<cask_file_view>& v, const std::vector<uint64_t>& row_off, RawBytes& hbuf,
            std::vector<uint64_t>& fo);

  // The rows of the files v reduced on the device to one keydir block (cask_shard_keydir; rows parsed
  // from hint bodies: cask_shard_keydir_hints) and brought to the host: alloc(bytes) gives the
  // block's place (nullptr: CASK_E_NOMEM). *nb is the block's size; ms2, when given, takes the time
  // of the reduction and of the copy.
  int block_to_host(bool from_hints, const std::vector<cask_file_view>& v, const cask_rows& rows,
                    const std::vector<uint64_t>& roff, const std::function<uint8_t*(uint64_t)>& alloc, uint64_t* nb,
                    double* ms2 = nullptr);
};

EngineDev* engine_dev(int device);

}  // namespace cask_engine

// The engine's files: Log::open's path checks and find_data_files (log.rs:36-85, 483-510), the file
// names (log.rs:473-481), whole-file reads and writes, and the hint file (log.rs:121-135, 432-447,
// 512-539; data.rs:242-276): its validity test, the walk over its records and its writer
// (HintWriter::drop, log.rs:389-395).
#pragma once
#include <sys/mman.h>

#include <cstdint>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "keydir_host.h"

CASK_ENGINE_NAMESPACE {

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

bool is_dir(const std::string& p);
bool exists(const std::string& p);
bool is_file_follow(const std::string& p);  // Path::is_file (follows symlinks)
std::string data_path(const std::string& dir, uint32_t id);  // log.rs:473-476
std::string hint_path(const std::string& dir, uint32_t id);  // log.rs:478-481
// a hint file's temporary name while the ranges of a multi-device open are still running
inline std::string part_path(const std::string& hp) { return hp + ".part"; }
void remove_gone_files(const std::string& dir);
bool find_data_files(const std::string& dir, std::vector<uint32_t>& out);

// Every byte of [p, p + n) to fd (at its position; at offset `at`), EINTR retried; false on an error.
bool write_all(int fd, const uint8_t* p, uint64_t n);
bool pwrite_all(int fd, const uint8_t* p, uint64_t n, uint64_t at);
// Up to n bytes from fd into p, EINTR retried, until the file ends: the bytes read, or -1 on an error.
int64_t read_all(int fd, uint8_t* p, uint64_t n);

// A host byte buffer that is not zero-filled (a std::vector<uint8_t> of the hint bodies would write
// every byte once more before the copy from the device overwrites it).
struct RawBytes {
  std::unique_ptr<uint8_t[]> p;
  uint64_t n = 0;
  bool resize(uint64_t b) {
    p.reset(b ? new (std::nothrow) uint8_t[b] : nullptr);
    n = p || !b ? b : 0;
    return p || !b;
  }
  uint8_t* data() { return p.get(); }
  const uint8_t* data() const { return p.get(); }
  uint64_t size() const { return n; }
  bool empty() const { return n == 0; }
};

// A host buffer of anonymous memory advised to huge pages (2 MiB faults instead of 4-KiB ones when a
// multi-GiB batch is first written), unmapped when dropped.
struct HostBuf {
  uint8_t* p = nullptr;
  size_t n = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept : p(o.p), n(o.n) {
    o.p = nullptr;
    o.n = 0;
  }
  HostBuf& operator=(HostBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p;
      n = o.n;
      o.p = nullptr;
      o.n = 0;
    }
    return *this;
  }
  ~HostBuf() { reset(); }
  void reset() {
    if (p) munmap(p, n);
    p = nullptr;
    n = 0;
  }
  bool alloc(size_t bytes) {
    reset();
    void* q = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (q == MAP_FAILED) return false;
    (void)madvise(q, bytes, MADV_HUGEPAGE);
    p = (uint8_t*)q;
    n = bytes;
    return true;
  }
  uint8_t* get() const { return p; }
};

// A whole file into a HostBuf (no zero fill before the read, huge pages); false on an I/O error.
bool read_file_buf(const std::string& p, HostBuf& out, uint64_t& len);

// A hint file: body + XXH32 trailer (HintWriter::drop, log.rs:389-395), created/truncated
// (util.rs:45-49), two write(2)s and no copy of the body.
bool write_hint_file(const std::string& p, const uint8_t* body, uint64_t n);

// is_valid_hint_file (log.rs:512-539): a regular file of at least 4 bytes whose trailer is the
// XXH32 of the bytes before it. On success buf holds the file and len its length (the body is
// buf[0, len - 4): Take(size - 4), log.rs:129); otherwise buf is released and len is 0.
bool load_valid_hint(const std::string& p, HostBuf& buf, uint64_t& len);

// The 22-byte header of a hint record (Hint::write_bytes, data.rs:242-256); its key follows it.
inline void wr_hint_header(uint8_t* h, uint64_t seq, uint16_t ksz, uint32_t vsz_raw, uint64_t pos) {
  wr64(h, seq);
  wr16(h + 8, ksz);
  wr32(h + 10, vsz_raw);
  wr64(h + 14, pos);
}

// Hints::next / Hint::from_read over a hint body (log.rs:437-447; data.rs:258-276): fn(offset, ksz)
// for every whole record (22-byte header + key) in order. Returns the offset of the first record cut
// short, or UINT64_MAX when the body ends on a record boundary.
template <class F>
inline uint64_t walk_hint_body(const uint8_t* b, uint64_t n, F&& fn) {
  for (uint64_t p = 0; p < n;) {
    if (n - p < 22) return p;
    const uint16_t k = rd16(b + p + 8);
    if (n - p - 22 < k) return p;
    fn(p, k);
    p += 22ull + k;
  }
  return UINT64_MAX;
}

// The fold's sources of one file's hint body: pieces of kFoldPiece whole records, appended to
// `out`. Returns what walk_hint_body returns (the pieces end before a record cut short); *max_seq,
// when given, is raised to the highest sequence walked.
inline uint64_t hint_fold_sources(const uint8_t* b, uint64_t n, uint32_t file_id, std::vector<FoldSrc>& out,
                                  uint64_t* max_seq = nullptr) {
  uint64_t p0 = 0, k = 0, ms = 0;
  const bool seq = max_seq != nullptr;
  const uint64_t bad = walk_hint_body(b, n, [&](uint64_t p, uint16_t) {
    if (k == kFoldPiece) {
      out.push_back(FoldSrc{b + p0, p - p0, k, file_id});
      p0 = p;
      k = 0;
    }
    if (seq) ms = std::max(ms, rd64(b + p));
    ++k;
  });
  if (k) out.push_back(FoldSrc{b + p0, (bad == UINT64_MAX ? n : bad) - p0, k, file_id});
  if (seq && ms > *max_seq) *max_seq = ms;
  return bad;
}

}  // namespace cask_engine

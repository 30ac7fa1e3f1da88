// EngineDev (engine_dev.h): the data files read straight to the device, the device scan, the hint
// bodies and the keydir block copied back to the host.
#include "engine_dev.h"

#include <fcntl.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <new>

#include "engine_db.h"
#include "knobs.h"

CASK_ENGINE_NAMESPACE {

void EngineDev::trim() {
  constexpr size_t kKeep = 4ull << 30;
  (void)hipSetDevice(device);
  for (Buf* b : {&data, &rows, &hint})
    if (b->cap > kKeep) {
      (void)hipFree(b->p);
      b->p = nullptr;
      b->cap = 0;
    }
}

int EngineDev::prepare() {
  if (hipSetDevice(device) != hipSuccess) return CASK_E_DEVICE;
  if (!ctx) {
    int st = CASK_OK;
    ctx = cask_ctx_create(device, &st);
    if (!ctx) return st;
  }
  return ring.init(device) ? CASK_OK : CASK_E_NOMEM;
}

int EngineDev::read_to_device(const std::vector<std::string>& paths, const std::vector<cask_file_view>& v, std::vector<char>& ok) {
  struct Piece {
    uint32_t f;
    uint64_t off, n;
  };
  std::vector<Piece> pieces;
  for (uint32_t f = 0; f < v.size(); ++f)
    for (uint64_t o = 0; o < v[f].len; o += kSlotBytes) pieces.push_back(Piece{f, o, std::min<uint64_t>(kSlotBytes, v[f].len - o)});
  // CASK_OPEN_READERS (tuning knob): reader threads, at most kReaders (default: the host threads)
  static const unsigned readers = cask_knobs::tune("CASK_OPEN_READERS") ? (unsigned)atoi(cask_knobs::tune("CASK_OPEN_READERS")) : 0u;
  const unsigned want = readers ? std::min<unsigned>(readers, (unsigned)kReaders) : (unsigned)kReaders;
  const unsigned nt = std::max(1u, std::min(want, host_lanes(pieces.size())));
  std::vector<int> status(nt, CASK_OK);
  parallel_for(nt, [&](unsigned t) {
    if (hipSetDevice(device) != hipSuccess) {
      status[t] = CASK_E_DEVICE;
      return;
    }
    std::vector<int> fds(v.size(), -1);
    unsigned k = 0;
    for (size_t j = t; j < pieces.size(); j += nt, k ^= 1) {
      const Piece& pc = pieces[j];
      if (!ok[pc.f]) continue;
      if (fds[pc.f] < 0 && (fds[pc.f] = open(paths[pc.f].c_str(), O_RDONLY)) < 0) {
        ok[pc.f] = 0;
        continue;
      }
      if (hipEventSynchronize(ring.ev[t][k]) != hipSuccess) {
        status[t] = CASK_E_DEVICE;
        break;
      }
      uint64_t got = 0;
      while (got < pc.n) {
        const ssize_t m = pread(fds[pc.f], (uint8_t*)ring.pin[t][k] + got, pc.n - got, (off_t)(pc.off + got));
        if (m < 0 && errno == EINTR) continue;
        if (m <= 0) break;
        got += (uint64_t)m;
      }
      if (got != pc.n) {  // the file shrank or could not be read
        ok[pc.f] = 0;
        continue;
      }
      if (hipMemcpyAsync((uint8_t*)v[pc.f].data + pc.off, ring.pin[t][k], pc.n, hipMemcpyHostToDevice, ring.rs[t]) != hipSuccess ||
          hipEventRecord(ring.ev[t][k], ring.rs[t]) != hipSuccess) {
        status[t] = CASK_E_DEVICE;
        break;
      }
    }
    for (int fd : fds)
      if (fd >= 0) close(fd);
    if (hipStreamSynchronize(ring.rs[t]) != hipSuccess) status[t] = CASK_E_DEVICE;
  });
  for (int s : status)
    if (s != CASK_OK) return s;
  return CASK_OK;
}

// Device -> pageable host copy staged through the pinned slots: threads take every nt-th 32-MiB
// piece (CASK_STAGE_MIN=0 stages every copy: the tests run the small cases through it), the DMA of one piece into a slot overlapping the host copy of the previous piece out of
// the other (a copy to pageable memory straight from the device runs at ~10 GB/s). Small copies
// take cask_copy. The device work that produced `src` (on the context's stream) is waited for first.
bool EngineDev::staged(uint64_t n) {
  const char* mv = cask_knobs::hook("CASK_STAGE_MIN");  // test knob: smallest copy staged (default 64 MiB)
  return n && n >= (mv ? strtoull(mv, nullptr, 10) : (64ull << 20));
}
int EngineDev::to_host(uint8_t* dst, const uint8_t* src, uint64_t n, cask_host::PinnedRing* rg) {
  if (!staged(n)) return cask_copy(ctx, dst, src, n);
  if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize((hipStream_t)cask_ctx_stream(ctx)) != hipSuccess)
    return CASK_E_DEVICE;
  std::vector<cask_host::PinnedRing::Piece> ps;
  cask_host::PinnedRing::split(dst, (uint8_t*)src, n, ps);
  return (rg ? rg : &ring)->d2h(ps) ? CASK_OK : CASK_E_DEVICE;
}

// rows [0, m) of `s` to rows [at, at + m) of `d`, column by column, waited for
static bool copy_rows(const cask_rows& d, uint64_t at, const cask_rows& s, uint64_t m, hipStream_t st) {
  return hipMemcpyAsync(d.pos + at, s.pos, 8 * m, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d.seq + at, s.seq, 8 * m, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d.vsz + at, s.vsz, 4 * m, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d.ksz + at, s.ksz, 2 * m, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipMemcpyAsync(d.status + at, s.status, m, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipStreamSynchronize(st) == hipSuccess;
}

int EngineDev::AllRows::append(const cask_rows& src, uint64_t m, hipStream_t st) {
  if (n + m > cap) {
    const uint64_t nc = std::max<uint64_t>(n + m, cap + cap / 2);
    uint8_t* q = nullptr;
    if (hipMalloc(&q, rows_bytes(nc)) != hipSuccess) return CASK_E_NOMEM;
    AllRows grown;
    grown.p = q;
    grown.cap = nc;
    if (n && !copy_rows(grown.view(), 0, view(), n, st)) return CASK_E_DEVICE;
    std::swap(p, grown.p);
    std::swap(cap, grown.cap);
  }
  if (m && !copy_rows(view(), n, src, m, st)) return CASK_E_DEVICE;
  n += m;
  return CASK_OK;
}

int EngineDev::scan(const std::vector<cask_file_view>& v, std::vector<uint64_t>& row_off, cask_scan_error& se) {
  uint64_t total = 0;
  for (const auto& f : v) total += f.len;
  const uint64_t bound = cask_rows_bound(v.data(), (uint32_t)v.size());
  uint64_t cap = std::min<uint64_t>(bound, total / 48 + v.size() + 1024);
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (!rows.ensure(rows_bytes(cap))) return CASK_E_NOMEM;
    r = carve_rows(rows.p, cap);
    const int st = cask_scan_device(ctx, v.data(), (uint32_t)v.size(), &r, row_off.data(), &se);
    if (st != CASK_E_CAPACITY) return st;
    cap = r.count;
  }
  return CASK_E_DEVICE;
}

int EngineDev::hints(const std::vector<cask_file_view>& v, const std::vector<uint64_t>& row_off, RawBytes& hbuf,
                     std::vector<uint64_t>& fo) {
  fo.assign(v.size() + 1, 0);
  int st = cask_hints_device(ctx, v.data(), (uint32_t)v.size(), &r, row_off.data(), nullptr, 0, fo.data());
  if (st != CASK_E_CAPACITY && st != CASK_OK) return st;
  if (!hint.ensure(fo[v.size()] + 256)) return CASK_E_NOMEM;
  st = cask_hints_device(ctx, v.data(), (uint32_t)v.size(), &r, row_off.data(), hint.p, hint.cap, fo.data());
  if (st != CASK_OK) return st;
  if (!hbuf.resize(fo[v.size()])) return CASK_E_NOMEM;
  if (hbuf.empty()) return CASK_OK;
  if (staged(hbuf.size()) && !ring_out_tried) {
    ring_out_tried = true;
    ring_out_ok = ring_out.init(device, kOutThreads);
    if (!ring_out_ok) ring_out.release();
  }
  if (staged(hbuf.size()) && !ring_out_ok) return cask_copy(ctx, hbuf.data(), hint.p, hbuf.size());
  return to_host(hbuf.data(), hint.p, hbuf.size(), &ring_out) != CASK_OK ? CASK_E_DEVICE : CASK_OK;
}

int EngineDev::block_to_host(bool from_hints, const std::vector<cask_file_view>& v, const cask_rows& rows,
                             const std::vector<uint64_t>& roff, const std::function<uint8_t*(uint64_t)>& alloc,
                             uint64_t* nb, double* ms2) {
  const auto tb = std::chrono::steady_clock::now();
  const void* blk = nullptr;
  *nb = 0;
  cask_rows rw = rows;
  int st = from_hints ? cask_shard_keydir_hints(ctx, v.data(), (uint32_t)v.size(), &rw, roff.data(), &blk, nb)
                      : cask_shard_keydir(ctx, v.data(), (uint32_t)v.size(), &rw, roff.data(), &blk, nb);
  if (st != CASK_OK) return st;
  if (ms2) ms2[0] = ms_since(tb);
  const auto tc = std::chrono::steady_clock::now();
  uint8_t* dst = alloc(*nb);
  if (!dst) return CASK_E_NOMEM;
  st = to_host(dst, (const uint8_t*)blk, *nb);
  if (ms2) ms2[1] = ms_since(tc);
  return st;
}

EngineDev* engine_dev(int device) {
  static std::mutex mu;
  static EngineDev* devs[64] = {};
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  if (!devs[device]) {
    devs[device] = new (std::nothrow) EngineDev();
    if (devs[device]) devs[device]->device = device;
  }
  return devs[device];
}

}  // namespace cask_engine

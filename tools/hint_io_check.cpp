// Host memory-safety check of the engine's hint-file helpers (cask_amd/csrc/engine_io.h), built
// with the address and undefined-behaviour sanitizers on the host side and run on its own:
//   hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//     tools/hint_io_check.cpp cask_amd/csrc/engine_io.cpp -o /tmp/hint_io_check && /tmp/hint_io_check [dir]
// write_hint_file -> load_valid_hint -> walk_hint_body / hint_fold_sources over bodies of 0, 1,
// kFoldPiece and kFoldPiece + 1 records and bodies cut inside a header and inside a key; the counts,
// the offset of the short record and the piece boundaries are checked against values computed here.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../cask_amd/csrc/engine_io.h"
#include "../cask_amd/csrc/xxh32.h"

using namespace cask_engine;

static int failures = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      ++failures;                                                  \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
    }                                                              \
  } while (0)

// record i: key of 3 + i % 29 bytes, sequence i + 1; returns every record's offset (+ the end)
static std::vector<uint64_t> build(uint64_t nrec, std::vector<uint8_t>& body) {
  std::vector<uint64_t> off;
  body.clear();
  for (uint64_t i = 0; i < nrec; ++i) {
    const uint16_t k = (uint16_t)(3 + i % 29);
    off.push_back(body.size());
    uint8_t h[22];
    wr_hint_header(h, i + 1, k, (uint32_t)(i * 7), i * 100);
    body.insert(body.end(), h, h + 22);
    for (uint16_t j = 0; j < k; ++j) body.push_back((uint8_t)(i + j));
  }
  off.push_back(body.size());
  return off;
}

// the body written as a hint file, loaded back, walked and cut; `cut`: bytes dropped from its end
static void run_case(const std::string& dir, uint64_t nrec, uint64_t cut, const char* what) {
  std::vector<uint8_t> full;
  const std::vector<uint64_t> off = build(nrec, full);
  CHECK(cut <= full.size());
  const uint64_t n = full.size() - cut;
  // whole records that fit in n bytes, and where the short one starts
  uint64_t whole = 0;
  while (whole < nrec && off[whole + 1] <= n) ++whole;
  const uint64_t want_bad = off[whole] == n ? UINT64_MAX : off[whole];

  const std::string p = dir + "/0000000001.cask.hint";
  // (an exact-size heap copy: a read past the body's end is a sanitizer report)
  std::vector<uint8_t> exact(full.begin(), full.begin() + (ptrdiff_t)n);
  CHECK(write_hint_file(p, exact.data(), n));
  HostBuf buf;
  uint64_t len = 0;
  CHECK(load_valid_hint(p, buf, len));
  CHECK(len == n + 4);
  const uint8_t none = 0;
  CHECK(len < 4 || rd32(buf.get() + len - 4) == cask_xxh::xxh32(n ? exact.data() : &none, n, 0));
  CHECK(n == 0 || memcmp(buf.get(), exact.data(), n) == 0);

  uint64_t cnt = 0, last = UINT64_MAX;
  bool in_order = true;
  const uint64_t bad = walk_hint_body(exact.data(), n, [&](uint64_t at, uint16_t ksz) {
    in_order = in_order && cnt < nrec && at == off[cnt] && ksz == 3 + cnt % 29;
    last = at;
    ++cnt;
  });
  CHECK(in_order);
  CHECK(cnt == whole);
  CHECK(bad == want_bad);

  std::vector<FoldSrc> src;
  uint64_t max_seq = 0;
  CHECK(hint_fold_sources(exact.data(), n, 7, src, &max_seq) == want_bad);
  CHECK(max_seq == whole);  // (sequences are 1..nrec)
  CHECK(src.size() == (whole + kFoldPiece - 1) / kFoldPiece);
  uint64_t r = 0;
  for (size_t c = 0; c < src.size(); ++c) {
    const uint64_t k = std::min<uint64_t>(kFoldPiece, whole - r);
    CHECK(src[c].b == exact.data() + off[r]);
    CHECK(src[c].cnt == k);
    CHECK(src[c].n == off[r + k] - off[r]);
    CHECK(src[c].file_id == 7);
    r += k;
  }
  CHECK(r == whole);
  fprintf(stderr, "%-34s records %llu of %llu, bad %lld, pieces %zu\n", what, (unsigned long long)whole,
          (unsigned long long)nrec, (long long)bad, src.size());
  unlink(p.c_str());
}

int main(int argc, char** argv) {
  char tmpl[] = "/tmp/hint_io_check.XXXXXX";
  const std::string dir = argc > 1 ? argv[1] : (mkdtemp(tmpl) ? tmpl : ".");
  run_case(dir, 0, 0, "no records");
  run_case(dir, 1, 0, "one record");
  run_case(dir, kFoldPiece, 0, "kFoldPiece records");
  run_case(dir, kFoldPiece + 1, 0, "kFoldPiece + 1 records");
  // 5 records; the last has a key of 3 + 4 = 7 bytes: 29 bytes in all
  run_case(dir, 5, 29 - 1, "cut 1 byte into a header");
  run_case(dir, 5, 29 - 21, "cut 21 bytes into a header");
  run_case(dir, 5, 3, "cut inside a key");
  run_case(dir, kFoldPiece + 1, 2, "cut inside the key after a piece");

  // files that are not valid hint files: absent, shorter than a trailer, a wrong trailer
  HostBuf buf;
  uint64_t len = 1;
  CHECK(!load_valid_hint(dir + "/absent.hint", buf, len) && len == 0 && !buf.get());
  const std::string p = dir + "/bad.hint";
  const uint8_t three[3] = {1, 2, 3};
  FILE* f = fopen(p.c_str(), "wb");
  CHECK(f && fwrite(three, 1, 3, f) == 3);
  if (f) fclose(f);
  CHECK(!load_valid_hint(p, buf, len) && len == 0 && !buf.get());
  std::vector<uint8_t> body;
  build(3, body);
  CHECK(write_hint_file(p, body.data(), body.size()));
  f = fopen(p.c_str(), "r+b");
  CHECK(f && fputc(body[0] ^ 1, f) != EOF);
  if (f) fclose(f);
  CHECK(!load_valid_hint(p, buf, len) && len == 0 && !buf.get());
  unlink(p.c_str());
  if (argc <= 1) rmdir(dir.c_str());
  fprintf(stderr, failures ? "FAILED: %d checks\n" : "ok\n", failures);
  return failures ? 1 : 0;
}

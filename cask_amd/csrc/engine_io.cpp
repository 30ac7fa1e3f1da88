// The engine's files (engine_io.h): path checks, file names, find_data_files (log.rs:483-510),
// whole-file reads and writes, the hint file's validity test and writer.
#include "engine_io.h"

#include <dirent.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <regex>

#include "xxh32.h"

CASK_ENGINE_NAMESPACE {

bool is_dir(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}
bool exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0;
}
bool is_file_follow(const std::string& p) {  // Path::is_file (follows symlinks)
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

std::string data_path(const std::string& dir, uint32_t id) {  // log.rs:473-476
  char b[32];
  snprintf(b, sizeof(b), "%010u.cask.data", id);
  return dir + "/" + b;
}
std::string hint_path(const std::string& dir, uint32_t id) {  // log.rs:478-481
  char b[32];
  snprintf(b, sizeof(b), "%010u.cask.hint", id);
  return dir + "/" + b;
}

bool write_all(int fd, const uint8_t* p, uint64_t n) {
  while (n) {
    const ssize_t w = write(fd, p, n);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    p += w;
    n -= (uint64_t)w;
  }
  return true;
}

bool pwrite_all(int fd, const uint8_t* p, uint64_t n, uint64_t at) {
  while (n) {
    const ssize_t w = pwrite(fd, p, n, (off_t)at);
    if (w < 0 && errno == EINTR) continue;
    if (w <= 0) return false;
    p += w;
    at += (uint64_t)w;
    n -= (uint64_t)w;
  }
  return true;
}

int64_t read_all(int fd, uint8_t* p, uint64_t n) {
  uint64_t got = 0;
  while (got < n) {
    const ssize_t r = read(fd, p + got, n - got);
    if (r < 0 && errno == EINTR) continue;
    if (r < 0) return -1;
    if (r == 0) break;
    got += (uint64_t)r;
  }
  return (int64_t)got;
}

// find_data_files (log.rs:483-510): regex "(\d+).cask.data$" (unescaped '.', unanchored),
// regular files only (DirEntry::metadata does not follow symlinks), u32 parse, ascending.
// Files a compaction renamed away (`<id>.cask.data.gone`, `<id>.cask.hint.gone`: no longer
// matched by find_data_files) are unlinked by the db's reclaim thread; a process that ended before
// that thread ran leaves them behind. Log::open removes them once it holds the lock (no compaction
// of this database can be running then). Not in the reference, whose swap_files removes the
// compacted files itself (log.rs:198-217).
void remove_gone_files(const std::string& dir) {
  DIR* d = opendir(dir.c_str());
  if (!d) return;
  std::vector<std::string> dead;
  auto ends = [](const std::string& n, const char* suf) {
    const size_t k = strlen(suf);
    return n.size() > k && n.compare(n.size() - k, k, suf) == 0;
  };
  while (struct dirent* e = readdir(d)) {
    const std::string name = e->d_name;
    if (ends(name, ".cask.data.gone") || ends(name, ".cask.hint.gone")) dead.push_back(dir + "/" + name);
  }
  closedir(d);
  for (const std::string& f : dead) (void)unlink(f.c_str());
}

bool find_data_files(const std::string& dir, std::vector<uint32_t>& out) {
  DIR* d = opendir(dir.c_str());
  if (!d) return false;
  static const std::regex re("(\\d+).cask.data$");
  while (struct dirent* e = readdir(d)) {
    std::string name = e->d_name;
    std::string full = dir + "/" + name;
    struct stat st;
    if (lstat(full.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) continue;
    std::smatch m;
    if (!std::regex_search(name, m, re)) continue;
    const std::string digits = m[1].str();
    // str::parse::<u32>: overflow -> Err -> skipped
    uint64_t v = 0;
    bool okp = true;
    for (char ch : digits) {
      v = v * 10 + (uint64_t)(ch - '0');
      if (v > 0xFFFFFFFFull) {
        okp = false;
        break;
      }
    }
    if (okp) out.push_back((uint32_t)v);
  }
  closedir(d);
  std::sort(out.begin(), out.end());
  return true;
}

bool write_hint_file(const std::string& p, const uint8_t* body, uint64_t n) {
  const int fd = open(p.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
  if (fd < 0) return false;
  uint8_t t[4];
  if (!body) body = t;  // (an empty body may come as a null pointer: no arithmetic on it)
  wr32(t, cask_xxh::xxh32(body, n, 0));
  const bool ok = write_all(fd, body, n) && write_all(fd, t, 4);
  close(fd);
  return ok;
}

bool read_file_buf(const std::string& p, HostBuf& out, uint64_t& len) {
  len = 0;
  const int fd = open(p.c_str(), O_RDONLY);
  if (fd < 0) return false;
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    return false;
  }
  if (!out.alloc(std::max<size_t>((size_t)st.st_size, 1))) {
    close(fd);
    throw std::bad_alloc();  // (mapping refused: the entry point's handler reports CASK_E_NOMEM)
  }
  const int64_t got = read_all(fd, out.get(), (uint64_t)st.st_size);
  close(fd);
  if (got < 0) return false;
  len = (uint64_t)got;
  return true;
}

bool load_valid_hint(const std::string& p, HostBuf& buf, uint64_t& len) {
  if (is_file_follow(p) && read_file_buf(p, buf, len) && len >= 4 &&
      cask_xxh::xxh32(buf.get(), len - 4, 0) == rd32(buf.get() + len - 4))
    return true;
  buf.reset();
  len = 0;
  return false;
}

}  // namespace cask_engine


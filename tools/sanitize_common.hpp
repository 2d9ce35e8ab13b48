// What the stand-alone host sanitizer programs (tools/*_sanitize.hip) share: the stubs for what
// the library's other files define, the fixed-seed generator, exact-size heap arrays, a file's
// bytes, and the loop over mutated windows of a text.  Included after the .hip or .hpp under test.
#pragma once

#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

void avdb_set_error(const char*, ...) {}
namespace avdb {
int text_line_starts(const uint8_t*, size_t, size_t, void*, uint64_t*, hipStream_t) { return AVDB_EHIP; }
}  // namespace avdb

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;  // xorshift64, fixed seed
static uint64_t rnd() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return g_seed;
}

// n entries and not one more, so a read or write outside them is reported
template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

[[maybe_unused]] static size_t count_lines(const uint8_t* t, size_t n) {
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) k += t[i] == '\n';
  return k + (n && t[n - 1] != '\n');
}

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> text;
  FILE* f = fopen(path, "rb");
  if (!f) {
    fprintf(stderr, "cannot read %s\n", path);
    exit(2);
  }
  uint8_t buf[65536];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.insert(text.end(), buf, buf + n);
  fclose(f);
  return text;
}

// `mutations` times: a window of the text (so a mutation costs little) with up to 11 bytes
// overwritten by bad[0 .. n_bad), and its line count, every fourth time one that is too large or
// too small; fn(m, window, bytes, n_lines) returns whether the run was accepted.  Returns how
// many were.
template <class F>
[[maybe_unused]] static long mutate_windows(const std::vector<uint8_t>& text, long mutations, const uint8_t* bad,
                                            size_t n_bad, F fn) {
  long ok = 0;
  for (long m = 0; m < mutations; ++m) {
    const size_t len = text.size() < 4096 ? text.size() : 1 + rnd() % 4096;
    const size_t at = text.size() > len ? rnd() % (text.size() - len) : 0;
    std::vector<uint8_t> t(text.begin() + at, text.begin() + at + len);
    for (int k = int(rnd() % 12); k > 0 && len; --k) t[rnd() % len] = bad[rnd() % n_bad];
    size_t n_lines = count_lines(t.data(), t.size());
    if (rnd() % 4 == 0) n_lines = rnd() % (t.size() + 2);  // (more lines than bytes is refused)
    ok += fn(m, t.data(), t.size(), n_lines);
  }
  return ok;
}

// K12's host entries and the per-line code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_existing.hip, avdb_existing.hpp) under the host sanitizers:
// a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/existing_sanitize.hip -o existing_sanitize
//   ./existing_sanitize export.tsv [mutations]
//
// The export goes through avdb_existing_size_host and avdb_existing_write_host from a
// heap copy of exactly its size into arrays of exactly n_lines entries and blobs of
// exactly the totals, so a read or write one byte outside any of them is reported.
// Then, from a fixed seed: copies of the text with bytes overwritten by tabs, carriage
// returns, newlines, quotes and high bytes, with a line count that is too large or too
// small, and with the length arrays and row offsets overwritten between the passes.
// Any return code is fine, any sanitizer report is not.  Exit status 0 and a last line
// "clean" when done.
#include "../annotatedvdb_amd/csrc/avdb_existing.hip"

#include "sanitize_common.hpp"

// both passes over text[0, bytes) with n_lines as given; hostile: overwrite some
// lengths / offsets between the passes.  Returns the write pass's return code.
static int run(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, bool hostile, uint64_t* rows_out) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto kl = exact<uint32_t>(n_lines), pl = exact<uint32_t>(n_lines), fl = exact<uint32_t>(n_lines);
  auto flags = exact<uint8_t>(n_lines);
  auto row_off = exact<uint64_t>(n_lines);
  uint64_t counts[AVDB_EXIST_N_COUNTS];
  int rc = avdb_existing_size_host(ctx, text.get(), bytes, n_lines, uint32_t(rnd() % 4 ? ~0u : rnd()), kl.get(), pl.get(),
                                   fl.get(), flags.get(), row_off.get(), counts);
  if (rc) return rc;
  const size_t rows = counts[AVDB_EXIST_COUNT_ROWS];
  *rows_out = rows;
  if (hostile)
    for (size_t k = 0; k < rows; ++k) {
      if (rnd() % 8 == 0) kl[k] = uint32_t(rnd() % 300);
      if (rnd() % 8 == 0) pl[k] = uint32_t(rnd() % 300);
      if (rnd() % 8 == 0) fl[k] = uint32_t(rnd() % 400);
      if (rnd() % 16 == 0) row_off[k] = rnd() % 3 ? rnd() % (bytes + 64) : rnd();
      if (rnd() % 16 == 0) flags[k] ^= 1;
    }
  uint64_t tot[3] = {0, 0, 0};
  for (size_t k = 0; k < rows; ++k) {
    tot[0] += kl[k];
    tot[1] += pl[k];
    tot[2] += fl[k];
  }
  auto keys = exact<uint64_t>((tot[0] + 7) / 8), pks = exact<uint64_t>((tot[1] + 7) / 8), frag = exact<uint64_t>((tot[2] + 7) / 8);
  auto ko = exact<uint64_t>(rows + 1), po = exact<uint64_t>(rows + 1), fo = exact<uint64_t>(rows + 1);
  uint64_t totals[4];
  return avdb_existing_write_host(ctx, text.get(), bytes, n_lines, rows, kl.get(), pl.get(), fl.get(), flags.get(),
                                  row_off.get(), reinterpret_cast<uint8_t*>(keys.get()), tot[0], ko.get(),
                                  reinterpret_cast<uint8_t*>(pks.get()), tot[1], po.get(),
                                  reinterpret_cast<uint8_t*>(frag.get()), tot[2], fo.get(), totals);
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s export.tsv [mutations]\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> text = read_file(argv[1]);
  const long mutations = argc > 2 ? atol(argv[2]) : 2000;
  avdb_ctx ctx_store{};
  const avdb_ctx* ctx = &ctx_store;
  uint64_t rows = 0;
  int rc = run(ctx, text.data(), text.size(), count_lines(text.data(), text.size()), false, &rows);
  printf("export: %zu bytes, %llu rows, rc %d\n", text.size(), (unsigned long long)rows, rc);
  if (rc) return 1;
  const uint8_t bad[] = {'\t', '\r', '\n', '\'', '\\', 0x01, 0x7f, 0xc3, ':', 0};
  const long ok = mutate_windows(text, mutations, bad, sizeof bad,
                                 [&](long m, const uint8_t* t, size_t bytes, size_t n_lines) {
    return run(ctx, t, bytes, n_lines, m % 2 == 1, &rows) == 0;
                                 });
  printf("%ld mutations, %ld with rc 0\nclean\n", mutations, ok);
  return 0;
}

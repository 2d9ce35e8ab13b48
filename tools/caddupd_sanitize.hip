// K13's host entries and the per-line code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_caddupd.hip, avdb_caddupd.hpp) under the host sanitizers:
// a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/caddupd_sanitize.hip -o caddupd_sanitize
//   ./caddupd_sanitize snv.tsv indel.tsv export.tsv [mutations]
//
// The two CADD texts become tables (avdb_cadd_table_build_host) in arrays of exactly
// their row counts; the export goes through avdb_cadd_update_size_host and
// avdb_cadd_update_write_host from a heap copy of exactly its size into arrays of
// exactly n_lines entries and an output of exactly the total, so a read or write one
// byte outside any of them is reported.  Then, from a fixed seed: copies of the text
// with bytes overwritten by tabs, colons, carriage returns, newlines, digits and high
// bytes, with a line count that is too large or too small, with and without a
// chromosome text, and with the row arrays overwritten between the passes; and
// avdb_cadd_score_text_host over mutated score texts.  Any return code is fine, any
// sanitizer report is not.  Exit status 0 and a last line "clean" when done.
#include "../annotatedvdb_amd/csrc/avdb_cadd.hip"
#include "../annotatedvdb_amd/csrc/avdb_caddupd.hip"

#include "sanitize_common.hpp"

// a table in arrays of exactly its rows
struct Table {
  std::unique_ptr<uint8_t[]> text, chrom, flags;
  std::unique_ptr<uint32_t[]> pos, ref_len, alt_len, first_row, end_row;
  std::unique_ptr<uint64_t[]> ref_off, alt_off;
  std::unique_ptr<double[]> raw, phred;
  avdb_cadd_table view;
};

static void build_table(const avdb_ctx* ctx, const std::vector<uint8_t>& src, Table* t) {
  const size_t n = count_lines(src.data(), src.size());
  auto chrom = exact<uint8_t>(n), flags = exact<uint8_t>(n);
  auto pos = exact<uint32_t>(n), rl = exact<uint32_t>(n), al = exact<uint32_t>(n);
  auto ro = exact<uint64_t>(n), ao = exact<uint64_t>(n);
  auto raw = exact<double>(n), phred = exact<double>(n);
  t->text = exact<uint8_t>(src.size());
  memcpy(t->text.get(), src.data(), src.size());
  t->first_row = exact<uint32_t>(AVDB_CADD_N_CONTIGS);
  t->end_row = exact<uint32_t>(AVDB_CADD_N_CONTIGS);
  uint64_t counts[AVDB_CADD_N_COUNTS];
  if (avdb_cadd_table_build_host(ctx, t->text.get(), src.size(), n, chrom.get(), pos.get(), ro.get(), rl.get(), ao.get(),
                                 al.get(), raw.get(), phred.get(), flags.get(), t->first_row.get(), t->end_row.get(),
                                 counts))
    exit(1);
  const size_t rows = counts[AVDB_CADD_COUNT_ROWS];
  auto shrink = [&](auto& dst, auto& from) {
    typedef typename std::remove_reference<decltype(from[0])>::type T;
    dst = exact<T>(rows);
    memcpy(dst.get(), from.get(), rows * sizeof(T));
  };
  shrink(t->chrom, chrom);
  shrink(t->flags, flags);
  shrink(t->pos, pos);
  shrink(t->ref_len, rl);
  shrink(t->alt_len, al);
  shrink(t->ref_off, ro);
  shrink(t->alt_off, ao);
  shrink(t->raw, raw);
  shrink(t->phred, phred);
  t->view = avdb_cadd_table{sizeof(avdb_cadd_table), 0, rows, t->text.get(), src.size(), t->chrom.get(), t->pos.get(),
                            t->ref_off.get(), t->ref_len.get(), t->alt_off.get(), t->alt_len.get(), t->raw.get(),
                            t->phred.get(), t->flags.get(), t->first_row.get(), t->end_row.get()};
}

// both passes over text[0, bytes) with n_lines as given; hostile: overwrite some of the
// row arrays between the passes; fixed: both tables, every contig, no chromosome text.
// Returns the write pass's return code.
static int run(const avdb_ctx* ctx, const Table& snv, const Table& indel, const uint8_t* src, size_t bytes,
               size_t n_lines, bool hostile, uint64_t* rows_out, uint64_t* bytes_out, bool fixed = false) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto start = exact<uint64_t>(n_lines);
  auto pk = exact<uint32_t>(n_lines), len = exact<uint32_t>(n_lines);
  auto match = exact<int32_t>(n_lines);
  auto kind = exact<uint8_t>(n_lines), flags = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_CADDUPD_N_COUNTS];
  const char* chrom = !fixed && rnd() % 2 ? "chr21" : nullptr;
  const size_t chrom_len = chrom ? 5 : 0;
  const avdb_cadd_table* vs = fixed || rnd() % 8 ? &snv.view : nullptr;
  const avdb_cadd_table* vi = fixed || rnd() % 8 ? &indel.view : nullptr;
  int rc = avdb_cadd_update_size_host(ctx, text.get(), bytes, n_lines, vs, vi, chrom, chrom_len,
                                      uint32_t(fixed || rnd() % 4 ? ~0u : rnd()), uint32_t(fixed || rnd() % 2),
                                      start.get(), pk.get(),
                                      kind.get(), match.get(), len.get(), flags.get(), counts);
  if (rc) return rc;
  const size_t rows = counts[AVDB_CADDUPD_COUNT_ROWS];
  *rows_out = rows;
  if (hostile)
    for (size_t k = 0; k < rows; ++k) {
      if (rnd() % 8 == 0) pk[k] = uint32_t(rnd() % 300);
      if (rnd() % 8 == 0) len[k] = uint32_t(rnd() % 400);
      if (rnd() % 8 == 0) match[k] = int32_t(rnd() % 3 ? rnd() % 5000 : rnd());
      if (rnd() % 8 == 0) kind[k] = uint8_t(rnd() % 4);
      if (rnd() % 16 == 0) start[k] = rnd() % 3 ? rnd() % (bytes + 64) : rnd();
      if (rnd() % 16 == 0) flags[k] ^= uint8_t(1 + rnd() % 3);
    }
  uint64_t total = 0;
  for (size_t k = 0; k < rows; ++k) total += len[k];
  *bytes_out = total;
  auto out = exact<uint64_t>((total + 7) / 8);
  auto off = exact<uint64_t>(rows + 1);
  uint64_t totals[2];
  return avdb_cadd_update_write_host(ctx, text.get(), bytes, n_lines, rows, vs, vi, chrom, chrom_len, start.get(),
                                     pk.get(), kind.get(), match.get(), len.get(), flags.get(),
                                     reinterpret_cast<uint8_t*>(out.get()), total, off.get(), totals);
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s snv.tsv indel.tsv export.tsv [mutations]\n", argv[0]);
    return 2;
  }
  const long mutations = argc > 4 ? atol(argv[4]) : 2000;
  avdb_ctx ctx_store{};
  const avdb_ctx* ctx = &ctx_store;
  Table snv, indel;
  build_table(ctx, read_file(argv[1]), &snv);
  build_table(ctx, read_file(argv[2]), &indel);
  const std::vector<uint8_t> text = read_file(argv[3]);
  uint64_t rows = 0, bytes_out = 0;
  int rc = run(ctx, snv, indel, text.data(), text.size(), count_lines(text.data(), text.size()), false, &rows,
               &bytes_out, true);
  printf("tables: %llu + %llu rows; export: %zu bytes, %llu rows, %llu bytes out, rc %d\n",
         (unsigned long long)snv.view.n_rows, (unsigned long long)indel.view.n_rows, text.size(),
         (unsigned long long)rows, (unsigned long long)bytes_out, rc);
  if (rc) return 1;
  const uint8_t bad[] = {'\t', '\r', '\n', ':', ':', '\\', 'N', '0', '9', 'A', 0x01, 0xc3, 0};
  const long ok = mutate_windows(text, mutations, bad, sizeof bad,
                                 [&](long m, const uint8_t* t, size_t bytes, size_t n_lines) {
    return run(ctx, snv, indel, t, bytes, n_lines, m % 2 == 1, &rows, &bytes_out) == 0;
  });
  // the score rewrite alone: mutated score texts in a buffer of exactly their size
  const char* seeds[] = {"0.000012", "-12.345000", "000123456789012345", "0.0000000000000000000001", "-0", "1e-05"};
  const uint8_t sbad[] = {'0', '9', '.', '-', 'e', '+', ' ', 0};
  long handled = 0;
  for (long m = 0; m < mutations * 10; ++m) {
    const char* s = seeds[rnd() % 6];
    const size_t n = strlen(s) - rnd() % 2;
    auto p = exact<uint8_t>(n);
    memcpy(p.get(), s, n);
    for (int k = int(rnd() % 3); k > 0 && n; --k) p[rnd() % n] = sbad[rnd() % sizeof sbad];
    auto out = exact<uint8_t>(AVDB_CADDUPD_SCORE_MAX);
    size_t len = 0;
    handled += avdb_cadd_score_text_host(p.get(), n, out.get(), AVDB_CADDUPD_SCORE_MAX, &len) == 1;
  }
  printf("%ld mutations, %ld with rc 0; %ld score texts, %ld rendered\nclean\n", mutations, ok, mutations * 10, handled);
  return 0;
}

// K14's host entries and the per-line code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_expvcf.hip, avdb_expvcf.hpp) under the host sanitizers:
// a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/expvcf_sanitize.hip -o expvcf_sanitize
//   ./expvcf_sanitize export.tsv [mutations]
//
// The export goes through avdb_export_vcf_size_host and, once per stream,
// avdb_export_vcf_write_host from a heap copy of exactly its size into arrays of exactly
// n_lines entries and outputs of exactly the totals, so a read or write one byte outside
// any of them is reported.  Then, from a fixed seed: copies of windows of the text with
// bytes overwritten by tabs, colons, carriage returns, newlines, backslashes, the four
// invalid letters and high bytes, with a line count that is too large or too small, with
// contig masks, and with the row arrays and flags (ROW_HOST and DROPPED among them)
// overwritten between the passes.  Any return code is fine, any sanitizer report is not.
// Exit status 0 and a last line "clean" when done.
#include "../annotatedvdb_amd/csrc/avdb_expvcf.hip"

#include "sanitize_common.hpp"

// the size pass and both write passes over text[0, bytes) with n_lines as given; hostile:
// overwrite some of the row arrays between the passes; fixed: every contig.  Returns the
// first non-zero return code, or 0.
static int run(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, bool hostile, uint64_t* counts,
               bool fixed = false) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto start = exact<uint64_t>(n_lines), hash = exact<uint64_t>(n_lines), istart = exact<uint64_t>(n_lines);
  auto pk = exact<uint32_t>(n_lines), ms = exact<uint32_t>(n_lines), len = exact<uint32_t>(n_lines);
  auto ipk = exact<uint32_t>(n_lines), ilen = exact<uint32_t>(n_lines);
  auto flags = exact<uint8_t>(n_lines);
  int rc = avdb_export_vcf_size_host(ctx, text.get(), bytes, n_lines, uint32_t(fixed || rnd() % 4 ? ~0u : rnd()),
                                     start.get(), pk.get(), ms.get(), len.get(), flags.get(), hash.get(), istart.get(),
                                     ipk.get(), ilen.get(), counts);
  if (rc) return rc;
  const size_t nv = counts[AVDB_EXPVCF_COUNT_VALID], ni = counts[AVDB_EXPVCF_COUNT_INVALID];
  if (hostile) {
    for (size_t k = 0; k < nv; ++k) {
      if (rnd() % 8 == 0) pk[k] = uint32_t(rnd() % 300);
      if (rnd() % 8 == 0) ms[k] = uint32_t(rnd() % 3 ? rnd() % 300 : rnd());
      if (rnd() % 8 == 0) len[k] = uint32_t(rnd() % 400);
      if (rnd() % 16 == 0) start[k] = rnd() % 3 ? rnd() % (bytes + 64) : rnd();
      if (rnd() % 8 == 0) flags[k] ^= uint8_t(1 + rnd() % 7);
    }
    for (size_t k = 0; k < ni; ++k) {
      if (rnd() % 8 == 0) ipk[k] = uint32_t(rnd() % 3 ? rnd() % 300 : rnd());
      if (rnd() % 8 == 0) ilen[k] = uint32_t(rnd() % 400);
      if (rnd() % 16 == 0) istart[k] = rnd() % 3 ? rnd() % (bytes + 64) : rnd();
    }
  }
  uint64_t totals[2];
  {
    uint64_t total = 0;
    for (size_t k = 0; k < nv; ++k) total += len[k];
    auto out = exact<uint64_t>((total + 7) / 8);
    auto off = exact<uint64_t>(nv + 1);
    rc = avdb_export_vcf_write_host(ctx, text.get(), bytes, n_lines, AVDB_EXPVCF_STREAM_VCF, nv, start.get(), pk.get(),
                                    ms.get(), len.get(), flags.get(), reinterpret_cast<uint8_t*>(out.get()), total,
                                    off.get(), totals);
  }
  uint64_t total = 0;
  for (size_t k = 0; k < ni; ++k) total += ilen[k];
  auto out = exact<uint64_t>((total + 7) / 8);
  auto off = exact<uint64_t>(ni + 1);
  const int rc2 = avdb_export_vcf_write_host(ctx, text.get(), bytes, n_lines, AVDB_EXPVCF_STREAM_INVALID, ni,
                                             istart.get(), ipk.get(), nullptr, ilen.get(), nullptr,
                                             reinterpret_cast<uint8_t*>(out.get()), total, off.get(), totals);
  return rc ? rc : rc2;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s export.tsv [mutations]\n", argv[0]);
    return 2;
  }
  const long mutations = argc > 2 ? atol(argv[2]) : 2000;
  avdb_ctx ctx_store{};
  const avdb_ctx* ctx = &ctx_store;
  const std::vector<uint8_t> text = read_file(argv[1]);
  uint64_t counts[AVDB_EXPVCF_N_COUNTS];
  int rc = run(ctx, text.data(), text.size(), count_lines(text.data(), text.size()), false, counts, true);
  printf("export: %zu bytes, %llu valid and %llu invalid rows, %llu + %llu bytes out, rc %d\n", text.size(),
         (unsigned long long)counts[AVDB_EXPVCF_COUNT_VALID], (unsigned long long)counts[AVDB_EXPVCF_COUNT_INVALID],
         (unsigned long long)counts[AVDB_EXPVCF_COUNT_VCF_BYTES],
         (unsigned long long)counts[AVDB_EXPVCF_COUNT_INVALID_BYTES], rc);
  if (rc) return 1;
  const uint8_t bad[] = {'\t', '\t', '\r', '\n', ':', ':', '\\', 'N', 'I', 'R', 'D', '0', 'A', 0x01, 0xc3, 0};
  const long ok = mutate_windows(text, mutations, bad, sizeof bad,
                                 [&](long m, const uint8_t* t, size_t bytes, size_t n_lines) {
    return run(ctx, t, bytes, n_lines, m % 2 == 1, counts) == 0;
                                 });
  printf("%ld mutations, %ld with rc 0\nclean\n", mutations, ok);
  return 0;
}

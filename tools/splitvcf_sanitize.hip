// K15's host entries and the per-line code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_splitvcf.hip, avdb_splitvcf.hpp) under the host sanitizers:
// a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/splitvcf_sanitize.hip -o splitvcf_sanitize
//   ./splitvcf_sanitize [genome.vcf [mutations]]
//
// The built-in edge slabs (empty text, one line without a newline, comments only, every
// label and near-label, whitespace-only lines, keys of 300 bytes, the bytes the host
// decides at the stripped end and mid-line) and, when given, the file go through
// avdb_vcf_split_size_host and avdb_vcf_split_write_host, without and with a chromosome
// map, from a heap copy of exactly the text's size into arrays of exactly n_lines entries
// and an output of exactly the total, so a read or write one byte outside any of them is
// reported.  Then, from a fixed seed: copies of windows of the text with bytes overwritten
// by tabs, blanks, carriage returns, newlines, '#', label bytes and high bytes, with a line
// count that is too large or too small, and with the per-line arrays (codes outside
// 0..25, lengths, bit 31, starts past the text) overwritten between the passes.  Any
// return code is fine, any sanitizer report is not.  Exit status 0 and a last line "clean"
// when done.
#include "../annotatedvdb_amd/csrc/avdb_splitvcf.hip"

#include "sanitize_common.hpp"

#include <string>

// the host half of an avdb_chrom_map, filled as avdb_chrom_map_create fills it
static void make_map(avdb_chrom_map* m, const std::vector<std::string>& keys, const std::vector<uint8_t>& codes) {
  size_t slots = 16;
  while (slots < 2 * keys.size() + 2) slots <<= 1;
  m->device = -1;
  m->d_mem = nullptr;
  m->slot.assign(slots, 0);
  m->key_off.assign(1, 0);
  m->code = codes;
  for (const std::string& k : keys) {
    m->keys.insert(m->keys.end(), k.begin(), k.end());
    m->key_off.push_back(uint32_t(m->keys.size()));
  }
  m->keys.push_back(0);
  for (size_t k = 0; k < keys.size(); ++k) {
    const uint64_t h = fnv1a(m->keys.data() + m->key_off[k], m->key_off[k + 1] - m->key_off[k]);
    uint32_t q = uint32_t(h) & uint32_t(slots - 1);
    while (m->slot[q]) q = (q + 1) & uint32_t(slots - 1);
    m->slot[q] = ((h >> 24) << 24) | uint64_t(k + 1);
  }
}

// both passes over text[0, bytes) with n_lines as given; hostile: overwrite some of the
// per-line arrays between the passes.  Returns the first non-zero return code, or 0.
static int run(const avdb_ctx* ctx, const avdb_chrom_map* map, const uint8_t* src, size_t bytes, size_t n_lines,
               bool hostile, uint64_t* counts) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto code = exact<uint8_t>(n_lines);
  auto start = exact<uint64_t>(n_lines), dst = exact<uint64_t>(n_lines);
  auto len = exact<uint32_t>(n_lines);
  int rc = avdb_vcf_split_size_host(ctx, text.get(), bytes, n_lines, map, code.get(), start.get(), len.get(), counts);
  if (rc) return rc;
  if (hostile) {
    for (size_t k = 0; k < n_lines; ++k) {
      if (rnd() % 8 == 0) code[k] = uint8_t(rnd() % 3 ? rnd() % 27 : rnd());
      if (rnd() % 8 == 0) len[k] = uint32_t(rnd() % 400) | (rnd() % 4 ? 0u : AVDB_SPLIT_LINE_HOST);
      if (rnd() % 16 == 0) start[k] = rnd() % 3 ? rnd() % (bytes + 64) : rnd();
    }
  }
  uint64_t total = 0;
  for (size_t k = 0; k < n_lines; ++k) {
    const uint32_t ol = len[k] & ~AVDB_SPLIT_LINE_HOST;
    if (splitvcf::stream_of(code[k], ol) < splitvcf::kStreams) total += ol;
  }
  auto out = exact<uint8_t>(total);
  uint64_t stream_off[AVDB_SPLIT_N_STREAMS + 1], totals[2];
  rc = avdb_vcf_split_write_host(ctx, text.get(), bytes, n_lines, code.get(), start.get(), len.get(), out.get(), total,
                                 stream_off, rnd() % 2 ? dst.get() : nullptr, totals);
  if (rc == 0 && (totals[0] != total || stream_off[AVDB_SPLIT_N_STREAMS] != total)) {
    fprintf(stderr, "totals differ: %llu != %llu\n", (unsigned long long)totals[0], (unsigned long long)total);
    exit(1);
  }
  if (total) {  // one byte short: nothing may be written (the output is exactly total - 1 bytes)
    auto small = exact<uint8_t>(total - 1);
    if (avdb_vcf_split_write_host(ctx, text.get(), bytes, n_lines, code.get(), start.get(), len.get(), small.get(),
                                  total - 1, stream_off, nullptr, totals) != AVDB_ERANGE) {
      fprintf(stderr, "a short output was not refused\n");
      exit(1);
    }
  }
  return rc;
}

int main(int argc, char** argv) {
  const long mutations = argc > 2 ? atol(argv[2]) : 2000;
  avdb_ctx ctx_store{};
  const avdb_ctx* ctx = &ctx_store;
  avdb_chrom_map map;
  make_map(&map, {"NC_000001.11", "NC_000002.12", "NC_000023.11", "NC_012920.1", "7", "NT_187361.1", "", "J01415.2"},
           {0, 1, 22, 24, 6, 0xFF, 3, 0xFF});
  uint64_t counts[AVDB_SPLIT_N_COUNTS];

  std::vector<std::string> slabs = {"", "1\t5\trs1\tA\tC", "\n", "##a\n#b\t\n#\n", " \n\t\t\n \r\n\v\f\n\r\n   ",
                                    "X\t\t\t\n1\t \t\r\nY \n M\n", " #not a comment\n\t#nor this\n#comment\n# \n",
                                    std::string(300, 'K') + "\t1\n1\t2\n" + std::string(300, 'Z') + "\n",
                                    "1\t5\r\n2\t6\r\r\n#c\r\n3\t7\r", "NC_000001.11\t5\n7\t6\nNT_187361.1\t7\n\t8\nNC_1\t9"};
  std::string labels;
  for (const char* k : {"1", "2", "9", "10", "19", "20", "22", "X", "Y", "M", "0", "01", "23", "chr1", "MT", "x", "1 ", ""})
    labels += std::string(k) + "\t100\trs1\tA\tC\n";
  slabs.push_back(labels);
  for (const char* t : {"\x1c", "\x1d", "\x1e", "\x1f", "\xc2\x85", "\xc2\xa0", "\xff"}) {
    const std::string s(t);
    slabs.push_back("1\t5\tA" + s + "\n2\t7" + s + " \t\r\n" + s + "\n#c" + s + "\nchr1" + s);
    slabs.push_back("1\t5" + s + "A\n" + s + "2\t7\n1" + s + "\t9\n");
  }
  std::vector<uint8_t> text;
  for (const std::string& s : slabs) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(s.data());
    for (const avdb_chrom_map* m : {static_cast<const avdb_chrom_map*>(nullptr), static_cast<const avdb_chrom_map*>(&map)})
      if (run(ctx, m, p, s.size(), count_lines(p, s.size()), false, counts)) {
        fprintf(stderr, "an edge slab was refused\n");
        return 1;
      }
    text.insert(text.end(), p, p + s.size());
    text.push_back('\n');
  }
  printf("%zu edge slabs, each without and with a map\n", slabs.size());
  if (argc > 1) {
    text = read_file(argv[1]);
    const int rc = run(ctx, nullptr, text.data(), text.size(), count_lines(text.data(), text.size()), false, counts);
    printf("%s: %zu bytes, %llu comments, %llu unplaced lines, rc %d\n", argv[1], text.size(),
           (unsigned long long)counts[AVDB_SPLIT_COUNT_COMMENTS],
           (unsigned long long)counts[AVDB_SPLIT_COUNT_LINES + AVDB_SPLIT_OTHER], rc);
    if (rc) return 1;
  }
  const uint8_t bad[] = {'\t', '\t', ' ', '\r', '\n', '\n', '#', '1', '2', 'X', 'M', 'c', 0x1c, 0x1f, 0x85, 0xc2, 0xff, 0};
  const long ok = mutate_windows(text, mutations, bad, sizeof bad,
                                 [&](long m, const uint8_t* t, size_t bytes, size_t n_lines) {
    return run(ctx, m % 3 ? nullptr : &map, t, bytes, n_lines, m % 2 == 1, counts) == 0;
                                 });
  printf("%ld mutations, %ld with rc 0\nclean\n", mutations, ok);
  return 0;
}

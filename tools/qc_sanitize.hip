// K17's host entries and the per-line code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_qc.hip, avdb_qc.hpp, avdb_lof.hpp, avdb_keyset.hpp) under the host
// sanitizers: a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/qc_sanitize.hip -o qc_sanitize
//   ./qc_sanitize qc.vcf export.tsv [mutations]
//
// The VCF goes through avdb_qc_table_size_host and avdb_qc_table_write_host from a heap copy of
// exactly its size into arrays of exactly n_lines entries, then of exactly the rows, key bytes and
// JSON bytes counted; the keys, reversed, through avdb_keyset_build_host into a table of exactly
// avdb_keyset_workspace_size bytes; the export through avdb_qc_update_size_host and
// avdb_qc_update_write_host in the same way, so a read or write one byte outside any of them is
// reported.  Then, from a fixed seed: copies of both texts with bytes overwritten by tabs, colons,
// semicolons, equals signs, quotes, braces, brackets, signs, dots, carriage returns, newlines, digits
// and high bytes, with a line count that is too large or too small, with the entry and row arrays
// overwritten between the passes, and with releases of every length.  Any return code is fine, any
// sanitizer report is not.  Exit status 0 and a last line "clean" when done.
#include "../annotatedvdb_amd/csrc/avdb_keyset.hip"
#include "../annotatedvdb_amd/csrc/avdb_qc.hip"

#include "sanitize_common.hpp"

struct QcTable {
  std::unique_ptr<uint8_t[]> rkeys, json, hit, keyset, flags;
  std::unique_ptr<uint64_t[]> rkey_off, json_off;
  std::unique_ptr<uint32_t[]> json_len;
  std::vector<uint8_t> release;
  avdb_qc_table view;
  size_t rows = 0;
};

// both table passes over text[0, bytes) with n_lines as given; hostile: overwrite entry columns
// between the passes.  Returns whether a table came of it.
static bool run_table(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, bool hostile,
                      const std::vector<uint8_t>& release, QcTable* t) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto rel = exact<uint8_t>(release.size());
  if (!release.empty()) memcpy(rel.get(), release.data(), release.size());
  auto es = exact<uint64_t>(n_lines);
  auto ea = exact<uint32_t>(n_lines), ek = exact<uint32_t>(n_lines), ej = exact<uint32_t>(n_lines);
  auto ef = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_QC_N_COUNTS], totals[4];
  if (avdb_qc_table_size_host(ctx, text.get(), bytes, n_lines, rel.get(), release.size(), es.get(), ea.get(), ek.get(),
                              ej.get(), ef.get(), counts))
    return false;
  const size_t ne = counts[AVDB_QC_COUNT_ENTRIES];
  uint64_t n = counts[AVDB_QC_COUNT_ROWS], kb = counts[AVDB_QC_COUNT_KEY_BYTES], jb = counts[AVDB_QC_COUNT_JSON_BYTES];
  if (hostile && ne) {
    for (int k = 0; k < 4; ++k) {
      const size_t e = rnd() % ne;
      switch (rnd() % 5) {
        case 0: es[e] = rnd() % (bytes + 9); break;
        case 1: ea[e] = uint32_t(rnd() % 7); break;
        case 2: ek[e] = uint32_t(rnd() % 300); break;
        case 3: ej[e] = uint32_t(rnd() % 3000); break;
        default: ef[e] = uint8_t(rnd()); break;
      }
    }
    n = kb = jb = 0;
    for (size_t e = 0; e < ne; ++e) {
      n += ea[e];
      kb += ek[e];
      jb += ej[e];
    }
  }
  auto keys = exact<uint8_t>(kb), json = exact<uint8_t>(jb), rf = exact<uint8_t>(n);
  auto key_off = exact<uint64_t>(n + 1), jo = exact<uint64_t>(n), ls = exact<uint64_t>(n);
  auto jl = exact<uint32_t>(n);
  if (avdb_qc_table_write_host(ctx, text.get(), bytes, n_lines, ne, n, rel.get(), release.size(), es.get(), ea.get(),
                               ek.get(), ej.get(), ef.get(), keys.get(), kb, key_off.get(), json.get(), jb, jo.get(),
                               jl.get(), ls.get(), rf.get(), totals))
    return false;
  for (size_t r = 0; r < n; ++r)
    if (key_off[r + 1] < key_off[r] || key_off[r + 1] > kb) return false;
  t->rows = n;
  t->rkeys = exact<uint8_t>(kb);
  t->rkey_off = exact<uint64_t>(n + 1);
  t->json = std::move(json);
  t->json_off = std::move(jo);
  t->json_len = std::move(jl);
  t->flags = std::move(rf);
  t->hit = exact<uint8_t>(n);
  t->release = release;
  memset(t->hit.get(), 0, n);
  uint64_t at = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t r = n - 1 - i;
    const uint64_t len = key_off[r + 1] - key_off[r];
    t->rkey_off[i] = at;
    memcpy(t->rkeys.get() + at, keys.get() + key_off[r], len);
    at += len;
  }
  t->rkey_off[n] = at;
  size_t need = 0;
  avdb_keyset_workspace_size(n, &need);
  t->keyset = exact<uint8_t>(need);
  if (avdb_keyset_build_host(ctx, t->rkeys.get(), t->rkey_off.get(), n, t->keyset.get(), need)) return false;
  t->view = avdb_qc_table{sizeof(avdb_qc_table), uint32_t(t->release.size()), n, t->rkeys.get(), t->rkey_off.get(),
                          t->keyset.get(), need, t->json.get(), jb, t->json_off.get(), t->json_len.get(),
                          t->flags.get(), t->hit.get(), t->release.data()};
  return true;
}

static bool run_update(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, const QcTable& t,
                       bool hostile, uint32_t flags) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto rs = exact<uint64_t>(n_lines);
  auto pl = exact<uint32_t>(n_lines), ol = exact<uint32_t>(n_lines);
  auto mt = exact<int32_t>(n_lines);
  auto fl = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_QCUPD_N_COUNTS], totals[2];
  if (avdb_qc_update_size_host(ctx, text.get(), bytes, n_lines, &t.view, hostile ? uint32_t(rnd()) : 0xFFFFFFFFu, flags,
                               rs.get(), pl.get(), mt.get(), ol.get(), fl.get(), counts))
    return false;
  const size_t n = counts[AVDB_QCUPD_COUNT_ROWS];
  uint64_t cap = counts[AVDB_QCUPD_COUNT_OUT_BYTES];
  if (hostile && n) {
    for (int k = 0; k < 4; ++k) {
      const size_t r = rnd() % n;
      switch (rnd() % 5) {
        case 0: rs[r] = rnd() % (bytes + 9); break;
        case 1: pl[r] = uint32_t(rnd() % 200); break;
        case 2: ol[r] = uint32_t(rnd() % 3000); break;
        case 3: mt[r] = int32_t(rnd() % (t.rows + 3)) - 1; break;
        default: fl[r] = uint8_t(rnd()); break;
      }
    }
    cap = 0;
    for (size_t r = 0; r < n; ++r) cap += ol[r];
  }
  auto out = exact<uint64_t>((cap + 7) / 8);  // (8-byte aligned, as the entry asks)
  auto row_off = exact<uint64_t>(n + 1);
  return avdb_qc_update_write_host(ctx, text.get(), bytes, n_lines, n, &t.view, rs.get(), pl.get(), mt.get(), ol.get(),
                                   fl.get(), reinterpret_cast<uint8_t*>(out.get()), cap, row_off.get(), totals) == 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s qc.vcf export.tsv [mutations]\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> vcf = read_file(argv[1]), exp = read_file(argv[2]);
  const long mutations = argc > 3 ? atol(argv[3]) : 20000;
  avdb_ctx ctx{};
  ctx.device = -1;
  const std::vector<uint8_t> release = {'1', '7', 'k'};
  QcTable table;
  if (!run_table(&ctx, vcf.data(), vcf.size(), count_lines(vcf.data(), vcf.size()), false, release, &table)) return 1;
  printf("table: %zu rows\n", table.rows);
  for (uint32_t flags = 0; flags < 2; ++flags)
    if (!run_update(&ctx, exp.data(), exp.size(), count_lines(exp.data(), exp.size()), table, false, flags)) return 1;
  // releases of every length the entry takes, and the ones it refuses
  long ok = 0;
  for (size_t n = 0; n <= AVDB_QC_RELEASE_MAX + 1; ++n) {
    QcTable t;
    const size_t some = vcf.size() < 20000 ? vcf.size() : 20000;
    ok += run_table(&ctx, vcf.data(), some, count_lines(vcf.data(), some), false, std::vector<uint8_t>(n, uint8_t('r')), &t) &&
          run_update(&ctx, exp.data(), exp.size(), count_lines(exp.data(), exp.size()), t, false, 0);
  }
  printf("release: %ld of %d lengths accepted\n", ok, AVDB_QC_RELEASE_MAX + 2);
  const uint8_t bad[] = {'\t', ':', ';', '=', '"', '{', '}', '[', ']', '-', '+', '.', 'e', ',', '\r', '\n', '0',
                         '9', 'I', '#', '\\', 0xC3, 0x7F, 0};
  ok = mutate_windows(exp, mutations, bad, sizeof bad, [&](long m, const uint8_t* t, size_t n, size_t n_lines) {
    return run_update(&ctx, t, n, n_lines, table, m % 3 == 0, uint32_t(m & 1));
  });
  printf("export: %ld of %ld mutated runs accepted\n", ok, mutations);
  ok = mutate_windows(vcf, mutations, bad, sizeof bad, [&](long m, const uint8_t* t, size_t n, size_t n_lines) {
    QcTable mt;
    if (!run_table(&ctx, t, n, n_lines, m % 3 == 0, release, &mt)) return false;
    const size_t some = exp.size() < 3000 ? exp.size() : 3000;
    return run_update(&ctx, exp.data(), some, count_lines(exp.data(), some), mt, false, 0);
  });
  printf("vcf: %ld of %ld mutated runs accepted\n", ok, mutations);
  printf("clean\n");
  return 0;
}

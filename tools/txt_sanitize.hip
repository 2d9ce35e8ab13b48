// K19's host entries and the per-line code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_txt.hip, avdb_txt.hpp, avdb_keyset.hpp) under the host sanitizers:
// a stand-alone program, never loaded into Python and never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/txt_sanitize.hip -o txt_sanitize
//   ./txt_sanitize file.txt export.tsv [mutations]
//
// file.txt is a tab-delimited file whose first line is the header; the program takes the field
// count from it and tries `variant` and the looked-up id in every column.  The file goes through
// avdb_txt_table_size_host and avdb_txt_table_write_host from a heap copy of exactly its size into
// arrays of exactly n_lines entries, then of exactly the rows, key bytes and body bytes counted;
// the keys, reversed, through avdb_keyset_build_host into a table of exactly
// avdb_keyset_workspace_size bytes; the export through avdb_txt_update_size_host and
// avdb_txt_update_write_host, and the file through avdb_txt_direct_size_host and
// avdb_txt_direct_write_host, in the same way, so a read or write one byte outside any of them is
// reported.  Then, from a fixed seed: copies of both texts with bytes overwritten by tabs, colons,
// quotes, backslashes, the letters of NULL, carriage returns, newlines and high bytes, with a line
// count that is too large or too small, with field counts 2 .. 32 and every column choice, and
// with the entry and row arrays overwritten between the passes.  Any return code is fine, any
// sanitizer report is not.  Exit status 0 and a last line "clean" when done.
#include "../annotatedvdb_amd/csrc/avdb_keyset.hip"
#include "../annotatedvdb_amd/csrc/avdb_txt.hip"

#include "sanitize_common.hpp"

struct TxtTable {
  std::unique_ptr<uint8_t[]> rkeys, body, flags, hit, keyset;
  std::unique_ptr<uint64_t[]> rkey_off, body_off;
  std::unique_ptr<uint32_t[]> body_len;
  avdb_txt_table view;
  size_t rows = 0;
};

struct Cols {
  uint32_t skip, n_fields, id_col, key_col;
};

// both table passes over text[0, bytes) with n_lines as given; hostile: overwrite entry columns
// between the passes.  Returns whether a table came of it.
static bool run_table(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, Cols c, bool hostile,
                      TxtTable* t) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto es = exact<uint64_t>(n_lines);
  auto ea = exact<uint32_t>(n_lines), ek = exact<uint32_t>(n_lines), eb = exact<uint32_t>(n_lines);
  auto ef = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_TXT_N_COUNTS], totals[4];
  if (avdb_txt_table_size_host(ctx, text.get(), bytes, n_lines, c.skip, c.n_fields, c.id_col, c.key_col, es.get(),
                               ea.get(), ek.get(), eb.get(), ef.get(), counts))
    return false;
  const size_t ne = counts[AVDB_TXT_COUNT_ENTRIES];
  uint64_t n = counts[AVDB_TXT_COUNT_ROWS], kb = counts[AVDB_TXT_COUNT_KEY_BYTES], bb = counts[AVDB_TXT_COUNT_JSON_BYTES];
  if (hostile && ne) {
    for (int k = 0; k < 4; ++k) {
      const size_t e = rnd() % ne;
      switch (rnd() % 5) {
        case 0: es[e] = rnd() % (bytes + 9); break;
        case 1: ea[e] = uint32_t(rnd() % 2); break;
        case 2: ek[e] = uint32_t(rnd() % 300); break;
        case 3: eb[e] = uint32_t(rnd() % 3000); break;
        default: ef[e] = uint8_t(rnd()); break;
      }
    }
    n = kb = bb = 0;
    for (size_t e = 0; e < ne; ++e) {
      n += ea[e];
      kb += ek[e];
      bb += eb[e];
    }
  }
  auto keys = exact<uint8_t>(kb), body = exact<uint8_t>(bb), rf = exact<uint8_t>(n);
  auto key_off = exact<uint64_t>(n + 1), bo = exact<uint64_t>(n), ls = exact<uint64_t>(n);
  auto bl = exact<uint32_t>(n);
  if (avdb_txt_table_write_host(ctx, text.get(), bytes, n_lines, ne, n, c.skip, c.n_fields, c.id_col, c.key_col,
                                es.get(), ea.get(), ek.get(), eb.get(), ef.get(), keys.get(), kb, key_off.get(),
                                body.get(), bb, bo.get(), bl.get(), ls.get(), rf.get(), totals))
    return false;
  for (size_t r = 0; r < n; ++r)
    if (key_off[r + 1] < key_off[r] || key_off[r + 1] > kb) return false;
  t->rows = n;
  t->rkeys = exact<uint8_t>(kb);
  t->rkey_off = exact<uint64_t>(n + 1);
  t->body = std::move(body);
  t->body_off = std::move(bo);
  t->body_len = std::move(bl);
  t->flags = std::move(rf);
  t->hit = exact<uint8_t>(n);
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
  t->view = avdb_txt_table{sizeof(avdb_txt_table), 0, n, t->rkeys.get(), t->rkey_off.get(), t->keyset.get(), need,
                           t->body.get(), bb, t->body_off.get(), t->body_len.get(), t->flags.get(), t->hit.get()};
  return true;
}

static bool run_update(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, const TxtTable& t,
                       bool hostile, uint32_t key_col, uint32_t flags) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto rs = exact<uint64_t>(n_lines);
  auto pl = exact<uint32_t>(n_lines), ol = exact<uint32_t>(n_lines);
  auto mt = exact<int32_t>(n_lines);
  auto fl = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_TXTUPD_N_COUNTS], totals[2];
  if (avdb_txt_update_size_host(ctx, text.get(), bytes, n_lines, &t.view, hostile ? uint32_t(rnd()) : 0xFFFFFFFFu,
                                key_col, flags, rs.get(), pl.get(), mt.get(), ol.get(), fl.get(), counts))
    return false;
  const size_t n = counts[AVDB_TXTUPD_COUNT_ROWS];
  uint64_t cap = counts[AVDB_TXTUPD_COUNT_OUT_BYTES];
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
  return avdb_txt_update_write_host(ctx, text.get(), bytes, n_lines, n, &t.view, flags, rs.get(), pl.get(), mt.get(),
                                    ol.get(), fl.get(), reinterpret_cast<uint8_t*>(out.get()), cap, row_off.get(),
                                    totals) == 0;
}

static bool run_direct(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, Cols c, bool hostile,
                       uint32_t flags) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto rs = exact<uint64_t>(n_lines);
  auto ol = exact<uint32_t>(n_lines);
  auto fl = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_TXTDIR_N_COUNTS], totals[2];
  if (avdb_txt_direct_size_host(ctx, text.get(), bytes, n_lines, c.skip, c.n_fields, c.id_col, flags, rs.get(), ol.get(),
                                fl.get(), counts))
    return false;
  const size_t n = counts[AVDB_TXTDIR_COUNT_ROWS];
  uint64_t cap = counts[AVDB_TXTDIR_COUNT_OUT_BYTES];
  if (hostile && n) {
    for (int k = 0; k < 4; ++k) {
      const size_t r = rnd() % n;
      switch (rnd() % 3) {
        case 0: rs[r] = rnd() % (bytes + 9); break;
        case 1: ol[r] = uint32_t(rnd() % 3000); break;
        default: fl[r] = uint8_t(rnd()); break;
      }
    }
    cap = 0;
    for (size_t r = 0; r < n; ++r) cap += ol[r];
  }
  auto out = exact<uint64_t>((cap + 7) / 8);
  auto row_off = exact<uint64_t>(n + 1);
  return avdb_txt_direct_write_host(ctx, text.get(), bytes, n_lines, n, c.skip, c.n_fields, c.id_col, flags, rs.get(),
                                    ol.get(), fl.get(), reinterpret_cast<uint8_t*>(out.get()), cap, row_off.get(),
                                    totals) == 0;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s file.txt export.tsv [mutations]\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> file = read_file(argv[1]), exp = read_file(argv[2]);
  const long mutations = argc > 3 ? atol(argv[3]) : 20000;
  avdb_ctx ctx{};
  ctx.device = -1;
  uint32_t n_fields = 1;
  for (size_t i = 0; i < file.size() && file[i] != '\n'; ++i) n_fields += file[i] == '\t';
  if (n_fields < 2 || n_fields > AVDB_TXT_MAX_FIELDS) {
    fprintf(stderr, "the header has %u fields\n", n_fields);
    return 2;
  }
  const size_t file_lines = count_lines(file.data(), file.size()), exp_lines = count_lines(exp.data(), exp.size());
  TxtTable table;
  for (uint32_t id = 0; id < n_fields; ++id)
    for (uint32_t key = 0; key < n_fields; ++key) {
      const Cols c{1, n_fields, id, key};
      if (!run_table(&ctx, file.data(), file.size(), file_lines, c, false, &table)) return 1;
      for (uint32_t flags = 0; flags < 2; ++flags) {
        if (!run_update(&ctx, exp.data(), exp.size(), exp_lines, table, false, 1 + flags, flags)) return 1;
        if (!run_direct(&ctx, file.data(), file.size(), file_lines, c, false, flags)) return 1;
      }
    }
  printf("table: %zu rows, %u fields\n", table.rows, n_fields);
  if (!run_table(&ctx, file.data(), file.size(), file_lines, Cols{1, n_fields, 0, 0}, false, &table)) return 1;
  const uint8_t bad[] = {'\t', ':', '"', '\\', 'N', 'U', 'L', '\r', '\n', '0', ' ', 0xC3, 0};
  long ok = mutate_windows(exp, mutations, bad, sizeof bad, [&](long m, const uint8_t* t, size_t n, size_t n_lines) {
    return run_update(&ctx, t, n, n_lines, table, m % 3 == 0, 1 + uint32_t(m & 1), uint32_t((m >> 1) & 1));
  });
  printf("export: %ld of %ld mutated runs accepted\n", ok, mutations);
  const size_t head = exp.size() < 3000 ? exp.size() : 3000;
  ok = mutate_windows(file, mutations, bad, sizeof bad, [&](long m, const uint8_t* t, size_t n, size_t n_lines) {
    const uint32_t nf = 2 + uint32_t(rnd() % (AVDB_TXT_MAX_FIELDS - 1));
    const Cols c{uint32_t(rnd() % 3), nf, uint32_t(rnd() % nf), uint32_t(rnd() % nf)};
    TxtTable mt;
    bool fine = run_direct(&ctx, t, n, n_lines, c, m % 3 == 1, uint32_t(m & 1));
    if (!run_table(&ctx, t, n, n_lines, c, m % 3 == 0, &mt)) return false;
    return run_update(&ctx, exp.data(), head, count_lines(exp.data(), head), mt, false, 1 + uint32_t(m & 1), 0) && fine;
  });
  printf("file: %ld of %ld mutated runs accepted\n", ok, mutations);
  printf("clean\n");
  return 0;
}

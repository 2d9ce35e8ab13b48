// K18b's host entries and the per-block, per-line and per-row code they share with the kernels
// (annotatedvdb_amd/csrc/avdb_vep_rows.hip, avdb_vep_rows.hpp, on avdb_vep.hip's host entries and
// avdb_keyset.hpp) under the host sanitizers: a stand-alone program, never loaded into Python and
// never run on a GPU.
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -I include \
//         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/vep_rows_sanitize.hip -o vep_rows_sanitize
//   ./vep_rows_sanitize lines.json ranking.tsv export.tsv [mutations]
//
// lines.json holds VEP --json lines (the golden's: for g in read_golden()["lines"] write g[3]),
// ranking.tsv is tests/golden/vep_ranking.tsv, export.tsv the golden's export.  The lines go through
// avdb_vep_index_size_host / _write_host, avdb_vep_rows_table_size_host / _write_host from a heap copy
// of exactly their size into arrays of exactly n_lines entries and exactly the consequences, rows,
// key bytes and body bytes counted; the keys, reversed, through avdb_keyset_build_host into a table
// of exactly avdb_keyset_workspace_size bytes; the export through avdb_vep_rows_update_size_host /
// _write_host in the same way, so a read or write one byte outside any of them is reported.  Then,
// from a fixed seed: windows of both texts with bytes overwritten by quotes, backslashes, braces,
// brackets, commas, colons, digits, dots, minus signs, the letters of \t and \u, carriage returns,
// newlines, control and high bytes, with a line count that is too large or too small, and with
// K18a's arrays, the rendered lengths and the entry and row arrays overwritten between the passes.
// Any return code is fine, any sanitizer report is not.  Exit status 0 and a last line "clean".
#include "../annotatedvdb_amd/csrc/avdb_keyset.hip"
#include "../annotatedvdb_amd/csrc/avdb_vep.hip"
#include "../annotatedvdb_amd/csrc/avdb_vep_rows.hip"

#include "sanitize_common.hpp"

#include <map>
#include <string>

struct Ranking {
  std::vector<uint64_t> words, masks, slot_mask;
  std::vector<uint32_t> off, len, order, rank_off;
  std::vector<int32_t> slot_entry;
  std::vector<uint8_t> rank_text;
  avdb_vep_table view;
};

// consequence<TAB>rank lines behind a header; the order of the ranks is the file's (ranks ascend in it)
static bool read_ranking(const avdb_ctx* ctx, const char* path, Ranking* R) {
  const std::vector<uint8_t> raw = read_file(path);
  std::map<std::string, uint32_t> ids;
  size_t at = 0, line = 0;
  R->rank_off.push_back(0);
  while (at < raw.size()) {
    size_t e = at;
    while (e < raw.size() && raw[e] != '\n') ++e;
    const std::string row(raw.begin() + at, raw.begin() + e);
    at = e + 1;
    if (line++ == 0 || row.empty()) continue;
    const size_t tab = row.find('\t');
    if (tab == std::string::npos) return false;
    uint64_t mask = 0;
    for (size_t a = 0; a <= tab;) {
      size_t b = row.find(',', a);
      if (b == std::string::npos || b > tab) b = tab;
      const std::string term = row.substr(a, b - a);
      auto it = ids.find(term);
      if (it == ids.end()) {
        if (ids.size() >= 64) return false;
        it = ids.emplace(term, uint32_t(ids.size())).first;
        R->off.push_back(uint32_t(R->words.size()));
        R->len.push_back(uint32_t(term.size()));
        for (size_t k = 0; k < term.size() || k == 0; k += 8) {
          uint64_t w = 0;
          for (size_t j = 0; j < 8 && k + j < term.size(); ++j) w |= uint64_t(uint8_t(term[k + j])) << (8 * j);
          R->words.push_back(w);
        }
      }
      mask |= 1ull << it->second;
      a = b + 1;
    }
    R->masks.push_back(mask);
    R->order.push_back(uint32_t(R->order.size()));
    for (size_t k = tab + 1; k < row.size(); ++k) R->rank_text.push_back(uint8_t(row[k]));
    R->rank_off.push_back(uint32_t(R->rank_text.size()));
  }
  size_t slots = 2;
  while (slots < 2 * R->masks.size()) slots *= 2;
  R->slot_mask.resize(slots);
  R->slot_entry.resize(slots);
  if (avdb_vep_table_build(ctx, uint32_t(ids.size()), R->masks.data(), R->masks.size(), R->slot_mask.data(),
                           R->slot_entry.data(), slots))
    return false;
  R->view = avdb_vep_table{sizeof(avdb_vep_table), uint32_t(ids.size()), R->words.data(), R->off.data(), R->len.data(),
                           R->slot_mask.data(), R->slot_entry.data(), uint32_t(slots), uint32_t(R->masks.size()),
                           R->order.data(), 0x5ull};
  return true;
}

struct RowsTable {
  std::unique_ptr<uint8_t[]> rkeys, json, hit, keyset;
  std::unique_ptr<uint64_t[]> rkey_off, json_off;
  std::unique_ptr<uint32_t[]> json_len;
  avdb_vep_rows_table view;
  size_t rows = 0;
};

template <class T>
static void scribble(T* a, size_t n, uint64_t range) {
  if (n) a[rnd() % n] = T(rnd() % range);
}

// K18a's two passes and K18b's two table passes over text[0, bytes) with n_lines as given; hostile:
// overwrite K18a's arrays before K18b reads them, and the rendered lengths and entry columns between
// its passes.  Returns whether a table came of it.
static bool run_table(const avdb_ctx* ctx, const Ranking& rk, const uint8_t* src, size_t bytes, size_t n_lines,
                      bool hostile, RowsTable* t) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto n_csq = exact<uint32_t>(n_lines);
  auto lf = exact<uint8_t>(n_lines), ty = exact<uint8_t>(n_lines);
  auto is = exact<uint64_t>(n_lines), ids = exact<uint64_t>(n_lines), co = exact<uint64_t>(n_lines);
  auto il = exact<int32_t>(n_lines), idl = exact<int32_t>(n_lines);
  uint64_t vc[AVDB_VEP_N_COUNTS], vt[2];
  if (avdb_vep_index_size_host(ctx, text.get(), bytes, n_lines, &rk.view, n_csq.get(), lf.get(), ty.get(), is.get(),
                               il.get(), ids.get(), idl.get(), vc))
    return false;
  uint64_t total = 0;
  for (size_t i = 0; i < n_lines; ++i) {
    co[i] = total;
    total += n_csq[i];
  }
  auto type = exact<uint8_t>(total), coding = exact<uint8_t>(total), head = exact<uint8_t>(total);
  auto order = exact<int32_t>(total), entry = exact<int32_t>(total), sorted = exact<int32_t>(total);
  auto els = exact<uint64_t>(total), als = exact<uint64_t>(total), mask = exact<uint64_t>(total);
  auto ell = exact<uint32_t>(total), all = exact<uint32_t>(total), rlen = exact<uint32_t>(total);
  if (avdb_vep_index_write_host(ctx, text.get(), bytes, n_lines, &rk.view, n_csq.get(), lf.get(), co.get(), total,
                                type.get(), order.get(), els.get(), ell.get(), als.get(), all.get(), mask.get(),
                                entry.get(), coding.get(), sorted.get(), head.get(), vt))
    return false;
  if (hostile) {
    for (int k = 0; k < 6; ++k) switch (rnd() % 12) {
        case 0: scribble(n_csq.get(), n_lines, 600); break;
        case 1: scribble(co.get(), n_lines, total + 9); break;
        case 2: scribble(is.get(), n_lines, bytes + 9); break;
        case 3: scribble(il.get(), n_lines, bytes + 9); break;
        case 4: scribble(lf.get(), n_lines, 256); break;
        case 5: scribble(els.get(), total, bytes + 9); break;
        case 6: scribble(ell.get(), total, bytes + 9); break;
        case 7: scribble(als.get(), total, bytes + 9); break;
        case 8: scribble(all.get(), total, bytes + 9); break;
        case 9: scribble(entry.get(), total, rk.masks.size() + 9); break;
        case 10: scribble(sorted.get(), total, 600); break;
        default: scribble(order.get(), total, 1ull << 32); break;
      }
  }
  const avdb_vep_rows_in in{sizeof(avdb_vep_rows_in), uint32_t(rk.masks.size()), total, rk.rank_text.data(),
                            rk.rank_text.size(), rk.rank_off.data(), lf.get(), n_csq.get(), co.get(), is.get(), il.get(),
                            type.get(), order.get(), els.get(), ell.get(), als.get(), all.get(), entry.get(),
                            coding.get(), sorted.get(), rlen.get()};
  auto es = exact<uint64_t>(n_lines);
  auto ea = exact<uint32_t>(n_lines), ek = exact<uint32_t>(n_lines), ej = exact<uint32_t>(n_lines);
  auto ef = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_VEPROWS_N_COUNTS], totals[4];
  if (avdb_vep_rows_table_size_host(ctx, text.get(), bytes, n_lines, &in, es.get(), ea.get(), ek.get(), ej.get(),
                                    ef.get(), counts))
    return false;
  const size_t ne = counts[AVDB_VEPROWS_COUNT_ENTRIES];
  uint64_t n = counts[AVDB_VEPROWS_COUNT_ROWS], kb = counts[AVDB_VEPROWS_COUNT_KEY_BYTES],
           jb = counts[AVDB_VEPROWS_COUNT_JSON_BYTES];
  if (hostile && ne) {
    for (int k = 0; k < 4; ++k) {
      const size_t e = rnd() % ne;
      switch (rnd() % 6) {
        case 0: es[e] = rnd() % (bytes + 9); break;
        case 1: ea[e] = uint32_t(rnd() % 7); break;
        case 2: ek[e] = uint32_t(rnd() % 300); break;
        case 3: ej[e] = uint32_t(rnd() % 30000); break;
        case 4: scribble(rlen.get(), total, 1ull << 32); break;
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
  auto keys = exact<uint8_t>(kb), rf = exact<uint8_t>(n);
  auto json = exact<uint64_t>((jb + 7) / 8);  // (8-byte aligned, as the entry asks)
  auto key_off = exact<uint64_t>(n + 1), jo = exact<uint64_t>(n), ls = exact<uint64_t>(n);
  auto jl = exact<uint32_t>(n);
  auto keys8 = exact<uint64_t>((kb + 7) / 8);
  if (avdb_vep_rows_table_write_host(ctx, text.get(), bytes, n_lines, ne, n, &in, es.get(), ea.get(), ek.get(), ej.get(),
                                     ef.get(), reinterpret_cast<uint8_t*>(keys8.get()), kb, key_off.get(),
                                     reinterpret_cast<uint8_t*>(json.get()), jb, jo.get(), jl.get(), ls.get(), rf.get(),
                                     totals))
    return false;
  memcpy(keys.get(), keys8.get(), kb);
  for (size_t r = 0; r < n; ++r)
    if (key_off[r + 1] < key_off[r] || key_off[r + 1] > kb || jo[r] > jb || jl[r] > jb - jo[r]) return false;
  t->rows = n;
  t->rkeys = exact<uint8_t>(kb);
  t->rkey_off = exact<uint64_t>(n + 1);
  t->json = exact<uint8_t>(jb);
  memcpy(t->json.get(), json.get(), jb);
  t->json_off = std::move(jo);
  t->json_len = std::move(jl);
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
  t->view = avdb_vep_rows_table{sizeof(avdb_vep_rows_table), 0, n, t->rkeys.get(), t->rkey_off.get(), t->keyset.get(),
                                need, t->json.get(), jb, t->json_off.get(), t->json_len.get(), t->hit.get()};
  return true;
}

static bool run_update(const avdb_ctx* ctx, const uint8_t* src, size_t bytes, size_t n_lines, const RowsTable& t,
                       bool hostile, uint32_t flags, uint64_t alg_id) {
  auto text = exact<uint8_t>(bytes);
  memcpy(text.get(), src, bytes);
  auto rs = exact<uint64_t>(n_lines);
  auto pl = exact<uint32_t>(n_lines), ol = exact<uint32_t>(n_lines);
  auto mt = exact<int32_t>(n_lines);
  auto fl = exact<uint8_t>(n_lines);
  uint64_t counts[AVDB_LOFUPD_N_COUNTS], totals[2];
  if (avdb_vep_rows_update_size_host(ctx, text.get(), bytes, n_lines, &t.view, hostile ? uint32_t(rnd()) : 0xFFFFFFFFu,
                                     flags, alg_id, rs.get(), pl.get(), mt.get(), ol.get(), fl.get(), counts))
    return false;
  const size_t n = counts[AVDB_LOFUPD_COUNT_ROWS];
  uint64_t cap = counts[AVDB_LOFUPD_COUNT_OUT_BYTES];
  if (hostile && n) {
    for (int k = 0; k < 4; ++k) {
      const size_t r = rnd() % n;
      switch (rnd() % 5) {
        case 0: rs[r] = rnd() % (bytes + 9); break;
        case 1: pl[r] = uint32_t(rnd() % 200); break;
        case 2: ol[r] = uint32_t(rnd() % 30000); break;
        case 3: mt[r] = int32_t(rnd() % (t.rows + 3)) - 1; break;
        default: fl[r] = uint8_t(rnd()); break;
      }
    }
    cap = 0;
    for (size_t r = 0; r < n; ++r) cap += ol[r];
  }
  auto out = exact<uint64_t>((cap + 7) / 8);
  auto row_off = exact<uint64_t>(n + 1);
  return avdb_vep_rows_update_write_host(ctx, text.get(), bytes, n_lines, n, &t.view, flags, alg_id, rs.get(), pl.get(),
                                         mt.get(), ol.get(), fl.get(), reinterpret_cast<uint8_t*>(out.get()), cap,
                                         row_off.get(), totals) == 0;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s lines.json ranking.tsv export.tsv [mutations]\n", argv[0]);
    return 2;
  }
  const std::vector<uint8_t> vep = read_file(argv[1]), exp = read_file(argv[3]);
  const long mutations = argc > 4 ? atol(argv[4]) : 4000;
  avdb_ctx ctx{};
  ctx.device = -1;
  Ranking rk;
  if (!read_ranking(&ctx, argv[2], &rk)) return 1;
  RowsTable table;
  if (!run_table(&ctx, rk, vep.data(), vep.size(), count_lines(vep.data(), vep.size()), false, &table)) return 1;
  printf("table: %zu rows\n", table.rows);
  for (uint32_t flags = 0; flags < 4; ++flags)
    if (!run_update(&ctx, exp.data(), exp.size(), count_lines(exp.data(), exp.size()), table, false, flags, 4242)) return 1;
  const uint8_t bad[] = {'"', '\\', '{', '}', '[', ']', ',', ':', '0', '9', '.', '-', 'e', 't', 'u', '\t', '\r', '\n', 1, 0xC3, 0};
  long ok = mutate_windows(exp, mutations, bad, sizeof bad, [&](long m, const uint8_t* t, size_t n, size_t n_lines) {
    return run_update(&ctx, t, n, n_lines, table, m % 3 == 0, uint32_t(m & 3), rnd() >> (rnd() % 64));
  });
  printf("export: %ld of %ld mutated runs accepted\n", ok, mutations);
  const size_t head = exp.size() < 3000 ? exp.size() : 3000;
  ok = mutate_windows(vep, mutations, bad, sizeof bad, [&](long m, const uint8_t* t, size_t n, size_t n_lines) {
    RowsTable mt;
    if (!run_table(&ctx, rk, t, n, n_lines, m % 3 == 0, &mt)) return false;
    return run_update(&ctx, exp.data(), head, count_lines(exp.data(), head), mt, false, 0, 7);
  });
  printf("lines: %ld of %ld mutated runs accepted\n", ok, mutations);
  // whole lines too: a window rarely holds one, and a line cut at its start is the host's at once
  size_t at = 0;
  long whole = 0, took = 0;
  while (at < vep.size() && whole < mutations) {
    size_t e = at;
    while (e < vep.size() && vep[e] != '\n') ++e;
    std::vector<uint8_t> line(vep.begin() + at, vep.begin() + (e < vep.size() ? e + 1 : e));
    at = e + 1;
    for (int rep = 0; rep < 4; ++rep, ++whole) {
      std::vector<uint8_t> t = line;
      for (int k = int(rnd() % 3); k > 0 && !t.empty(); --k) t[rnd() % t.size()] = bad[rnd() % sizeof bad];
      RowsTable mt;
      took += run_table(&ctx, rk, t.data(), t.size(), count_lines(t.data(), t.size()), rep == 3, &mt);
    }
  }
  printf("whole lines: %ld of %ld mutated runs accepted\n", took, whole);
  printf("clean\n");
  return 0;
}

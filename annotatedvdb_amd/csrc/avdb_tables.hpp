// The skeleton K16 (avdb_lof.hip), K17 (avdb_qc.hip), K18b (avdb_vep_rows.hip) and K19 (avdb_txt.hip)
// share, on avdb_rows.hpp: a table build over the annotation file and an export join against that
// table, each a size entry and a write entry with a _host twin.  A pass keeps what differs: its
// line kernels, its key and JSON (K19: body) write kernels, its stage sizes, its renderers, and one
// policy struct per half.
//   the table build (avdb_*_table_size / _write)
//     the pass's line kernel: info[li] = {alts, key_bytes, json_len, class | flags << 8}, a mark per entry
//     k_compact<P>    one lane per line: an entry's columns to its entry number; the counts
//     (the write entry: three exclusive scans, of the entries' alts, key bytes and JSON lengths;
//      k_totals: the totals against the caller's capacities)
//     the pass's two rows::write_rows kernels, one lane per entry (load_entry gives a lane its entry)
//   the export join (avdb_*_update_size / _write): K13's shape (avdb_caddupd.hip) with the K6 text
//   probe (avdb_keyset.hpp) in place of the K10 join
//     the pass's line kernel around UpdTally: info[li] = {pk_len, out_len, match, flags | is_row << 8}
//     k_upd_compact<P>, rows::begin_write, k_upd_write<stage, Render>
// A table policy P gives the count indices ROWS, LINES, KEY_BYTES, JSON_BYTES, HOST_LINES, BAD and
// ENTRIES, the flag bits HOST_BIT and BAD_BIT, one more counted bit EXTRA_BIT with its index EXTRA
// (-1: none), ROW_PER_ENTRY (the write entry refuses more rows than entries) and is_entry(info.w).
// An update policy gives ROWS, SKIPPED_LINES, SKIPPED (-1: the pass has no such records), MISSED,
// BAD, OUT_BYTES and LONE_CR, BAD_BIT, and HOST_BIT with its index HOST_ROWS (-1: none).
// Compiled for both sides, as avdb_rows.hpp is.
#pragma once

#include "avdb_lof.hpp"
#include "avdb_rows.hpp"

#include <stdio.h>
#include <string.h>

namespace avdb {
namespace tables {

using lof::EntryRow;
using lof::RowCols;
using lof::Table;
using lof::UpdRow;

struct Slab {  // the text every entry reads
  const uint8_t* text;
  size_t text_bytes, n_lines;
};

// An entry's call: its name (for the error texts), the context, the slab, and what the pass's own
// argument checks gave: `err` of those in front of the common checks (K17's release, the table view
// of an update entry), `own` of those behind the null-argument check (K19's shape, its key_col).
struct Entry {
  const char* fn;
  const avdb_ctx* ctx;
  Slab in;
  const char* err = nullptr;
  const char* own = nullptr;
};

struct Work {  // a device entry's
  void* workspace;
  size_t bytes;
  hipStream_t s;
};

struct EntCols {  // per entry, n_lines entries allocated
  uint64_t* start;
  uint32_t* alts;
  uint32_t* key_bytes;
  uint32_t* json_len;
  uint8_t* flags;
};

struct EntScans {  // n_entries + 1 each
  uint64_t* row;
  uint64_t* key;
  uint64_t* json;
};

struct TableOut {  // what a table write entry fills (R.key_off: n_rows + 1 offsets)
  uint8_t* keys;
  size_t key_cap;
  uint8_t* json;
  size_t json_cap;
  RowCols R;
  uint64_t* totals;
};

struct UpdCols {  // per row, n_lines entries allocated
  uint64_t* row_start;
  uint32_t* pk_len;
  int32_t* match;
  uint32_t* out_len;
  uint8_t* flags;
};

struct UpdOut {  // what an update write entry fills
  uint8_t* out;
  size_t out_cap;
  uint64_t* row_off;
  uint64_t* totals;
};

inline bool any_null(const EntCols& o) { return !o.start || !o.alts || !o.key_bytes || !o.json_len || !o.flags; }
inline bool any_null(const UpdCols& o) { return !o.row_start || !o.pk_len || !o.match || !o.out_len || !o.flags; }

// The table's workspace: rows::Layout with 16 bytes of info per line and, for the write pass, three
// scanned arrays of n_entries + 1 <= n_lines + 1 offsets (32 bytes a line cover them)
inline rows::Layout table_layout(size_t n_lines) { return rows::layout(n_lines, 16, 32); }
inline rows::Layout upd_layout(size_t n_lines) { return rows::layout(n_lines, 16); }

inline EntScans ent_scans(char* w, const rows::Layout& L, size_t n_lines) {
  auto* base = reinterpret_cast<uint64_t*>(w + L.extra);
  return EntScans{base, base + (n_lines + 1), base + 2 * (n_lines + 1)};
}

// ---- the argument checks ---------------------------------------------------------------------
inline int invalid(const char* fn, const char* err) {
  avdb_set_error("%s: %s", fn, err);
  return AVDB_EINVAL;
}

// AVDB_LAUNCH_CHECK for a shared kernel: the message names the entry too, and with it the pass
#define AVDB_TABLES_LAUNCH_CHECK(kernel, fn)                    \
  do {                                                          \
    char name_[96];                                             \
    snprintf(name_, sizeof(name_), "%s of %s", kernel, fn);     \
    AVDB_LAUNCH_CHECK(name_);                                   \
  } while (0)

template <class Cols>
const char* size_error(const Entry& c, const Cols& o, const uint64_t* counts) {
  if (c.err) return c.err;
  if (!c.ctx || !counts) return "null argument";
  if (c.own) return c.own;
  if (const char* e = lines::text_args_error(c.in.text, c.in.text_bytes, c.in.n_lines)) return e;
  if (c.in.n_lines && any_null(o)) return "null output array";
  return nullptr;
}

template <class P>
const char* table_write_error(const Entry& c, size_t n_entries, size_t n_rows, const EntCols& o, const TableOut& t) {
  if (c.err) return c.err;
  if (!c.ctx || !t.totals || !t.R.key_off) return "null argument";
  if (c.own) return c.own;
  if (const char* e = rows::text_rows_error(c.in.text, c.in.text_bytes, c.in.n_lines, n_entries)) return e;
  if (P::ROW_PER_ENTRY ? n_rows > n_entries : n_rows >= 0x7FFFFFFFull)
    return P::ROW_PER_ENTRY ? "more rows than entries (an entry is one row)" : "too many rows (rows are numbered in int32)";
  if (n_entries && any_null(o)) return "null entry array";
  if (n_rows && (!t.R.json_off || !t.R.json_len || !t.R.line_start || !t.R.flags)) return "null row array";
  if (const char* e = rows::out_error(t.keys, t.key_cap)) return e;
  return rows::out_error(t.json, t.json_cap);
}

inline const char* upd_write_error(const Entry& c, size_t n_rows, const UpdCols& o, const UpdOut& u) {
  if (c.err) return c.err;
  if (!c.ctx || !u.totals || !u.row_off) return "null argument";
  if (const char* e = rows::text_rows_error(c.in.text, c.in.text_bytes, c.in.n_lines, n_rows)) return e;
  if (n_rows && any_null(o)) return "null row array";
  return rows::out_error(u.out, u.out_cap);
}

// The members of a table view the three passes share, behind the pass's own struct-size check (and
// K17's release); flags_missing: the pass's table has a flags array and it is null.
inline const char* fill_table_view(Table* T, uint64_t n_rows, const uint8_t* keys, const uint64_t* key_off,
                                   const void* keyset, uint64_t keyset_bytes, const uint8_t* json, uint64_t json_bytes,
                                   const uint64_t* json_off, const uint32_t* json_len, uint8_t* hit,
                                   bool flags_missing = false) {
  if (n_rows >= 0x7FFFFFFFull) return "too many table rows";
  if (n_rows == 0) return nullptr;
  if (!keys || !key_off || !keyset || !json_off || !json_len || flags_missing || (json_bytes && !json))
    return "null table array";
  const uint64_t slots = keyset::slots(size_t(n_rows));
  if (keyset_bytes < slots * 12) return "key set smaller than avdb_keyset_workspace_size";
  T->n_rows = n_rows;
  T->keys = keys;
  T->key_off = key_off;
  T->tkey = static_cast<const unsigned long long*>(keyset);
  T->tidx = reinterpret_cast<const uint32_t*>(T->tkey + slots);
  T->mask = slots - 1;
  T->json = json;
  T->json_bytes = json_bytes;
  T->json_off = json_off;
  T->json_len = json_len;
  T->hit = hit;
  return nullptr;
}

// ---- the size pass of both halves ------------------------------------------------------------
template <class Cols>
using CompactKernel = void (*)(const uint64_t*, size_t, size_t, const u32x4*, const uint64_t*, Cols,
                               unsigned long long*);

// A size entry: the checks, the workspace L, the counts zeroed, the line starts, the pass's line
// kernel (launch_lines(grid, starts, info, marks, counts) launches it: 16 bytes of info and a mark
// per line, marks[n_lines] = 0), the marks scanned, the compaction.
template <class Cols, class Lines>
int size_pass(const Entry& c, const Cols& o, uint64_t* counts, size_t n_counts, const rows::Layout& L, const Work& k,
              const char* lines_kernel, Lines launch_lines, CompactKernel<Cols> compact, const char* compact_kernel) {
  const Slab& in = c.in;
  if (const char* e = size_error(c, o, counts)) return invalid(c.fn, e);
  if (int e = rows::begin_size(c.fn, c.ctx, L.total, in.n_lines, k.workspace, k.bytes, counts, n_counts, k.s)) return e;
  if (in.n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(k.workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(in.n_lines, kBlock, 4096);
  auto mark = [&](const uint64_t* starts, uint64_t* marks) { launch_lines(grid, starts, info, marks, cnt); };
  if (int e = lines::number_rows(in.text, in.text_bytes, in.n_lines, w, L, k.s, lines_kernel, mark)) return e;
  hipLaunchKernelGGL(compact, dim3(grid), dim3(kBlock), 0, k.s, reinterpret_cast<const uint64_t*>(w + L.starts),
                     in.text_bytes, in.n_lines, info, reinterpret_cast<const uint64_t*>(w + L.row_of), o, cnt);
  AVDB_TABLES_LAUNCH_CHECK(compact_kernel, c.fn);
  return AVDB_OK;
}

// the same on the host: per_line(li, s, line, len, nl) handles line li, which starts at s
template <class Cols, class PerLine>
int size_pass_host(const Entry& c, const Cols& o, uint64_t* counts, size_t n_counts, PerLine per_line) {
  const Slab& in = c.in;
  if (const char* e = size_error(c, o, counts)) return invalid(c.fn, e);
  memset(counts, 0, 8 * n_counts);
  if (in.n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(in.text, in.text_bytes, in.n_lines);
  for (size_t li = 0; li < in.n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(in.text, in.text_bytes, starts.data(), in.n_lines, li, &s, &e, &nl);
    per_line(li, s, in.text + s, e - s, nl);
  }
  return AVDB_OK;
}

// ---- the table build -------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(kBlock) void k_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                    size_t n_lines, const u32x4* __restrict__ info,
                                                    const uint64_t* __restrict__ ent_of, EntCols o,
                                                    unsigned long long* __restrict__ counts) {
  uint64_t rows = 0, kb = 0, jb = 0;
  uint32_t n_host = 0, n_bad = 0, n_extra = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if (!P::is_entry(v.w)) continue;
    const uint64_t e = ent_of[li];  // e < n_lines: at most one entry per line (rows are numbered by the write pass)
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    const uint32_t flags = (v.w >> 8) & 0xFFu;
    o.start[e] = s;
    o.alts[e] = v.x;
    o.key_bytes[e] = v.y;
    o.json_len[e] = v.z;
    o.flags[e] = uint8_t(flags);
    rows += v.x;
    kb += v.y;
    jb += v.z;
    n_host += (flags & P::HOST_BIT) != 0;
    n_bad += (flags & P::BAD_BIT) != 0;
    n_extra += (flags & P::EXTRA_BIT) != 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    counts[P::ENTRIES] = ent_of[n_lines];
    counts[P::LINES] = n_lines;
  }
  wave_add(&counts[P::ROWS], rows);
  wave_add(&counts[P::KEY_BYTES], kb);
  wave_add(&counts[P::JSON_BYTES], jb);
  wave_add(&counts[P::HOST_LINES], n_host);
  wave_add(&counts[P::BAD], n_bad);
  if constexpr (P::EXTRA >= 0) wave_add(&counts[P::EXTRA], n_extra);
}

// the three totals against the capacities; totals[3]: 1 when they do not fit (nothing is written)
// (a template, so every translation unit including this header may define it)
template <class Cols>
__global__ void k_totals(Cols o, EntScans sc, size_t n_entries, uint64_t n_rows, uint64_t key_cap, uint64_t json_cap,
                         uint64_t* __restrict__ key_off, uint64_t* __restrict__ totals) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t r = 0, k = 0, j = 0;
  if (n_entries) {
    r = sc.row[n_entries - 1] + o.alts[n_entries - 1];
    k = sc.key[n_entries - 1] + o.key_bytes[n_entries - 1];
    j = sc.json[n_entries - 1] + o.json_len[n_entries - 1];
  }
  sc.row[n_entries] = r;
  sc.key[n_entries] = k;
  sc.json[n_entries] = j;
  const bool over = k > key_cap || j > json_cap || r != n_rows;
  totals[0] = k;
  totals[1] = j;
  totals[2] = r;
  totals[3] = over;
  if (!over) key_off[n_rows] = k;
}

__device__ __forceinline__ EntryRow load_entry(const EntCols& o, const EntScans& sc, size_t e) {
  return EntryRow{o.start[e], o.alts[e], o.key_bytes[e], o.json_len[e], o.flags[e], sc.row[e], sc.key[e], sc.json[e]};
}

template <class P, class Lines>
int table_size(const Entry& c, const EntCols& o, uint64_t* counts, size_t n_counts, const Work& k,
               const char* lines_kernel, Lines launch_lines) {
  return size_pass(c, o, counts, n_counts, table_layout(c.in.n_lines), k, lines_kernel, launch_lines, &k_compact<P>,
                   "k_compact");
}

// entry(li, line, len, nl, &E): the pass's line rule and its own counts; whether the line is an entry
template <class P, class Line>
int table_size_host(const Entry& c, const EntCols& o, uint64_t* counts, size_t n_counts, Line entry) {
  uint64_t n = 0;
  const int rc = size_pass_host(c, o, counts, n_counts,
                                [&](size_t li, uint64_t s, const uint8_t* line, uint64_t len, bool nl) {
    lof::Entry E;
    if (!entry(li, line, len, nl, &E)) return;
    o.start[n] = s;
    o.alts[n] = E.n_alts;
    o.key_bytes[n] = E.key_bytes;
    o.json_len[n] = E.json_len;
    o.flags[n] = uint8_t(E.flags);
    ++n;
    counts[P::ROWS] += E.n_alts;
    counts[P::KEY_BYTES] += E.key_bytes;
    counts[P::JSON_BYTES] += E.json_len;
    counts[P::HOST_LINES] += (E.flags & P::HOST_BIT) != 0;
    counts[P::BAD] += (E.flags & P::BAD_BIT) != 0;
    if constexpr (P::EXTRA >= 0) counts[P::EXTRA] += (E.flags & P::EXTRA_BIT) != 0;
  });
  if (rc || c.in.n_lines == 0) return rc;
  counts[P::ENTRIES] = n;
  counts[P::LINES] = c.in.n_lines;
  return AVDB_OK;
}

// A table write entry: the checks, the workspace, the three scans and the totals, then the pass's
// two write kernels (launch_keys(grid, sc) and launch_json(grid, sc) launch them).  An overflow is
// reported through totals and the entry returns AVDB_OK.
template <class P, class Keys, class Json>
int table_write(const Entry& c, size_t n_entries, size_t n_rows, const EntCols& o, const TableOut& t, const Work& k,
                const char* keys_kernel, Keys launch_keys, const char* json_kernel, Json launch_json) {
  const Slab& in = c.in;
  if (const char* e = table_write_error<P>(c, n_entries, n_rows, o, t)) return invalid(c.fn, e);
  const rows::Layout L = table_layout(in.n_lines);
  if (int e = in.n_lines ? lines::workspace_error(c.fn, L.total, k.workspace, k.bytes) : 0) return e;
  AVDB_HIP_TRY(hipSetDevice(c.ctx->device));
  if (in.n_lines == 0) {  // no entries and no workspace: zero totals, or rows that nothing bears out
    AVDB_HIP_TRY(hipMemsetAsync(t.totals, 0, 32, k.s));
    AVDB_HIP_TRY(hipMemsetAsync(n_rows ? t.totals + 3 : t.R.key_off, n_rows ? 1 : 0, n_rows ? 1 : 8, k.s));
    return AVDB_OK;
  }
  char* w = static_cast<char*>(k.workspace);
  const EntScans sc = ent_scans(w, L, in.n_lines);
  if (n_entries) {
    if (int e = scan::exclusive_u64(o.alts, sc.row, n_entries, w + L.scan, L.scan_bytes, k.s)) return e;
    if (int e = scan::exclusive_u64(o.key_bytes, sc.key, n_entries, w + L.scan, L.scan_bytes, k.s)) return e;
    if (int e = scan::exclusive_u64(o.json_len, sc.json, n_entries, w + L.scan, L.scan_bytes, k.s)) return e;
  }
  hipLaunchKernelGGL(k_totals<EntCols>, dim3(1), dim3(kWave), 0, k.s, o, sc, n_entries, uint64_t(n_rows), uint64_t(t.key_cap),
                     uint64_t(t.json_cap), t.R.key_off, t.totals);
  AVDB_TABLES_LAUNCH_CHECK("k_totals", c.fn);
  if (n_entries == 0) return AVDB_OK;
  const unsigned grid = stream_grid(n_entries, kBlock, 2048);
  launch_keys(grid, sc);
  AVDB_LAUNCH_CHECK(keys_kernel);
  launch_json(grid, sc);
  AVDB_LAUNCH_CHECK(json_kernel);
  return AVDB_OK;
}

// the same on the host; an overflow is AVDB_ERANGE, `blob` the word for the second blob in its
// message.  render(E, put_key, put_json) renders entry E's keys and its JSON.
template <class P, class Render>
int table_write_host(const Entry& c, size_t n_entries, size_t n_rows, const EntCols& o, const TableOut& t,
                     const char* blob, Render render) {
  if (const char* e = table_write_error<P>(c, n_entries, n_rows, o, t)) return invalid(c.fn, e);
  uint64_t r = 0, k = 0, j = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    r += o.alts[e];
    k += o.key_bytes[e];
    j += o.json_len[e];
  }
  const bool over = k > t.key_cap || j > t.json_cap || r != n_rows;
  t.totals[0] = k;
  t.totals[1] = j;
  t.totals[2] = r;
  t.totals[3] = over;
  if (over) {
    avdb_set_error("%s: %llu key bytes, %llu %s bytes and %llu rows required", c.fn, (unsigned long long)k,
                   (unsigned long long)j, blob, (unsigned long long)r);
    return AVDB_ERANGE;
  }
  t.R.key_off[n_rows] = k;
  r = k = j = 0;
  for (size_t e = 0; e < n_entries; ++e) {
    const EntryRow E{o.start[e], o.alts[e], o.key_bytes[e], o.json_len[e], o.flags[e], r, k, j};
    render(E, [&](uint32_t i, uint32_t c) { t.keys[k + i] = uint8_t(c); },
           [&](uint32_t i, uint32_t c) { t.json[j + i] = uint8_t(c); });
    r += E.alts;
    k += E.key_bytes;
    j += E.json_len;
  }
  return AVDB_OK;
}

// ---- the export join -------------------------------------------------------------------------
// What a lane of an update line kernel keeps of its lines: line(L, ...) behind the pass's
// scan_export_line (L: its UpdLine), finish() behind lines::for_each_line.
template <class P>
struct UpdTally {
  uint64_t n_cr = 0;
  uint32_t n_skip = 0, n_miss = 0;

  // info[li] = {pk_len, out_len, match, flags | is_row << 8}
  template <class L>
  __device__ __forceinline__ void line(const L& l, size_t li, u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                       uint8_t* hit) {
    info[li] = u32x4{l.pk_len, l.out_len, uint32_t(l.row), l.flags | (l.is_row << 8)};
    mark[li] = l.is_row;
    if (l.row >= 0 && hit) hit[l.row] = 1;  // (every writer stores the same byte)
    n_cr += l.lone_cr;
    if constexpr (P::SKIPPED >= 0) n_skip += l.skipped;
    n_miss += l.missed;
  }

  __device__ __forceinline__ void finish(uint64_t* __restrict__ mark, size_t n_lines,
                                         unsigned long long* __restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the row count there
    wave_add(&counts[P::LONE_CR], n_cr);
    if constexpr (P::SKIPPED >= 0) wave_add(&counts[P::SKIPPED], n_skip);
    wave_add(&counts[P::MISSED], n_miss);
  }
};

// the lines that are neither a row nor a record counted otherwise
template <class P, class C>
AVDB_HD uint64_t skipped_lines(uint64_t n_lines, uint64_t rows, const C* counts) {
  uint64_t n = n_lines - rows;
  if constexpr (P::SKIPPED >= 0) n -= counts[P::SKIPPED];
  return n - counts[P::MISSED];
}

template <class P>
__global__ __launch_bounds__(kBlock) void k_upd_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                        size_t n_lines, const u32x4* __restrict__ info,
                                                        const uint64_t* __restrict__ row_of, UpdCols o,
                                                        unsigned long long* __restrict__ counts) {
  uint64_t bytes = 0;
  uint32_t n_bad = 0, n_host = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if (!((v.w >> 8) & 1u)) continue;
    const uint64_t r = row_of[li];  // r < n_lines: at most one row per line
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    const uint32_t flags = v.w & 0xFFu;
    o.row_start[r] = s;
    o.pk_len[r] = v.x;
    o.out_len[r] = v.y;
    o.match[r] = int32_t(v.z);
    o.flags[r] = uint8_t(flags);
    bytes += v.y;
    n_bad += (flags & P::BAD_BIT) != 0;
    n_host += (flags & P::HOST_BIT) != 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // (the line kernel, which counts the records that are no rows, has finished)
    const uint64_t rows = row_of[n_lines];
    counts[P::ROWS] = rows;
    counts[P::SKIPPED_LINES] = skipped_lines<P>(n_lines, rows, counts);
  }
  wave_add(&counts[P::OUT_BYTES], bytes);
  wave_add(&counts[P::BAD], n_bad);
  if constexpr (P::HOST_ROWS >= 0) wave_add(&counts[P::HOST_ROWS], n_host);
}

// render(row, text_at, put): the pass's render_update_row with its table (a functor passed by value)
template <uint32_t kStageBytes, class Render>
__global__ __launch_bounds__(kBlock) void k_upd_write(const uint8_t* __restrict__ text, size_t text_bytes,
                                                      Render render, UpdCols o, const uint64_t* __restrict__ row_off,
                                                      size_t n_rows, uint8_t* __restrict__ out,
                                                      const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kStageBytes / 8];
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  rows::write_rows<kStageBytes>(
      row_off, n_rows, out, totals, s_out,
      [&](size_t r) { return UpdRow{o.row_start[r], o.pk_len[r], o.out_len[r], o.flags[r], o.match[r]}; },
      [&](const UpdRow& row, auto put) { render(row, tb, put); });
}

template <class P, class Lines>
int update_size(const Entry& c, const UpdCols& o, uint64_t* counts, size_t n_counts, const Work& k,
                const char* lines_kernel, Lines launch_lines) {
  return size_pass(c, o, counts, n_counts, upd_layout(c.in.n_lines), k, lines_kernel, launch_lines, &k_upd_compact<P>,
                   "k_upd_compact");
}

// scan(line, len, nl): the pass's scan_export_line; hit: the table's hit bytes (may be null)
template <class P, class Scan>
int update_size_host(const Entry& c, const UpdCols& o, uint64_t* counts, size_t n_counts, uint8_t* hit, Scan scan) {
  uint64_t rows = 0;
  const int rc = size_pass_host(c, o, counts, n_counts,
                                [&](size_t, uint64_t s, const uint8_t* line, uint64_t len, bool nl) {
    const auto L = scan(line, len, nl);
    counts[P::LONE_CR] += L.lone_cr;
    if constexpr (P::SKIPPED >= 0) counts[P::SKIPPED] += L.skipped;
    counts[P::MISSED] += L.missed;
    if (L.row >= 0 && hit) hit[L.row] = 1;
    if (!L.is_row) return;
    o.row_start[rows] = s;
    o.pk_len[rows] = L.pk_len;
    o.match[rows] = L.row;
    o.out_len[rows] = L.out_len;
    o.flags[rows] = uint8_t(L.flags);
    ++rows;
    counts[P::OUT_BYTES] += L.out_len;
    counts[P::BAD] += (L.flags & P::BAD_BIT) != 0;
    if constexpr (P::HOST_ROWS >= 0) counts[P::HOST_ROWS] += (L.flags & P::HOST_BIT) != 0;
  });
  if (rc || c.in.n_lines == 0) return rc;
  counts[P::ROWS] = rows;
  counts[P::SKIPPED_LINES] = skipped_lines<P>(c.in.n_lines, rows, counts);
  return AVDB_OK;
}

template <uint32_t kStageBytes, class Render>
int update_write(const Entry& c, size_t n_rows, const UpdCols& o, const UpdOut& u, const Work& k, Render render) {
  const Slab& in = c.in;
  if (const char* e = upd_write_error(c, n_rows, o, u)) return invalid(c.fn, e);
  if (int e = rows::begin_write(c.fn, c.ctx, upd_layout(in.n_lines), in.n_lines, k.workspace, k.bytes, o.out_len, n_rows,
                                u.out_cap, u.row_off, u.totals, k.s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL((k_upd_write<kStageBytes, Render>), dim3(stream_grid(n_rows, kBlock, 2048)), dim3(kBlock), 0, k.s,
                     in.text, in.text_bytes, render, o, u.row_off, n_rows, u.out, u.totals);
  AVDB_TABLES_LAUNCH_CHECK("k_upd_write", c.fn);
  return AVDB_OK;
}

template <class Render>
int update_write_host(const Entry& c, size_t n_rows, const UpdCols& o, const UpdOut& u, Render render) {
  const Slab& in = c.in;
  if (const char* e = upd_write_error(c, n_rows, o, u)) return invalid(c.fn, e);
  if (int e = rows::host_row_offsets(c.fn, o.out_len, n_rows, u.out_cap, u.row_off, u.totals)) return e;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < in.text_bytes ? uint32_t(in.text[pos]) : 0u; };
  for (size_t r = 0; r < n_rows; ++r) {
    const UpdRow row{o.row_start[r], o.pk_len[r], o.out_len[r], o.flags[r], o.match[r]};
    const uint64_t off = u.row_off[r];
    render(row, tb, [&](uint32_t k, uint32_t c) { u.out[off + k] = uint8_t(c); });
  }
  return AVDB_OK;
}

}  // namespace tables
}  // namespace avdb

// K12 — the --skipExisting key set built from an export of AnnotatedVDB.Variant
// (gfx950).
//
// Replaces the per-row Python loop of ExistingVariants.from_tsv and its constructor
// (a split, a one-entry list of a dict, two encodes, a repr and three joins per
// exported row) with two passes over the export text on the device:
//   size pass (avdb_existing_size)
//     (avdb_lines.hpp, the front end shared with K10, K13 and K14: one start per line, the marks
//      scanned into row numbers; rows::begin_size)
//     k_exist_lines    one lane per line (lines::for_each_line: 256 lines' text staged
//                      in LDS): from_tsv's row rule, the three field lengths, the row's
//                      flags, the lone '\r' count; 16 bytes of info and a mark per line
//     k_exist_compact  one lane per line: a row's lengths, flags and line start to
//                      its row number; the counts
//   write pass (avdb_existing_write; the workspace, the argument checks and the host entry's
//   offsets are avdb_rows.hpp's, the back end shared with K13 and K14)
//     (exclusive scan of the three length arrays into the three offset arrays)
//     k_exist_totals   the blob totals against the caller's caps
//     k_exist_write    one workgroup per 128 rows: their text staged in LDS, then
//                      each blob's span of the trip written as aligned 8-byte words,
//                      one word per lane (see below)
// The per-line and per-row code is avdb_existing.hpp, shared with the _host entries.
#include "avdb_existing.hpp"
#include "avdb_rows.hpp"

#include <string.h>

namespace avdb {

using exist::Line;
using exist::Row;

// Export lines average about 140 bytes (a metaseq id, a primary key of the same
// length or a refSNP-suffixed one, a 13-level bin path): 256 lines are 36 KB, so the
// size pass stages up to 48 KB (3 workgroups per CU in 160 KB LDS).  The write pass
// takes 128 rows per trip and a 32 KB stage: with its offset and row arrays a
// workgroup holds 37 KB (4 per CU).  A trip whose text does not fit is read from
// global memory.
constexpr uint32_t kExistSizeStage = 48 * 1024;
constexpr uint32_t kExistWriteStage = 32 * 1024;
constexpr uint32_t kTripRows = 128;

// info[li] = {key_len, pk_len, frag_len, flags | is_row << 8}
__global__ __launch_bounds__(kBlock) void k_exist_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                        const uint64_t* __restrict__ starts, size_t n_lines,
                                                        uint32_t contig_mask, u32x4* __restrict__ info,
                                                        uint64_t* __restrict__ mark,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kExistSizeStage / 16];
  uint64_t n_cr = 0;
  lines::for_each_line<kExistSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const Line L = exist::scan_line(line, len, nl, contig_mask);
      info[li] = u32x4{L.key_len, L.pk_len, L.frag_len, L.flags | (L.is_row << 8)};
      mark[li] = L.is_row;
      n_cr += L.lone_cr;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the row count there
  wave_add(&counts[AVDB_EXIST_COUNT_LONE_CR], n_cr);
}

__global__ __launch_bounds__(kBlock) void k_exist_compact(const uint64_t* __restrict__ starts, size_t text_bytes,
                                                          size_t n_lines, const u32x4* __restrict__ info,
                                                          const uint64_t* __restrict__ row_of,
                                                          uint32_t* __restrict__ key_len, uint32_t* __restrict__ pk_len,
                                                          uint32_t* __restrict__ frag_len, uint8_t* __restrict__ flags,
                                                          uint64_t* __restrict__ row_start,
                                                          unsigned long long* __restrict__ counts) {
  uint64_t kb = 0, pb = 0, fb = 0, n_host = 0, n_non = 0;
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const u32x4 v = info[li];
    if (!(v.w >> 8)) continue;
    const uint64_t r = row_of[li];  // r < n_lines: at most one row per line
    uint64_t s = starts[li];
    if (s > text_bytes) s = text_bytes;
    key_len[r] = v.x;
    pk_len[r] = v.y;
    frag_len[r] = v.z;
    flags[r] = uint8_t(v.w);
    row_start[r] = s;
    kb += v.x;
    pb += v.y;
    fb += v.z;
    n_host += (v.w & AVDB_EXIST_FRAG_HOST) != 0;
    n_non += (v.w & AVDB_EXIST_NONCANON) != 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const uint64_t rows = row_of[n_lines];
    counts[AVDB_EXIST_COUNT_ROWS] = rows;
    counts[AVDB_EXIST_COUNT_SKIPPED] = n_lines - rows;
  }
  wave_add(&counts[AVDB_EXIST_COUNT_KEY_BYTES], kb);
  wave_add(&counts[AVDB_EXIST_COUNT_PK_BYTES], pb);
  wave_add(&counts[AVDB_EXIST_COUNT_FRAG_BYTES], fb);
  wave_add(&counts[AVDB_EXIST_COUNT_FRAG_HOST], n_host);
  wave_add(&counts[AVDB_EXIST_COUNT_NONCANON], n_non);
}

struct ExistOut {
  const uint32_t* len[3];  // key_len, pk_len, frag_len
  uint64_t* off[3];        // key_off, pk_off, frag_off (n_rows + 1 entries)
  uint8_t* out[3];         // keys, pks, frag
  uint64_t cap[3];
};

// off[n_rows] = the total of each blob; totals[0..2] the same, totals[3] the number
// of blobs over their cap (the write kernel then writes nothing)
__global__ void k_exist_totals(ExistOut o, size_t n_rows, uint64_t* __restrict__ totals) {
  if (blockIdx.x || threadIdx.x) return;
  uint64_t over = 0;
  for (int a = 0; a < 3; ++a) {
    const uint64_t t = n_rows ? o.off[a][n_rows - 1] + o.len[a][n_rows - 1] : 0ull;
    o.off[a][n_rows] = t;
    totals[a] = t;
    over += t > o.cap[a];
  }
  totals[3] = over;
}

// The write pass stores about 180 bytes per row to three streams.  A lane that
// writes its own row's spans issues one store instruction per 8 bytes with 64
// different cache lines under it (K5's write pass is bound by exactly that).  Here
// the stores follow the output instead: the 128 rows of a trip own one contiguous
// span of each blob, and lane i takes the i-th aligned 8-byte word of that span —
// a wave's store instruction covers 512 contiguous bytes.  The lane finds the row
// its word starts in by a binary search of the trip's offsets (LDS) and gathers the
// word's bytes from the staged text and the fragment's fixed text, crossing into
// the following rows as the word does.  Only the span's two edge words, which it
// shares with the neighbouring trips, and words touching a FRAG_HOST row's fragment
// (left unwritten) are stored bytewise.
template <int S, class T>
__device__ __forceinline__ void write_stream(uint8_t* __restrict__ out, const uint64_t* s_off, const uint64_t* s_foff,
                                             const uint64_t* s_start, const uint32_t* s_kl, const uint32_t* s_pl,
                                             const uint8_t* s_fl, uint32_t nr, T text) {
  const uint64_t b = s_off[0], e = s_off[nr];
  for (uint64_t c = (b & ~7ull) + 8ull * threadIdx.x; c < e; c += 8ull * kBlock) {
    const uint64_t lo = c > b ? c : b, hi = c + 8 < e ? c + 8 : e;
    uint32_t r = 0, R = nr;  // s_off[r] <= lo < s_off[R]
    while (R - r > 1) {
      const uint32_t m = (r + R) / 2;
      if (s_off[m] <= lo) r = m;
      else R = m;
    }
    uint64_t rb = s_off[r], re = s_off[r + 1];
    Row row{s_start[r], s_kl[r], s_pl[r], uint32_t(s_foff[r + 1] - s_foff[r]), s_fl[r]};
    uint64_t word = 0;
    uint32_t keep = 0;
    for (uint64_t p = lo; p < hi; ++p) {
      while (p >= re) {  // (p < e = s_off[nr]: ends at a row of the trip)
        ++r;
        rb = re;
        re = s_off[r + 1];
        row = Row{s_start[r], s_kl[r], s_pl[r], uint32_t(s_foff[r + 1] - s_foff[r]), s_fl[r]};
      }
      const uint32_t k = uint32_t(p - rb), j = uint32_t(p - c);
      uint32_t v;
      if (S == 0) v = exist::key_byte(row, k, text);
      else if (S == 1) v = exist::pk_byte(row, k, text);
      else v = exist::frag_byte(row, k, text);
      word |= uint64_t(v & 0xFFu) << (8 * j);
      if (S != 2 || !(row.flags & AVDB_EXIST_FRAG_HOST)) keep |= 1u << j;
    }
    if (keep == 0xFFu) {
      *reinterpret_cast<uint64_t*>(out + c) = word;
    } else {
      for (uint32_t j = 0; j < 8; ++j)
        if ((keep >> j) & 1u) out[c + j] = uint8_t(word >> (8 * j));
    }
  }
}

__global__ __launch_bounds__(kBlock) void k_exist_write(const uint8_t* __restrict__ text, size_t text_bytes,
                                                        const uint64_t* __restrict__ row_start,
                                                        const uint8_t* __restrict__ flags, ExistOut o, size_t n_rows,
                                                        const uint64_t* __restrict__ totals) {
  __shared__ u32x4 s_text[kExistWriteStage / 16];
  __shared__ uint64_t s_off[3][kTripRows + 1];
  __shared__ uint64_t s_start[kTripRows];
  __shared__ uint32_t s_kl[kTripRows], s_pl[kTripRows];
  __shared__ uint8_t s_fl[kTripRows];
  if (totals[3]) return;  // a cap is too small: nothing is written
  const Heap h = make_heap(text, text_bytes);
  for (size_t r0 = size_t(blockIdx.x) * kTripRows; r0 < n_rows; r0 += size_t(gridDim.x) * kTripRows) {
    const uint32_t nr = n_rows - r0 < kTripRows ? uint32_t(n_rows - r0) : kTripRows;
    const uint32_t t = threadIdx.x;
    if (t <= nr) {
      s_off[0][t] = o.off[0][r0 + t];
      s_off[1][t] = o.off[1][r0 + t];
      s_off[2][t] = o.off[2][r0 + t];
    }
    if (t < nr) {
      uint64_t s = row_start[r0 + t];
      s_start[t] = s < text_bytes ? s : text_bytes;
      s_kl[t] = o.len[0][r0 + t];
      s_pl[t] = o.len[1][r0 + t];
      s_fl[t] = flags[r0 + t];
    }
    // the trip's text: from its first row's line to the line of the next trip's
    // first row (the skipped lines between rows ride along)
    uint64_t s0, s1;
    lines::trip_span(row_start, r0, r0 + nr, n_rows, text_bytes, &s0, &s1);
    const Window w = stage_window<kBlock, kExistWriteStage>(h, s0, s1, s_text);  // (ends in a barrier)
    const lds_cp lds = (lds_cp)(reinterpret_cast<const uint8_t*>(s_text));
    const uint32_t lds0 = uint32_t(h.lo + s0 - w.a0);
    const bool staged = w.staged;
    auto tb = [&](uint64_t pos) -> uint32_t {
      if (pos < s0 || pos >= s1) return 0u;
      return staged ? uint32_t(lds[lds0 + uint32_t(pos - s0)]) : uint32_t(text[pos]);
    };
    write_stream<0>(o.out[0], s_off[0], s_off[2], s_start, s_kl, s_pl, s_fl, nr, tb);
    write_stream<1>(o.out[1], s_off[1], s_off[2], s_start, s_kl, s_pl, s_fl, nr, tb);
    write_stream<2>(o.out[2], s_off[2], s_off[2], s_start, s_kl, s_pl, s_fl, nr, tb);
    __syncthreads();  // the stage and the row arrays are reused by the next trip
  }
}

}  // namespace avdb

using namespace avdb;

// workspace: rows::Layout with 16 bytes of info per line; the write pass scans three length arrays
static rows::Layout exist_layout(size_t n_lines) { return rows::layout(n_lines, 16, 0, 3); }

extern "C" int avdb_existing_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(exist_layout(n_lines).total, bytes);
}

static const char* size_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const uint32_t* key_len, const uint32_t* pk_len, const uint32_t* frag_len,
                                   const uint8_t* flags, const uint64_t* row_off, const uint64_t* counts) {
  if (!ctx || !counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!key_len || !pk_len || !frag_len || !flags || !row_off)) return "null output array";
  return nullptr;
}

static const char* write_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    size_t n_rows, const uint32_t* key_len, const uint32_t* pk_len,
                                    const uint32_t* frag_len, const uint8_t* flags, const uint64_t* row_off,
                                    const ExistOut& o, const uint64_t* totals) {
  if (!ctx || !totals || !o.off[0] || !o.off[1] || !o.off[2]) return "null argument";
  if (const char* err = rows::text_rows_error(text, text_bytes, n_lines, n_rows)) return err;
  if (n_rows && (!key_len || !pk_len || !frag_len || !flags || !row_off)) return "null row array";
  for (int a = 0; a < 3; ++a) {
    if (o.cap[a] && !o.out[a]) return "null blob";
    if (reinterpret_cast<uintptr_t>(o.out[a]) % 8) return "blobs must be 8-byte aligned";
  }
  return nullptr;
}

extern "C" int avdb_existing_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                  uint32_t contig_mask, uint32_t* key_len, uint32_t* pk_len, uint32_t* frag_len,
                                  uint8_t* flags, uint64_t* row_off, uint64_t* counts, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  if (const char* err =
          size_args_error(ctx, text, text_bytes, n_lines, key_len, pk_len, frag_len, flags, row_off, counts)) {
    avdb_set_error("avdb_existing_size: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = exist_layout(n_lines);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_existing_size", ctx, L.total, n_lines, workspace, workspace_bytes, counts,
                               AVDB_EXIST_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* info = reinterpret_cast<u32x4*>(w + L.info);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  const unsigned grid = stream_grid(n_lines, kBlock, 4096);
  auto mark = [&](const uint64_t* starts, uint64_t* marks) {
    hipLaunchKernelGGL(k_exist_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, contig_mask,
                       info, marks, cnt);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_exist_lines", mark)) return e;
  hipLaunchKernelGGL(k_exist_compact, dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const uint64_t*>(w + L.starts),
                     text_bytes, n_lines, info, reinterpret_cast<const uint64_t*>(w + L.row_of), key_len, pk_len,
                     frag_len, flags, row_off, cnt);
  AVDB_LAUNCH_CHECK("k_exist_compact");
  return AVDB_OK;
}

extern "C" int avdb_existing_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   size_t n_rows, const uint32_t* key_len, const uint32_t* pk_len,
                                   const uint32_t* frag_len, const uint8_t* flags, const uint64_t* row_off,
                                   uint8_t* keys, size_t keys_cap, uint64_t* key_off, uint8_t* pks, size_t pks_cap,
                                   uint64_t* pk_off, uint8_t* frag, size_t frag_cap, uint64_t* frag_off,
                                   uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  const ExistOut o{{key_len, pk_len, frag_len}, {key_off, pk_off, frag_off}, {keys, pks, frag},
                   {keys_cap, pks_cap, frag_cap}};
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, n_rows, key_len, pk_len, frag_len, flags,
                                         row_off, o, totals)) {
    avdb_set_error("avdb_existing_write: %s", err);
    return AVDB_EINVAL;
  }
  const rows::Layout L = exist_layout(n_lines);
  if (int e = n_lines ? lines::workspace_error("avdb_existing_write", L.total, workspace, workspace_bytes) : 0) return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  if (n_rows) {
    scan::Arrays<uint32_t, 3> A{{key_len, pk_len, frag_len}, {key_off, pk_off, frag_off}};
    if (int e = scan::exclusive_n(A, n_rows, w + L.scan, L.scan_bytes, s)) return e;
  }
  hipLaunchKernelGGL(k_exist_totals, dim3(1), dim3(kWave), 0, s, o, n_rows, totals);
  AVDB_LAUNCH_CHECK("k_exist_totals");
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL(k_exist_write, dim3(stream_grid(n_rows, kTripRows, 4096)), dim3(kBlock), 0, s, text, text_bytes,
                     row_off, flags, o, n_rows, totals);
  AVDB_LAUNCH_CHECK("k_exist_write");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------
extern "C" int avdb_existing_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                       uint32_t contig_mask, uint32_t* key_len, uint32_t* pk_len, uint32_t* frag_len,
                                       uint8_t* flags, uint64_t* row_off, uint64_t* counts) {
  if (const char* err =
          size_args_error(ctx, text, text_bytes, n_lines, key_len, pk_len, frag_len, flags, row_off, counts)) {
    avdb_set_error("avdb_existing_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_EXIST_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  uint64_t rows = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    bool nl;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e, &nl);
    const Line L = exist::scan_line(text + s, e - s, nl, contig_mask);
    counts[AVDB_EXIST_COUNT_LONE_CR] += L.lone_cr;
    if (!L.is_row) continue;
    key_len[rows] = L.key_len;
    pk_len[rows] = L.pk_len;
    frag_len[rows] = L.frag_len;
    flags[rows] = uint8_t(L.flags);
    row_off[rows] = s;
    ++rows;
    counts[AVDB_EXIST_COUNT_KEY_BYTES] += L.key_len;
    counts[AVDB_EXIST_COUNT_PK_BYTES] += L.pk_len;
    counts[AVDB_EXIST_COUNT_FRAG_BYTES] += L.frag_len;
    counts[AVDB_EXIST_COUNT_FRAG_HOST] += (L.flags & AVDB_EXIST_FRAG_HOST) != 0;
    counts[AVDB_EXIST_COUNT_NONCANON] += (L.flags & AVDB_EXIST_NONCANON) != 0;
  }
  counts[AVDB_EXIST_COUNT_ROWS] = rows;
  counts[AVDB_EXIST_COUNT_SKIPPED] = n_lines - rows;
  return AVDB_OK;
}

extern "C" int avdb_existing_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        size_t n_rows, const uint32_t* key_len, const uint32_t* pk_len,
                                        const uint32_t* frag_len, const uint8_t* flags, const uint64_t* row_off,
                                        uint8_t* keys, size_t keys_cap, uint64_t* key_off, uint8_t* pks,
                                        size_t pks_cap, uint64_t* pk_off, uint8_t* frag, size_t frag_cap,
                                        uint64_t* frag_off, uint64_t* totals) {
  const ExistOut o{{key_len, pk_len, frag_len}, {key_off, pk_off, frag_off}, {keys, pks, frag},
                   {keys_cap, pks_cap, frag_cap}};
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, n_rows, key_len, pk_len, frag_len, flags,
                                         row_off, o, totals)) {
    avdb_set_error("avdb_existing_write_host: %s", err);
    return AVDB_EINVAL;
  }
  totals[3] = 0;
  for (int a = 0; a < 3; ++a) totals[3] += rows::host_offsets(o.len[a], n_rows, o.cap[a], o.off[a], &totals[a]);
  if (totals[3]) {
    avdb_set_error("avdb_existing_write_host: blobs of %llu / %llu / %llu bytes required",
                   (unsigned long long)totals[0], (unsigned long long)totals[1], (unsigned long long)totals[2]);
    return AVDB_ERANGE;
  }
  if (n_rows == 0) return AVDB_OK;
  for (size_t r = 0; r < n_rows; ++r) {
    const uint64_t s0 = row_off[r] < text_bytes ? row_off[r] : text_bytes;
    const uint64_t s1 = r + 1 < n_rows && row_off[r + 1] >= s0 && row_off[r + 1] <= text_bytes ? row_off[r + 1] : text_bytes;
    auto tb = [&](uint64_t pos) -> uint32_t { return pos >= s0 && pos < s1 ? text[pos] : 0u; };
    const Row row{s0, key_len[r], pk_len[r], frag_len[r], flags[r]};
    for (uint32_t k = 0; k < row.key_len; ++k) keys[key_off[r] + k] = uint8_t(exist::key_byte(row, k, tb));
    for (uint32_t k = 0; k < row.pk_len; ++k) pks[pk_off[r] + k] = uint8_t(exist::pk_byte(row, k, tb));
    if (!(row.flags & AVDB_EXIST_FRAG_HOST))
      for (uint32_t k = 0; k < row.frag_len; ++k) frag[frag_off[r] + k] = uint8_t(exist::frag_byte(row, k, tb));
  }
  return AVDB_OK;
}

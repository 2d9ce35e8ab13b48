// K10 — CADD score annotation (gfx950).
//
// Replaces CADDUpdater.buffer_variant's per-variant tabix fetch, row scan and
// allele membership test (Util/lib/python/loaders/cadd_updater.py:175-221, driven
// by Load/bin/load_cadd_scores.py) with a table built once from the CADD text and
// a sort-merge join of each record batch against it:
//   (avdb_lines.hpp, shared with K12: one start per line, the marks scanned into row numbers)
//   k_cadd_mark    one lane per line: 1 for a data line (not empty, not '#')
//   k_cadd_parse   one lane per line (lines::for_each_line: 256 lines' text staged in
//                  LDS): tab fields, contig code, POS, allele spans (offsets into the slab,
//                  nothing copied), the two scores as correctly rounded doubles (parse_score)
//   k_cadd_index   one lane per row: run starts / ends per contig -> first_row /
//                  end_row, and the order violations tabix would refuse
//   k_cadd_match   one lane per record: table by allele lengths, lower_bound of pos
//                  in the contig's rows, first row at pos passing the reference's
//                  membership test; a position-sorted batch sends neighbouring
//                  lanes to neighbouring rows
// The per-line and per-record code is avdb_cadd.hpp, shared with the _host entries.
#include "avdb_cadd.hpp"

#include <string.h>

namespace avdb {

using cadd::Cols;
using cadd::View;

constexpr uint32_t kCaddStage = 16 * 1024;  // 256 lines of up to 64 bytes on average

__global__ __launch_bounds__(kBlock) void k_cadd_mark(const uint8_t* __restrict__ text, size_t text_bytes,
                                                      const uint64_t* __restrict__ starts, size_t n_lines,
                                                      uint64_t* __restrict__ mark) {
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li <= n_lines; li += size_t(gridDim.x) * blockDim.x) {
    uint64_t m = 0;
    if (li < n_lines) {
      uint64_t s, e;
      lines::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
      m = cadd::is_data_line(text, s, e);
    }
    mark[li] = m;  // mark[n_lines] = 0: the scan leaves the row count there
  }
}

__global__ __launch_bounds__(kBlock) void k_cadd_parse(const uint8_t* __restrict__ text, size_t text_bytes,
                                                       const uint64_t* __restrict__ starts, size_t n_lines,
                                                       const uint64_t* __restrict__ row_of, Cols o,
                                                       unsigned long long* __restrict__ counts) {
  // (reading global bytes this kernel took 12.6 ms of a 17.3 ms build of 104 M lines; staged, the build takes 9.4 ms)
  __shared__ u32x4 s_text[kCaddStage / 16];
  uint32_t n_host = 0, n_bad = 0;
  lines::for_each_line<kCaddStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    const uint64_t r = row_of[li];
    if (row_of[li + 1] == r) return;  // not a data line
    with_line([&](uint64_t s, uint64_t len, bool, auto line) {
      const uint32_t f = cadd::parse_row(line, s, len, r, o);
      n_host += (f & AVDB_CADD_ROW_SCORE_HOST) != 0;
      n_bad += (f & AVDB_CADD_ROW_BAD) != 0;
    });
  });
  if (blockIdx.x == 0 && threadIdx.x == 0) counts[AVDB_CADD_COUNT_ROWS] = row_of[n_lines];
  wave_add(&counts[AVDB_CADD_COUNT_SCORE_HOST], n_host);
  wave_add(&counts[AVDB_CADD_COUNT_BAD], n_bad);
}

// runs: u32[kContigs] run starts seen per contig (zeroed by the caller)
__global__ __launch_bounds__(kBlock) void k_cadd_index(const uint8_t* __restrict__ chrom, uint32_t* pos,
                                                       const uint8_t* __restrict__ flags,
                                                       const uint64_t* __restrict__ n_rows_p, size_t max_rows,
                                                       uint32_t* __restrict__ first_row, uint32_t* __restrict__ end_row,
                                                       uint32_t* __restrict__ runs,
                                                       unsigned long long* __restrict__ counts) {
  uint64_t n = *n_rows_p;
  if (n > max_rows) n = max_rows;
  uint32_t viol = 0;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    const cadd::IndexEvent ev = cadd::index_row(chrom, pos, flags, n, i);
    viol += ev.violation;
    if (ev.contig < cadd::kContigs) {
      if (ev.start) {
        atomicMin(&first_row[ev.contig], uint32_t(i));
        if (atomicAdd(&runs[ev.contig], 1u) != 0) ++viol;  // a second run of this contig
      }
      if (ev.end) atomicMax(&end_row[ev.contig], uint32_t(i + 1));
    }
  }
  wave_add(&counts[AVDB_CADD_COUNT_ORDER_VIOLATIONS], viol);
}

__global__ __launch_bounds__(kBlock) void k_cadd_match(View snv, View indel, const uint8_t* __restrict__ chrom,
                                                       const uint32_t* __restrict__ pos,
                                                       const uint64_t* __restrict__ off,
                                                       const uint32_t* __restrict__ rl, const uint32_t* __restrict__ al,
                                                       const uint8_t* __restrict__ heap, size_t heap_bytes, size_t n,
                                                       int32_t* __restrict__ row, uint8_t* __restrict__ kind,
                                                       double* __restrict__ raw, double* __restrict__ phred,
                                                       unsigned long long* __restrict__ ctr) {
  uint32_t n_snv = 0, n_indel = 0, n_none = 0;
  for (size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += size_t(gridDim.x) * blockDim.x) {
    int32_t r;
    double x, y;
    const uint32_t k = cadd::match_record(snv, indel, chrom[i], pos[i], heap, heap_bytes, off[i], rl[i], al[i], &r, &x, &y);
    row[i] = r;
    kind[i] = uint8_t(k);
    if (r >= 0) {
      raw[i] = x;
      phred[i] = y;
    }
    n_snv += k == AVDB_CADD_SNV;
    n_indel += k == AVDB_CADD_INDEL;
    n_none += k == AVDB_CADD_NONE;
  }
  if (ctr) {
    wave_add(&ctr[AVDB_CADD_CTR_SNV], n_snv);
    wave_add(&ctr[AVDB_CADD_CTR_INDEL], n_indel);
    wave_add(&ctr[AVDB_CADD_CTR_NOT_MATCHED], n_none);
  }
}

}  // namespace avdb

using namespace avdb;

// workspace: lines::Layout | scan temp | runs
struct CaddLayout : lines::Layout {
  size_t runs, total;
};
static CaddLayout cadd_layout(size_t n_lines) {
  CaddLayout L{lines::layout(n_lines)};
  L.scan = L.next;
  L.scan_bytes = lines::pad256(scan::workspace_bytes(n_lines + 1));
  L.runs = L.scan + L.scan_bytes;
  L.total = L.runs + 256;
  return L;
}

extern "C" int avdb_cadd_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  if (!bytes) return AVDB_EINVAL;
  *bytes = cadd_layout(n_lines).total;
  return AVDB_OK;
}

static const char* build_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const Cols& o, const uint32_t* first_row, const uint32_t* end_row,
                                    const uint64_t* counts) {
  if (!ctx || !first_row || !end_row || !counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (n_lines && (!o.chrom || !o.pos || !o.ref_off || !o.ref_len || !o.alt_off || !o.alt_len || !o.raw || !o.phred ||
                  !o.flags))
    return "null column";
  return nullptr;
}

extern "C" int avdb_cadd_table_build(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     uint8_t* chrom, uint32_t* pos, uint64_t* ref_off, uint32_t* ref_len,
                                     uint64_t* alt_off, uint32_t* alt_len, double* raw, double* phred, uint8_t* flags,
                                     uint32_t* first_row, uint32_t* end_row, uint64_t* counts, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  const Cols o{chrom, pos, ref_off, ref_len, alt_off, alt_len, raw, phred, flags};
  if (const char* err = build_args_error(ctx, text, text_bytes, n_lines, o, first_row, end_row, counts)) {
    avdb_set_error("avdb_cadd_table_build: %s", err);
    return AVDB_EINVAL;
  }
  const CaddLayout L = cadd_layout(n_lines);
  if (n_lines)
    if (int e = lines::workspace_error("avdb_cadd_table_build", L.total, workspace, workspace_bytes)) return e;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  AVDB_HIP_TRY(hipMemsetAsync(counts, 0, 8 * AVDB_CADD_N_COUNTS, s));
  AVDB_HIP_TRY(hipMemsetAsync(first_row, 0xFF, 4 * AVDB_CADD_N_CONTIGS, s));
  AVDB_HIP_TRY(hipMemsetAsync(end_row, 0, 4 * AVDB_CADD_N_CONTIGS, s));
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* starts = reinterpret_cast<const uint64_t*>(w + L.starts);
  auto* row_of = reinterpret_cast<const uint64_t*>(w + L.row_of);
  auto* runs = reinterpret_cast<uint32_t*>(w + L.runs);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  AVDB_HIP_TRY(hipMemsetAsync(runs, 0, 256, s));
  const unsigned grid = stream_grid(n_lines + 1, kBlock, 4096);
  auto mark = [&](const uint64_t* st, uint64_t* marks) {
    hipLaunchKernelGGL(k_cadd_mark, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, st, n_lines, marks);
  };
  if (int e = lines::number_rows(text, text_bytes, n_lines, w, L, s, "k_cadd_mark", mark)) return e;
  hipLaunchKernelGGL(k_cadd_parse, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, row_of, o, cnt);
  AVDB_LAUNCH_CHECK("k_cadd_parse");
  hipLaunchKernelGGL(k_cadd_index, dim3(grid), dim3(kBlock), 0, s, chrom, pos, flags, row_of + n_lines, n_lines,
                     first_row, end_row, runs, cnt);
  AVDB_LAUNCH_CHECK("k_cadd_index");
  return AVDB_OK;
}

static const char* match_args_error(const void* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel, View* vs,
                                    View* vi, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                                    const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t n,
                                    const int32_t* row, const uint8_t* kind, const double* raw, const double* phred) {
  if (!ctx) return "null context";
  const char* err = nullptr;
  if (!cadd::table_view(snv, vs, &err) || !cadd::table_view(indel, vi, &err)) return err;
  if (n == 0) return nullptr;
  if (!chrom || !pos || !allele_off || !ref_len || !alt_len || !heap) return "null record array";
  if (!row || !kind || !raw || !phred) return "null output array";
  return nullptr;
}

extern "C" int avdb_cadd_match(avdb_ctx* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                               const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                               const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap,
                               size_t heap_bytes, size_t n, int32_t* row, uint8_t* kind, double* raw, double* phred,
                               uint64_t* counters, void* stream) {
  View vs, vi;
  if (const char* err = match_args_error(ctx, snv, indel, &vs, &vi, chrom, pos, allele_off, ref_len, alt_len, heap, n,
                                         row, kind, raw, phred)) {
    avdb_set_error("avdb_cadd_match: %s", err);
    return AVDB_EINVAL;
  }
  if (n == 0) return AVDB_OK;
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_cadd_match, dim3(stream_grid(n, kBlock, 4096)), dim3(kBlock), 0,
                     static_cast<hipStream_t>(stream), vs, vi, chrom, pos, allele_off, ref_len, alt_len, heap,
                     heap_bytes, n, row, kind, raw, phred, reinterpret_cast<unsigned long long*>(counters));
  AVDB_LAUNCH_CHECK("k_cadd_match");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------
extern "C" int avdb_cadd_table_build_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          uint8_t* chrom, uint32_t* pos, uint64_t* ref_off, uint32_t* ref_len,
                                          uint64_t* alt_off, uint32_t* alt_len, double* raw, double* phred,
                                          uint8_t* flags, uint32_t* first_row, uint32_t* end_row, uint64_t* counts) {
  const Cols o{chrom, pos, ref_off, ref_len, alt_off, alt_len, raw, phred, flags};
  if (const char* err = build_args_error(ctx, text, text_bytes, n_lines, o, first_row, end_row, counts)) {
    avdb_set_error("avdb_cadd_table_build_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_CADD_N_COUNTS);
  memset(first_row, 0xFF, 4 * AVDB_CADD_N_CONTIGS);
  memset(end_row, 0, 4 * AVDB_CADD_N_CONTIGS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  uint64_t rows = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e);
    if (!cadd::is_data_line(text, s, e)) continue;
    const uint32_t f = cadd::parse_row(text + s, s, e - s, rows++, o);
    counts[AVDB_CADD_COUNT_SCORE_HOST] += (f & AVDB_CADD_ROW_SCORE_HOST) != 0;
    counts[AVDB_CADD_COUNT_BAD] += (f & AVDB_CADD_ROW_BAD) != 0;
  }
  counts[AVDB_CADD_COUNT_ROWS] = rows;
  uint32_t runs[AVDB_CADD_N_CONTIGS] = {};
  for (uint64_t i = 0; i < rows; ++i) {
    const cadd::IndexEvent ev = cadd::index_row(chrom, pos, flags, rows, i);
    uint64_t viol = ev.violation;
    if (ev.contig < cadd::kContigs) {
      if (ev.start) {
        if (uint32_t(i) < first_row[ev.contig]) first_row[ev.contig] = uint32_t(i);
        if (runs[ev.contig]++ != 0) ++viol;
      }
      if (ev.end && uint32_t(i + 1) > end_row[ev.contig]) end_row[ev.contig] = uint32_t(i + 1);
    }
    counts[AVDB_CADD_COUNT_ORDER_VIOLATIONS] += viol;
  }
  return AVDB_OK;
}

extern "C" int avdb_cadd_match_host(const avdb_ctx* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel,
                                    const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                                    const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap,
                                    size_t heap_bytes, size_t n, int32_t* row, uint8_t* kind, double* raw,
                                    double* phred, uint64_t* counters) {
  View vs, vi;
  if (const char* err = match_args_error(ctx, snv, indel, &vs, &vi, chrom, pos, allele_off, ref_len, alt_len, heap, n,
                                         row, kind, raw, phred)) {
    avdb_set_error("avdb_cadd_match_host: %s", err);
    return AVDB_EINVAL;
  }
  for (size_t i = 0; i < n; ++i) {
    double x, y;
    const uint32_t k = cadd::match_record(vs, vi, chrom[i], pos[i], heap, heap_bytes, allele_off[i], ref_len[i],
                                          alt_len[i], &row[i], &x, &y);
    kind[i] = uint8_t(k);
    if (row[i] >= 0) {
      raw[i] = x;
      phred[i] = y;
    }
    if (counters && k != AVDB_CADD_HOST)
      ++counters[k == AVDB_CADD_SNV ? AVDB_CADD_CTR_SNV : k == AVDB_CADD_INDEL ? AVDB_CADD_CTR_INDEL
                                                                               : AVDB_CADD_CTR_NOT_MATCHED];
  }
  return AVDB_OK;
}

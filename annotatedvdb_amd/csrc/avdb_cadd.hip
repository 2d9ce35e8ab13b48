// K10 — CADD score annotation (gfx950).
//
// Replaces CADDUpdater.buffer_variant's per-variant tabix fetch, row scan and
// allele membership test (Util/lib/python/loaders/cadd_updater.py:175-221, driven
// by Load/bin/load_cadd_scores.py) with a table built once from the CADD text and
// a sort-merge join of each record batch against it:
//   (K0's count and line-starts passes, avdb::text_line_starts: one start per line)
//   k_cadd_mark    one lane per line: 1 for a data line (not empty, not '#'); the
//                  exclusive scan of the marks (avdb_scan.hpp) numbers the rows
//   k_cadd_parse   one lane per line (256 lines' text staged in LDS): tab fields,
//                  contig code, POS, allele spans
//                  (offsets into the slab, nothing copied), the two scores as
//                  correctly rounded doubles (avdb_cadd.hpp parse_score)
//   k_cadd_index   one lane per row: run starts / ends per contig -> first_row /
//                  end_row, and the order violations tabix would refuse
//   k_cadd_match   one lane per record: table by allele lengths, lower_bound of pos
//                  in the contig's rows, first row at pos passing the reference's
//                  membership test; a position-sorted batch sends neighbouring
//                  lanes to neighbouring rows
// The per-line and per-record code is avdb_cadd.hpp, shared with the _host entries.
#include "avdb_cadd.hpp"

#include "avdb_scan.hpp"
#include "avdb_text.hpp"

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
      cadd::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
      m = cadd::is_data_line(text, s, e);
    }
    mark[li] = m;  // mark[n_lines] = 0: the scan leaves the row count there
  }
}

__device__ __forceinline__ void wave_add(unsigned long long* dst, uint32_t v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, kWave);
  if (__lane_id() == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

__global__ __launch_bounds__(kBlock) void k_cadd_parse(const uint8_t* __restrict__ text, size_t text_bytes,
                                                       const uint64_t* __restrict__ starts, size_t n_lines,
                                                       const uint64_t* __restrict__ row_of, Cols o,
                                                       unsigned long long* __restrict__ counts) {
  // 256 consecutive lines per trip, their text staged in LDS with coalesced 16-byte
  // loads (as k_vcf_parse): a lane's byte-by-byte walk of its line then waits on LDS,
  // not on one global round trip per byte (reading global bytes this kernel took
  // 12.6 ms of a 17.3 ms build of 104 M lines; staged, the build takes 9.4 ms).  A
  // span over kCaddStage bytes is parsed from global memory.
  __shared__ u32x4 s_text[kCaddStage / 16];
  const Heap h = make_heap(text, text_bytes);
  uint32_t n_host = 0, n_bad = 0;
  for (size_t base = size_t(blockIdx.x) * kBlock; base < n_lines; base += size_t(gridDim.x) * kBlock) {
    const size_t last = base + kBlock < n_lines ? base + kBlock : n_lines;
    uint64_t s0 = starts[base], s1 = last < n_lines ? starts[last] : text_bytes;
    if (s0 > text_bytes) s0 = text_bytes;
    if (s1 > text_bytes || s1 < s0) s1 = text_bytes;
    const Window w = stage_window<kBlock, kCaddStage>(h, s0, s1, s_text);
    const size_t li = base + threadIdx.x;
    if (li < n_lines) {
      const uint64_t r = row_of[li];
      if (row_of[li + 1] != r) {  // a data line
        uint64_t s, e;
        cadd::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
        uint32_t f;
        if (w.staged && s >= s0 && e <= s1)
          f = cadd::parse_row((lds_cp)(reinterpret_cast<const uint8_t*>(s_text) + (h.lo + s - w.a0)), s, e - s, r, o);
        else
          f = cadd::parse_row((glb_cp)(text + s), s, e - s, r, o);
        n_host += (f & AVDB_CADD_ROW_SCORE_HOST) != 0;
        n_bad += (f & AVDB_CADD_ROW_BAD) != 0;
      }
    }
    __syncthreads();  // the stage is reused by the next trip
  }
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

static size_t pad256(size_t x) { return (x + 255) & ~size_t(255); }

// workspace: count workspace | line starts | marks / row numbers | scan temp | runs
struct CaddLayout {
  size_t starts, row_of, scan, scan_bytes, runs, total;
};
static CaddLayout cadd_layout(size_t n_lines) {
  CaddLayout L;
  L.starts = AVDB_VCF_COUNT_WORKSPACE_BYTES;
  L.row_of = L.starts + pad256(8 * n_lines);
  L.scan = L.row_of + pad256(8 * (n_lines + 1));
  L.scan_bytes = pad256(scan::workspace_bytes(n_lines + 1));
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
  if (text_bytes && !text) return "null text";
  if (n_lines >= 0x7FFFFFFFull) return "too many lines (rows are numbered in int32)";
  if (n_lines > text_bytes) return "more lines than text bytes";
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
  if (n_lines && (!workspace || workspace_bytes < L.total || reinterpret_cast<uintptr_t>(workspace) % 256)) {
    avdb_set_error("avdb_cadd_table_build: 256-byte aligned workspace of %zu bytes required", L.total);
    return AVDB_ERANGE;
  }
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  AVDB_HIP_TRY(hipMemsetAsync(counts, 0, 8 * AVDB_CADD_N_COUNTS, s));
  AVDB_HIP_TRY(hipMemsetAsync(first_row, 0xFF, 4 * AVDB_CADD_N_CONTIGS, s));
  AVDB_HIP_TRY(hipMemsetAsync(end_row, 0, 4 * AVDB_CADD_N_CONTIGS, s));
  if (n_lines == 0) return AVDB_OK;
  char* w = static_cast<char*>(workspace);
  auto* starts = reinterpret_cast<uint64_t*>(w + L.starts);
  auto* row_of = reinterpret_cast<uint64_t*>(w + L.row_of);
  auto* runs = reinterpret_cast<uint32_t*>(w + L.runs);
  auto* cnt = reinterpret_cast<unsigned long long*>(counts);
  AVDB_HIP_TRY(hipMemsetAsync(runs, 0, 256, s));
  // a start the starts pass does not write (n_lines above the text's own count)
  // stays past the text: line_span reads such a line as empty
  AVDB_HIP_TRY(hipMemsetAsync(starts, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, w, starts, s)) return e;
  const unsigned grid = stream_grid(n_lines + 1, kBlock, 4096);
  hipLaunchKernelGGL(k_cadd_mark, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, row_of);
  AVDB_LAUNCH_CHECK("k_cadd_mark");
  if (int e = scan::exclusive_u64(row_of, row_of, n_lines + 1, w + L.scan, L.scan_bytes, s)) return e;
  hipLaunchKernelGGL(k_cadd_parse, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, row_of, o, cnt);
  AVDB_LAUNCH_CHECK("k_cadd_parse");
  hipLaunchKernelGGL(k_cadd_index, dim3(grid), dim3(kBlock), 0, s, chrom, pos, flags, row_of + n_lines, n_lines,
                     first_row, end_row, runs, cnt);
  AVDB_LAUNCH_CHECK("k_cadd_index");
  return AVDB_OK;
}

// a caller's table as the join reads it; false: a struct this library cannot read
static bool cadd_view(const avdb_cadd_table* t, View* v, const char** err) {
  *v = View{};
  if (!t) return true;
  if (t->struct_size != sizeof(avdb_cadd_table)) { *err = "avdb_cadd_table.struct_size does not match this library"; return false; }
  if (t->n_rows == 0) return true;
  if (t->n_rows >= 0x7FFFFFFFull) { *err = "table of 2^31 rows or more"; return false; }
  if (!t->text || !t->chrom || !t->pos || !t->ref_off || !t->ref_len || !t->alt_off || !t->alt_len || !t->raw ||
      !t->phred || !t->flags || !t->first_row || !t->end_row) {
    *err = "null table column";
    return false;
  }
  *v = View{t->n_rows, t->text,  t->chrom, t->pos,   t->ref_off,   t->ref_len, t->alt_off,
            t->alt_len, t->raw, t->phred, t->flags, t->first_row, t->end_row};
  return true;
}

static const char* match_args_error(const void* ctx, const avdb_cadd_table* snv, const avdb_cadd_table* indel, View* vs,
                                    View* vi, const uint8_t* chrom, const uint32_t* pos, const uint64_t* allele_off,
                                    const uint32_t* ref_len, const uint32_t* alt_len, const uint8_t* heap, size_t n,
                                    const int32_t* row, const uint8_t* kind, const double* raw, const double* phred) {
  if (!ctx) return "null context";
  const char* err = nullptr;
  if (!cadd_view(snv, vs, &err) || !cadd_view(indel, vi, &err)) return err;
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
  // line 0 starts at 0, line k + 1 after the k-th newline (as k_vcf_starts)
  std::vector<uint64_t> starts(n_lines, ~0ull);
  starts[0] = 0;
  size_t k = 1;
  for (size_t i = 0; i < text_bytes && k < n_lines; ++i)
    if (text[i] == '\n') starts[k++] = i + 1;
  uint64_t rows = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    cadd::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e);
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

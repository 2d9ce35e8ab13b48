// The front end of the passes over a '\n'-separated text slab (K10, avdb_cadd.hip; K12,
// avdb_existing.hip; K13, avdb_caddupd.hip; K14, avdb_expvcf.hip; the line spans also K15,
// avdb_splitvcf.hip): one start per line, the lines walked 256 per workgroup trip with their text
// staged in LDS, a mark per line scanned into row numbers.  What follows the row numbers in the
// two-pass exports (workspace, prologues, offsets and totals, the staged row writer) is
// avdb_rows.hpp.  Compiled for both sides, as avdb_cadd.hpp is.
#pragma once

#include "avdb_scan.hpp"
#include "avdb_text.hpp"

namespace avdb {

// K0's count pass + line-starts pass over any '\n'-separated text (avdb_vcf.hip):
// starts[0 .. n_lines); count_ws of AVDB_VCF_COUNT_WORKSPACE_BYTES bytes
int text_line_starts(const uint8_t* text, size_t text_bytes, size_t n_lines, void* count_ws, uint64_t* starts,
                     hipStream_t s);

namespace lines {

// line li of the text is bytes [*s, *e) without its '\n'; *nl (if asked for): a '\n' ends it.
// starts[] comes from the line-starts pass; a start the caller's n_lines does not
// bear out gives an empty span, so nothing is read outside the text.
AVDB_HD void line_span(const uint8_t* text, uint64_t text_bytes, const uint64_t* starts, uint64_t n_lines, uint64_t li,
                       uint64_t* s, uint64_t* e, bool* nl = nullptr) {
  uint64_t a = starts[li];
  const bool last = li + 1 >= n_lines || starts[li + 1] > text_bytes;
  uint64_t b = last ? text_bytes : starts[li + 1] - 1;
  if (a > text_bytes) a = text_bytes;
  if (b > text_bytes) b = text_bytes;
  if (b < a) b = a;
  const bool own_nl = last && b > a && text[b - 1] == '\n';  // the last line's own newline
  *s = a;
  *e = own_nl ? b - 1 : b;
  if (nl) *nl = !last || own_nl;
}

// the host entries' starts: line 0 at 0, line k + 1 after the k-th newline (as k_vcf_starts)
inline std::vector<uint64_t> host_line_starts(const uint8_t* text, size_t text_bytes, size_t n_lines) {
  std::vector<uint64_t> starts(n_lines, ~0ull);
  if (n_lines) starts[0] = 0;
  size_t k = 1;
  for (size_t i = 0; i < text_bytes && k < n_lines; ++i)
    if (text[i] == '\n') starts[k++] = i + 1;
  return starts;
}

// [*s0, *s1): the text of entries [first, last) of at[0 .. n) (line starts, or those of rows), clamped to the text
AVDB_HD void trip_span(const uint64_t* at, size_t first, size_t last, size_t n, uint64_t text_bytes, uint64_t* s0,
                       uint64_t* s1) {
  const uint64_t a = at[first] < text_bytes ? at[first] : text_bytes, b = last < n ? at[last] : text_bytes;
  *s0 = a;
  *s1 = b > text_bytes || b < a ? text_bytes : b;
}

// A workgroup's walk over the lines, kBlock consecutive lines per trip and one lane per
// line, the trip's text staged in the caller's kStageBytes of LDS with coalesced 16-byte
// loads (as k_vcf_parse): a lane's byte-by-byte walk of its line waits on LDS, not on a
// global round trip per byte.  f(li, with_line) runs for every line; with_line(g) calls
// g(s, len, nl, p): the line as line_span gives it, p pointing to its bytes, an lds_cp, or
// a glb_cp where the trip's span does not fit the stage.
template <uint32_t kStageBytes, class F>
__device__ __forceinline__ void for_each_line(const uint8_t* __restrict__ text, size_t text_bytes,
                                              const uint64_t* __restrict__ starts, size_t n_lines, u32x4* s_text, F f) {
  const Heap h = make_heap(text, text_bytes);
  for (size_t base = size_t(blockIdx.x) * kBlock; base < n_lines; base += size_t(gridDim.x) * kBlock) {
    const size_t last = base + kBlock < n_lines ? base + kBlock : n_lines;
    uint64_t s0, s1;
    trip_span(starts, base, last, n_lines, text_bytes, &s0, &s1);
    const Window w = stage_window<kBlock, kStageBytes>(h, s0, s1, s_text);
    const size_t li = base + threadIdx.x;
    if (li < n_lines)
      f(li, [&](auto g) {
        uint64_t s, e;
        bool nl;
        line_span(text, text_bytes, starts, n_lines, li, &s, &e, &nl);
        if (w.staged && s >= s0 && e <= s1)
          g(s, e - s, nl, (lds_cp)(reinterpret_cast<const uint8_t*>(s_text) + (h.lo + s - w.a0)));
        else
          g(s, e - s, nl, (glb_cp)(text + s));
      });
    __syncthreads();  // the stage is reused by the next trip
  }
}

inline size_t pad256(size_t x) { return (x + 255) & ~size_t(255); }

// a table's workspace: count workspace | line starts | marks / row numbers | from next: its own, the scan's temp too
struct Layout {
  size_t starts, row_of, next, scan, scan_bytes;
};
inline Layout layout(size_t n_lines) {
  const size_t starts = AVDB_VCF_COUNT_WORKSPACE_BYTES, row_of = starts + pad256(8 * n_lines);
  return Layout{starts, row_of, row_of + pad256(8 * (n_lines + 1)), 0, 0};
}

inline int workspace_error(const char* fn, size_t total, const void* workspace, size_t workspace_bytes) {
  if (workspace && workspace_bytes >= total && reinterpret_cast<uintptr_t>(workspace) % 256 == 0) return AVDB_OK;
  avdb_set_error("%s: 256-byte aligned workspace of %zu bytes required", fn, total);
  return AVDB_ERANGE;
}

inline const char* text_args_error(const uint8_t* text, size_t text_bytes, size_t n_lines) {
  if (text_bytes && !text) return "null text";
  if (n_lines >= 0x7FFFFFFFull) return "too many lines (rows are numbered in int32)";
  if (n_lines > text_bytes) return "more lines than text bytes";
  return nullptr;
}

// The line starts (one the starts pass does not write, n_lines above the text's own count, stays
// past the text: line_span reads such a line as empty), the caller's mark kernel (launch(starts,
// row_of) launches it: 1 per row and row_of[n_lines] = 0), then the marks scanned in place: row_of[li]
// is line li's row number and row_of[n_lines] the row count.  w: the workspace L lays out.
template <class Launch>
inline int number_rows(const uint8_t* text, size_t text_bytes, size_t n_lines, char* w, const Layout& L, hipStream_t s,
                       const char* mark_kernel, Launch launch) {
  uint64_t *starts = reinterpret_cast<uint64_t*>(w + L.starts), *row_of = reinterpret_cast<uint64_t*>(w + L.row_of);
  AVDB_HIP_TRY(hipMemsetAsync(starts, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, w, starts, s)) return e;
  launch(starts, row_of);
  AVDB_LAUNCH_CHECK(mark_kernel);
  return scan::exclusive_u64(row_of, row_of, n_lines + 1, w + L.scan, L.scan_bytes, s);
}

}  // namespace lines
}  // namespace avdb

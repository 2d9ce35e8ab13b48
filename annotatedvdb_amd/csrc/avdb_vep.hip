// K18a — VEP's JSON lines: every consequence ranked, and the order they end up in (gfx950).
//
// Replaces, for the four <type>_consequences keys, the json.loads, the two deepcopies and the
// Python sort per line of Load/bin/load_vep_result.py on VepJsonParser
// (adsp_rank_and_sort_consequences, vep_parser.py:145-175) with two passes in the house shape:
//   size pass (avdb_vep_index_size)
//     (K0's count and line-starts passes)
//     k_vep_index<false>  one wave per line, 64 bytes a step: the block's bytes as 64-bit ballots,
//                         the escaped quotes, the string mask and the depth from them with one
//                         carry each over the block edge; the keys read back from the bracket or
//                         quote behind them; a line's elements collected in LDS (allele span, term
//                         mask), each looked up in the ranking; per line its count, its flags byte
//                         and the spans of `input` and `id`
//   write pass (avdb_vep_index_write; the caller scanned the counts)
//     k_vep_index<true>   the same walk for the lines the device answers, then per line the rows
//                         in text order, each element's allele group and its place in the order
//                         (type, the allele's first appearance, rank, index): quadratic per line,
//                         AVDB_VEP_MAX_CSQ bounds it
// The per-block code is avdb_vep.hpp, shared with the _host entries.
#include "avdb_vep.hpp"
#include "avdb_rows.hpp"

#include <string.h>

namespace avdb {

using namespace vep;

struct DevOps {
  static __device__ __forceinline__ void add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
  static __device__ __forceinline__ uint64_t or64(uint64_t* p, uint64_t v) {
    return atomicOr(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
  }
};
struct HostOps {
  static void add(uint32_t* p, uint32_t v) { *p += v; }
  static uint64_t or64(uint64_t* p, uint64_t v) {
    const uint64_t old = *p;
    *p |= v;
    return old;
  }
};

struct LineCols {
  uint32_t* n_csq;
  uint8_t* flags;
  uint8_t* types;
  uint64_t* input_start;
  int32_t* input_len;
  uint64_t* id_start;
  int32_t* id_len;
};

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v |= uint32_t(__shfl_xor(int(v), d, kWave));
  return v;
}

// ctr: the size pass's counts, or the write pass's totals
template <bool kWrite>
__global__ __launch_bounds__(kWave) void k_vep_index(const uint8_t* __restrict__ text, size_t text_bytes,
                                                     const uint64_t* __restrict__ starts, size_t n_lines, TableView tab,
                                                     LineCols lc, const uint64_t* __restrict__ csq_off, uint64_t n_total,
                                                     CsqOut out, unsigned long long* __restrict__ ctr) {
  __shared__ Elem s_el[kMaxCsq];
  __shared__ uint32_t s_term_len[64], s_term_off[64];  // a term lookup walks these: LDS, not a global load a step
  const uint32_t lane = __lane_id();
  if (lane < tab.n_terms) {
    s_term_len[lane] = tab.term_len[lane];
    s_term_off[lane] = tab.term_off[lane];
  }
  __syncthreads();
  tab.term_len = s_term_len;
  tab.term_off = s_term_off;
  const Heap h = make_heap(text, text_bytes);
  unsigned long long acc = 0;  // lane k: what this wave adds to ctr[k]
  for (size_t li = blockIdx.x; li < n_lines; li += gridDim.x) {
    uint64_t s, e;
    lines::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
    if (e > s && text[e - 1] == '\r') --e;
    uint32_t want = 0;
    uint64_t off = 0;
    if (kWrite) {
      want = lc.n_csq[li];
      off = csq_off[li];
      if (off > n_total || want > n_total - off) {  // (never, with the arrays the size pass gave)
        acc += lane == 1;
        continue;
      }
      if (lc.flags[li]) {
        for (uint32_t i = lane; i < want; i += kWave) blank_row(out, off + i, i);
        if (lane == 0) acc += want;
        continue;
      }
    }
    State st;
    init_state(st);
    if (e == s || text[s] != '{') st.reasons |= 1u << kStruct;
    uint32_t why = 0;
    uint8_t c_next = s + lane < e ? text[s + lane] : uint8_t(0);
    for (uint64_t b0 = s; b0 < e; b0 += kWave) {
      const uint64_t pos = b0 + lane;
      const bool v = pos < e;
      bool f[10];
      raw_of_byte(c_next, f);
      c_next = pos + kWave < e ? text[pos + kWave] : uint8_t(0);  // the next block's byte, under this block's work
      const Raw r{__ballot(f[0]), __ballot(f[1]), __ballot(f[2]), __ballot(f[3]), __ballot(f[4]), __ballot(f[5]),
                  __ballot(f[6]), __ballot(f[7]), __ballot(f[8]), __ballot(f[9]), __ballot(v)};
      const Masks m = derive(r, st);
      const int32_t d = depth_at(m, st.depth, lane);
      const Depths dm{__ballot(v && d == 1), __ballot(v && d == 2), __ballot(v && d == 3), __ballot(v && d == 4),
                      __ballot(v && (d < 0 || d > kMaxDepth))};
      st.depth += int32_t(popc(m.open)) - int32_t(popc(m.close));
      const uint32_t kind = v ? lane_kind(h, s, pos, lane, r, m, dm) : uint32_t(kNone);
      Kinds k;
#pragma unroll
      for (uint32_t t = 0; t < 4; ++t) {
        k.arr[t] = __ballot(kind == kArr0 + t);
        k.key[t] = __ballot(kind == kKey0 + t);
      }
      k.terms_arr = __ballot(kind == kTermsArr);
      k.allele = __ballot(kind == kAllele);
      k.input = __ballot(kind == kInput);
      k.id = __ballot(kind == kId);
      Regions g;
      const uint32_t blk = uint32_t(b0 - s);
      regions(r, m, dm, k, st, g, blk);
      elem_init(lane, g, st, blk, s_el);
      __syncthreads();  // (one wave: the records are in LDS before the positions inside them add to them)
      why |= lane_events<DevOps>(h, s, tab, lane, m, k, g, blk, s_el);
    }
    __syncthreads();
    why = wave_or(why) | end_reasons(st);
    const uint32_t n = st.n_elems;
    if (n <= kMaxCsq) {
      uint32_t ew = 0;
      for (uint32_t i = lane; i < n; i += kWave) {
        int32_t entry;
        ew |= check_elem(h, s, tab, s_el[i], &entry);
        s_el[i].seen = uint32_t(entry);
      }
      why |= wave_or(ew);
    }
    if (!kWrite) {
      if (lane == 0) {
        lc.n_csq[li] = n;
        lc.flags[li] = flags_of(why);
        lc.types[li] = uint8_t((st.n_arrays[0] != 0) | (st.n_arrays[1] != 0) << 1 | (st.n_arrays[2] != 0) << 2 | (st.n_arrays[3] != 0) << 3);
        lc.input_start[li] = st.input_len < 0 ? 0 : s + st.input_start;
        lc.input_len[li] = st.input_len;
        lc.id_start[li] = st.id_len < 0 ? 0 : s + st.id_start;
        lc.id_len[li] = st.id_len;
      }
      acc += lane == AVDB_VEP_COUNT_LINES;
      if (lane == AVDB_VEP_COUNT_CSQ) acc += n;
      if (why) acc += lane == AVDB_VEP_COUNT_HOST_LINES || lane == AVDB_VEP_COUNT_REASON0 + ctz(why);
      continue;
    }
    if (why || n != want) {  // (never: the text is the one the size pass read)
      acc += lane == 1;
      continue;
    }
    __syncthreads();
    for (uint32_t i = lane; i < n; i += kWave) {
      const Elem el = s_el[i];
      const int32_t entry = int32_t(el.seen);
      write_row(out, off + i, s, tab, el, entry);
      s_el[i].mask = sort_key(el, leader_of(h, s, s_el, i), tab.rank_order[entry], i);
    }
    __syncthreads();
    for (uint32_t i = lane; i < n; i += kWave) {
      bool head;
      const uint32_t p = place(s_el, n, i, &head);
      out.sorted[off + p] = int32_t(i);
      out.head[off + p] = head;
    }
    if (lane == 0) acc += n;
    __syncthreads();  // the records are reused by the next line
  }
  if (acc && lane < (kWrite ? 2u : uint32_t(AVDB_VEP_N_COUNTS))) atomicAdd(&ctr[lane], acc);
}

// ---- the same code on the host: the ballots and the lanes are loops ------------------------
template <bool kWrite>
static void host_line(const uint8_t* text, size_t text_bytes, const uint64_t* starts, size_t n_lines, size_t li,
                      const TableView& tab, const LineCols& lc, const uint64_t* csq_off, uint64_t n_total,
                      const CsqOut& out, uint64_t* ctr, Elem* el) {
  const Heap h = make_heap(text, text_bytes);
  uint64_t s, e;
  lines::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
  if (e > s && text[e - 1] == '\r') --e;
  uint32_t want = 0;
  uint64_t off = 0;
  if (kWrite) {
    want = lc.n_csq[li];
    off = csq_off[li];
    if (off > n_total || want > n_total - off) {
      ++ctr[1];
      return;
    }
    if (lc.flags[li]) {
      for (uint32_t i = 0; i < want; ++i) blank_row(out, off + i, i);
      ctr[0] += want;
      return;
    }
  }
  State st;
  init_state(st);
  if (e == s || text[s] != '{') st.reasons |= 1u << kStruct;
  uint32_t why = 0;
  for (uint64_t b0 = s; b0 < e; b0 += kWave) {
    uint64_t rb[11] = {0};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      bool f[10];
      raw_of_byte(text[b0 + lane], f);
      for (int a = 0; a < 10; ++a) rb[a] |= uint64_t(f[a]) << lane;
      rb[10] |= 1ull << lane;
    }
    const Raw r{rb[0], rb[1], rb[2], rb[3], rb[4], rb[5], rb[6], rb[7], rb[8], rb[9], rb[10]};
    const Masks m = derive(r, st);
    Depths dm{0, 0, 0, 0, 0};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      const int32_t d = depth_at(m, st.depth, lane);
      const uint64_t bit = 1ull << lane;
      dm.d1 |= d == 1 ? bit : 0;
      dm.d2 |= d == 2 ? bit : 0;
      dm.d3 |= d == 3 ? bit : 0;
      dm.d4 |= d == 4 ? bit : 0;
      dm.bad |= d < 0 || d > kMaxDepth ? bit : 0;
    }
    st.depth += int32_t(popc(m.open)) - int32_t(popc(m.close));
    Kinds k{};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      const uint32_t kind = lane_kind(h, s, b0 + lane, lane, r, m, dm);
      const uint64_t bit = 1ull << lane;
      if (kind >= kArr0 && kind < kArr0 + 4) k.arr[kind - kArr0] |= bit;
      if (kind >= kKey0 && kind < kKey0 + 4) k.key[kind - kKey0] |= bit;
      if (kind == kTermsArr) k.terms_arr |= bit;
      if (kind == kAllele) k.allele |= bit;
      if (kind == kInput) k.input |= bit;
      if (kind == kId) k.id |= bit;
    }
    Regions g;
    const uint32_t blk = uint32_t(b0 - s);
    regions(r, m, dm, k, st, g, blk);
    for (uint32_t lane = 0; lane < uint32_t(kWave); ++lane) elem_init(lane, g, st, blk, el);
    for (uint32_t lane = 0; lane < uint32_t(kWave); ++lane) why |= lane_events<HostOps>(h, s, tab, lane, m, k, g, blk, el);
  }
  why |= end_reasons(st);
  const uint32_t n = st.n_elems;
  if (n <= kMaxCsq)
    for (uint32_t i = 0; i < n; ++i) {
      int32_t entry;
      why |= check_elem(h, s, tab, el[i], &entry);
      el[i].seen = uint32_t(entry);
    }
  if (!kWrite) {
    lc.n_csq[li] = n;
    lc.flags[li] = flags_of(why);
    lc.types[li] = uint8_t((st.n_arrays[0] != 0) | (st.n_arrays[1] != 0) << 1 | (st.n_arrays[2] != 0) << 2 | (st.n_arrays[3] != 0) << 3);
    lc.input_start[li] = st.input_len < 0 ? 0 : s + st.input_start;
    lc.input_len[li] = st.input_len;
    lc.id_start[li] = st.id_len < 0 ? 0 : s + st.id_start;
    lc.id_len[li] = st.id_len;
    ++ctr[AVDB_VEP_COUNT_LINES];
    ctr[AVDB_VEP_COUNT_CSQ] += n;
    if (why) {
      ++ctr[AVDB_VEP_COUNT_HOST_LINES];
      ++ctr[AVDB_VEP_COUNT_REASON0 + ctz(why)];
    }
    return;
  }
  if (why || n != want) {
    ++ctr[1];
    return;
  }
  for (uint32_t i = 0; i < n; ++i) {
    const Elem x = el[i];
    const int32_t entry = int32_t(x.seen);
    write_row(out, off + i, s, tab, x, entry);
    el[i].mask = sort_key(x, leader_of(h, s, el, i), tab.rank_order[entry], i);
  }
  for (uint32_t i = 0; i < n; ++i) {
    bool head;
    const uint32_t p = place(el, n, i, &head);
    out.sorted[off + p] = int32_t(i);
    out.head[off + p] = head;
  }
  ctr[0] += n;
}

}  // namespace avdb

using namespace avdb;

// the waves of a pass: what is resident at once (the records and the term table of seven one-wave
// workgroups fit a CU's LDS), so that no workgroup waits for another's whole share of the lines
static unsigned vep_grid(const avdb_ctx* ctx, size_t n_lines) {
  const unsigned resident = ctx->n_cu > 0 ? unsigned(ctx->n_cu) * 7u : unsigned(AVDB_VEP_GRID_WAVES);
  return stream_grid(n_lines, 1, resident < unsigned(AVDB_VEP_GRID_WAVES) ? resident : unsigned(AVDB_VEP_GRID_WAVES));
}

// workspace: count workspace | line starts
static size_t vep_workspace(size_t n_lines) { return AVDB_VCF_COUNT_WORKSPACE_BYTES + lines::pad256(8 * n_lines); }

extern "C" int avdb_vep_index_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(vep_workspace(n_lines), bytes);
}

extern "C" int avdb_vep_table_build(const avdb_ctx* ctx, uint32_t n_terms, const uint64_t* entry_mask, size_t n_entries,
                                    uint64_t* slot_mask, int32_t* slot_entry, size_t n_slots) {
  const char* err = nullptr;
  if (!ctx) err = "null context";
  else if (n_terms > 64) err = "more than 64 terms";
  else if (n_entries >= 0x7FFFFFFFull || (n_entries && !entry_mask)) err = "null or too many entries";
  else if (!slot_mask || !slot_entry || !n_slots || (n_slots & (n_slots - 1)) || n_slots > 0x80000000ull ||
           n_slots < 2 * n_entries)
    err = "the slots: a power of two, at least twice the entries";
  if (!err)
    for (size_t i = 0; i < n_entries; ++i)
      if (n_terms < 64 && (entry_mask[i] >> n_terms)) err = "an entry with a term beyond n_terms";
  if (err) {
    avdb_set_error("avdb_vep_table_build: %s", err);
    return AVDB_EINVAL;
  }
  for (size_t k = 0; k < n_slots; ++k) {
    slot_mask[k] = 0;
    slot_entry[k] = -1;
  }
  for (size_t i = 0; i < n_entries; ++i) {
    uint32_t s = vep::slot_of(entry_mask[i], uint32_t(n_slots));
    while (slot_entry[s] >= 0 && slot_mask[s] != entry_mask[i]) s = (s + 1) & uint32_t(n_slots - 1);
    if (slot_entry[s] < 0) {
      slot_mask[s] = entry_mask[i];
      slot_entry[s] = int32_t(i);
    }
  }
  return AVDB_OK;
}

static const char* size_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const avdb_vep_table* table, const LineCols& lc, const uint64_t* counts) {
  if (!ctx) return "null context";
  if (!counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (const char* err = vep::table_error(table)) return err;
  if (n_lines && (!lc.n_csq || !lc.flags || !lc.types || !lc.input_start || !lc.input_len || !lc.id_start || !lc.id_len))
    return "null line array";
  return nullptr;
}

static const char* write_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const avdb_vep_table* table, const LineCols& lc, const uint64_t* csq_off,
                                    size_t n_total, const CsqOut& o, const uint64_t* totals) {
  if (!ctx) return "null context";
  if (!totals) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (const char* err = vep::table_error(table)) return err;
  if (n_lines && (!lc.n_csq || !lc.flags || !csq_off)) return "null line array";
  if (n_total && (!o.type || !o.order || !o.el_start || !o.el_len || !o.al_start || !o.al_len || !o.mask || !o.entry ||
                  !o.coding || !o.sorted || !o.head))
    return "null consequence array";
  return nullptr;
}

extern "C" int avdb_vep_index_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                   const avdb_vep_table* table, uint32_t* n_csq, uint8_t* flags, uint8_t* types, uint64_t* input_start,
                                   int32_t* input_len, uint64_t* id_start, int32_t* id_len, uint64_t* counts,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  const LineCols lc{n_csq, flags, types, input_start, input_len, id_start, id_len};
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, table, lc, counts)) {
    avdb_set_error("avdb_vep_index_size: %s", err);
    return AVDB_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_vep_index_size", ctx, vep_workspace(n_lines), n_lines, workspace, workspace_bytes,
                               counts, AVDB_VEP_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  uint64_t* starts = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + AVDB_VCF_COUNT_WORKSPACE_BYTES);
  AVDB_HIP_TRY(hipMemsetAsync(starts, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, workspace, starts, s)) return e;
  hipLaunchKernelGGL(k_vep_index<false>, dim3(vep_grid(ctx, n_lines)), dim3(kWave), 0, s, text,
                     text_bytes, starts, n_lines, vep::view_of(table), lc, static_cast<const uint64_t*>(nullptr),
                     uint64_t(0), CsqOut{}, reinterpret_cast<unsigned long long*>(counts));
  AVDB_LAUNCH_CHECK("k_vep_index<size>");
  return AVDB_OK;
}

extern "C" int avdb_vep_index_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const avdb_vep_table* table, const uint32_t* n_csq, const uint8_t* flags,
                                    const uint64_t* csq_off, size_t n_csq_total, uint8_t* type, int32_t* order,
                                    uint64_t* el_start, uint32_t* el_len, uint64_t* al_start, uint32_t* al_len,
                                    uint64_t* mask, int32_t* entry, uint8_t* coding, int32_t* sorted, uint8_t* head,
                                    uint64_t* totals, void* workspace, size_t workspace_bytes, void* stream) {
  const LineCols lc{const_cast<uint32_t*>(n_csq), const_cast<uint8_t*>(flags), nullptr, nullptr, nullptr, nullptr, nullptr};
  const CsqOut out{type, order, el_start, el_len, al_start, al_len, mask, entry, coding, sorted, head};
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, table, lc, csq_off, n_csq_total, out, totals)) {
    avdb_set_error("avdb_vep_index_write: %s", err);
    return AVDB_EINVAL;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_vep_index_write", ctx, vep_workspace(n_lines), n_lines, workspace, workspace_bytes,
                               totals, 2, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  uint64_t* starts = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + AVDB_VCF_COUNT_WORKSPACE_BYTES);
  AVDB_HIP_TRY(hipMemsetAsync(starts, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, workspace, starts, s)) return e;
  hipLaunchKernelGGL(k_vep_index<true>, dim3(vep_grid(ctx, n_lines)), dim3(kWave), 0, s, text,
                     text_bytes, starts, n_lines, vep::view_of(table), lc, csq_off, uint64_t(n_csq_total), out,
                     reinterpret_cast<unsigned long long*>(totals));
  AVDB_LAUNCH_CHECK("k_vep_index<write>");
  return AVDB_OK;
}

extern "C" int avdb_vep_index_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        const avdb_vep_table* table, uint32_t* n_csq, uint8_t* flags, uint8_t* types,
                                        uint64_t* input_start, int32_t* input_len, uint64_t* id_start, int32_t* id_len,
                                        uint64_t* counts) {
  const LineCols lc{n_csq, flags, types, input_start, input_len, id_start, id_len};
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, table, lc, counts)) {
    avdb_set_error("avdb_vep_index_size_host: %s", err);
    return AVDB_EINVAL;
  }
  memset(counts, 0, 8 * AVDB_VEP_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  std::vector<Elem> el(kMaxCsq);
  const TableView tab = vep::view_of(table);
  for (size_t li = 0; li < n_lines; ++li)
    host_line<false>(text, text_bytes, starts.data(), n_lines, li, tab, lc, nullptr, 0, CsqOut{}, counts, el.data());
  return AVDB_OK;
}

extern "C" int avdb_vep_index_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         const avdb_vep_table* table, const uint32_t* n_csq, const uint8_t* flags,
                                         const uint64_t* csq_off, size_t n_csq_total, uint8_t* type, int32_t* order,
                                         uint64_t* el_start, uint32_t* el_len, uint64_t* al_start, uint32_t* al_len,
                                         uint64_t* mask, int32_t* entry, uint8_t* coding, int32_t* sorted,
                                         uint8_t* head, uint64_t* totals) {
  const LineCols lc{const_cast<uint32_t*>(n_csq), const_cast<uint8_t*>(flags), nullptr, nullptr, nullptr, nullptr, nullptr};
  const CsqOut out{type, order, el_start, el_len, al_start, al_len, mask, entry, coding, sorted, head};
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, table, lc, csq_off, n_csq_total, out, totals)) {
    avdb_set_error("avdb_vep_index_write_host: %s", err);
    return AVDB_EINVAL;
  }
  totals[0] = totals[1] = 0;
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  std::vector<Elem> el(kMaxCsq);
  const TableView tab = vep::view_of(table);
  for (size_t li = 0; li < n_lines; ++li)
    host_line<true>(text, text_bytes, starts.data(), n_lines, li, tab, lc, csq_off, n_csq_total, out, totals, el.data());
  return AVDB_OK;
}

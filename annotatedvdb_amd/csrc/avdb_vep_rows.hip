// K18b — VEP consequence update rows from VEP JSON and an export of AnnotatedVDB.Variant (gfx950).
//
// Replaces, for adsp_most_severe_consequence and adsp_ranked_consequences, the per-line Python of
// Load/bin/load_vep_result.py on VEPVariantLoader (vep_variant_loader.py:153-213: a VcfEntryParser
// of `input`, a VariantAnnotator per ALT allele, get_most_severe_consequence and
// get_allele_consequences, two xstr(dict) per allele, a bulk SQL lookup per id) with two device
// passes of two steps each on K18a's arrays of the same slab and on the skeleton of
// avdb_tables.hpp (its compaction, scans, totals, checks and host loops).
//   the table (avdb_vep_rows_table_size / _write) over the VEP JSON
//     k_vr_elem_size   one wave per consequence, 64 bytes a step: the escape mask and the string
//                      mask of avdb_vep.hpp from ballots, the separators outside strings counted,
//                      every token outside strings checked by the lane it begins in; the rendered
//                      length of the element, or why its line is the host's
//     k_vr_lines       one lane per line: the five fields of `input`, per ALT allele the elements
//                      of its normalised allele in `sorted` order and the length of its body
//     tables::k_compact<VepRowsBuild>, tables::k_totals
//     k_vr_keys        rows::write_rows over the key blob, one lane per entry: chrom:pos:ref:alt_k
//                      back to back, and the columns of its rows
//     k_vr_body        one wave per entry: the walk of k_vr_lines with the whole wave, every
//                      element stored by the same 64-byte steps (a lane's byte goes out behind the
//                      spaces of the separators below it in the block and before the block), the
//                      suffix a byte a lane; a row's own span of the body
//   the update rows (avdb_vep_rows_update_size / _write) over the export
//     k_vrupd_lines, tables::k_upd_compact<VepJoin>, rows::begin_write,
//     tables::k_upd_write<kVrWriteStage, VepUpdRows>
// The per-block, per-line and per-row code is avdb_vep_rows.hpp, shared with the _host entries.
#include "avdb_vep_rows.hpp"

namespace avdb {

using namespace vrows;
using lof::Table;
using lof::UpdLine;
using tables::EntCols;
using tables::EntScans;
using tables::UpdCols;
using tables::UpdRow;

// metaseq ids are about 12 bytes an alt: 256 entries' keys fit 32 KB; an export row is its body
// (kilobytes) and a trip of 256 rarely fits: such a trip is written bytewise
constexpr uint32_t kVrWriteStage = 32 * 1024;
constexpr uint32_t kVrUpdSizeStage = 32 * 1024;
constexpr unsigned kWavesPerBlock = unsigned(kBlock) / unsigned(kWave);

struct VepRowsBuild {
  static constexpr int ROWS = AVDB_VEPROWS_COUNT_ROWS, LINES = AVDB_VEPROWS_COUNT_LINES,
                       KEY_BYTES = AVDB_VEPROWS_COUNT_KEY_BYTES, JSON_BYTES = AVDB_VEPROWS_COUNT_JSON_BYTES,
                       HOST_LINES = AVDB_VEPROWS_COUNT_HOST_LINES, BAD = AVDB_VEPROWS_COUNT_BAD,
                       ENTRIES = AVDB_VEPROWS_COUNT_ENTRIES, EXTRA = -1;
  static constexpr uint32_t HOST_BIT = AVDB_VEPROWS_LINE_HOST, BAD_BIT = AVDB_VEPROWS_LINE_BAD, EXTRA_BIT = 0;
  static constexpr bool ROW_PER_ENTRY = false;
  static AVDB_HD bool is_entry(uint32_t) { return true; }  // every line: entry e is line e
};

struct VepJoin {
  static constexpr int ROWS = AVDB_LOFUPD_COUNT_ROWS, SKIPPED_LINES = AVDB_LOFUPD_COUNT_SKIPPED_LINES,
                       SKIPPED = AVDB_LOFUPD_COUNT_SKIPPED, MISSED = AVDB_LOFUPD_COUNT_NOT_ANNOTATED,
                       BAD = AVDB_LOFUPD_COUNT_BAD, OUT_BYTES = AVDB_LOFUPD_COUNT_OUT_BYTES,
                       LONE_CR = AVDB_LOFUPD_COUNT_LONE_CR, HOST_ROWS = -1;
  static constexpr uint32_t BAD_BIT = AVDB_LOFUPD_BAD, HOST_BIT = 0;
};

struct VepUpdRows {  // an update row against the table
  Table T;
  uint64_t alg_id;
  uint32_t flags;
  template <class TextAt, class Put>
  AVDB_HD void operator()(const UpdRow& row, TextAt text, Put put) const {
    vrows::render_update_row(row, T, alg_id, flags, text, put);
  }
};

// a block of an element as the wave sees it: lane `lane` holds byte b0 + lane
struct WaveBlock {
  uint32_t idx, c;
  bool v;
  ElemBlock B;
};
__device__ __forceinline__ WaveBlock wave_block(const uint8_t* __restrict__ text, const ElemRef& e, uint32_t b0,
                                                uint32_t lane, ElemState& st) {
  WaveBlock w;
  w.idx = b0 + lane;
  w.v = w.idx < e.len;
  w.c = w.v ? text[e.s + w.idx] : 0u;
  bool f[6];
  elem_raw_of_byte(uint8_t(w.c), f);
  const ElemRaw raw{__ballot(w.v && f[0]), __ballot(w.v && f[1]), __ballot(w.v && f[2]),
                    __ballot(w.v && f[3]), __ballot(w.v && f[4]), __ballot(w.v && f[5])};
  w.B = elem_block(raw, __ballot(w.v), st);
  return w;
}

__global__ __launch_bounds__(kBlock) void k_vr_elem_size(const uint8_t* __restrict__ text, size_t text_bytes, In in) {
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kWavesPerBlock;
  for (uint64_t r = wave; r < in.n_csq_total; r += n_waves) {
    const ElemRef e = elem_ref(in, r, text_bytes);
    uint32_t rl = kUnsafe | uint32_t(vep::kStruct);  // (a blank row of a line K18a left to the host; never read)
    if (e.ok) {
      ElemState st{};
      bool bad_token = false;
      for (uint32_t b0 = 0; b0 < e.len; b0 += uint32_t(kWave)) {
        const WaveBlock w = wave_block(text, e, b0, lane, st);
        if (((w.B.tok_start >> lane) & 1) && !token_at_ok(text + e.s + w.idx, e.len - w.idx)) bad_token = true;
      }
      uint32_t why = st.why;
      if (__ballot(bad_token)) why |= 1u << kToken;
      if (st.in_str) why |= 1u << vep::kStruct;  // (never: K18a closed the element outside a string)
      Suffix S;
      const bool has = suffix_of(in, r, &S);
      rl = rlen_of(e.len, st.n_sep, why, has, S);
    }
    if (lane == 0) in.el_rlen[r] = rl;
  }
}

// info[li] = {alts, key_bytes, json_len, 1 | flags << 8}
__global__ __launch_bounds__(kBlock) void k_vr_lines(const uint8_t* __restrict__ text, size_t text_bytes, size_t n_lines,
                                                     In in, u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                     unsigned long long* __restrict__ counts) {
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const LineOut L = line_entry(in, text, text_bytes, li);
    info[li] = u32x4{L.alts, L.key_bytes, L.json_len, 1u | (L.flags << 8)};
    mark[li] = 1;
    if (L.flags) atomicAdd(&counts[AVDB_VEPROWS_COUNT_REASON0 + reason_of(L.flags)], 1ull);  // (host lines are few)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) mark[n_lines] = 0;  // the scan leaves the entry count there
}

struct EntryAt {
  tables::EntryRow E;
  size_t e;  // its number, which is its line's
};

__global__ __launch_bounds__(kBlock) void k_vr_keys(const uint8_t* __restrict__ text, size_t text_bytes, In in, EntCols o,
                                                    EntScans sc, size_t n_entries, RowCols R,
                                                    uint8_t* __restrict__ keys, const uint64_t* __restrict__ totals) {
  __shared__ uint64_t s_out[kVrWriteStage / 8];
  rows::write_rows<kVrWriteStage>(
      sc.key, n_entries, keys, totals + 2, s_out, [&](size_t e) { return EntryAt{tables::load_entry(o, sc, e), e}; },
      [&](const EntryAt& x, auto put) { render_keys(in, text, text_bytes, x.e, x.E, R, put); });
}

// row_body's sink for a whole wave: every lane runs the same walk (one entry, wave-uniform control
// flow); lit stores a byte a lane, elem the element's bytes by the 64-byte steps of k_vr_elem_size
struct WaveSink {
  const In& in;
  const uint8_t* text;
  uint64_t text_bytes;
  uint64_t k;      // from the entry's base
  uint64_t limit;  // the entry's json_len
  uint8_t* out;    // the entry's span of the body blob
  uint32_t lane;
  __device__ __forceinline__ void put(uint64_t at, uint32_t c) {
    if (at < limit) out[at] = uint8_t(c);
  }
  __device__ __forceinline__ void lit(const char* s, uint32_t n) {
    for (uint32_t i = lane; i < n; i += uint32_t(kWave)) put(k + i, uint8_t(s[i]));
    k += n;
  }
  __device__ __forceinline__ void elem(uint64_t r) {
    const uint32_t rl = in.el_rlen[r];
    const ElemRef e = elem_ref(in, r, text_bytes);
    Suffix S;
    if ((rl & kUnsafe) || !e.ok || !suffix_of(in, r, &S)) return;  // (never, for a line the size pass kept)
    ElemState st{};
    const uint64_t base = k;
    for (uint32_t b0 = 0; b0 < e.len; b0 += uint32_t(kWave)) {
      const WaveBlock w = wave_block(text, e, b0, lane, st);
      if (w.v) elem_lane_put(lane, w.idx, e.len - 1, w.c, w.B, [&](uint32_t j, uint32_t c) { put(base + j, c); });
    }
    const uint64_t at = base + e.len - 1 + st.n_sep;
    for (uint32_t j = lane; j < S.len; j += uint32_t(kWave)) put(at + j, suffix_at(S, j));
    k += rl;
  }
};

__global__ __launch_bounds__(kBlock) void k_vr_body(const uint8_t* __restrict__ text, size_t text_bytes, In in, EntCols o,
                                                    EntScans sc, size_t n_entries, RowCols R,
                                                    uint8_t* __restrict__ json, const uint64_t* __restrict__ totals) {
  if (totals[3]) return;  // the capacities are too small: nothing is written
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kWavesPerBlock;
  for (uint64_t e = wave; e < n_entries; e += n_waves) {
    const tables::EntryRow E = tables::load_entry(o, sc, e);
    // (k_totals found the blob large enough: [json_base, json_base + json_len) lies inside it)
    WaveSink sink{in, text, text_bytes, 0, E.json_len, json + E.json_base, lane};
    Input I;
    LineCsq C;
    if (entry_input(in, text, text_bytes, e, E, &I, &C)) {
      uint32_t cursor = 0;
      for (uint32_t a = 0; a < I.n_alts; ++a) {
        const Alt A = next_alt(text, I, &cursor);
        const uint64_t at = sink.k;
        row_body(in, text, text_bytes, C, A, sink);
        if (lane == 0) set_row_json(E, R, a, at, sink.k - at);
      }
    }
    for (uint64_t k = sink.k + lane; k < E.json_len; k += uint64_t(kWave)) sink.out[k] = uint8_t(' ');
  }
}

// ---- the export join ----------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_vrupd_lines(const uint8_t* __restrict__ text, size_t text_bytes,
                                                        const uint64_t* __restrict__ starts, size_t n_lines, Table T,
                                                        uint32_t contig_mask, uint32_t update_existing, uint32_t tail,
                                                        u32x4* __restrict__ info, uint64_t* __restrict__ mark,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ u32x4 s_text[kVrUpdSizeStage / 16];
  tables::UpdTally<VepJoin> tally;
  lines::for_each_line<kVrUpdSizeStage>(text, text_bytes, starts, n_lines, s_text, [&](size_t li, auto with_line) {
    with_line([&](uint64_t, uint64_t len, bool nl, auto line) {
      const UpdLine L = vrows::scan_export_line(line, len, nl, contig_mask, update_existing != 0, T, tail);
      tally.line(L, li, info, mark, T.hit);
    });
  });
  tally.finish(mark, n_lines, counts);
}

}  // namespace avdb

using namespace avdb;

extern "C" int avdb_vep_rows_table_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::table_layout(n_lines).total, bytes);
}

extern "C" int avdb_vep_rows_update_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(tables::upd_layout(n_lines).total, bytes);
}

extern "C" int avdb_vep_rows_token_ok_host(const uint8_t* token, size_t n) {
  return token && n <= kMaxToken && token_ok(token, uint32_t(n)) ? 1 : 0;
}

extern "C" int avdb_vep_rows_table_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        const avdb_vep_rows_in* in, uint64_t* ent_start, uint32_t* ent_alts,
                                        uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags,
                                        uint64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* err = in_error(in, n_lines);
  return tables::table_size<VepRowsBuild>(
      {"avdb_vep_rows_table_size", ctx, {text, text_bytes, n_lines}, err}, o, counts, AVDB_VEPROWS_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_vr_elem_size, k_vr_lines",
      [&](unsigned grid, const uint64_t*, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        if (in->n_csq_total)
          hipLaunchKernelGGL(k_vr_elem_size, dim3(stream_grid(in->n_csq_total, kWavesPerBlock, 4096)), dim3(kBlock), 0, s,
                             text, text_bytes, *in);
        hipLaunchKernelGGL(k_vr_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, n_lines, *in, info, marks, cnt);
      });
}

extern "C" int avdb_vep_rows_table_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         size_t n_entries, size_t n_rows, const avdb_vep_rows_in* in,
                                         const uint64_t* ent_start, const uint32_t* ent_alts,
                                         const uint32_t* ent_key_bytes, const uint32_t* ent_json_len,
                                         const uint8_t* ent_flags, uint8_t* keys, size_t key_cap, uint64_t* key_off,
                                         uint8_t* json, size_t json_cap, uint64_t* row_json_off, uint32_t* row_json_len,
                                         uint64_t* row_line_start, uint8_t* row_flags, uint64_t* totals, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* err = in_error(in, n_lines);
  return tables::table_write<VepRowsBuild>(
      {"avdb_vep_rows_table_write", ctx, {text, text_bytes, n_lines}, err}, n_entries, n_rows, o,
      {keys, key_cap, json, json_cap, R, totals}, {workspace, workspace_bytes, s}, "k_vr_keys",
      [&](unsigned grid, const EntScans& sc) {
        hipLaunchKernelGGL(k_vr_keys, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, *in, o, sc, n_entries, R, keys,
                           totals);
      },
      "k_vr_body",
      [&](unsigned, const EntScans& sc) {
        hipLaunchKernelGGL(k_vr_body, dim3(stream_grid(n_entries, kWavesPerBlock, 4096)), dim3(kBlock), 0, s, text,
                           text_bytes, *in, o, sc, n_entries, R, json, totals);
      });
}

// ---- the table on the host ----------------------------------------------------------------------
extern "C" int avdb_vep_rows_table_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                             const avdb_vep_rows_in* in, uint64_t* ent_start, uint32_t* ent_alts,
                                             uint32_t* ent_key_bytes, uint32_t* ent_json_len, uint8_t* ent_flags,
                                             uint64_t* counts) {
  const EntCols o{ent_start, ent_alts, ent_key_bytes, ent_json_len, ent_flags};
  const char* err = in_error(in, n_lines);
  bool sized = false;
  return tables::table_size_host<VepRowsBuild>(
      {"avdb_vep_rows_table_size_host", ctx, {text, text_bytes, n_lines}, err}, o, counts, AVDB_VEPROWS_N_COUNTS,
      [&](size_t li, const uint8_t*, uint64_t, bool, lof::Entry* E) {
        if (!sized) {  // (behind the argument checks: the elements first, as the device sizes them)
          for (uint64_t r = 0; r < in->n_csq_total; ++r) {
            const ElemRef e = elem_ref(*in, r, text_bytes);
            uint32_t rl = kUnsafe | uint32_t(vep::kStruct);
            if (e.ok) {
              uint32_t why;
              const uint32_t n_sep = elem_walk_host<false>(text, e.s, e.len, [](uint32_t, uint32_t) {}, &why);
              Suffix S;
              const bool has = suffix_of(*in, r, &S);
              rl = rlen_of(e.len, n_sep, why, has, S);
            }
            in->el_rlen[r] = rl;
          }
          sized = true;
        }
        const LineOut L = line_entry(*in, text, text_bytes, li);
        *E = lof::Entry{L.alts, L.key_bytes, L.json_len, L.flags};
        if (L.flags) ++counts[AVDB_VEPROWS_COUNT_REASON0 + reason_of(L.flags)];
        return true;
      });
}

extern "C" int avdb_vep_rows_table_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes,
                                              size_t n_lines, size_t n_entries, size_t n_rows,
                                              const avdb_vep_rows_in* in, const uint64_t* ent_start,
                                              const uint32_t* ent_alts, const uint32_t* ent_key_bytes,
                                              const uint32_t* ent_json_len, const uint8_t* ent_flags, uint8_t* keys,
                                              size_t key_cap, uint64_t* key_off, uint8_t* json, size_t json_cap,
                                              uint64_t* row_json_off, uint32_t* row_json_len, uint64_t* row_line_start,
                                              uint8_t* row_flags, uint64_t* totals) {
  const EntCols o{const_cast<uint64_t*>(ent_start), const_cast<uint32_t*>(ent_alts),
                  const_cast<uint32_t*>(ent_key_bytes), const_cast<uint32_t*>(ent_json_len),
                  const_cast<uint8_t*>(ent_flags)};
  const RowCols R{key_off, row_json_off, row_json_len, row_line_start, row_flags, n_rows};
  const char* err = in_error(in, n_lines);
  size_t e = 0;  // entries come in order, and entry e is line e
  return tables::table_write_host<VepRowsBuild>(
      {"avdb_vep_rows_table_write_host", ctx, {text, text_bytes, n_lines}, err}, n_entries, n_rows, o,
      {keys, key_cap, json, json_cap, R, totals}, "body", [&](const tables::EntryRow& E, auto put_key, auto) {
        render_keys(*in, text, text_bytes, e, E, R, put_key);
        render_body_host(*in, text, text_bytes, e, E, R, json + E.json_base);  // (the totals fit the capacities)
        ++e;
      });
}

// ---- the update rows' entries -------------------------------------------------------------------
static const char* table_view(const avdb_vep_rows_table* t, Table* T) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_vep_rows_table)) return "avdb_vep_rows_table of another size";
  memset(T, 0, sizeof(*T));
  return tables::fill_table_view(T, t->n_rows, t->keys, t->key_off, t->keyset, t->keyset_bytes, t->json, t->json_bytes,
                                 t->json_off, t->json_len, t->hit);
}

extern "C" int avdb_vep_rows_update_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         const avdb_vep_rows_table* table, uint32_t contig_mask, uint32_t flags,
                                         uint64_t alg_id, uint64_t* row_start, uint32_t* pk_len, int32_t* match,
                                         uint32_t* out_len, uint8_t* row_flags, uint64_t* counts, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  Table T;
  const char* err = table_view(table, &T);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t upd = (flags & AVDB_VEPUPD_UPDATE_EXISTING) != 0, tail = tail_len(alg_id, flags);
  return tables::update_size<VepJoin>(
      {"avdb_vep_rows_update_size", ctx, {text, text_bytes, n_lines}, err},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_LOFUPD_N_COUNTS,
      {workspace, workspace_bytes, s}, "k_vrupd_lines",
      [&](unsigned grid, const uint64_t* starts, u32x4* info, uint64_t* marks, unsigned long long* cnt) {
        hipLaunchKernelGGL(k_vrupd_lines, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, starts, n_lines, T,
                           contig_mask, upd, tail, info, marks, cnt);
      });
}

extern "C" int avdb_vep_rows_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          size_t n_rows, const avdb_vep_rows_table* table, uint32_t flags,
                                          uint64_t alg_id, const uint64_t* row_start, const uint32_t* pk_len,
                                          const int32_t* match, const uint32_t* out_len, const uint8_t* row_flags,
                                          uint8_t* out, size_t out_cap, uint64_t* row_off, uint64_t* totals,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  VepUpdRows render{};
  const char* err = table_view(table, &render.T);
  render.alg_id = alg_id;
  render.flags = flags;
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write<kVrWriteStage>({"avdb_vep_rows_update_write", ctx, {text, text_bytes, n_lines}, err},
                                             n_rows, o, {out, out_cap, row_off, totals},
                                             {workspace, workspace_bytes, static_cast<hipStream_t>(stream)}, render);
}

extern "C" int avdb_vep_rows_update_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes,
                                              size_t n_lines, const avdb_vep_rows_table* table, uint32_t contig_mask,
                                              uint32_t flags, uint64_t alg_id, uint64_t* row_start, uint32_t* pk_len,
                                              int32_t* match, uint32_t* out_len, uint8_t* row_flags, uint64_t* counts) {
  Table T;
  const char* err = table_view(table, &T);
  const bool upd = (flags & AVDB_VEPUPD_UPDATE_EXISTING) != 0;
  const uint32_t tail = tail_len(alg_id, flags);
  return tables::update_size_host<VepJoin>(
      {"avdb_vep_rows_update_size_host", ctx, {text, text_bytes, n_lines}, err},
      UpdCols{row_start, pk_len, match, out_len, row_flags}, counts, AVDB_LOFUPD_N_COUNTS, err ? nullptr : T.hit,
      [&](const uint8_t* line, uint64_t len, bool nl) {
        return vrows::scan_export_line(line, len, nl, contig_mask, upd, T, tail);
      });
}

extern "C" int avdb_vep_rows_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes,
                                               size_t n_lines, size_t n_rows, const avdb_vep_rows_table* table,
                                               uint32_t flags, uint64_t alg_id, const uint64_t* row_start,
                                               const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                               const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                               uint64_t* totals) {
  VepUpdRows render{};
  const char* err = table_view(table, &render.T);
  render.alg_id = alg_id;
  render.flags = flags;
  const UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                  const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  return tables::update_write_host({"avdb_vep_rows_update_write_host", ctx, {text, text_bytes, n_lines}, err}, n_rows, o,
                                   {out, out_cap, row_off, totals}, render);
}

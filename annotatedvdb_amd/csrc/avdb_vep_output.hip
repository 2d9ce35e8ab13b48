// K18c — the vep_output column of the VEP update rows (gfx950).
//
// Replaces, for the cleaned result of VEPVariantLoader (vep_variant_loader.py:112-123, 202: a deep
// copy of the annotation, five pops and an xstr(dict) per line, the VcfEntryParser dict in place of
// `input`), the host loop with two passes on K18a's arrays of the same slab:
//   size pass (avdb_vep_output_size)
//     k_vo_dict<false>   one lane per line: the fields of `input` and the length of the entry dict,
//                        or why the line is the host's (K18a's and K18b's verdicts first)
//     k_vo_clean<false>  one wave per line, 64 bytes a step: the masks of avdb_vep.hpp from ballots,
//                        the top-level members found at their key's quote and compared with the five
//                        dropped names, every kept token checked by the lane it begins in; the
//                        output length and where the dict goes
//   write pass (avdb_vep_output_write; the caller scanned the lengths)
//     k_vo_clean<true>   the same walk; a lane's byte goes out at its input position minus the
//                        dropped bytes below it plus the spaces and ", " added below it
//     k_vo_dict<true>    the dict, rendered straight to its place in the line's text
//   the update rows with the extra column (avdb_vep_output_update_write, behind
//   avdb_vep_rows_update_size)
//     k_vo_upd_write     one wave per output row: head, body, cleaned text and tail copied 64 bytes
//                        a step from the export, the table's body blob and the cleaned texts
// The per-block, per-line and per-row code is avdb_vep_output.hpp, shared with the _host entries.
#include "avdb_vep_output.hpp"

#include <string.h>

namespace avdb {
namespace vout {

constexpr unsigned kVoWavesPerBlock = unsigned(kBlock) / unsigned(kWave);

struct OutCols {
  uint64_t* line_start;
  uint32_t* out_len;
  uint32_t* dict_at;
  uint32_t* dict_len;
  uint8_t* flags;
};

// size: dict_len[li]; write: the dict of every line the device answers, at out + out_off + dict_at
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void k_vo_dict(const uint8_t* __restrict__ text, size_t text_bytes, size_t n_lines,
                                                    In in, const uint8_t* __restrict__ ent_flags, uint32_t identity_only,
                                                    OutCols lc, const uint64_t* __restrict__ out_off,
                                                    uint8_t* __restrict__ out, uint64_t out_cap) {
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    if (!kWrite) {
      lc.dict_len[li] = dict_entry(in, ent_flags, text, text_bytes, li, identity_only != 0);
      continue;
    }
    if (lc.flags[li]) continue;
    const uint64_t off = out_off[li];
    const uint32_t len = lc.out_len[li], at = lc.dict_at[li], dn = lc.dict_len[li];
    if (off > out_cap || len > out_cap - off || at > len || dn > len - at) continue;  // (k_vo_clean counts the line)
    uint8_t* dst = out + off + at;
    dict_json(text, text_bytes, in.input_start[li], in.input_len[li], identity_only != 0, [&](uint32_t k, uint32_t c) {
      if (k < dn) dst[k] = uint8_t(c);
    });
  }
}

// ctr: the size pass's counts, or the write pass's totals
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void k_vo_clean(const uint8_t* __restrict__ text, size_t text_bytes,
                                                     const uint64_t* __restrict__ starts, size_t n_lines, In in,
                                                     OutCols lc, const uint64_t* __restrict__ out_off,
                                                     uint8_t* __restrict__ out, uint64_t out_cap,
                                                     unsigned long long* __restrict__ ctr) {
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kVoWavesPerBlock;
  unsigned long long acc = 0;  // lane k: what this wave adds to ctr[k]
  for (uint64_t li = wave; li < n_lines; li += n_waves) {
    uint64_t s, e;
    lines::line_span(text, text_bytes, starts, n_lines, li, &s, &e);
    if (e > s && text[e - 1] == '\r') --e;
    const uint32_t dl = lc.dict_len[li];
    uint32_t why = 0, want = 0;
    uint8_t* dst = nullptr;
    if (!kWrite) {
      if (lane == 0) lc.line_start[li] = s;
      acc += lane == AVDB_VEPOUT_COUNT_LINES;
      if (dl & kUnsafe) why = 1u << (dl & 31u);
      else if (e - s > kMaxLine) why = 1u << vep::kCap;
    } else {
      if (lc.flags[li]) continue;
      const uint64_t off = out_off[li];
      want = lc.out_len[li];
      if ((dl & kUnsafe) || off > out_cap || want > out_cap - off) {
        acc += lane == 1;
        continue;
      }
      dst = out + off;
    }
    uint32_t dict_at = 0;
    State st{};
    if (!why) {
      const uint64_t lo = in.input_start[li] - 1, hi = in.input_start[li] + uint32_t(in.input_len[li]);
      bool bad_token = false;
      for (uint64_t b0 = s; b0 < e; b0 += uint64_t(kWave)) {
        const uint64_t pos = b0 + lane;
        const bool v = pos < e;
        const uint32_t c = v ? text[pos] : 0u;
        bool f[9];
        raw_of_byte(uint8_t(c), f);
        const Raw r{__ballot(v && f[0]), __ballot(v && f[1]), __ballot(v && f[2]), __ballot(v && f[3]),
                    __ballot(v && f[4]), __ballot(v && f[5]), __ballot(v && f[6]), __ballot(v && f[7]),
                    __ballot(v && f[8]), __ballot(v)};
        const Masks M = derive(r, st);
        const uint64_t d1 = __ballot(v && vep::depth_at(M.m, st.depth, lane) == 1);
        st.depth += int32_t(popc(M.m.open)) - int32_t(popc(M.m.close));
        const uint64_t mstart = member_starts(r, M, d1, st);
        const uint64_t drop_start = __ballot(((mstart >> lane) & 1) && dropped_key(text + pos, e - pos));
        const uint64_t inp = __ballot(v && pos >= lo && pos <= hi), inp_close = __ballot(v && pos == hi);
        const Block B = block(r, M, d1, mstart, drop_start, inp, inp_close, dl, st);
        if (b0 <= lo && lo < b0 + uint64_t(kWave) && lo < e) dict_at = out_at(B, uint32_t(lo - b0));
        if (kWrite) {
          if (v) lane_put(B, lane, c, [&](uint32_t k, uint32_t ch) {
            if (k < want) dst[k] = uint8_t(ch);
          });
        } else if (((B.tok_start >> lane) & 1) && !vrows::token_at_ok(text + pos, e - pos)) {
          bad_token = true;
        }
      }
      why = st.why;
      if (__ballot(bad_token)) why |= 1u << kKeptText;
    }
    if (!kWrite) {
      if (lane == 0) {
        lc.out_len[li] = why ? 0u : st.out;
        lc.dict_at[li] = why ? 0u : dict_at;
        lc.flags[li] = why ? uint8_t(1 + ctz(why)) : uint8_t(0);
      }
      if (why) acc += lane == AVDB_VEPOUT_COUNT_HOST_LINES || lane == AVDB_VEPOUT_COUNT_REASON0 + ctz(why);
      else if (lane == AVDB_VEPOUT_COUNT_OUT_BYTES) acc += st.out;
    } else {
      if (st.out != want || dict_at != lc.dict_at[li]) acc += lane == 1;  // (never: the text is the one the size pass read)
      else if (lane == 0) acc += want;
    }
  }
  if (acc && lane < (kWrite ? 2u : uint32_t(AVDB_VEPOUT_N_COUNTS))) atomicAdd(&ctr[lane], acc);
}

// One wave per output row: the head a byte a lane, the body and the cleaned text copied 64 bytes a
// step from their blobs, the tail a byte a lane.  A row whose parts do not add up is left blank.
__global__ __launch_bounds__(kBlock) void k_vo_upd_write(const uint8_t* __restrict__ text, size_t text_bytes,
                                                         lof::Table T, Cleaned C, uint64_t alg_id, uint32_t flags,
                                                         tables::UpdCols o, const uint64_t* __restrict__ row_off,
                                                         size_t n_rows, uint8_t* __restrict__ out,
                                                         const uint64_t* __restrict__ totals) {
  if (totals[1]) return;  // the capacity is too small: nothing is written
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kVoWavesPerBlock;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (uint64_t r = wave; r < n_rows; r += n_waves) {
    const lof::UpdRow row{o.row_start[r], o.pk_len[r], o.out_len[r], o.flags[r], o.match[r]};
    // (k_row_totals found the output large enough: [row_off[r], row_off[r] + out_len) lies inside it)
    uint8_t* dst = out + row_off[r];
    const RowParts P = row_parts(row, T, C, alg_id, flags, tb);
    if (!P.ok) {
      for (uint32_t k = lane; k < row.out_len; k += uint32_t(kWave)) dst[k] = uint8_t(' ');
      continue;
    }
    for (uint32_t j = lane; j < P.head_n; j += uint32_t(kWave)) dst[j] = uint8_t(head_byte(row, P, j, tb));
    uint8_t* d = dst + P.head_n;
    const uint8_t* src = T.json + P.body_s;
    for (uint32_t j = lane; j < P.body_n; j += uint32_t(kWave)) d[j] = src[j];
    d += P.body_n;
    if (lane == 0) d[0] = uint8_t('\t');
    d += 1;
    src = C.text + P.clean_s;
    for (uint32_t j = lane; j < P.clean_n; j += uint32_t(kWave)) d[j] = src[j];
    d += P.clean_n;
    for (uint32_t j = lane; j < P.tail_n; j += uint32_t(kWave)) d[j] = uint8_t(tail_byte(P, alg_id, j));
  }
}

}  // namespace vout
}  // namespace avdb

using namespace avdb;

// workspace: count workspace | line starts
static size_t vo_workspace(size_t n_lines) { return AVDB_VCF_COUNT_WORKSPACE_BYTES + lines::pad256(8 * n_lines); }

extern "C" int avdb_vep_output_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(vo_workspace(n_lines), bytes);
}

static const char* size_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, const avdb_vep_rows_in* in,
                                   const uint8_t* ent_flags, const vout::OutCols& lc, const uint64_t* counts) {
  if (!ctx || !counts) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (const char* err = vout::in_error(in, n_lines)) return err;
  if (n_lines && (!ent_flags || !lc.line_start || !lc.out_len || !lc.dict_at || !lc.dict_len || !lc.flags))
    return "null line array";
  return nullptr;
}

static const char* write_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const avdb_vep_rows_in* in, const uint64_t* out_off, const vout::OutCols& lc, const uint8_t* out,
                                    size_t out_cap, const uint64_t* totals) {
  if (!ctx || !totals) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (const char* err = vout::in_error(in, n_lines)) return err;
  if (n_lines && (!out_off || !lc.out_len || !lc.dict_at || !lc.dict_len || !lc.flags)) return "null line array";
  return rows::out_error(out, out_cap);
}

extern "C" int avdb_vep_output_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                    const avdb_vep_rows_in* in, const uint8_t* ent_flags, uint32_t flags,
                                    uint64_t* line_start, uint32_t* out_len, uint32_t* dict_at, uint32_t* dict_len,
                                    uint8_t* out_flags, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const vout::OutCols lc{line_start, out_len, dict_at, dict_len, out_flags};
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, in, ent_flags, lc, counts))
    return tables::invalid("avdb_vep_output_size", err);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_vep_output_size", ctx, vo_workspace(n_lines), n_lines, workspace, workspace_bytes,
                               counts, AVDB_VEPOUT_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  uint64_t* starts = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + AVDB_VCF_COUNT_WORKSPACE_BYTES);
  AVDB_HIP_TRY(hipMemsetAsync(starts, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, workspace, starts, s)) return e;
  hipLaunchKernelGGL(vout::k_vo_dict<false>, dim3(stream_grid(n_lines, kBlock, 4096)), dim3(kBlock), 0, s, text, text_bytes,
                     n_lines, *in, ent_flags, flags & AVDB_VEPOUT_IDENTITY_ONLY, lc, static_cast<const uint64_t*>(nullptr),
                     static_cast<uint8_t*>(nullptr), uint64_t(0));
  AVDB_LAUNCH_CHECK("k_vo_dict<size>");
  hipLaunchKernelGGL(vout::k_vo_clean<false>, dim3(stream_grid(n_lines, vout::kVoWavesPerBlock, 4096)), dim3(kBlock), 0, s, text,
                     text_bytes, starts, n_lines, *in, lc, static_cast<const uint64_t*>(nullptr),
                     static_cast<uint8_t*>(nullptr), uint64_t(0), reinterpret_cast<unsigned long long*>(counts));
  AVDB_LAUNCH_CHECK("k_vo_clean<size>");
  return AVDB_OK;
}

extern "C" int avdb_vep_output_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                     const avdb_vep_rows_in* in, uint32_t flags, const uint64_t* out_off,
                                     const uint32_t* out_len, const uint32_t* dict_at, const uint32_t* dict_len,
                                     const uint8_t* out_flags, uint8_t* out, size_t out_cap, uint64_t* totals,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  const vout::OutCols lc{nullptr, const_cast<uint32_t*>(out_len), const_cast<uint32_t*>(dict_at),
                    const_cast<uint32_t*>(dict_len), const_cast<uint8_t*>(out_flags)};
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, in, out_off, lc, out, out_cap, totals))
    return tables::invalid("avdb_vep_output_write", err);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_vep_output_write", ctx, vo_workspace(n_lines), n_lines, workspace, workspace_bytes,
                               totals, 2, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  uint64_t* starts = reinterpret_cast<uint64_t*>(static_cast<char*>(workspace) + AVDB_VCF_COUNT_WORKSPACE_BYTES);
  AVDB_HIP_TRY(hipMemsetAsync(starts, 0xFF, 8 * n_lines, s));
  if (int e = text_line_starts(text, text_bytes, n_lines, workspace, starts, s)) return e;
  hipLaunchKernelGGL(vout::k_vo_clean<true>, dim3(stream_grid(n_lines, vout::kVoWavesPerBlock, 4096)), dim3(kBlock), 0, s, text,
                     text_bytes, starts, n_lines, *in, lc, out_off, out, uint64_t(out_cap),
                     reinterpret_cast<unsigned long long*>(totals));
  AVDB_LAUNCH_CHECK("k_vo_clean<write>");
  hipLaunchKernelGGL(vout::k_vo_dict<true>, dim3(stream_grid(n_lines, kBlock, 4096)), dim3(kBlock), 0, s, text, text_bytes,
                     n_lines, *in, static_cast<const uint8_t*>(nullptr), flags & AVDB_VEPOUT_IDENTITY_ONLY, lc, out_off, out,
                     uint64_t(out_cap));
  AVDB_LAUNCH_CHECK("k_vo_dict<write>");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------------------------
extern "C" int avdb_vep_output_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                         const avdb_vep_rows_in* in, const uint8_t* ent_flags, uint32_t flags,
                                         uint64_t* line_start, uint32_t* out_len, uint32_t* dict_at, uint32_t* dict_len,
                                         uint8_t* out_flags, uint64_t* counts) {
  const vout::OutCols lc{line_start, out_len, dict_at, dict_len, out_flags};
  if (const char* err = size_args_error(ctx, text, text_bytes, n_lines, in, ent_flags, lc, counts))
    return tables::invalid("avdb_vep_output_size_host", err);
  memset(counts, 0, 8 * AVDB_VEPOUT_N_COUNTS);
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  const bool identity_only = (flags & AVDB_VEPOUT_IDENTITY_ONLY) != 0;
  for (size_t li = 0; li < n_lines; ++li) {
    uint64_t s, e;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e);
    if (e > s && text[e - 1] == '\r') --e;
    line_start[li] = s;
    ++counts[AVDB_VEPOUT_COUNT_LINES];
    const uint32_t dl = dict_len[li] = vout::dict_entry(*in, ent_flags, text, text_bytes, li, identity_only);
    uint32_t why = 0, at = 0, n = 0;
    if (dl & vout::kUnsafe) why = 1u << (dl & 31u);
    else if (e - s > vout::kMaxLine) why = 1u << vep::kCap;
    else
      n = vout::walk_host<false>(text, s, e, in->input_start[li], uint32_t(in->input_len[li]), dl, [](uint32_t, uint32_t) {},
                           &at, &why);
    out_len[li] = why ? 0u : n;
    dict_at[li] = why ? 0u : at;
    out_flags[li] = why ? uint8_t(1 + vout::ctz(why)) : uint8_t(0);
    if (why) {
      ++counts[AVDB_VEPOUT_COUNT_HOST_LINES];
      ++counts[AVDB_VEPOUT_COUNT_REASON0 + vout::ctz(why)];
    } else {
      counts[AVDB_VEPOUT_COUNT_OUT_BYTES] += n;
    }
  }
  return AVDB_OK;
}

extern "C" int avdb_vep_output_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          const avdb_vep_rows_in* in, uint32_t flags, const uint64_t* out_off,
                                          const uint32_t* out_len, const uint32_t* dict_at, const uint32_t* dict_len,
                                          const uint8_t* out_flags, uint8_t* out, size_t out_cap, uint64_t* totals) {
  const vout::OutCols lc{nullptr, const_cast<uint32_t*>(out_len), const_cast<uint32_t*>(dict_at),
                    const_cast<uint32_t*>(dict_len), const_cast<uint8_t*>(out_flags)};
  if (const char* err = write_args_error(ctx, text, text_bytes, n_lines, in, out_off, lc, out, out_cap, totals))
    return tables::invalid("avdb_vep_output_write_host", err);
  totals[0] = totals[1] = 0;
  if (n_lines == 0) return AVDB_OK;
  const std::vector<uint64_t> starts = lines::host_line_starts(text, text_bytes, n_lines);
  const bool identity_only = (flags & AVDB_VEPOUT_IDENTITY_ONLY) != 0;
  for (size_t li = 0; li < n_lines; ++li) {
    if (out_flags[li]) continue;
    uint64_t s, e;
    lines::line_span(text, text_bytes, starts.data(), n_lines, li, &s, &e);
    if (e > s && text[e - 1] == '\r') --e;
    const uint64_t off = out_off[li];
    const uint32_t want = out_len[li], dl = dict_len[li], da = dict_at[li];
    if ((dl & vout::kUnsafe) || off > out_cap || want > out_cap - off || da > want || dl > want - da || in->input_len[li] < 0 ||
        in->line_flags[li]) {
      ++totals[1];
      continue;
    }
    uint8_t* dst = out + off;
    uint32_t at, why;
    const uint32_t n = vout::walk_host<true>(text, s, e, in->input_start[li], uint32_t(in->input_len[li]), dl,
                                       [&](uint32_t k, uint32_t c) {
                                         if (k < want) dst[k] = uint8_t(c);
                                       },
                                       &at, &why);
    if (n != want || at != da) {
      ++totals[1];
      continue;
    }
    vout::dict_json(text, text_bytes, in->input_start[li], in->input_len[li], identity_only, [&](uint32_t k, uint32_t c) {
      if (k < dl) dst[da + k] = uint8_t(c);
    });
    totals[0] += want;
  }
  return AVDB_OK;
}

// ---- the update rows with the extra column -------------------------------------------------------
static const char* upd_views(const avdb_vep_rows_table* t, const avdb_vep_output_table* c, lof::Table* T) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_vep_rows_table)) return "avdb_vep_rows_table of another size";
  memset(T, 0, sizeof(*T));
  if (const char* err = tables::fill_table_view(T, t->n_rows, t->keys, t->key_off, t->keyset, t->keyset_bytes, t->json,
                                                t->json_bytes, t->json_off, t->json_len, t->hit))
    return err;
  return vout::cleaned_error(c, t->n_rows);
}

extern "C" int avdb_vep_output_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                            size_t n_rows, const avdb_vep_rows_table* table,
                                            const avdb_vep_output_table* cleaned, uint32_t flags, uint64_t alg_id,
                                            const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                            const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                                            size_t out_cap, uint64_t* row_off, uint64_t* totals, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  lof::Table T;
  const char* err = upd_views(table, cleaned, &T);
  const tables::UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                          const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const tables::Entry c{"avdb_vep_output_update_write", ctx, {text, text_bytes, n_lines}, err};
  const tables::UpdOut u{out, out_cap, row_off, totals};
  if (const char* e = tables::upd_write_error(c, n_rows, o, u)) return tables::invalid(c.fn, e);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_write(c.fn, ctx, tables::upd_layout(n_lines), n_lines, workspace, workspace_bytes, out_len,
                                n_rows, out_cap, row_off, totals, s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL(vout::k_vo_upd_write, dim3(stream_grid(n_rows, vout::kVoWavesPerBlock, 4096)), dim3(kBlock), 0, s, text, text_bytes,
                     T, *cleaned, alg_id, flags, o, row_off, n_rows, out, totals);
  AVDB_LAUNCH_CHECK("k_vo_upd_write");
  return AVDB_OK;
}

extern "C" int avdb_vep_output_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes,
                                                 size_t n_lines, size_t n_rows, const avdb_vep_rows_table* table,
                                                 const avdb_vep_output_table* cleaned, uint32_t flags, uint64_t alg_id,
                                                 const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                                 const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out,
                                                 size_t out_cap, uint64_t* row_off, uint64_t* totals) {
  lof::Table T;
  const char* err = upd_views(table, cleaned, &T);
  const tables::UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                          const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const tables::Entry c{"avdb_vep_output_update_write_host", ctx, {text, text_bytes, n_lines}, err};
  const tables::UpdOut u{out, out_cap, row_off, totals};
  if (const char* e = tables::upd_write_error(c, n_rows, o, u)) return tables::invalid(c.fn, e);
  if (int e = rows::host_row_offsets(c.fn, out_len, n_rows, out_cap, row_off, totals)) return e;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (size_t r = 0; r < n_rows; ++r) {
    const lof::UpdRow row{row_start[r], pk_len[r], out_len[r], row_flags[r], match[r]};
    uint8_t* dst = out + row_off[r];
    const vout::RowParts P = vout::row_parts(row, T, *cleaned, alg_id, flags, tb);
    if (!P.ok) {
      memset(dst, ' ', row.out_len);
      continue;
    }
    for (uint32_t j = 0; j < P.head_n; ++j) dst[j] = uint8_t(vout::head_byte(row, P, j, tb));
    uint8_t* d = dst + P.head_n;
    memcpy(d, T.json + P.body_s, P.body_n);
    d += P.body_n;
    *d++ = uint8_t('\t');
    memcpy(d, cleaned->text + P.clean_s, P.clean_n);
    d += P.clean_n;
    for (uint32_t j = 0; j < P.tail_n; ++j) d[j] = uint8_t(vout::tail_byte(P, alg_id, j));
  }
  return AVDB_OK;
}

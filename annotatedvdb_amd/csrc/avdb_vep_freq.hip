// K18d — the allele_frequencies column of the VEP update rows (gfx950).
//
// Replaces, for xstr(alleleFreq) of VEPVariantLoader.__parse_alt_alleles (vep_variant_loader.py:85-109,
// 126-142, 190-199: VepJsonParser.get_frequencies, the allele's regrouped frequencies, the INFO FREQ
// column of the ALT merged into them), the host loop with passes on K18a's arrays and K18b's entries
// of the same slab:
//   size pass (avdb_vep_freq_size)
//     k_vf_input        one lane per line: K18a's and K18b's verdicts first, then `input`: the id to
//                       match, the span of INFO FREQ, two ALTs with one normalised allele
//     k_vf_find         one wave per line, 64 bytes a step: colocated_variants, its elements and their
//                       keys from ballots, the selection over wave-uniform running state; the span of
//                       the chosen `frequencies` object
//     k_vf_rows<false>  one wave per line, its ALTs in turn: the chosen object walked 64 bytes a step,
//                       the allele's members one per lane, a ballot rank and a wave scan per group;
//                       the FREQ part by one lane; a length per table row, the counts
//   write pass (avdb_vep_freq_write; the caller scanned the lengths)
//     k_vf_rows<true>   the same walk; a lane stores its member, lane 0 the braces, the group headers
//                       and the FREQ part
//   the update rows with the column (avdb_vep_freq_update_write, behind avdb_vep_rows_update_size)
//     k_vf_upd_write    one wave per output row, as k_vo_upd_write, with one more part
// The per-block, per-line and per-row code is avdb_vep_freq.hpp, shared with the _host entries.
#include "avdb_vep_freq.hpp"

#include <string.h>

namespace avdb {
namespace vfreq {

constexpr unsigned kVfWavesPerBlock = unsigned(kBlock) / unsigned(kWave);

struct LineCols {
  uint64_t* fr_start;
  uint32_t* fr_len;
  uint64_t* fq_start;
  uint32_t* fq_len;
  uint8_t* flags;
};

__global__ __launch_bounds__(kBlock) void k_vf_input(const uint8_t* __restrict__ text, size_t text_bytes, size_t n_lines,
                                                     In in, const uint32_t* __restrict__ ent_alts,
                                                     const uint8_t* __restrict__ ent_flags, uint32_t flags, LineCols lc,
                                                     uint64_t* __restrict__ id_start, uint32_t* __restrict__ id_len) {
  for (size_t li = size_t(blockIdx.x) * blockDim.x + threadIdx.x; li < n_lines; li += size_t(gridDim.x) * blockDim.x) {
    const LineIn L = line_input(in, ent_flags, text, text_bytes, li, ent_alts[li], (flags & AVDB_VEPFREQ_IDENTITY_ONLY) != 0,
                                (flags & AVDB_VEPFREQ_MATCH_REFSNP) != 0);
    lc.flags[li] = L.flags;
    lc.fq_start[li] = L.fq_s;
    lc.fq_len[li] = L.fq_n;
    lc.fr_start[li] = 0;
    lc.fr_len[li] = 0;
    id_start[li] = L.id_s;
    id_len[li] = L.id_len;
  }
}

// a block of a span as ballots: lane `lane` holds byte b0 + lane of [.., e)
__device__ __forceinline__ Raw raw_ballots(const uint8_t* __restrict__ text, uint64_t pos, uint64_t e) {
  const bool v = pos < e;
  const uint32_t c = v ? text[pos] : 0u;
  bool f[8];
  raw_of_byte(uint8_t(c), f);
  return Raw{__ballot(v && f[0]), __ballot(v && f[1]), __ballot(v && f[2]), __ballot(v && f[3]), __ballot(v && f[4]),
             __ballot(v && f[5]), __ballot(v && f[6]), __ballot(v && f[7]), __ballot(v)};
}

__global__ __launch_bounds__(kBlock) void k_vf_find(const uint8_t* __restrict__ text, size_t text_bytes,
                                                    const uint64_t* __restrict__ line_start, size_t n_lines, LineCols lc,
                                                    const uint64_t* __restrict__ id_start,
                                                    const uint32_t* __restrict__ id_len) {
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kVfWavesPerBlock;
  for (uint64_t li = wave; li < n_lines; li += n_waves) {
    if (lc.flags[li]) continue;
    uint64_t s, e;
    lines::line_span(text, text_bytes, line_start, n_lines, li, &s, &e);
    if (e > s && text[e - 1] == '\r') --e;
    const LineIn L{0, id_start[li], 0, id_len[li], 0};
    const bool want_id = L.id_len != 0xFFFFFFFFu;
    Find st{};
    if (e - s > vout::kMaxLine) st.why |= 1u << vep::kCap;
    for (uint64_t b0 = s; b0 < e && !st.why; b0 += uint64_t(kWave)) {
      const uint64_t pos = b0 + lane;
      const bool v = pos < e;
      const Raw r = raw_ballots(text, pos, e);
      const Masks M = derive(r, st.c);
      const int32_t dep = v ? vep::depth_at(M.m, st.c.depth, lane) : 0;
      const uint64_t d1 = __ballot(dep == 1), d2 = __ballot(dep == 2), d3 = __ballot(dep == 3), d4 = __ballot(dep == 4);
      step_depth(M, st.c);
      const bool k1 = ((find_key1(M, d1) >> lane) & 1) && vout::key_is(text + pos, e - pos, "\"colocated_variants\":");
      const uint64_t cvk = __ballot(k1), cva = __ballot(k1 && e - pos > 21 && text[pos + 21] == '[');
      const FindMasks F = find_masks(r, M, d1, d2, d3, d4, cvk, cva, st);
      KeyHit H{kKeyNone, false, false};
      if ((F.key3 >> lane) & 1) H = key3_at(text + pos, e - pos, text, L);
      const uint64_t k_as = __ballot(H.kind == kKeyAs), k_id = __ballot(H.kind == kKeyId), k_fr = __ballot(H.kind == kKeyFr);
      const uint64_t k_ok = __ballot(H.ok), k_x = __ballot(H.x);
      find_events(F, k_as, k_id, k_fr, k_ok, k_x, want_id, b0, st);
    }
    const Chosen C = st.why ? Chosen{st.why, 0, 0} : find_end(st);
    if (lane == 0) {
      lc.fr_start[li] = C.fs;
      lc.fr_len[li] = C.fn;
      if (C.why) lc.flags[li] = uint8_t(1 + ctz(C.why));
    }
  }
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t from) {
  return (uint64_t(uint32_t(__shfl(uint32_t(v >> 32), int(from), kWave))) << 32) | uint32_t(__shfl(uint32_t(v), int(from), kWave));
}

// One row by the whole wave: the chosen object [fs, fs + fn) walked for ALT A (number alt_k from 1).
// Returns the length, or kBad | the reason; kWrite: its bytes go to dst[0, want).
template <bool kWrite>
__device__ __forceinline__ uint32_t row_wave(const uint8_t* __restrict__ text, uint64_t fs, uint32_t fn,
                                             const vrows::Alt& A, uint32_t alt_k, uint64_t fq_s, uint32_t fq_n,
                                             uint8_t* __restrict__ dst, uint32_t want) {
  const uint32_t lane = __lane_id();
  RowWalk st{};
  uint64_t key_at = ~0ull;
  const uint64_t e = fs + fn;
  for (uint64_t b0 = fs; b0 < e; b0 += uint64_t(kWave)) {
    const uint64_t pos = b0 + lane;
    const bool v = pos < e;
    const Raw r = raw_ballots(text, pos, e);
    const Masks M = derive(r, st.c);
    const int32_t dep = v ? vep::depth_at(M.m, st.c.depth, lane) : 0;
    const uint64_t d1 = __ballot(dep == 1), d2 = __ballot(dep == 2), d3 = __ballot(dep == 3);
    step_depth(M, st.c);
    bool obj = false;
    const bool hit = ((row_akey(M, d1) >> lane) & 1) && allele_key_is(text + pos, e - pos, text, A, &obj);
    const uint64_t am = __ballot(hit), aobj = __ballot(hit && obj);
    const RowMasks R = row_masks(r, M, d1, d2, d3, am, aobj, st);
    const uint64_t at = lane_member(R, lane, b0);
    if (at != ~0ull) key_at = at;
  }
  uint32_t why = st.why;
  if (st.n_match > 1) why |= 1u << kDupKey;
  if (st.n_mem > kMaxMembers) why |= 1u << kMembers;
  if (why) return kBad | ctz(why);
  const bool has = lane < st.n_mem;
  Mem m{0, 0, 0, 0, kNoGroup, 0, false};
  if (has) m = member_at(text, key_at, e);
  if (__ballot(has && m.why)) why |= 1u << kValue;
  bool dup = false;
  for (uint32_t i = 0; i + 1 < st.n_mem; ++i) {  // a member's key against those of the lanes below it
    const uint64_t ks = shfl64(m.ks, i), k8 = shfl64(m.k8, i);
    const uint32_t kn = uint32_t(__shfl(m.kn, int(i), kWave));
    if (has && i < lane && same_key(text, m, ks, kn, k8)) dup = true;
  }
  if (__ballot(dup)) why |= 1u << kDupKey;
  if (why) return kBad | ctz(why);
  const uint32_t len = has ? mem_len(m) : 0u;
  const uint64_t g0 = __ballot(has && m.grp == kGnomad), g1 = __ballot(has && m.grp == kGenomes),
                 g2 = __ballot(has && m.grp == kEsp);
  const uint32_t s0 = wave_incl_sum(m.grp == kGnomad ? len : 0u), s1 = wave_incl_sum(m.grp == kGenomes ? len : 0u),
                 s2 = wave_incl_sum(m.grp == kEsp ? len : 0u);
  Layout Y{};
  Y.cnt0 = popc(g0);
  Y.cnt1 = popc(g1);
  Y.cnt2 = popc(g2);
  Y.len0 = uint32_t(__shfl(s0, kWave - 1, kWave));
  Y.len1 = uint32_t(__shfl(s1, kWave - 1, kWave));
  Y.len2 = uint32_t(__shfl(s2, kWave - 1, kWave));
  const uint32_t gmaf_groups = (__ballot(has && m.gmaf && m.grp == kGnomad) ? 1u : 0u) |
                               (__ballot(has && m.gmaf && m.grp == kGenomes) ? 2u : 0u) |
                               (__ballot(has && m.gmaf && m.grp == kEsp) ? 4u : 0u);
  FreqPart F{};
  if (fq_n) {  // one lane walks FREQ; the wave takes what it found
    if (lane == 0)
      F = freq_part(text, fq_s, fq_n, alt_k, present_of(Y), [](uint32_t, uint32_t, uint32_t) {}, [](uint32_t, uint32_t) {});
    F.why = uint32_t(__shfl(F.why, 0, kWave));
    F.gm0 = uint32_t(__shfl(F.gm0, 0, kWave));
    F.gm1 = uint32_t(__shfl(F.gm1, 0, kWave));
    F.gm2 = uint32_t(__shfl(F.gm2, 0, kWave));
    F.tail = uint32_t(__shfl(F.tail, 0, kWave));
  }
  Y.F = F;
  why |= F.why | gmaf_clash(Y, gmaf_groups);
  if (why) return kBad | ctz(why);
  lay_out(Y);
  if (kWrite && Y.total == want) {
    auto put = [=](uint32_t k, uint32_t c) {
      if (k < want) dst[k] = uint8_t(c);
    };
    if (has) {
      const uint64_t g = m.grp == kGnomad ? g0 : m.grp == kGenomes ? g1 : g2;
      const uint32_t incl = m.grp == kGnomad ? s0 : m.grp == kGenomes ? s1 : s2;
      put_member(text, Y, m.grp, m.ks, m.kn, m.vn, popc(g & bits_lt(lane)), incl - len, put);
    }
    if (lane == 0) put_frame(text, Y, fq_s, fq_n, alt_k, put);
  }
  return Y.total;
}

// ctr: the size pass's counts, or the write pass's totals
template <bool kWrite>
__global__ __launch_bounds__(kBlock) void k_vf_rows(const uint8_t* __restrict__ text, size_t text_bytes, size_t n_lines,
                                                    size_t n_rows, In in, const uint32_t* __restrict__ ent_alts,
                                                    const uint64_t* __restrict__ row0, LineCols lc,
                                                    uint32_t* __restrict__ freq_len,
                                                    const uint64_t* __restrict__ freq_off, uint8_t* __restrict__ out,
                                                    uint64_t out_cap, unsigned long long* __restrict__ ctr) {
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kVfWavesPerBlock;
  unsigned long long acc = 0;  // lane k: what this wave adds to ctr[k]
  for (uint64_t li = wave; li < n_lines; li += n_waves) {
    const uint32_t alts = ent_alts[li];
    const uint64_t first = row0[li];
    uint32_t why = 0;
    const uint32_t f = lc.flags[li];
    if (!kWrite) acc += lane == AVDB_VEPFREQ_COUNT_LINES;
    if (f) {
      if (kWrite) continue;
      why = 1u << ((f - 1u) & 31u);
    } else if (first > n_rows || alts > n_rows - first) {
      why = 1u << vep::kStruct;  // (never: row0 are the sums of ent_alts)
    }
    uint64_t bytes = 0;
    if (!why) {
      const vrows::Input I = vrows::parse_input(text, text_bytes, in.input_start[li], in.input_len[li]);
      if (I.why || I.n_alts != alts) why = 1u << vep::kStruct;  // (never: k_vf_input read it)
      const uint64_t fs = lc.fr_start[li], fq_s = lc.fq_start[li];
      const uint32_t fn = lc.fr_len[li], fq_n = lc.fq_len[li];
      if (fs > text_bytes || fn > text_bytes - fs || fq_s > text_bytes || fq_n > text_bytes - fq_s) why = 1u << vep::kStruct;
      uint32_t cursor = 0;
      for (uint32_t a = 0; a < alts && !why; ++a) {
        const vrows::Alt A = vrows::next_alt(text, I, &cursor);
        const uint64_t r = first + a;
        uint8_t* dst = nullptr;
        uint32_t want = 0;
        if (kWrite) {
          const uint64_t off = freq_off[r];
          want = freq_len[r];
          if (off > out_cap || want > out_cap - off) {
            acc += lane == 1;
            continue;
          }
          dst = out + off;
        }
        const uint32_t n = row_wave<kWrite>(text, fs, fn, A, a + 1, fq_s, fq_n, dst, want);
        if (kWrite) {
          if (n != want) acc += lane == 1;  // (never: the text is the one the size pass read)
          else if (lane == 0) acc += want;
        } else if (n & kBad) {
          why = 1u << (n & 31u);
        } else {
          if (lane == 0) freq_len[r] = n;
          bytes += n;
        }
      }
    }
    if (kWrite) continue;
    if (why) {
      for (uint64_t a = lane; a < alts && first + a < n_rows; a += uint64_t(kWave)) freq_len[first + a] = 0;
      if (lane == 0) lc.flags[li] = uint8_t(1 + ctz(why));
      acc += lane == AVDB_VEPFREQ_COUNT_HOST_LINES || lane == AVDB_VEPFREQ_COUNT_REASON0 + ctz(why);
    } else {
      if (lane == AVDB_VEPFREQ_COUNT_ROWS) acc += alts;
      if (lane == AVDB_VEPFREQ_COUNT_OUT_BYTES) acc += bytes;
    }
  }
  if (acc && lane < (kWrite ? 2u : uint32_t(AVDB_VEPFREQ_N_COUNTS))) atomicAdd(&ctr[lane], acc);
}

// One wave per output row: the head a byte a lane, the frequency text, the body and the cleaned text
// copied 64 bytes a step from their blobs, the tail a byte a lane.  A row whose parts do not add up
// is left blank.
__global__ __launch_bounds__(kBlock) void k_vf_upd_write(const uint8_t* __restrict__ text, size_t text_bytes, lof::Table T,
                                                         Freq Q, vout::Cleaned C, uint32_t has_clean, uint64_t alg_id,
                                                         uint32_t flags, tables::UpdCols o,
                                                         const uint64_t* __restrict__ row_off, size_t n_rows,
                                                         uint8_t* __restrict__ out, const uint64_t* __restrict__ totals) {
  if (totals[1]) return;  // the capacity is too small: nothing is written
  const uint32_t lane = __lane_id();
  const uint64_t wave = (uint64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave;
  const uint64_t n_waves = uint64_t(gridDim.x) * kVfWavesPerBlock;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (uint64_t r = wave; r < n_rows; r += n_waves) {
    const lof::UpdRow row{o.row_start[r], o.pk_len[r], o.out_len[r], o.flags[r], o.match[r]};
    // (k_row_totals found the output large enough: [row_off[r], row_off[r] + out_len) lies inside it)
    uint8_t* dst = out + row_off[r];
    const RowParts X = row_parts(row, T, Q, has_clean ? &C : nullptr, alg_id, flags, tb);
    const vout::RowParts& P = X.P;
    if (!P.ok) {
      for (uint32_t k = lane; k < row.out_len; k += uint32_t(kWave)) dst[k] = uint8_t(' ');
      continue;
    }
    for (uint32_t j = lane; j < P.head_n; j += uint32_t(kWave)) dst[j] = uint8_t(vout::head_byte(row, P, j, tb));
    uint8_t* d = dst + P.head_n;
    const uint8_t* src = Q.text + X.fq_s;
    for (uint32_t j = lane; j < X.fq_n; j += uint32_t(kWave)) d[j] = src[j];
    d += X.fq_n;
    if (lane == 0) d[0] = uint8_t('\t');
    d += 1;
    src = T.json + P.body_s;
    for (uint32_t j = lane; j < P.body_n; j += uint32_t(kWave)) d[j] = src[j];
    d += P.body_n;
    if (has_clean) {
      if (lane == 0) d[0] = uint8_t('\t');
      d += 1;
      src = C.text + P.clean_s;
      for (uint32_t j = lane; j < P.clean_n; j += uint32_t(kWave)) d[j] = src[j];
      d += P.clean_n;
    }
    for (uint32_t j = lane; j < P.tail_n; j += uint32_t(kWave)) d[j] = uint8_t(vout::tail_byte(P, alg_id, j));
  }
}

}  // namespace vfreq
}  // namespace avdb

using namespace avdb;

// workspace: the id to match, per line: its start | its length
static size_t vf_workspace(size_t n_lines) { return lines::pad256(8 * n_lines) + lines::pad256(4 * n_lines); }

extern "C" int avdb_vep_freq_workspace_size(size_t text_bytes, size_t n_lines, size_t* bytes) {
  (void)text_bytes;
  return rows::workspace_size(vf_workspace(n_lines), bytes);
}

extern "C" int avdb_vep_freq_token_ok_host(const uint8_t* token, size_t n) {
  return token && n <= 0xFFFFu && vfreq::token_ok(token, uint32_t(n)) ? 1 : 0;
}

static const char* line_args_error(const void* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                                   const avdb_vep_rows_in* in, const uint64_t* line_start, const uint32_t* ent_alts,
                                   const uint64_t* row0, const vfreq::LineCols& lc, const uint32_t* freq_len) {
  if (!ctx) return "null argument";
  if (const char* err = lines::text_args_error(text, text_bytes, n_lines)) return err;
  if (const char* err = vfreq::in_error(in, n_lines)) return err;
  if (n_rows >= 0x7FFFFFFFull) return "too many rows";
  if (n_lines && (!line_start || !ent_alts || !row0 || !lc.fr_start || !lc.fr_len || !lc.fq_start || !lc.fq_len || !lc.flags))
    return "null line array";
  if (n_rows && !freq_len) return "null row array";
  return nullptr;
}

extern "C" int avdb_vep_freq_size(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                                  const avdb_vep_rows_in* in, const uint64_t* line_start, const uint32_t* ent_alts,
                                  const uint8_t* ent_flags, const uint64_t* row0, uint32_t flags, uint64_t* fr_start,
                                  uint32_t* fr_len, uint64_t* fq_start, uint32_t* fq_len, uint8_t* out_flags,
                                  uint32_t* freq_len, uint64_t* counts, void* workspace, size_t workspace_bytes,
                                  void* stream) {
  const vfreq::LineCols lc{fr_start, fr_len, fq_start, fq_len, out_flags};
  const char* err = line_args_error(ctx, text, text_bytes, n_lines, n_rows, in, line_start, ent_alts, row0, lc, freq_len);
  if (!err && (!counts || (n_lines && !ent_flags))) err = "null argument";
  if (err) return tables::invalid("avdb_vep_freq_size", err);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_size("avdb_vep_freq_size", ctx, vf_workspace(n_lines), n_lines, workspace, workspace_bytes, counts,
                               AVDB_VEPFREQ_N_COUNTS, s))
    return e;
  if (n_lines == 0) return AVDB_OK;
  uint64_t* id_start = static_cast<uint64_t*>(workspace);
  uint32_t* id_len = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + lines::pad256(8 * n_lines));
  hipLaunchKernelGGL(vfreq::k_vf_input, dim3(stream_grid(n_lines, kBlock, 4096)), dim3(kBlock), 0, s, text, text_bytes, n_lines,
                     *in, ent_alts, ent_flags, flags, lc, id_start, id_len);
  AVDB_LAUNCH_CHECK("k_vf_input");
  const unsigned grid = stream_grid(n_lines, vfreq::kVfWavesPerBlock, 4096);
  hipLaunchKernelGGL(vfreq::k_vf_find, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, line_start, n_lines, lc,
                     static_cast<const uint64_t*>(id_start), static_cast<const uint32_t*>(id_len));
  AVDB_LAUNCH_CHECK("k_vf_find");
  hipLaunchKernelGGL(vfreq::k_vf_rows<false>, dim3(grid), dim3(kBlock), 0, s, text, text_bytes, n_lines, n_rows, *in, ent_alts,
                     row0, lc, freq_len, static_cast<const uint64_t*>(nullptr), static_cast<uint8_t*>(nullptr), uint64_t(0),
                     reinterpret_cast<unsigned long long*>(counts));
  AVDB_LAUNCH_CHECK("k_vf_rows<size>");
  return AVDB_OK;
}

extern "C" int avdb_vep_freq_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines, size_t n_rows,
                                   const avdb_vep_rows_in* in, const uint32_t* ent_alts, const uint64_t* row0,
                                   const uint64_t* fr_start, const uint32_t* fr_len, const uint64_t* fq_start,
                                   const uint32_t* fq_len, const uint8_t* out_flags, const uint64_t* freq_off,
                                   const uint32_t* freq_len, uint8_t* out, size_t out_cap, uint64_t* totals,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  const vfreq::LineCols lc{const_cast<uint64_t*>(fr_start), const_cast<uint32_t*>(fr_len), const_cast<uint64_t*>(fq_start),
                           const_cast<uint32_t*>(fq_len), const_cast<uint8_t*>(out_flags)};
  const char* err = line_args_error(ctx, text, text_bytes, n_lines, n_rows, in, fr_start, ent_alts, row0, lc, freq_len);
  if (!err && (!totals || (n_rows && !freq_off))) err = "null argument";
  if (!err) err = rows::out_error(out, out_cap);
  if (err) return tables::invalid("avdb_vep_freq_write", err);
  (void)workspace;
  (void)workspace_bytes;
  hipStream_t s = static_cast<hipStream_t>(stream);
  AVDB_HIP_TRY(hipSetDevice(ctx->device));
  AVDB_HIP_TRY(hipMemsetAsync(totals, 0, 16, s));
  if (n_lines == 0) return AVDB_OK;
  hipLaunchKernelGGL(vfreq::k_vf_rows<true>, dim3(stream_grid(n_lines, vfreq::kVfWavesPerBlock, 4096)), dim3(kBlock), 0, s, text,
                     text_bytes, n_lines, n_rows, *in, ent_alts, row0, lc, const_cast<uint32_t*>(freq_len), freq_off, out,
                     uint64_t(out_cap), reinterpret_cast<unsigned long long*>(totals));
  AVDB_LAUNCH_CHECK("k_vf_rows<write>");
  return AVDB_OK;
}

// ---- the same code on the host ------------------------------------------------------------------
extern "C" int avdb_vep_freq_size_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                       size_t n_rows, const avdb_vep_rows_in* in, const uint64_t* line_start,
                                       const uint32_t* ent_alts, const uint8_t* ent_flags, const uint64_t* row0,
                                       uint32_t flags, uint64_t* fr_start, uint32_t* fr_len, uint64_t* fq_start,
                                       uint32_t* fq_len, uint8_t* out_flags, uint32_t* freq_len, uint64_t* counts) {
  const vfreq::LineCols lc{fr_start, fr_len, fq_start, fq_len, out_flags};
  const char* err = line_args_error(ctx, text, text_bytes, n_lines, n_rows, in, line_start, ent_alts, row0, lc, freq_len);
  if (!err && (!counts || (n_lines && !ent_flags))) err = "null argument";
  if (err) return tables::invalid("avdb_vep_freq_size_host", err);
  memset(counts, 0, 8 * AVDB_VEPFREQ_N_COUNTS);
  const bool identity_only = (flags & AVDB_VEPFREQ_IDENTITY_ONLY) != 0, match = (flags & AVDB_VEPFREQ_MATCH_REFSNP) != 0;
  for (size_t li = 0; li < n_lines; ++li) {
    ++counts[AVDB_VEPFREQ_COUNT_LINES];
    const uint32_t alts = ent_alts[li];
    const uint64_t first = row0[li];
    const vfreq::LineIn L = vfreq::line_input(*in, ent_flags, text, text_bytes, li, alts, identity_only, match);
    fq_start[li] = L.fq_s;
    fq_len[li] = L.fq_n;
    fr_start[li] = 0;
    fr_len[li] = 0;
    uint32_t why = L.flags ? 1u << ((L.flags - 1u) & 31u) : 0u;
    uint64_t s, e;
    lines::line_span(text, text_bytes, line_start, n_lines, li, &s, &e);
    if (e > s && text[e - 1] == '\r') --e;
    if (!why && e - s > vout::kMaxLine) why = 1u << vep::kCap;
    if (!why && (first > n_rows || alts > n_rows - first)) why = 1u << vep::kStruct;
    uint64_t bytes = 0;
    if (!why) {
      const vfreq::Chosen C = vfreq::find_host(text, s, e, L);
      why = C.why;
      fr_start[li] = C.fs;
      fr_len[li] = C.fn;
      const vrows::Input I = vrows::parse_input(text, text_bytes, in->input_start[li], in->input_len[li]);
      uint32_t cursor = 0;
      for (uint32_t a = 0; a < alts && !why; ++a) {
        const vrows::Alt A = vrows::next_alt(text, I, &cursor);
        const uint32_t n = vfreq::row_host<false>(text, C.fs, C.fn, A, a + 1, L.fq_s, L.fq_n, [](uint32_t, uint32_t) {});
        if (n & vfreq::kBad) why = 1u << (n & 31u);
        else freq_len[first + a] = n, bytes += n;
      }
    }
    out_flags[li] = why ? uint8_t(1 + vfreq::ctz(why)) : uint8_t(0);
    if (why) {
      for (uint64_t a = 0; a < alts && first + a < n_rows; ++a) freq_len[first + a] = 0;
      ++counts[AVDB_VEPFREQ_COUNT_HOST_LINES];
      ++counts[AVDB_VEPFREQ_COUNT_REASON0 + vfreq::ctz(why)];
    } else {
      counts[AVDB_VEPFREQ_COUNT_ROWS] += alts;
      counts[AVDB_VEPFREQ_COUNT_OUT_BYTES] += bytes;
    }
  }
  return AVDB_OK;
}

extern "C" int avdb_vep_freq_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                        size_t n_rows, const avdb_vep_rows_in* in, const uint32_t* ent_alts,
                                        const uint64_t* row0, const uint64_t* fr_start, const uint32_t* fr_len,
                                        const uint64_t* fq_start, const uint32_t* fq_len, const uint8_t* out_flags,
                                        const uint64_t* freq_off, const uint32_t* freq_len, uint8_t* out, size_t out_cap,
                                        uint64_t* totals) {
  const vfreq::LineCols lc{const_cast<uint64_t*>(fr_start), const_cast<uint32_t*>(fr_len), const_cast<uint64_t*>(fq_start),
                           const_cast<uint32_t*>(fq_len), const_cast<uint8_t*>(out_flags)};
  const char* err = line_args_error(ctx, text, text_bytes, n_lines, n_rows, in, fr_start, ent_alts, row0, lc, freq_len);
  if (!err && (!totals || (n_rows && !freq_off))) err = "null argument";
  if (!err) err = rows::out_error(out, out_cap);
  if (err) return tables::invalid("avdb_vep_freq_write_host", err);
  totals[0] = totals[1] = 0;
  for (size_t li = 0; li < n_lines; ++li) {
    if (out_flags[li]) continue;
    const uint32_t alts = ent_alts[li];
    const uint64_t first = row0[li], fs = fr_start[li], fq_s = fq_start[li];
    const uint32_t fn = fr_len[li], fq_n = fq_len[li];
    const vrows::Input I = vrows::parse_input(text, text_bytes, in->input_start[li], in->input_len[li]);
    if (first > n_rows || alts > n_rows - first || I.why || I.n_alts != alts || in->line_flags[li] || fs > text_bytes ||
        fn > text_bytes - fs || fq_s > text_bytes || fq_n > text_bytes - fq_s) {
      ++totals[1];
      continue;
    }
    uint32_t cursor = 0;
    for (uint32_t a = 0; a < alts; ++a) {
      const vrows::Alt A = vrows::next_alt(text, I, &cursor);
      const uint64_t off = freq_off[first + a];
      const uint32_t want = freq_len[first + a];
      if (off > out_cap || want > out_cap - off) {
        ++totals[1];
        continue;
      }
      uint8_t* dst = out + off;
      // (a first walk without stores: a text that differs from the size pass's is not written)
      if (vfreq::row_host<false>(text, fs, fn, A, a + 1, fq_s, fq_n, [](uint32_t, uint32_t) {}) != want) {
        ++totals[1];
        continue;
      }
      vfreq::row_host<true>(text, fs, fn, A, a + 1, fq_s, fq_n, [&](uint32_t k, uint32_t c) {
        if (k < want) dst[k] = uint8_t(c);
      });
      totals[0] += want;
    }
  }
  return AVDB_OK;
}

// ---- the update rows with the column -------------------------------------------------------------
static const char* upd_views(const avdb_vep_rows_table* t, const avdb_vep_freq_table* q, const avdb_vep_output_table* c,
                             lof::Table* T) {
  if (!t) return "null table";
  if (t->struct_size != sizeof(avdb_vep_rows_table)) return "avdb_vep_rows_table of another size";
  memset(T, 0, sizeof(*T));
  if (const char* err = tables::fill_table_view(T, t->n_rows, t->keys, t->key_off, t->keyset, t->keyset_bytes, t->json,
                                                t->json_bytes, t->json_off, t->json_len, t->hit))
    return err;
  if (const char* err = vfreq::freq_error(q, t->n_rows)) return err;
  return c ? vout::cleaned_error(c, t->n_rows) : nullptr;
}

extern "C" int avdb_vep_freq_update_write(avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                          size_t n_rows, const avdb_vep_rows_table* table, const avdb_vep_freq_table* freq,
                                          const avdb_vep_output_table* cleaned, uint32_t flags, uint64_t alg_id,
                                          const uint64_t* row_start, const uint32_t* pk_len, const int32_t* match,
                                          const uint32_t* out_len, const uint8_t* row_flags, uint8_t* out, size_t out_cap,
                                          uint64_t* row_off, uint64_t* totals, void* workspace, size_t workspace_bytes,
                                          void* stream) {
  lof::Table T;
  const char* err = upd_views(table, freq, cleaned, &T);
  const tables::UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                          const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const tables::Entry c{"avdb_vep_freq_update_write", ctx, {text, text_bytes, n_lines}, err};
  const tables::UpdOut u{out, out_cap, row_off, totals};
  if (const char* e = tables::upd_write_error(c, n_rows, o, u)) return tables::invalid(c.fn, e);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int e = rows::begin_write(c.fn, ctx, tables::upd_layout(n_lines), n_lines, workspace, workspace_bytes, out_len, n_rows,
                                out_cap, row_off, totals, s))
    return e;
  if (n_rows == 0) return AVDB_OK;
  hipLaunchKernelGGL(vfreq::k_vf_upd_write, dim3(stream_grid(n_rows, vfreq::kVfWavesPerBlock, 4096)), dim3(kBlock), 0, s, text,
                     text_bytes, T, *freq, cleaned ? *cleaned : avdb_vep_output_table{}, cleaned ? 1u : 0u, alg_id, flags, o,
                     row_off, n_rows, out, totals);
  AVDB_LAUNCH_CHECK("k_vf_upd_write");
  return AVDB_OK;
}

extern "C" int avdb_vep_freq_update_write_host(const avdb_ctx* ctx, const uint8_t* text, size_t text_bytes, size_t n_lines,
                                               size_t n_rows, const avdb_vep_rows_table* table,
                                               const avdb_vep_freq_table* freq, const avdb_vep_output_table* cleaned,
                                               uint32_t flags, uint64_t alg_id, const uint64_t* row_start,
                                               const uint32_t* pk_len, const int32_t* match, const uint32_t* out_len,
                                               const uint8_t* row_flags, uint8_t* out, size_t out_cap, uint64_t* row_off,
                                               uint64_t* totals) {
  lof::Table T;
  const char* err = upd_views(table, freq, cleaned, &T);
  const tables::UpdCols o{const_cast<uint64_t*>(row_start), const_cast<uint32_t*>(pk_len), const_cast<int32_t*>(match),
                          const_cast<uint32_t*>(out_len), const_cast<uint8_t*>(row_flags)};
  const tables::Entry c{"avdb_vep_freq_update_write_host", ctx, {text, text_bytes, n_lines}, err};
  const tables::UpdOut u{out, out_cap, row_off, totals};
  if (const char* e = tables::upd_write_error(c, n_rows, o, u)) return tables::invalid(c.fn, e);
  if (int e = rows::host_row_offsets(c.fn, out_len, n_rows, out_cap, row_off, totals)) return e;
  auto tb = [&](uint64_t pos) -> uint32_t { return pos < text_bytes ? uint32_t(text[pos]) : 0u; };
  for (size_t r = 0; r < n_rows; ++r) {
    const lof::UpdRow row{row_start[r], pk_len[r], out_len[r], row_flags[r], match[r]};
    uint8_t* dst = out + row_off[r];
    const vfreq::RowParts X = vfreq::row_parts(row, T, *freq, cleaned, alg_id, flags, tb);
    const vout::RowParts& P = X.P;
    if (!P.ok) {
      memset(dst, ' ', row.out_len);
      continue;
    }
    for (uint32_t j = 0; j < P.head_n; ++j) dst[j] = uint8_t(vout::head_byte(row, P, j, tb));
    uint8_t* d = dst + P.head_n;
    memcpy(d, freq->text + X.fq_s, X.fq_n);
    d += X.fq_n;
    *d++ = uint8_t('\t');
    memcpy(d, T.json + P.body_s, P.body_n);
    d += P.body_n;
    if (cleaned) {
      *d++ = uint8_t('\t');
      memcpy(d, cleaned->text + P.clean_s, P.clean_n);
      d += P.clean_n;
    }
    for (uint32_t j = 0; j < P.tail_n; ++j) d[j] = uint8_t(vout::tail_byte(P, alg_id, j));
  }
  return AVDB_OK;
}

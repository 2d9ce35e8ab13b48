// K18c — the vep_output column of the VEP update rows (avdb_vep_output.hip): the code a line's
// cleaned result, its entry dict and an update row with the extra column are made of, compiled for
// both sides as avdb_vep.hpp and avdb_vep_rows.hpp are.
//
// The cleaned result is the line's own top-level object, read in blocks of 64 bytes as K18a reads it
// (the escape mask, the string mask and the depth of avdb_vep.hpp): the caller turns a block into
// 64-bit masks (ballots on the device, a loop in the _host entries); member_starts finds the keys of
// the top-level members by K18a's read-back rule, dropped_key names the five that are dropped, and
// block derives what is the same for the whole block: the bytes that are copied, the ',' and ':'
// outside strings a space follows (K18b's rule), where a token begins, and what a position's output
// offset is made of.  What crosses a block edge is State: the carries of avdb_vep.hpp, whether the
// block begins inside a dropped member, the kept members and the output bytes so far.  The value of
// `input` (K18a's span) is not copied: the entry dict goes where it stood, rendered by one lane
// (dict_json: K18b's fields, K17's values).
#pragma once

#include "avdb_qc.hpp"
#include "avdb_vep_rows.hpp"

namespace avdb {
namespace vout {

using vep::bits_le;
using vep::bits_lt;
using vep::ctz;
using vep::popc;
using In = avdb_vep_rows_in;

// why a line is left to the host, behind K18b's reasons
enum : uint32_t { kKeptText = vrows::kToken + 1, kEightFields, kInputValue };
static_assert(kInputValue + 1 == AVDB_VEPOUT_N_REASONS, "reasons");
constexpr uint32_t kUnsafe = vrows::kUnsafe;  // dict_len: the line is the host's, its reason in the low bits
constexpr uint64_t kMaxLine = 1ull << 28;     // a longer line is the host's: lengths are u32, a dict is a few times its input

inline const char* in_error(const In* in, size_t n_lines) {
  if (!in || in->struct_size != sizeof(In)) return "null avdb_vep_rows_in, or one of another size";
  if (n_lines && (!in->line_flags || !in->input_start || !in->input_len)) return "null line array of K18a";
  return nullptr;
}

// the reason K18a or K18b left line li to the host, or -1
AVDB_HD int32_t prior_reason(const In& in, const uint8_t* ent_flags, uint64_t li) {
  const uint32_t f = in.line_flags[li];
  if (f) return f <= uint32_t(AVDB_VEP_N_REASONS) ? int32_t(f - 1u) : int32_t(vep::kStruct);  // (a flags byte K18a does not give)
  const uint32_t e = ent_flags[li];
  if (e & AVDB_VEPROWS_LINE_HOST) {
    const int32_t r = vrows::reason_of(e);
    return r >= 0 && r < int32_t(AVDB_VEPROWS_N_REASONS) ? r : int32_t(vep::kStruct);
  }
  return in.input_len[li] < 0 ? int32_t(vrows::kNoInput) : -1;  // (never: K18b flagged it)
}

// ---- the cleaned result, 64 bytes a step ---------------------------------------------------------
struct Raw {  // a block's bytes, a bit each (the line's bytes only)
  uint64_t bs, qt, open, close, comma, colon, okesc, ctl, hi, valid;
};
AVDB_HD void raw_of_byte(uint8_t c, bool* f) {  // in Raw's order, without valid
  f[0] = c == '\\';
  f[1] = c == '"';
  f[2] = c == '{' || c == '[';
  f[3] = c == '}' || c == ']';
  f[4] = c == ',';
  f[5] = c == ':';
  f[6] = c == '"' || c == '\\' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't';
  f[7] = c < 0x20;
  f[8] = c >= 0x80;
}

struct State {  // what crosses a block edge
  uint64_t esc, in_str;
  int32_t depth;
  uint32_t prev_oc;   // the last byte was a bracket that opens or a ',', outside a string
  uint32_t prev_tok;  // the last byte was a kept token's
  uint32_t in_drop;   // the next block begins inside a dropped member
  uint32_t n_kept;    // kept members so far
  uint32_t out;       // output bytes so far
  uint32_t why;
};

struct Masks {
  vep::Masks m;
  uint64_t escaped;
};
AVDB_HD Masks derive(const Raw& r, State& st) {
  Masks M;
  M.escaped = vep::escaped_of(r.bs, st.esc);
  M.m.quotes = r.qt & ~M.escaped;
  M.m.in_str = vep::prefix_xor(M.m.quotes) ^ st.in_str;
  st.in_str = (M.m.in_str >> 63) ? ~0ull : 0ull;
  M.m.sopen = M.m.quotes & M.m.in_str;
  M.m.outside = ~M.m.in_str;
  M.m.open = r.open & M.m.outside;
  M.m.close = r.close & M.m.outside;
  return M;
}

// where a top-level member begins: the opening quote of a string at depth 1 behind a '{' or a ','
// outside a string (a '[' puts what follows it at depth 2), K18a's read-back rule for `input`
AVDB_HD uint64_t member_starts(const Raw& r, const Masks& M, uint64_t d1, State& st) {
  const uint64_t oc = (r.open | r.comma) & M.m.outside;
  const uint64_t starts = M.m.sopen & d1 & ((oc << 1) | st.prev_oc);
  st.prev_oc = uint32_t(oc >> 63);
  return starts;
}

template <int N>
AVDB_HD bool key_is(const uint8_t* p, uint64_t avail, const char (&lit)[N]) {
  constexpr uint32_t n = N - 1;
  if (avail < n) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (p[i] != uint8_t(lit[i])) return false;
  return true;
}
// the member whose key opens at p (avail bytes to the line's end) is one __clean_result pops
AVDB_HD bool dropped_key(const uint8_t* p, uint64_t avail) {
  if (avail < 2) return false;
  switch (p[1]) {  // (the five names differ in their first byte)
    case 'c': return key_is(p, avail, "\"colocated_variants\":");
    case 't': return key_is(p, avail, "\"transcript_consequences\":");
    case 'r': return key_is(p, avail, "\"regulatory_feature_consequences\":");
    case 'm': return key_is(p, avail, "\"motif_feature_consequences\":");
    case 'i': return key_is(p, avail, "\"intergenic_consequences\":");
    default: return false;
  }
}

struct Block {
  uint64_t kept;       // the bytes that are copied
  uint64_t sep;        // the kept ',' and ':' outside strings: a space follows each
  uint64_t kstart;     // the first byte of every kept member: ", " precedes it when a kept member came before
  uint64_t tok_start;  // where a kept token outside strings begins
  uint64_t after;      // the positions behind the closing quote of input's value: they follow the dict
  uint32_t out0;       // output bytes before this block
  uint32_t first;      // 1: no kept member came before this block
  uint32_t dict_len;
};

// d1: the positions at depth 1; mstart: member_starts; drop_start: those of mstart whose key is
// dropped; inp: the positions of input's value, quotes included; inp_close: its closing quote.
// A member runs to before the next ',' at depth 1 or the '}' that closes depth 1; neither the bytes
// of a dropped member nor any ',' at depth 1 are copied.
AVDB_HD Block block(const Raw& r, const Masks& M, uint64_t d1, uint64_t mstart, uint64_t drop_start, uint64_t inp,
                    uint64_t inp_close, uint32_t dict_len, State& st) {
  const uint64_t d1comma = r.comma & M.m.outside & d1;
  const uint64_t run = ~(d1comma | (M.m.close & d1));
  const uint64_t dropped = vep::runs_from(run, drop_start | (uint64_t(st.in_drop) & run & 1));
  st.in_drop = uint32_t(dropped >> 63);
  Block B;
  B.kept = r.valid & ~dropped & ~d1comma & ~inp;
  B.kstart = mstart & ~drop_start;
  B.sep = (r.comma | r.colon) & M.m.outside & B.kept;
  const uint64_t tok = M.m.outside & ~(r.qt | r.comma | r.colon | r.open | r.close) & B.kept;
  B.tok_start = tok & ~((tok << 1) | st.prev_tok);  // (a backslash outside a string is a token byte: no token holds one)
  st.prev_tok = uint32_t(tok >> 63);
  if (M.escaped & M.m.in_str & ~r.okesc & (B.kept | inp)) st.why |= 1u << kKeptText;
  if (r.ctl | (r.hi & B.kept)) st.why |= 1u << kKeptText;
  B.after = inp_close ? ~bits_le(ctz(inp_close)) : 0ull;
  B.out0 = st.out;
  B.first = st.n_kept == 0;
  B.dict_len = dict_len;
  const uint32_t ns = popc(B.kstart);
  st.out += popc(B.kept) + popc(B.sep) + (ns ? 2u * (ns - B.first) : 0u) + (inp_close ? dict_len : 0u);
  st.n_kept += ns;
  return B;
}

// where the byte at bit `lane` goes: its input position minus what is dropped below it, plus the
// spaces and the ", " added below it (its own ", " included), plus the dict when it stands behind it
AVDB_HD uint32_t out_at(const Block& B, uint32_t lane) {
  const uint32_t ns = popc(B.kstart & bits_le(lane));
  return B.out0 + popc(B.kept & bits_lt(lane)) + popc(B.sep & bits_lt(lane)) + (ns ? 2u * (ns - B.first) : 0u) +
         (((B.after >> lane) & 1) ? B.dict_len : 0u);
}

template <class Put>
AVDB_HD void lane_put(const Block& B, uint32_t lane, uint32_t c, Put put) {
  if (!((B.kept >> lane) & 1)) return;
  const uint32_t k = out_at(B, lane);
  if (((B.kstart >> lane) & 1) && popc(B.kstart & bits_le(lane)) > B.first) {
    put(k - 2, uint32_t(','));
    put(k - 1, uint32_t(' '));
  }
  put(k, c);
  if ((B.sep >> lane) & 1) put(k + 1, uint32_t(' '));
}

// what the size pass keeps of a line it walked: the flags byte and the length
AVDB_HD uint8_t flags_of_reason(int32_t r) { return r < 0 ? uint8_t(0) : uint8_t(1 + r); }

// the walk of one line on the host: the masks and the lanes are loops.  [s, e): the line; is, il:
// the span of input's value between its quotes.  kWrite: its bytes through put(k, c).  Returns the
// output length; *dict_at: where the dict goes.
template <bool kWrite, class Put>
inline uint32_t walk_host(const uint8_t* text, uint64_t s, uint64_t e, uint64_t is, uint32_t il, uint32_t dict_len,
                          Put put, uint32_t* dict_at, uint32_t* why) {
  State st{};
  const uint64_t lo = is - 1, hi = is + il;
  *dict_at = 0;
  for (uint64_t b0 = s; b0 < e; b0 += uint64_t(kWave)) {
    uint64_t rb[10] = {0};
    uint64_t inp = 0, inp_close = 0;
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      bool f[9];
      raw_of_byte(text[b0 + lane], f);
      for (int a = 0; a < 9; ++a) rb[a] |= uint64_t(f[a]) << lane;
      rb[9] |= 1ull << lane;
      const uint64_t pos = b0 + lane;
      inp |= uint64_t(pos >= lo && pos <= hi) << lane;
      inp_close |= uint64_t(pos == hi) << lane;
    }
    const Raw r{rb[0], rb[1], rb[2], rb[3], rb[4], rb[5], rb[6], rb[7], rb[8], rb[9]};
    const Masks M = derive(r, st);
    uint64_t d1 = 0;
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane)
      d1 |= uint64_t(vep::depth_at(M.m, st.depth, lane) == 1) << lane;
    st.depth += int32_t(popc(M.m.open)) - int32_t(popc(M.m.close));
    const uint64_t mstart = member_starts(r, M, d1, st);
    uint64_t drop_start = 0;
    for (uint64_t q = mstart; q; q &= q - 1) {
      const uint32_t lane = ctz(q);
      if (dropped_key(text + b0 + lane, e - (b0 + lane))) drop_start |= 1ull << lane;
    }
    const Block B = block(r, M, d1, mstart, drop_start, inp, inp_close, dict_len, st);
    if (b0 <= lo && lo < b0 + uint64_t(kWave) && lo < e) *dict_at = out_at(B, uint32_t(lo - b0));
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      if (kWrite)
        lane_put(B, lane, text[b0 + lane], put);
      else if (((B.tok_start >> lane) & 1) && !vrows::token_at_ok(text + b0 + lane, e - (b0 + lane)))
        st.why |= 1u << kKeptText;
    }
  }
  *why = st.why;
  return st.out;
}

// ---- the entry dict -------------------------------------------------------------------------------
AVDB_HD bool is_letter(uint32_t c) {
  const uint32_t l = lof::lower(c);
  return l >= 'a' && l <= 'z';
}

// json.dumps(to_numeric(text)) of one field or INFO value whose bytes are all qc::plain_byte: K17's
// value_json, in front of it the one form it leaves to Python that needs no Python: letters only.
// float() takes no text of letters but inf, nan and infinity (lof::is_float_word), int() none, so
// such a text stays a string: 'A', 'T', 'Y', 'INT'.
template <class Put>
AVDB_HD uint32_t field_json(const uint8_t* p, uint32_t n, bool info, Put put) {
  bool letters = n > 0;
  for (uint32_t i = 0; i < n && letters; ++i) letters = is_letter(p[i]);
  if (letters && !lof::is_float_word(p, n)) {
    put(0u, uint32_t('"'));
    for (uint32_t i = 0; i < n; ++i) put(1u + i, uint32_t(p[i]));
    put(1u + n, uint32_t('"'));
    return n + 2;
  }
  return qc::value_json(p, n, info, put);
}

struct Dict {
  uint32_t len, why;
};

// json.dumps(VcfEntryParser(input, identityOnly).get_entry()) of the string text[s, s + len32):
// {"chrom": v, "pos": v, "id": v, "ref": v, "alt": v[, "qual": v, "filter": v, "info": {...}]},
// the fields separated by the two bytes \t, every value through to_numeric, INFO by
// parse_entry's rule (qc::line_json's: '#' as ':', a bare item true, '=' split once).  The first
// five fields are K18b's (vrows::parse_input); a line with fewer than eight where eight are wanted
// raises IndexError, fields beyond them are ignored.  put(k, c): byte k.
template <class Put>
AVDB_HD Dict dict_json(const uint8_t* text, uint64_t text_bytes, uint64_t s, int32_t len32, bool identity_only,
                       Put put) {
  const vrows::Input I = vrows::parse_input(text, text_bytes, s, len32);
  if (I.why) return Dict{0, I.why};
  const uint8_t* p = text + s;
  const uint32_t len = uint32_t(len32), want = identity_only ? 5u : 8u;
  uint32_t k = 0, at = 0, nf = 0, why = 0;
  auto lit = [&](const char* t) {
    for (uint32_t i = 0; t[i]; ++i) put(k++, uint32_t(uint8_t(t[i])));
  };
  auto value = [&](uint32_t a, uint32_t b, bool info) {
    const uint32_t n = field_json(p + a, b - a, info, [&](uint32_t j, uint32_t c) { put(k + j, c); });
    if (n == qc::kHost) why |= 1u << kInputValue;
    else k += n;
  };
  while (nf < want && !why) {
    uint32_t j = at;
    while (j < len && p[j] != '\\') {
      if (!qc::plain_byte(p[j])) why |= 1u << kInputValue;
      ++j;
    }
    const bool last = j >= len;
    if (!last && (j + 1 >= len || p[j + 1] != 't')) why |= 1u << kInputValue;
    if (why) break;
    lit(nf == 0   ? "{\"chrom\": "
        : nf == 1 ? ", \"pos\": "
        : nf == 2 ? ", \"id\": "
        : nf == 3 ? ", \"ref\": "
        : nf == 4 ? ", \"alt\": "
        : nf == 5 ? ", \"qual\": "
        : nf == 6 ? ", \"filter\": "
                  : ", \"info\": {");
    if (nf < 7) {
      value(at, j, false);
    } else {
      // INFO: a text to_numeric leaves a string (a number has no .replace: parse_entry raises), no key twice
      bool text_info = j - at == 1 && p[at] == '.';
      for (uint32_t i = at; i < j && !text_info; ++i) text_info = !lof::numberish(p[i]);
      if (!text_info || qc::repeats_key(p, at, j)) {
        why |= 1u << kInputValue;
        break;
      }
      for (uint32_t a = at; a <= j && !why;) {
        uint32_t b, ke;
        qc::item_at(p, a, j, &b, &ke);
        if (a != at) lit(", ");
        put(k++, uint32_t('"'));
        for (uint32_t i = a; i < ke; ++i) put(k++, qc::key_byte(p, i));
        lit("\": ");
        if (ke == b) lit("true");
        else value(ke + 1, b, true);
        a = b + 1;
      }
      put(k++, uint32_t('}'));
    }
    ++nf;
    if (last) break;
    at = j + 2;
  }
  if (!why && nf < want) why |= 1u << (identity_only ? uint32_t(vrows::kInputFields) : uint32_t(kEightFields));
  if (why) return Dict{0, why};
  put(k++, uint32_t('}'));
  return Dict{k, 0};
}

// what dict_len keeps of a line: the dict's length, or kUnsafe | the reason the line is the host's
AVDB_HD uint32_t dict_entry(const In& in, const uint8_t* ent_flags, const uint8_t* text, uint64_t text_bytes,
                            uint64_t li, bool identity_only) {
  const int32_t prior = prior_reason(in, ent_flags, li);
  if (prior >= 0) return kUnsafe | uint32_t(prior);
  const Dict D = dict_json(text, text_bytes, in.input_start[li], in.input_len[li], identity_only,
                           [](uint32_t, uint32_t) {});
  if (D.why) return kUnsafe | ctz(D.why);
  return D.len < kUnsafe ? D.len : kUnsafe | uint32_t(vep::kCap);
}

// ---- an update row with the extra column --------------------------------------------------------
using Cleaned = avdb_vep_output_table;

inline const char* cleaned_error(const Cleaned* c, uint64_t table_rows) {
  if (!c || c->struct_size != sizeof(Cleaned)) return "null avdb_vep_output_table, or one of another size";
  if (c->n_entries >= 0x7FFFFFFFull) return "too many entries";
  if (c->n_entries && (!c->off || !c->len || (c->text_bytes && !c->text))) return "null cleaned-text array";
  if (table_rows && !c->row_entry) return "null row_entry";
  return nullptr;
}

// pk<TAB>chr<label><TAB> | body | <TAB> | cleaned text | <TAB>alg_id[<TAB>true]<LF>
struct RowParts {
  bool ok;  // the parts add up to the row's out_len
  uint32_t head_n, label_n, body_n, clean_n, tail_n, digits;
  uint64_t body_s, clean_s;
};
template <class TextAt>
AVDB_HD RowParts row_parts(const lof::UpdRow& row, const lof::Table& T, const Cleaned& C, uint64_t alg_id,
                           uint32_t flags, TextAt text) {
  RowParts P{};
  if ((row.flags & AVDB_LOFUPD_BAD) || row.row < 0 || uint64_t(row.row) >= T.n_rows) return P;
  const int32_t e = C.row_entry[row.row];
  if (e < 0 || uint64_t(e) >= C.n_entries) return P;
  P.clean_s = C.off[e];
  P.clean_n = C.len[e];
  if (P.clean_s > C.text_bytes || P.clean_n > C.text_bytes - P.clean_s) return P;
  for (uint64_t p = row.start + row.pk_len + 1; P.label_n < row.out_len; ++p, ++P.label_n) {
    const uint32_t c = text(p);
    if (c == ':' || c == '\t' || c == '\n' || c == 0) break;
  }
  P.head_n = row.pk_len + 1 + 3 + P.label_n + 1;
  lof::json_span(T, uint64_t(row.row), &P.body_s, &P.body_n);
  P.digits = vrows::digits_of(alg_id);
  P.tail_n = vrows::tail_len(alg_id, flags) + 1;
  P.ok = uint64_t(P.head_n) + P.body_n + 1 + P.clean_n + P.tail_n == row.out_len;
  return P;
}
template <class TextAt>
AVDB_HD uint32_t head_byte(const lof::UpdRow& row, const RowParts& P, uint32_t j, TextAt text) {
  if (j < row.pk_len) return text(row.start + j);
  j -= row.pk_len;
  if (j < 4) return uint8_t("\tchr"[j]);
  j -= 4;
  return j < P.label_n ? text(row.start + row.pk_len + 1 + j) : uint32_t('\t');
}
AVDB_HD uint32_t tail_byte(const RowParts& P, uint64_t alg_id, uint32_t j) {
  if (j == 0) return uint32_t('\t');
  if (j + 1 == P.tail_n) return uint32_t('\n');
  j -= 1;
  return j < P.digits ? vrows::digit_at(alg_id, P.digits, j) : uint8_t("\ttrue"[j - P.digits]);
}

}  // namespace vout
}  // namespace avdb

// K18b — the update rows of adsp_most_severe_consequence and adsp_ranked_consequences
// (avdb_vep_rows.hip): the code a consequence's rendering, a line's `input` and a table row's body
// are made of, compiled for both sides as avdb_vep.hpp and avdb_tables.hpp are.
//
// An element is read in blocks of 64 bytes, as K18a reads a line: the caller turns a block into
// 64-bit masks (ballots on the device, a loop in the _host entries), elem_block derives from them
// what is the same for the whole block (the string mask, the separators outside strings, where a
// token begins) with one carry each over the block edge, and elem_lane_put is the step of one byte
// position.  What a line and a row are made of (parse_input, next_alt, row_body, line_entry,
// render_keys) is sequential code over K18a's arrays; row_body drives a sink, which counts, writes
// on the host, or writes with a whole wave on the device.
#pragma once

#include "avdb_tables.hpp"
#include "avdb_vep.hpp"

namespace avdb {
namespace vrows {

using tables::EntryRow;
using tables::RowCols;
using vep::bits_lt;
using vep::ctz;
using vep::popc;
using In = avdb_vep_rows_in;

// why a line is left to the host, behind K18a's reasons
enum : uint32_t { kNoInput = vep::kCap + 1, kInputFields, kEscape, kByte, kToken };
static_assert(kToken + 1 == AVDB_VEPROWS_N_REASONS, "reasons");
constexpr uint32_t kUnsafe = 0x80000000u;  // el_rlen: the element is the host's, its reason in the low bits
constexpr uint32_t kMaxToken = AVDB_VEPROWS_MAX_TOKEN;

inline const char* in_error(const In* in, size_t n_lines) {
  if (!in || in->struct_size != sizeof(In)) return "null avdb_vep_rows_in, or one of another size";
  if (in->n_ranks >= 0x7FFFFFFFu) return "too many ranking entries";
  if (in->n_ranks && (!in->rank_off || (in->rank_text_bytes && !in->rank_text))) return "null rank text";
  if (n_lines && (!in->line_flags || !in->n_csq || !in->csq_off || !in->input_start || !in->input_len))
    return "null line array of K18a";
  if (in->n_csq_total && (!in->type || !in->order || !in->el_start || !in->el_len || !in->al_start || !in->al_len ||
                          !in->entry || !in->coding || !in->sorted || !in->el_rlen))
    return "null consequence array of K18a";
  return nullptr;
}

// ---- a token outside strings ------------------------------------------------------------------
AVDB_HD bool is_structural(uint32_t c) {
  return c == '"' || c == ',' || c == ':' || c == '{' || c == '}' || c == '[' || c == ']';
}
AVDB_HD bool is_digit(uint32_t c) { return c >= '0' && c <= '9'; }

// json.dumps(json.loads(token)) is the token: true, false, null, an integer without a leading zero
// (not -0), or -?int.frac of at most 15 significant digits, without a trailing zero unless the
// fraction is exactly 0, of magnitude in [1e-4, 1e16): repr() prints such a double in positional
// notation, and as the shortest digits that round-trip, which these are
template <class CP>
AVDB_HD bool token_ok(CP p, uint32_t n) {
  if (n == 0 || n > kMaxToken) return false;
  if (n == 4 && p[0] == 't' && p[1] == 'r' && p[2] == 'u' && p[3] == 'e') return true;
  if (n == 4 && p[0] == 'n' && p[1] == 'u' && p[2] == 'l' && p[3] == 'l') return true;
  if (n == 5 && p[0] == 'f' && p[1] == 'a' && p[2] == 'l' && p[3] == 's' && p[4] == 'e') return true;
  uint32_t i = p[0] == '-';
  const bool neg = i != 0;
  const uint32_t is = i;
  while (i < n && is_digit(p[i])) ++i;
  const uint32_t id = i - is;
  if (!id || (id > 1 && p[is] == '0')) return false;
  const bool int_zero = p[is] == '0';
  if (i == n) return !(neg && int_zero);
  if (p[i] != '.') return false;
  const uint32_t fs = ++i;
  while (i < n && is_digit(p[i])) ++i;
  const uint32_t fd = i - fs;
  if (i != n || !fd || (fd > 1 && p[n - 1] == '0')) return false;
  if (!int_zero) return id + fd <= 15;
  uint32_t lz = 0;
  while (lz < fd && p[fs + lz] == '0') ++lz;
  return lz < fd && lz <= 3 && fd - lz <= 15;  // (0.0 and -0.0 round-trip too; the rule leaves them out)
}

// the token that begins at p, `avail` bytes before its element's end
AVDB_HD bool token_at_ok(const uint8_t* p, uint64_t avail) {
  uint32_t n = 0;
  while (n < avail && n <= kMaxToken && !is_structural(p[n])) ++n;
  return token_ok(p, n);
}

// ---- an element, 64 bytes a step ----------------------------------------------------------------
struct ElemRaw {  // a block's bytes, a bit each (the element's bytes only)
  uint64_t bs, qt, sep, structural, okesc, bad;
};
AVDB_HD void elem_raw_of_byte(uint8_t c, bool* f) {  // in ElemRaw's order
  f[0] = c == '\\';
  f[1] = c == '"';
  f[2] = c == ',' || c == ':';
  f[3] = is_structural(c);
  f[4] = c == '"' || c == '\\' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't';
  f[5] = c < 0x20 || c >= 0x80;
}

struct ElemState {  // what crosses a block edge
  uint64_t esc, in_str;
  uint32_t prev_tok;  // the last byte was a token's
  uint32_t n_sep;     // separators outside strings so far
  uint32_t why;
};
struct ElemBlock {
  uint64_t sep;        // the ',' and ':' outside strings: a space follows each
  uint64_t tok_start;  // where a token outside strings begins
  uint32_t n0;         // separators before this block
};

// An element begins with '{' outside a string, so st starts from zeros.  valid: the block's bytes
// that are the element's.
AVDB_HD ElemBlock elem_block(const ElemRaw& r, uint64_t valid, ElemState& st) {
  const uint64_t escaped = vep::escaped_of(r.bs, st.esc);
  const uint64_t quotes = r.qt & ~escaped;
  const uint64_t in_str = vep::prefix_xor(quotes) ^ st.in_str;  // (the opening quote and the bytes, not the closing quote)
  st.in_str = (in_str >> 63) ? ~0ull : 0ull;
  const uint64_t outside = ~in_str & valid;
  if (escaped & in_str & ~r.okesc & valid) st.why |= 1u << kEscape;
  if (r.bad) st.why |= 1u << kByte;
  const uint64_t tok = outside & ~r.structural;  // (a backslash outside a string is a token byte: no token holds one)
  ElemBlock B;
  B.tok_start = tok & ~((tok << 1) | st.prev_tok);
  st.prev_tok = uint32_t(tok >> 63);
  B.sep = r.sep & outside;
  B.n0 = st.n_sep;
  st.n_sep += popc(B.sep);
  return B;
}

// byte idx of the element (bit `lane` of its block) goes out behind the spaces of the separators
// before it; the closing brace (idx == last) is the suffix's
template <class Put>
AVDB_HD void elem_lane_put(uint32_t lane, uint32_t idx, uint32_t last, uint32_t c, const ElemBlock& B, Put put) {
  if (idx >= last) return;
  const uint32_t k = idx + B.n0 + popc(B.sep & bits_lt(lane));
  put(k, c);
  if ((B.sep >> lane) & 1) put(k + 1, uint32_t(' '));
}

// the span of consequence r, inside the text
struct ElemRef {
  uint64_t s;
  uint32_t len;
  bool ok;
};
AVDB_HD ElemRef elem_ref(const In& in, uint64_t r, uint64_t text_bytes) {
  const uint64_t s = in.el_start[r];
  const uint32_t len = in.el_len[r];
  return ElemRef{s, len, len >= 2 && s <= text_bytes && len <= text_bytes - s};
}

// , "vep_consequence_order_num": <k>, "rank": <rank text>, "consequence_is_coding": true|false}
struct Suffix {
  const uint8_t* rank;
  uint32_t rank_n, order, digits, coding, len;
};
#define AVDB_VR_SUF_ORDER ", \"vep_consequence_order_num\": "
#define AVDB_VR_SUF_RANK ", \"rank\": "
#define AVDB_VR_SUF_CODING ", \"consequence_is_coding\": "
constexpr uint32_t kSufOrderN = sizeof(AVDB_VR_SUF_ORDER) - 1, kSufRankN = sizeof(AVDB_VR_SUF_RANK) - 1,
                   kSufCodingN = sizeof(AVDB_VR_SUF_CODING) - 1;

AVDB_HD uint32_t digits_of(uint64_t v) {
  uint32_t d = 1;
  while (v >= 10) {
    v /= 10;
    ++d;
  }
  return d;
}
AVDB_HD uint32_t digit_at(uint64_t v, uint32_t digits, uint32_t j) {  // the j-th from the left
  for (uint32_t k = digits - 1; k > j; --k) v /= 10;
  return uint32_t('0' + v % 10);
}

AVDB_HD bool suffix_of(const In& in, uint64_t r, Suffix* S) {
  const int32_t e = in.entry[r], order = in.order[r];
  if (e < 0 || uint32_t(e) >= in.n_ranks || order < 0) return false;
  const uint32_t a = in.rank_off[e], b = in.rank_off[e + 1];
  if (b < a || b > in.rank_text_bytes) return false;
  S->rank = in.rank_text + a;
  S->rank_n = b - a;
  S->order = uint32_t(order);
  S->digits = digits_of(S->order);
  S->coding = in.coding[r] != 0;
  S->len = kSufOrderN + S->digits + kSufRankN + S->rank_n + kSufCodingN + (S->coding ? 4u : 5u) + 1u;
  return true;
}
AVDB_HD uint32_t suffix_at(const Suffix& S, uint32_t j) {  // byte j of S.len
  if (j < kSufOrderN) return uint8_t(AVDB_VR_SUF_ORDER[j]);
  j -= kSufOrderN;
  if (j < S.digits) return digit_at(S.order, S.digits, j);
  j -= S.digits;
  if (j < kSufRankN) return uint8_t(AVDB_VR_SUF_RANK[j]);
  j -= kSufRankN;
  if (j < S.rank_n) return S.rank[j];
  j -= S.rank_n;
  if (j < kSufCodingN) return uint8_t(AVDB_VR_SUF_CODING[j]);
  j -= kSufCodingN;
  return uint8_t((S.coding ? "true}" : "false}")[j]);
}

// what el_rlen keeps of an element the size pass walked
AVDB_HD uint32_t rlen_of(uint32_t len, uint32_t n_sep, uint32_t why, bool has_suffix, const Suffix& S) {
  if (!has_suffix) why |= 1u << vep::kStruct;  // (never: K18a gave the element an entry)
  if (why) return kUnsafe | ctz(why);
  const uint64_t n = uint64_t(len) - 1 + n_sep + S.len;  // (the closing brace is the suffix's)
  return n < kUnsafe ? uint32_t(n) : kUnsafe | uint32_t(vep::kCap);
}

// the walk of one element on the host: the masks and the lanes are loops.  kWrite: its bytes through
// put(k, c), the suffix not included.  Returns the separators outside strings.
template <bool kWrite, class Put>
inline uint32_t elem_walk_host(const uint8_t* text, uint64_t s, uint32_t len, Put put, uint32_t* why) {
  ElemState st{};
  for (uint32_t b0 = 0; b0 < len; b0 += uint32_t(kWave)) {
    uint64_t rb[6] = {0}, valid = 0;
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < len; ++lane) {
      bool f[6];
      elem_raw_of_byte(text[s + b0 + lane], f);
      for (int a = 0; a < 6; ++a) rb[a] |= uint64_t(f[a]) << lane;
      valid |= 1ull << lane;
    }
    const ElemBlock B = elem_block(ElemRaw{rb[0], rb[1], rb[2], rb[3], rb[4], rb[5]}, valid, st);
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < len; ++lane) {
      const uint32_t idx = b0 + lane;
      if (kWrite)
        elem_lane_put(lane, idx, len - 1, text[s + idx], B, put);
      else if (((B.tok_start >> lane) & 1) && !token_at_ok(text + s + idx, len - idx))
        st.why |= 1u << kToken;
    }
  }
  if (st.in_str) st.why |= 1u << vep::kStruct;  // (never: K18a closed the element outside a string)
  *why = st.why;
  return st.n_sep;
}

// ---- a line's `input`: the first five fields of its VCF line -------------------------------------
struct Input {
  uint32_t why;  // 0: inside the device subset
  uint64_t chrom_s, pos_s, ref_s, alt_s;  // in the text
  uint32_t chrom_n, pos_n, ref_n, alt_n, n_alts;
};

// K16's first-five-field subset (lof::parse_line) over the string's bytes, the fields separated by
// the two bytes \t; any other backslash, a byte >= 0x80 or < 0x20 in the five fields is the host's
AVDB_HD Input parse_input(const uint8_t* text, uint64_t text_bytes, uint64_t s, int32_t len32) {
  Input I{};
  I.why = 1u << kInputFields;  // until every check has passed
  if (len32 < 0) {
    I.why = 1u << kNoInput;
    return I;
  }
  const uint32_t len = uint32_t(len32);
  if (s > text_bytes || len > text_bytes - s) return I;
  const uint8_t* p = text + s;
  uint32_t fs[5], fe[5], nf = 0, at = 0, i = 0;
  while (i < len && nf < 5) {
    const uint32_t c = p[i];
    if (c == '\\') {
      if (i + 1 >= len || p[i + 1] != 't') return I;
      fs[nf] = at;
      fe[nf] = i;
      ++nf;
      i += 2;
      at = i;
      continue;
    }
    if (c >= 0x80u || c < 0x20u) return I;
    ++i;
  }
  if (nf == 4) {  // ALT is the last field
    fs[4] = at;
    fe[4] = len;
    nf = 5;
  }
  if (nf < 5) return I;  // values[index] raises IndexError
  // CHROM: an optional 'chr' and one of the 25 labels, or MT
  uint32_t cs = fs[0], cn = fe[0] - fs[0];
  if (cn == 2 && p[cs] == 'M' && p[cs + 1] == 'T') {
    cn = 1;
  } else {
    if (cn > 3 && p[cs] == 'c' && p[cs + 1] == 'h' && p[cs + 2] == 'r') {
      cs += 3;
      cn -= 3;
    }
    if (exist::contig_bit(p + cs, cn) == exist::kOtherBit) return I;
  }
  // POS: plain digits
  uint32_t ps = fs[1];
  const uint32_t pe = fe[1];
  if (ps >= pe || pe - ps > lof::kMaxDigits) return I;
  for (uint32_t k = ps; k < pe; ++k)
    if (!is_digit(p[k])) return I;
  while (ps + 1 < pe && p[ps] == '0') ++ps;
  // ID: '.' or a text to_numeric leaves a string
  bool text_id = false;
  for (uint32_t k = fs[2]; k < fe[2] && !text_id; ++k) text_id = !lof::numberish(p[k]);
  if (!text_id && !(fe[2] - fs[2] == 1 && p[fs[2]] == '.')) return I;
  if (!lof::allele_field_ok(p + fs[3], fe[3] - fs[3]) || !lof::allele_field_ok(p + fs[4], fe[4] - fs[4])) return I;
  I.chrom_s = s + cs;
  I.chrom_n = cn;
  I.pos_s = s + ps;
  I.pos_n = pe - ps;
  I.ref_s = s + fs[3];
  I.ref_n = fe[3] - fs[3];
  I.alt_s = s + fs[4];
  I.alt_n = fe[4] - fs[4];
  I.n_alts = 1;
  for (uint32_t k = fs[4]; k < fe[4]; ++k) I.n_alts += p[k] == ',';
  I.why = 0;
  return I;
}

// an ALT allele and what get_normalized_alleles(snvDivMinus=True) makes of it: the allele behind the
// prefix it shares with REF, '-' when nothing is left; an SNV as it is
struct Alt {
  uint64_t s, norm_s;
  uint32_t n, norm_n;
  bool dash;
};
AVDB_HD Alt next_alt(const uint8_t* text, const Input& I, uint32_t* cursor) {  // *cursor: an offset into the ALT field
  Alt A{};
  A.s = I.alt_s + *cursor;
  while (*cursor + A.n < I.alt_n && text[A.s + A.n] != ',') ++A.n;
  *cursor += A.n + 1;
  uint32_t lcp = 0;
  if (!(I.ref_n == 1 && A.n == 1)) {
    const uint32_t m = I.ref_n < A.n ? I.ref_n : A.n;
    while (lcp < m && text[I.ref_s + lcp] == text[A.s + lcp]) ++lcp;
  }
  A.norm_s = A.s + lcp;
  A.norm_n = A.n - lcp;
  A.dash = lcp > 0 && A.norm_n == 0;
  return A;
}

// consequence r's allele is the normalised ALT, byte for byte
AVDB_HD bool allele_is(const uint8_t* text, uint64_t text_bytes, const In& in, uint64_t r, const Alt& A) {
  const uint64_t s = in.al_start[r];
  const uint32_t n = in.al_len[r];
  if (s > text_bytes || n > text_bytes - s) return false;
  if (A.dash) return n == 1 && text[s] == '-';
  if (n != A.norm_n) return false;
  for (uint32_t i = 0; i < n; ++i)
    if (text[s + i] != text[A.norm_s + i]) return false;
  return true;
}

// a line's consequences: rows [off, off + n) of K18a's arrays; n = 0 where they do not describe it
struct LineCsq {
  uint64_t off;
  uint32_t n;
  bool ok;
};
AVDB_HD LineCsq line_csq(const In& in, uint64_t li) {
  const uint64_t off = in.csq_off[li];
  const uint32_t n = in.n_csq[li];
  const bool ok = off <= in.n_csq_total && n <= in.n_csq_total - off && n <= vep::kMaxCsq;
  return LineCsq{off, ok ? n : 0u, ok};
}
// the consequence at place p of the reference's order, or -1
AVDB_HD int64_t csq_at(const In& in, const LineCsq& C, uint32_t p) {
  const int32_t k = in.sorted[C.off + p];
  return k >= 0 && uint32_t(k) < C.n ? int64_t(C.off + uint32_t(k)) : -1;
}

#define AVDB_VR_KEY0 "\"transcript_consequences\": ["
#define AVDB_VR_KEY1 "\"regulatory_feature_consequences\": ["
#define AVDB_VR_KEY2 "\"motif_feature_consequences\": ["
#define AVDB_VR_KEY3 "\"intergenic_consequences\": ["
AVDB_HD const char* type_key(uint32_t t) {
  return t == 0 ? AVDB_VR_KEY0 : t == 1 ? AVDB_VR_KEY1 : t == 2 ? AVDB_VR_KEY2 : AVDB_VR_KEY3;
}
AVDB_HD uint32_t type_key_len(uint32_t t) {
  return uint32_t(t == 0 ? sizeof(AVDB_VR_KEY0) : t == 1 ? sizeof(AVDB_VR_KEY1) : t == 2 ? sizeof(AVDB_VR_KEY2) : sizeof(AVDB_VR_KEY3)) - 1u;
}

// A row's body, <most severe><TAB><ranked>, through a sink: lit(text, n) and elem(r), the rendered
// consequence r.  The elements of the line whose allele is the normalised ALT, in `sorted` order:
// the first is the most severe (types come in CONSEQUENCE_TYPES order), and per type they are the
// (rank, order number) list of get_allele_consequences.
template <class Sink>
AVDB_HD void row_body(const In& in, const uint8_t* text, uint64_t text_bytes, const LineCsq& C, const Alt& A,
                      Sink& sink) {
  int32_t cur = -1;
  for (uint32_t p = 0; p < C.n; ++p) {
    const int64_t r = csq_at(in, C, p);
    if (r < 0 || !allele_is(text, text_bytes, in, uint64_t(r), A)) continue;
    const int32_t t = in.type[r] & 3;
    if (cur < 0) {
      sink.elem(uint64_t(r));
      sink.lit("\t{", 2);
    }
    if (t != cur) {
      if (cur >= 0) sink.lit("], ", 3);
      sink.lit(type_key(uint32_t(t)), type_key_len(uint32_t(t)));
      cur = t;
    } else {
      sink.lit(", ", 2);
    }
    sink.elem(uint64_t(r));
  }
  if (cur < 0)
    sink.lit("{}\t{}", 5);
  else
    sink.lit("]}", 2);
}

struct SizeSink {
  const In& in;
  uint64_t k;
  AVDB_HD void lit(const char*, uint32_t n) { k += n; }
  AVDB_HD void elem(uint64_t r) { k += in.el_rlen[r] & ~kUnsafe; }
};

// ---- a line as the size pass keeps it ----------------------------------------------------------
struct LineOut {
  uint32_t alts, key_bytes, json_len, flags;
};
AVDB_HD uint32_t host_flags(uint32_t why) {
  uint32_t r = ctz(why);
  if (r >= uint32_t(AVDB_VEPROWS_N_REASONS)) r = vep::kStruct;  // (never: no such reason is given)
  return AVDB_VEPROWS_LINE_HOST | ((r + 1u) << 2);
}
AVDB_HD int32_t reason_of(uint32_t flags) { return int32_t(flags >> 2) - 1; }  // of an entry's flags, or -1

AVDB_HD LineOut line_entry(const In& in, const uint8_t* text, uint64_t text_bytes, uint64_t li) {
  const uint32_t f = in.line_flags[li];
  if (f) return LineOut{0, 0, 0, host_flags(1u << ((f - 1u) & 31u))};
  const LineCsq C = line_csq(in, li);
  if (!C.ok) return LineOut{0, 0, 0, host_flags(1u << vep::kStruct)};  // (never, with K18a's arrays)
  const Input I = parse_input(text, text_bytes, in.input_start[li], in.input_len[li]);
  uint32_t why = I.why;
  for (uint32_t k = 0; k < C.n; ++k) {
    const uint32_t rl = in.el_rlen[C.off + k];
    if (rl & kUnsafe) why |= 1u << (rl & 31u);
  }
  if (why) return LineOut{0, 0, 0, host_flags(why)};
  const uint64_t keys = uint64_t(I.n_alts) * (I.chrom_n + 1 + I.pos_n + 1 + I.ref_n + 1) + (I.alt_n - (I.n_alts - 1));
  uint64_t body = 0;
  uint32_t cursor = 0;
  for (uint32_t a = 0; a < I.n_alts; ++a) {
    const Alt A = next_alt(text, I, &cursor);
    SizeSink sink{in, 0};
    row_body(in, text, text_bytes, C, A, sink);
    body += sink.k;
  }
  if (keys > 0xFFFFFFFFull || body > 0xFFFFFFFFull) return LineOut{0, 0, 0, host_flags(1u << vep::kCap)};
  return LineOut{I.n_alts, uint32_t(keys), uint32_t(body), 0};
}

// the input of entry E, line li, when the entry's columns describe it (a host line: never)
AVDB_HD bool entry_input(const In& in, const uint8_t* text, uint64_t text_bytes, uint64_t li, const EntryRow& E,
                         Input* I, LineCsq* C) {
  if ((E.flags & AVDB_VEPROWS_LINE_HOST) || in.line_flags[li]) return false;
  *C = line_csq(in, li);
  if (!C->ok) return false;
  *I = parse_input(text, text_bytes, in.input_start[li], in.input_len[li]);
  return !I->why && I->n_alts == E.alts;
}

// The keys of entry E (line li), chrom:pos:ref:alt_k back to back through put(k, c), k < E.key_bytes,
// and the columns of its rows.  A host line's span is left blank and its rows all point to the
// span's start, as K16a leaves them; a row's JSON columns are the entry's until its body is written.
template <class Put>
AVDB_HD void render_keys(const In& in, const uint8_t* text, uint64_t text_bytes, uint64_t li, const EntryRow& E,
                         const RowCols& R, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < E.key_bytes) put_any(k, c);
  };
  auto row = [&](uint32_t a, uint32_t off, uint32_t host) {
    const uint64_t r = E.first_row + a;
    if (a >= E.alts || r >= R.n_rows) return;
    R.key_off[r] = E.key_base + (off < E.key_bytes ? off : E.key_bytes);
    R.json_off[r] = E.json_base;
    R.json_len[r] = E.json_len;
    R.line_start[r] = E.start;
    R.flags[r] = uint8_t(host | (a == 0 ? AVDB_VEPROWS_ROW_FIRST : 0u));
  };
  Input I;
  LineCsq C;
  uint32_t k = 0;
  if (entry_input(in, text, text_bytes, li, E, &I, &C)) {
    uint32_t cursor = 0;
    for (uint32_t a = 0; a < I.n_alts; ++a) {
      row(a, k, 0u);
      for (uint32_t i = 0; i < I.chrom_n; ++i) put(k++, text[I.chrom_s + i]);  // (MT: its first byte)
      put(k++, uint32_t(':'));
      for (uint32_t i = 0; i < I.pos_n; ++i) put(k++, text[I.pos_s + i]);
      put(k++, uint32_t(':'));
      for (uint32_t i = 0; i < I.ref_n; ++i) put(k++, text[I.ref_s + i]);
      put(k++, uint32_t(':'));
      const Alt A = next_alt(text, I, &cursor);
      for (uint32_t i = 0; i < A.n; ++i) put(k++, text[A.s + i]);
    }
  } else {
    for (uint32_t a = 0; a < E.alts; ++a) row(a, 0u, AVDB_VEPROWS_LINE_HOST);
  }
  for (; k < E.key_bytes; ++k) put(k, uint32_t(' '));
}

// a row's own span of its entry's body
AVDB_HD void set_row_json(const EntryRow& E, const RowCols& R, uint32_t a, uint64_t at, uint64_t len) {
  const uint64_t r = E.first_row + a;
  if (a >= E.alts || r >= R.n_rows) return;
  const uint64_t s = at < E.json_len ? at : E.json_len;
  R.json_off[r] = E.json_base + s;
  R.json_len[r] = uint32_t(len < E.json_len - s ? len : E.json_len - s);
}

// the bodies of entry E's rows on the host, through put(k, c), k < E.json_len; blank for a host line
struct HostSink {
  const In& in;
  const uint8_t* text;
  uint64_t text_bytes;
  uint64_t k;  // from the entry's base
  uint64_t limit;
  uint8_t* out;  // the entry's span
  void put(uint64_t at, uint32_t c) {
    if (at < limit) out[at] = uint8_t(c);
  }
  void lit(const char* s, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) put(k + i, uint8_t(s[i]));
    k += n;
  }
  void elem(uint64_t r) {
    const uint32_t rl = in.el_rlen[r];
    const ElemRef e = elem_ref(in, r, text_bytes);
    Suffix S;
    if ((rl & kUnsafe) || !e.ok || !suffix_of(in, r, &S)) return;  // (never, for a line the size pass kept)
    uint32_t why;
    const uint64_t base = k;
    const uint32_t n_sep =
        elem_walk_host<true>(text, e.s, e.len, [&](uint32_t j, uint32_t c) { put(base + j, c); }, &why);
    const uint64_t at = base + e.len - 1 + n_sep;
    for (uint32_t j = 0; j < S.len; ++j) put(at + j, suffix_at(S, j));
    k += rl;
  }
};

inline void render_body_host(const In& in, const uint8_t* text, uint64_t text_bytes, uint64_t li, const EntryRow& E,
                             const RowCols& R, uint8_t* out) {
  Input I;
  LineCsq C;
  HostSink sink{in, text, text_bytes, 0, E.json_len, out};
  if (entry_input(in, text, text_bytes, li, E, &I, &C)) {
    uint32_t cursor = 0;
    for (uint32_t a = 0; a < I.n_alts; ++a) {
      const Alt A = next_alt(text, I, &cursor);
      const uint64_t at = sink.k;
      row_body(in, text, text_bytes, C, A, sink);
      set_row_json(E, R, a, at, sink.k - at);
    }
  }
  for (uint64_t k = sink.k; k < E.json_len; ++k) out[k] = uint8_t(' ');
}

// ---- the export join -----------------------------------------------------------------------------
// what follows the body in a row: <TAB>alg_id[<TAB>true]
AVDB_HD uint32_t tail_len(uint64_t alg_id, uint32_t flags) {
  return 1u + digits_of(alg_id) + ((flags & AVDB_VEPUPD_ADSP) ? 5u : 0u);
}

// K16b's line (lof::scan_export_line: the third column is vep_output) with the longer row
template <class CP>
AVDB_HD lof::UpdLine scan_export_line(CP line, uint64_t len, bool nl, uint32_t contig_mask, bool update_existing,
                                      const lof::Table& T, uint32_t tail) {
  lof::UpdLine L = lof::scan_export_line(line, len, nl, contig_mask, update_existing, T);
  if (L.is_row && !(L.flags & AVDB_LOFUPD_BAD)) {
    const uint64_t out = uint64_t(L.out_len) + tail;
    if (out > 0xFFFFFFFFull) {
      L.flags = AVDB_LOFUPD_BAD;
      L.out_len = 0;
    } else {
      L.out_len = uint32_t(out);
    }
  }
  return L;
}

// one row's text: pk<TAB>chr<label of the metaseq id><TAB>body<TAB>alg_id[<TAB>true]<LF>
template <class TextAt, class Put>
AVDB_HD void render_update_row(const lof::UpdRow& row, const lof::Table& T, uint64_t alg_id, uint32_t flags,
                               TextAt text, Put put_any) {
  auto put = [&](uint32_t k, uint32_t c) {
    if (k < row.out_len) put_any(k, c);
  };
  uint32_t k = 0;
  if (!(row.flags & AVDB_LOFUPD_BAD) && row.row >= 0 && uint64_t(row.row) < T.n_rows) {
    for (uint32_t i = 0; i < row.pk_len; ++i) put(k++, text(row.start + i));
    put(k++, uint32_t('\t'));
    put(k++, uint32_t('c'));
    put(k++, uint32_t('h'));
    put(k++, uint32_t('r'));
    for (uint64_t p = row.start + row.pk_len + 1; k < row.out_len; ++p) {
      const uint32_t c = text(p);
      if (c == ':' || c == '\t' || c == '\n' || c == 0) break;
      put(k++, c);
    }
    put(k++, uint32_t('\t'));
    uint64_t js;
    uint32_t jn;
    lof::json_span(T, uint64_t(row.row), &js, &jn);
    for (uint32_t j = 0; j < jn; ++j) put(k++, uint32_t(T.json[js + j]));
    put(k++, uint32_t('\t'));
    const uint32_t d = digits_of(alg_id);
    for (uint32_t j = 0; j < d; ++j) put(k++, digit_at(alg_id, d, j));
    if (flags & AVDB_VEPUPD_ADSP) {
      const char t[] = "\ttrue";
      for (uint32_t j = 0; j < 5; ++j) put(k++, uint32_t(uint8_t(t[j])));
    }
    put(k++, uint32_t('\n'));
  }
  for (; k < row.out_len; ++k) put(k, uint32_t(' '));
}

}  // namespace vrows
}  // namespace avdb

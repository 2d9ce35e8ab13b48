// K18d — the allele_frequencies column of the VEP update rows (avdb_vep_freq.hip): the code a line's
// chosen `frequencies` object, a row's regrouped text and an update row with the column are made of,
// compiled for both sides as avdb_vep.hpp, avdb_vep_rows.hpp and avdb_vep_output.hpp are.
//
// Two walks read text in blocks of 64 bytes with the masks of avdb_vep.hpp (escaped_of, the
// prefix-xor string mask, depth_at, one carry each over the block edge); the caller turns a block
// into 64-bit masks (ballots on the device, loops in the _host entries):
//   find  a line: the top-level colocated_variants member (K18a's read-back rule: a key's quote at
//         depth 1 behind '{' or ','), its elements (depth 3) and their keys allele_string, id and
//         frequencies, classified by the lane they begin in; the events of a block then run in text
//         order over running state that is the same for the whole wave (Find), which applies
//         VepJsonParser.get_frequencies' selection.
//   row   the chosen object: its allele keys (depth 1) compared with the row's normalised ALT, the
//         matched object's member keys (depth 2) handed out one per lane (select_bit); a lane then
//         reads its member (member_at), and the regrouped text is laid out from three group sums.
// `input` is read by one lane per line (input_info): the ID field or INFO RS to match, INFO FREQ.
#pragma once

#include "avdb_vep_output.hpp"

namespace avdb {
namespace vfreq {

using vep::bits_le;
using vep::bits_lt;
using vep::ctz;
using vep::popc;
using In = avdb_vep_rows_in;

// why a line is left to the host, behind K18b's reasons
enum : uint32_t {
  kColoc = vrows::kToken + 1,  // colocated_variants is no array, is empty, or holds what is no object
  kElemKey,     // allele_string or id: missing where the reference reads it, or no string
  kDupKey,      // a key of interest twice
  kBytes,       // a backslash or a byte outside printable ASCII inside colocated_variants
  kNotObject,   // frequencies, or the allele's value, is no object
  kValue,       // a member's value outside the token rule
  kMembers,     // more than AVDB_VEPFREQ_MAX_MEMBERS members
  kGmaf,        // a member named gmaf in a group FREQ names too
  kInfo,        // fewer than eight fields, INFO outside the subset, an RS that is not plain digits
  kFreqItem,    // a FREQ freq_plain refuses, a bare FREQ, '#' in it
  kFreqNumber,  // a FREQ number outside json_number's forms, or too few comma items
  kSameAllele   // two ALTs with one normalised allele: the reference merges in place
};
static_assert(kSameAllele + 1 == AVDB_VEPFREQ_N_REASONS, "reasons");
constexpr uint32_t kMaxMembers = AVDB_VEPFREQ_MAX_MEMBERS;
static_assert(kMaxMembers == uint32_t(kWave), "a member a lane");
constexpr uint32_t kMaxPops = 64;      // avdb_k5.hpp's kMaxPops
constexpr uint32_t kIdRs = 1u << 30;   // id_len: the id is "rs" and the span's digits
constexpr uint32_t kBad = 0x80000000u; // a row's length: the line is the host's, its reason in the low bits

inline const char* in_error(const In* in, size_t n_lines) { return vout::in_error(in, n_lines); }

// ---- a token: K18b's rule, and the exponent form -------------------------------------------------
// D[.F]e-XX as repr() prints a double below 1e-4: D in 1..9, F without a trailing zero, at most 15
// significant digits, XX of two digits, or three without a leading zero, its value in 5..300
template <class CP>
AVDB_HD bool exp_token_ok(CP p, uint32_t n) {
  if (n < 5 || n > vrows::kMaxToken || p[0] < '1' || p[0] > '9') return false;
  uint32_t i = 1, sig = 1;
  if (p[i] == '.') {
    const uint32_t fs = ++i;
    while (i < n && vrows::is_digit(p[i])) ++i;
    if (i == fs || p[i - 1] == '0') return false;
    sig += i - fs;
  }
  if (sig > 15 || i + 2 > n || p[i] != 'e' || p[i + 1] != '-') return false;
  i += 2;
  const uint32_t xs = i;
  uint32_t x = 0;
  while (i < n && vrows::is_digit(p[i])) x = x * 10u + (p[i++] - '0');
  const uint32_t xd = i - xs;
  if (i != n || xd < 2 || xd > 3 || (xd == 3 && p[xs] == '0')) return false;
  return x >= 5 && x <= 300;
}
template <class CP>
AVDB_HD bool token_ok(CP p, uint32_t n) {
  return vrows::token_ok(p, n) || exp_token_ok(p, n);
}

// ---- `input`: what is matched against, and INFO FREQ -------------------------------------------
struct InputInfo {
  uint32_t why;
  uint64_t id_s, fq_s;  // in the text
  uint32_t id_n, fq_n;
  bool has_id, id_rs, has_fq;
};

// FREQ's value p[v0, v1): freq_plain's rules (avdb_k5.hpp) byte by byte, and no '#' (parse_entry
// writes it as ':' before the value is split)
AVDB_HD bool freq_items_ok(const uint8_t* p, uint32_t v0, uint32_t v1) {
  uint32_t np = 0;
  for (uint32_t p0 = v0; p0 <= v1; ++np) {
    uint32_t p1 = p0, c1 = v1 + 1;
    for (; p1 < v1 && p[p1] != '|'; ++p1) {
      if (p[p1] == '#') return false;
      if (p[p1] == ':' && c1 > v1) c1 = p1;
    }
    if (c1 > v1 || np >= kMaxPops) return false;  // pop.split(':')[1] raises
    for (uint32_t i = p0; i < c1; ++i)
      if (!qc::plain_byte(p[i])) return false;
    for (uint32_t q0 = v0; q0 < p0;) {  // a name twice: the dict keeps the last value at the first place
      uint32_t d1 = q0;
      while (p[d1] != ':') ++d1;
      bool same = d1 - q0 == c1 - p0;
      for (uint32_t i = 0; same && i < c1 - p0; ++i) same = p[q0 + i] == p[p0 + i];
      if (same) return false;
      while (q0 < p0 && p[q0] != '|') ++q0;
      ++q0;
    }
    p0 = p1 + 1;
  }
  return true;
}

// The string text[s, s + len32) K18b read its five fields from (parse_input passed): the ID field
// when it holds "rs", else "rs" + INFO RS (get_refsnp, vcf_parser.py:158-169), and the last FREQ
// item of INFO.  identity_only: the entry has no INFO.  match: an id is wanted.
AVDB_HD InputInfo input_info(const uint8_t* text, uint64_t text_bytes, uint64_t s, int32_t len32, bool identity_only,
                             bool match) {
  InputInfo R{};
  if (len32 < 0 || s > text_bytes || uint32_t(len32) > text_bytes - s) {
    R.why = 1u << kInfo;  // (never: K18b read it)
    return R;
  }
  const uint8_t* p = text + s;
  const uint32_t len = uint32_t(len32), want = identity_only ? 3u : 8u;
  uint32_t nf = 0, at = 0, id0 = 0, id1 = 0, in0 = 0, in1 = 0;
  while (nf < want) {
    uint32_t j = at;
    while (j < len && p[j] != '\\') {
      if (p[j] < 0x20u) R.why |= 1u << kInfo;
      ++j;
    }
    const bool last = j >= len;
    if (!last && (j + 1 >= len || p[j + 1] != 't')) R.why |= 1u << kInfo;
    if (R.why) return R;
    if (nf == 2) id0 = at, id1 = j;
    if (nf == 7) in0 = at, in1 = j;
    ++nf;
    if (last) break;
    at = j + 2;
  }
  if (nf < want) {  // IndexError
    R.why = 1u << kInfo;
    return R;
  }
  bool id_has_rs = false;
  for (uint32_t i = id0; i + 1 < id1 && !id_has_rs; ++i) id_has_rs = p[i] == 'r' && p[i + 1] == 's';
  if (match && id_has_rs) {
    R.has_id = true;
    R.id_s = s + id0;
    R.id_n = id1 - id0;
  }
  if (identity_only) return R;
  // INFO: a text to_numeric leaves a string (a number has no .replace: parse_entry raises)
  bool text_info = in1 - in0 == 1 && p[in0] == '.';
  for (uint32_t i = in0; i < in1 && !text_info; ++i) text_info = !lof::numberish(p[i]);
  if (!text_info) {
    R.why = 1u << kInfo;
    return R;
  }
  bool has_rs = false, rs_bare = false;
  uint32_t rs0 = 0, rs1 = 0, fq0 = 0, fq1 = 0;
  for (uint32_t a = in0; a <= in1;) {  // the dict keeps an item's last value
    uint32_t b = a;
    while (b < in1 && p[b] != ';') ++b;
    const uint32_t n = b - a;
    if (n >= 4 && p[a] == 'F' && p[a + 1] == 'R' && p[a + 2] == 'E' && p[a + 3] == 'Q') {
      if (n == 4) R.why |= 1u << kFreqItem;  // True.split: AttributeError
      else if (p[a + 4] == '=') R.has_fq = true, fq0 = a + 5, fq1 = b;
    }
    if (n >= 2 && p[a] == 'R' && p[a + 1] == 'S') {
      if (n == 2) has_rs = rs_bare = true;
      else if (p[a + 2] == '=') has_rs = true, rs_bare = false, rs0 = a + 3, rs1 = b;
    }
    a = b + 1;
  }
  if (R.has_fq && !freq_items_ok(p, fq0, fq1)) R.why |= 1u << kFreqItem;
  R.fq_s = s + fq0;
  R.fq_n = fq1 - fq0;
  if (match && !id_has_rs && has_rs) {  // 'rs' + str(to_numeric(RS)): the digits themselves when they are plain
    bool plain = !rs_bare && rs1 > rs0 && rs1 - rs0 <= 18 && !(rs1 - rs0 > 1 && p[rs0] == '0');
    for (uint32_t i = rs0; i < rs1 && plain; ++i) plain = vrows::is_digit(p[i]);
    if (!plain) R.why |= 1u << kInfo;
    R.has_id = R.id_rs = true;
    R.id_s = s + rs0;
    R.id_n = rs1 - rs0;
  }
  return R;
}

// what the input pass keeps of a line: 0, or 1 + the reason it is the host's
struct LineIn {
  uint8_t flags;
  uint64_t id_s, fq_s;
  uint32_t id_len, fq_n;  // id_len: 0xFFFFFFFF none; kIdRs: "rs" + the span
};
AVDB_HD LineIn line_input(const In& in, const uint8_t* ent_flags, const uint8_t* text, uint64_t text_bytes, uint64_t li,
                          uint32_t n_alts, bool identity_only, bool match) {
  LineIn L{0, 0, 0, 0xFFFFFFFFu, 0};
  const int32_t prior = vout::prior_reason(in, ent_flags, li);
  if (prior >= 0) {
    L.flags = vout::flags_of_reason(prior);
    return L;
  }
  const vrows::Input I = vrows::parse_input(text, text_bytes, in.input_start[li], in.input_len[li]);
  uint32_t why = I.why;
  if (!why && I.n_alts != n_alts) why = 1u << vep::kStruct;  // (never: the entry is K18b's)
  if (!why) {
    const InputInfo R = input_info(text, text_bytes, in.input_start[li], in.input_len[li], identity_only, match);
    why = R.why;
    if (R.has_id) L.id_s = R.id_s, L.id_len = R.id_n | (R.id_rs ? kIdRs : 0u);
    if (R.has_fq) L.fq_s = R.fq_s, L.fq_n = R.fq_n;
    // two ALTs with one normalised allele share frequencies[normAlt], which __add_vcf_frequencies changes
    uint32_t ca = 0;
    for (uint32_t a = 0; a < I.n_alts && !why; ++a) {
      const vrows::Alt A = vrows::next_alt(text, I, &ca);
      uint32_t cb = 0;
      for (uint32_t b = 0; b < a; ++b) {
        const vrows::Alt B = vrows::next_alt(text, I, &cb);
        bool same = A.dash == B.dash && A.norm_n == B.norm_n;
        for (uint32_t i = 0; same && i < A.norm_n; ++i) same = text[A.norm_s + i] == text[B.norm_s + i];
        if (same) why |= 1u << kSameAllele;
      }
    }
  }
  if (why) L = LineIn{uint8_t(1 + ctz(why)), 0, 0, 0xFFFFFFFFu, 0};
  return L;
}

// ---- a block's bytes and what both walks derive from them ---------------------------------------
struct Raw {  // a bit each (the span's bytes only)
  uint64_t bs, qt, lbrace, lbrack, close, comma, colon, bad, valid;
};
AVDB_HD void raw_of_byte(uint8_t c, bool* f) {  // in Raw's order, without valid
  f[0] = c == '\\';
  f[1] = c == '"';
  f[2] = c == '{';
  f[3] = c == '[';
  f[4] = c == '}' || c == ']';
  f[5] = c == ',';
  f[6] = c == ':';
  f[7] = c < 0x20 || c >= 0x7F;
}

struct Carry {  // what crosses a block edge in either walk
  uint64_t esc, in_str;
  int32_t depth;
  uint32_t prev_oc;  // the last byte was a bracket that opens or a ',', outside a string
};
struct Masks {
  vep::Masks m;
  uint64_t behind;  // the positions behind a bracket that opens or a ',' outside a string
  uint64_t comma;   // the ',' outside strings
};
AVDB_HD Masks derive(const Raw& r, Carry& st) {
  Masks M;
  const uint64_t escaped = vep::escaped_of(r.bs, st.esc);
  M.m.quotes = r.qt & ~escaped;
  M.m.in_str = vep::prefix_xor(M.m.quotes) ^ st.in_str;
  st.in_str = (M.m.in_str >> 63) ? ~0ull : 0ull;
  M.m.sopen = M.m.quotes & M.m.in_str;
  M.m.outside = ~M.m.in_str;
  M.m.open = (r.lbrace | r.lbrack) & M.m.outside;
  M.m.close = r.close & M.m.outside;
  M.comma = r.comma & M.m.outside;
  const uint64_t oc = M.m.open | M.comma;
  M.behind = (oc << 1) | st.prev_oc;
  st.prev_oc = uint32_t(oc >> 63);
  return M;
}
// after the lanes took their depths from st.depth
AVDB_HD void step_depth(const Masks& M, Carry& st) { st.depth += int32_t(popc(M.m.open)) - int32_t(popc(M.m.close)); }

// ---- find: the element VepJsonParser.get_frequencies takes (vep_parser.py:178-216) ---------------
struct Find {
  Carry c;
  uint32_t in_cv;    // the next block begins inside the colocated_variants member
  uint32_t n_cv;     // such members
  uint32_t n_elems;  // elements of its array
  // the element being read
  uint32_t e_as, e_id, e_fr;  // its keys allele_string, id, frequencies
  uint32_t e_cosmic, e_match, fr_open, e_has;
  uint64_t e_fs;
  uint32_t e_fn;
  // cv[0]'s object (an array of one), and the last element that qualifies (a longer array)
  uint64_t one_fs, sel_fs;
  uint32_t one_fn, sel_fn, one_has, sel_has;
  uint32_t multi_err;  // what the loop over a longer array raises
  uint32_t why;
};

// the key that opens at p, `avail` bytes before the line's end
enum : uint32_t { kKeyNone = 0, kKeyAs, kKeyId, kKeyFr };
struct KeyHit {
  uint32_t kind;
  bool ok;  // its value is what the device takes: a string, an object
  bool x;   // allele_string: it is COSMIC_MUTATION; id: it is the wanted id
};
AVDB_HD KeyHit key3_at(const uint8_t* p, uint64_t avail, const uint8_t* text, const LineIn& L) {
  KeyHit H{kKeyNone, false, false};
  if (avail < 2) return H;
  if (p[1] == 'a' && vout::key_is(p, avail, "\"allele_string\":")) {
    H.kind = kKeyAs;
    H.ok = avail > 16 && p[16] == '"';
    H.x = H.ok && vout::key_is(p + 16, avail - 16, "\"COSMIC_MUTATION\"");
  } else if (p[1] == 'i' && vout::key_is(p, avail, "\"id\":")) {
    H.kind = kKeyId;
    H.ok = avail > 5 && p[5] == '"';
    if (H.ok && L.id_len != 0xFFFFFFFFu) {
      const uint32_t n = L.id_len & ~kIdRs, pre = (L.id_len & kIdRs) ? 2u : 0u;
      const uint8_t* q = p + 6;
      bool same = avail - 6 > uint64_t(pre) + n && q[pre + n] == '"' && (!pre || (q[0] == 'r' && q[1] == 's'));
      for (uint32_t i = 0; same && i < n; ++i) same = q[pre + i] == text[L.id_s + i];
      H.x = same;
    }
  } else if (p[1] == 'f' && vout::key_is(p, avail, "\"frequencies\":")) {
    H.kind = kKeyFr;
    H.ok = avail > 14 && p[14] == '{';
  }
  return H;
}

struct FindMasks {  // a block of the line
  uint64_t key1;  // the top-level keys
  uint64_t in_cv, key3, elem_open, elem_close, fr_close;
};
// d1 .. d4: the positions at those depths.  Before the lanes look at key1.
AVDB_HD uint64_t find_key1(const Masks& M, uint64_t d1) { return M.m.sopen & d1 & M.behind; }
// cvk: the positions of key1 whose key is colocated_variants; cva: those an array follows
AVDB_HD FindMasks find_masks(const Raw& r, const Masks& M, uint64_t d1, uint64_t d2, uint64_t d3, uint64_t d4,
                             uint64_t cvk, uint64_t cva, Find& st) {
  FindMasks F;
  F.key1 = 0;
  const uint64_t run = ~((M.comma | M.m.close) & d1);  // a member runs to before the next ',' at depth 1 or the '}'
  F.in_cv = vep::runs_from(run, cvk | (uint64_t(st.in_cv) & run & 1)) & r.valid;
  st.in_cv = uint32_t(F.in_cv >> 63);
  st.n_cv += popc(cvk);
  if (cvk & ~cva) st.why |= 1u << kColoc;
  if ((r.bs | r.bad) & F.in_cv) st.why |= 1u << kBytes;
  // the array holds objects only: at depth 2 its own brackets and commas, at depth 3 no '['
  const uint64_t ok2 = (M.m.open & r.lbrack) | M.m.close | M.comma;
  if (F.in_cv & d2 & (M.m.in_str | ~ok2)) st.why |= 1u << kColoc;
  if (F.in_cv & d3 & M.m.open & r.lbrack) st.why |= 1u << kColoc;
  F.elem_open = M.m.open & r.lbrace & d3 & F.in_cv;
  F.elem_close = M.m.close & d3 & F.in_cv;
  F.fr_close = M.m.close & d4 & F.in_cv;
  F.key3 = M.m.sopen & d3 & M.behind & F.in_cv;
  return F;
}

// the block's events in text order.  k_as, k_id, k_fr: the positions of key3 by key; k_ok, k_x: KeyHit's.
// b0: the block's first byte in the text.
AVDB_HD void find_events(const FindMasks& F, uint64_t k_as, uint64_t k_id, uint64_t k_fr, uint64_t k_ok, uint64_t k_x,
                         bool want_id, uint64_t b0, Find& st) {
  for (uint64_t ev = F.elem_open | k_as | k_id | k_fr | F.fr_close | F.elem_close; ev; ev &= ev - 1) {
    const uint32_t e = ctz(ev);
    const uint64_t bit = 1ull << e;
    if (F.elem_open & bit) {
      st.e_as = st.e_id = st.e_fr = st.e_cosmic = st.e_match = st.fr_open = st.e_has = 0;
    } else if (k_as & bit) {
      ++st.e_as;
      if (!(k_ok & bit)) st.why |= 1u << kElemKey;
      st.e_cosmic = (k_x & bit) != 0;
    } else if (k_id & bit) {
      ++st.e_id;
      if (want_id && !(k_ok & bit)) st.why |= 1u << kElemKey;
      st.e_match = (k_x & bit) != 0;
    } else if (k_fr & bit) {
      ++st.e_fr;
      if (!(k_ok & bit)) st.why |= 1u << kNotObject;
      st.fr_open = 1;
      st.e_fs = b0 + e + 14;  // its '{'
    } else if (F.fr_close & bit) {
      if (st.fr_open) {  // the first bracket that closes depth 4 behind the key is the object's own
        st.fr_open = 0;
        st.e_has = 1;
        st.e_fn = uint32_t(b0 + e + 1 - st.e_fs);
      }
    } else {  // the element ends
      if (st.e_as > 1 || st.e_id > 1 || st.e_fr > 1) st.why |= 1u << kDupKey;
      if (st.n_elems == 0) st.one_has = st.e_has, st.one_fs = st.e_fs, st.one_fn = st.e_fn;
      bool take = false;
      if (!st.e_as) st.multi_err = 1;  // covar['allele_string']: KeyError
      else if (!st.e_cosmic && st.e_fr) {
        if (want_id && !st.e_id) st.multi_err = 1;  // covar['id']: KeyError
        take = !want_id || st.e_match;
      }
      if (take) st.sel_has = st.e_has, st.sel_fs = st.e_fs, st.sel_fn = st.e_fn;
      ++st.n_elems;
    }
  }
}

struct Chosen {
  uint32_t why;
  uint64_t fs;
  uint32_t fn;  // 0: none
};
AVDB_HD Chosen find_end(const Find& st) {
  Chosen C{st.why, 0, 0};
  if (st.c.depth != 0 || st.c.in_str) C.why |= 1u << vep::kStruct;  // (never: K18a read the line)
  if (st.n_cv > 1) C.why |= 1u << kDupKey;
  if (st.n_cv == 1) {
    if (st.n_elems == 0) C.why |= 1u << kColoc;  // cv[0]: IndexError
    else if (st.n_elems == 1) {
      if (st.one_has) C.fs = st.one_fs, C.fn = st.one_fn;
    } else {
      if (st.multi_err) C.why |= 1u << kElemKey;
      if (st.sel_has) C.fs = st.sel_fs, C.fn = st.sel_fn;
    }
  }
  if (C.why) C.fs = 0, C.fn = 0;
  return C;
}

// the walk of one line on the host: the masks and the lanes are loops
inline Chosen find_host(const uint8_t* text, uint64_t s, uint64_t e, const LineIn& L) {
  Find st{};
  const bool want_id = L.id_len != 0xFFFFFFFFu;
  for (uint64_t b0 = s; b0 < e; b0 += uint64_t(kWave)) {
    if (st.why) return Chosen{st.why, 0, 0};  // the first block that gives a reason ends the walk
    uint64_t rb[9] = {0};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      bool f[8];
      raw_of_byte(text[b0 + lane], f);
      for (int a = 0; a < 8; ++a) rb[a] |= uint64_t(f[a]) << lane;
      rb[8] |= 1ull << lane;
    }
    const Raw r{rb[0], rb[1], rb[2], rb[3], rb[4], rb[5], rb[6], rb[7], rb[8]};
    const Masks M = derive(r, st.c);
    uint64_t d[5] = {0};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      const int32_t dep = vep::depth_at(M.m, st.c.depth, lane);
      if (dep >= 1 && dep <= 4) d[dep] |= 1ull << lane;
    }
    step_depth(M, st.c);
    uint64_t cvk = 0, cva = 0;
    for (uint64_t q = find_key1(M, d[1]); q; q &= q - 1) {
      const uint32_t lane = ctz(q);
      const uint8_t* p = text + b0 + lane;
      const uint64_t avail = e - (b0 + lane);
      if (vout::key_is(p, avail, "\"colocated_variants\":")) {
        cvk |= 1ull << lane;
        if (avail > 21 && p[21] == '[') cva |= 1ull << lane;
      }
    }
    const FindMasks F = find_masks(r, M, d[1], d[2], d[3], d[4], cvk, cva, st);
    uint64_t k_as = 0, k_id = 0, k_fr = 0, k_ok = 0, k_x = 0;
    for (uint64_t q = F.key3; q; q &= q - 1) {
      const uint32_t lane = ctz(q);
      const KeyHit H = key3_at(text + b0 + lane, e - (b0 + lane), text, L);
      const uint64_t bit = 1ull << lane;
      if (H.kind == kKeyAs) k_as |= bit;
      if (H.kind == kKeyId) k_id |= bit;
      if (H.kind == kKeyFr) k_fr |= bit;
      if (H.ok) k_ok |= bit;
      if (H.x) k_x |= bit;
    }
    find_events(F, k_as, k_id, k_fr, k_ok, k_x, want_id, b0, st);
  }
  return st.why ? Chosen{st.why, 0, 0} : find_end(st);
}

// ---- row: the allele's object inside the chosen one ---------------------------------------------
struct RowWalk {
  Carry c;
  uint32_t in_obj;    // the next block begins inside the matched allele's member
  uint32_t n_match;   // allele keys equal to the normalised ALT
  uint32_t n_mem;     // the matched object's members so far
  uint32_t why;
};

// the allele key that opens at p is the normalised ALT; *obj: an object follows it
AVDB_HD bool allele_key_is(const uint8_t* p, uint64_t avail, const uint8_t* text, const vrows::Alt& A, bool* obj) {
  const uint32_t n = A.dash ? 1u : A.norm_n;
  if (avail < uint64_t(n) + 3 || p[n + 1] != '"' || p[n + 2] != ':') return false;
  if (A.dash) {
    if (p[1] != '-') return false;
  } else {
    for (uint32_t i = 0; i < n; ++i)
      if (p[1 + i] != text[A.norm_s + i]) return false;
  }
  *obj = avail > uint64_t(n) + 3 && p[n + 3] == '{';
  return true;
}

struct RowMasks {
  uint64_t akey;  // the allele keys
  uint64_t mkey;  // the member keys of the matched allele's object
  uint32_t n0;    // its members before this block
};
AVDB_HD uint64_t row_akey(const Masks& M, uint64_t d1) { return M.m.sopen & d1 & M.behind; }
// am: the positions of akey whose key is the ALT; aobj: those an object follows
AVDB_HD RowMasks row_masks(const Raw& r, const Masks& M, uint64_t d1, uint64_t d2, uint64_t d3, uint64_t am,
                           uint64_t aobj, RowWalk& st) {
  RowMasks R;
  R.akey = 0;
  // every allele's value is an object (frequencies[allele].items() raises for any other): at depth 1 keys, ':',
  // ',' and the object's own braces only, at depth 2 no '['
  const uint64_t ok1 = r.lbrace | r.close | r.comma | r.colon | r.qt;
  if ((M.m.sopen & d1 & ~M.behind) | (M.m.outside & d1 & ~ok1 & r.valid) | (M.m.open & r.lbrack & d2))
    st.why |= 1u << kNotObject;
  const uint64_t run = ~(M.m.close & d2);  // from the key to before the '}' that closes its object
  const uint64_t obj = vep::runs_from(run, am | (uint64_t(st.in_obj) & run & 1)) & r.valid;
  st.in_obj = uint32_t(obj >> 63);
  st.n_match += popc(am);
  if (am & ~aobj) st.why |= 1u << kNotObject;
  if (obj & d3 & M.m.open) st.why |= 1u << kValue;  // a member that is an object or an array
  if ((r.bs | r.bad) & r.valid) st.why |= 1u << kBytes;  // (never: the find walk read these bytes)
  R.mkey = M.m.sopen & d2 & M.behind & obj;
  R.n0 = st.n_mem;
  st.n_mem += popc(R.mkey);
  return R;
}

// the position of the k-th set bit of m (k < popc(m))
AVDB_HD uint32_t select_bit(uint64_t m, uint32_t k) {
  uint32_t at = 0;
#pragma unroll
  for (uint32_t w = 32; w; w >>= 1) {
    const uint32_t c = popc(m & ((1ull << w) - 1));
    if (k >= c) {
      k -= c;
      m >>= w;
      at += w;
    }
  }
  return at;
}
// the key lane `lane` takes from this block, or ~0
AVDB_HD uint64_t lane_member(const RowMasks& R, uint32_t lane, uint64_t b0) {
  const uint32_t n = popc(R.mkey);
  if (lane < R.n0 || lane >= R.n0 + n) return ~0ull;
  return b0 + select_bit(R.mkey, lane - R.n0);
}

enum : uint32_t { kGnomad = 0, kGenomes, kEsp, kNoGroup };
struct Mem {
  uint64_t ks;  // its key's first byte; its value begins at ks + kn + 2
  uint64_t k8;  // the key's first eight bytes
  uint32_t kn, vn, grp, why;
  bool gmaf;
};
// the member whose key opens at pos, inside [.., end)
AVDB_HD Mem member_at(const uint8_t* text, uint64_t pos, uint64_t end) {
  Mem m{pos + 1, 0, 0, 0, kGenomes, 0, false};
  while (m.ks + m.kn < end && text[m.ks + m.kn] != '"') ++m.kn;
  const uint64_t vs = m.ks + m.kn + 2;
  if (vs >= end || text[vs - 1] != ':') {
    m.why = 1u << kValue;  // (never: a key is followed by ':')
    m.kn = 0;
    return m;
  }
  const uint8_t* k = text + m.ks;
  const uint8_t* v = text + vs;
  while (vs + m.vn < end && m.vn <= vrows::kMaxToken && !vrows::is_structural(v[m.vn])) ++m.vn;
  const uint32_t c = vs + m.vn < end ? v[m.vn] : 0u;
  if ((c != ',' && c != '}') || !token_ok(v, m.vn)) m.why = 1u << kValue;
  for (uint32_t i = 0; i < m.kn && i < 8; ++i) m.k8 |= uint64_t(k[i]) << (8 * i);
  bool gnomad = false;
  for (uint32_t i = 0; i + 6 <= m.kn && !gnomad; ++i)
    gnomad = k[i] == 'g' && k[i + 1] == 'n' && k[i + 2] == 'o' && k[i + 3] == 'm' && k[i + 4] == 'a' && k[i + 5] == 'd';
  if (gnomad) m.grp = kGnomad;
  else if (m.kn == 2 && (k[0] == 'a' || k[0] == 'e') && k[1] == 'a') m.grp = kEsp;
  m.gmaf = m.kn == 4 && k[0] == 'g' && k[1] == 'm' && k[2] == 'a' && k[3] == 'f';
  return m;
}
AVDB_HD uint32_t mem_len(const Mem& m) { return m.kn + 4 + m.vn; }  // "key": value
// a's key is b's
AVDB_HD bool same_key(const uint8_t* text, const Mem& a, uint64_t b_ks, uint32_t b_kn, uint64_t b_k8) {
  if (a.kn != b_kn || a.k8 != b_k8) return false;
  for (uint32_t i = 8; i < a.kn; ++i)
    if (text[a.ks + i] != text[b_ks + i]) return false;
  return true;
}

#define AVDB_VF_HDR0 "\"GnomAD\": {"
#define AVDB_VF_HDR1 "\"1000Genomes\": {"
#define AVDB_VF_HDR2 "\"ESP\": {"
#define AVDB_VF_GMAF "\"gmaf\": "
constexpr uint32_t kGmafN = sizeof(AVDB_VF_GMAF) - 1;
AVDB_HD const char* hdr_of(uint32_t g) { return g == 0 ? AVDB_VF_HDR0 : g == 1 ? AVDB_VF_HDR1 : AVDB_VF_HDR2; }
AVDB_HD uint32_t hdr_len(uint32_t g) {
  return uint32_t(g == 0 ? sizeof(AVDB_VF_HDR0) : g == 1 ? sizeof(AVDB_VF_HDR1) : sizeof(AVDB_VF_HDR2)) - 1u;
}

// the FREQ part of ALT number k (from 1): per VEP group a "gmaf" that goes inside it, and the
// populations that follow the groups, in FREQ order (VcfEntryParser.get_frequencies and the
// recursive deep_update)
struct FreqPart {
  uint32_t why;
  uint32_t gm0, gm1, gm2;  // the length of the number that goes into the group, 0: none
  uint32_t tail;           // the bytes behind the groups, every ", " included
};
AVDB_HD uint32_t group_of_name(const uint8_t* p, uint32_t n) {
  auto is = [&](const char* t, uint32_t tn) {
    if (n != tn) return false;
    for (uint32_t i = 0; i < n; ++i)
      if (p[i] != uint8_t(t[i])) return false;
    return true;
  };
  return is("GnomAD", 6) ? kGnomad : is("1000Genomes", 11) ? kGenomes : is("ESP", 3) ? kEsp : kNoGroup;
}
// json.dumps(to_numeric(text)) of a FREQ number, json_number's forms (avdb_fmt.hpp): digits, or
// digits with one '.', of at most 15 significant digits; qc::kHost otherwise
template <class Put>
AVDB_HD uint32_t freq_number(const uint8_t* p, uint32_t n, Put put) {
  if (!number_plain(p, n)) return qc::kHost;
  bool digits = true;
  for (uint32_t i = 0; i < n; ++i) digits = digits && p[i] != '.';
  if (!digits) return qc::float_json(p, n, false, put);
  uint32_t d = 0, k = 0;
  while (d + 1 < n && p[d] == '0') ++d;
  for (; d < n; ++d) put(k++, uint32_t(p[d]));
  return k;
}
// present: bit g when the VEP part has group g; parts: the groups it has.  put_gm(g, j, c): byte j of
// the number of group g; put_tail(j, c): byte j behind the groups.
template <class PutGm, class PutTail>
AVDB_HD FreqPart freq_part(const uint8_t* text, uint64_t fq_s, uint32_t fq_n, uint32_t k, uint32_t present,
                           PutGm put_gm, PutTail put_tail) {
  FreqPart F{};
  if (!fq_n) return F;
  const uint8_t* p = text + fq_s;
  uint32_t parts = popc(uint64_t(present));
  auto lit = [&](const char* t) {
    for (uint32_t i = 0; t[i]; ++i) put_tail(F.tail++, uint32_t(uint8_t(t[i])));
  };
  for (uint32_t p0 = 0; p0 <= fq_n;) {
    uint32_t p1 = p0;
    while (p1 < fq_n && p[p1] != '|') ++p1;
    uint32_t c1 = p0;
    while (p[c1] != ':') ++c1;  // (freq_items_ok found one)
    uint32_t c2 = c1 + 1;
    while (c2 < p1 && p[c2] != ':') ++c2;  // pop.split(':')[1]
    uint32_t f0 = c1 + 1;
    for (uint32_t idx = 0; idx < k; ++idx) {
      while (f0 < c2 && p[f0] != ',') ++f0;
      if (f0 >= c2) {  // IndexError
        F.why |= 1u << kFreqNumber;
        return F;
      }
      ++f0;
    }
    uint32_t f1 = f0;
    while (f1 < c2 && p[f1] != ',') ++f1;
    const uint32_t fn = f1 - f0;
    if (!(fn == 1 && (p[f0] == '.' || p[f0] == '0'))) {
      const uint32_t g = group_of_name(p + p0, c1 - p0);
      uint32_t n;
      if (g != kNoGroup && ((present >> g) & 1)) {
        // (a branch per group: with g a constant in each, put_gm's choice of the group's place folds away)
        if (g == 0) F.gm0 = n = freq_number(p + f0, fn, [&](uint32_t j, uint32_t c) { put_gm(0u, j, c); });
        else if (g == 1) F.gm1 = n = freq_number(p + f0, fn, [&](uint32_t j, uint32_t c) { put_gm(1u, j, c); });
        else F.gm2 = n = freq_number(p + f0, fn, [&](uint32_t j, uint32_t c) { put_gm(2u, j, c); });
      } else {
        if (parts++) lit(", ");
        put_tail(F.tail++, uint32_t('"'));
        for (uint32_t i = p0; i < c1; ++i) put_tail(F.tail++, uint32_t(p[i]));
        lit("\": {" AVDB_VF_GMAF);
        const uint32_t at = F.tail;
        n = freq_number(p + f0, fn, [&](uint32_t j, uint32_t c) { put_tail(at + j, c); });
        if (n != qc::kHost) F.tail += n;
        put_tail(F.tail++, uint32_t('}'));
      }
      if (n == qc::kHost || n == 0) {
        F.why |= 1u << kFreqNumber;
        return F;
      }
    }
    p0 = p1 + 1;
  }
  return F;
}

// a row's text: where the groups, the numbers that go into them and the tail stand
struct Layout {
  uint32_t cnt0, cnt1, cnt2;  // members by group
  uint32_t len0, len1, len2;  // their bytes, without what separates them
  FreqPart F;
  uint32_t at0, at1, at2;  // where each group's header begins
  uint32_t tail_at, total;
};
AVDB_HD uint32_t group_body(uint32_t cnt, uint32_t len, uint32_t gm) {  // between the braces of a group
  return len + 2u * (cnt - 1u) + (gm ? 2u + kGmafN + gm : 0u);
}
AVDB_HD void lay_out(Layout& Y) {
  uint32_t off = 1, parts = 0;
  Y.at0 = Y.at1 = Y.at2 = 0;
  if (Y.cnt0) {
    Y.at0 = off;
    off += hdr_len(0) + group_body(Y.cnt0, Y.len0, Y.F.gm0) + 1;
    ++parts;
  }
  if (Y.cnt1) {
    if (parts++) off += 2;
    Y.at1 = off;
    off += hdr_len(1) + group_body(Y.cnt1, Y.len1, Y.F.gm1) + 1;
  }
  if (Y.cnt2) {
    if (parts++) off += 2;
    Y.at2 = off;
    off += hdr_len(2) + group_body(Y.cnt2, Y.len2, Y.F.gm2) + 1;
  }
  Y.tail_at = off;
  Y.total = off + Y.F.tail + 1;
}
AVDB_HD uint32_t present_of(const Layout& Y) { return (Y.cnt0 ? 1u : 0u) | (Y.cnt1 ? 2u : 0u) | (Y.cnt2 ? 4u : 0u); }

// a member's bytes (group grp, key text[ks, ks + kn), value of vn bytes behind "\":"): rank members of its group
// and `before` of their bytes stand before it
template <class Put>
AVDB_HD void put_member(const uint8_t* text, const Layout& Y, uint32_t grp, uint64_t ks, uint32_t kn, uint32_t vn,
                        uint32_t rank, uint32_t before, Put put) {
  const uint32_t at = grp == 0 ? Y.at0 : grp == 1 ? Y.at1 : Y.at2;
  uint32_t k = at + hdr_len(grp) + before + 2u * rank;
  if (rank) {
    put(k - 2, uint32_t(','));
    put(k - 1, uint32_t(' '));
  }
  put(k++, uint32_t('"'));
  for (uint32_t i = 0; i < kn; ++i) put(k++, uint32_t(text[ks + i]));
  put(k++, uint32_t('"'));
  put(k++, uint32_t(':'));
  put(k++, uint32_t(' '));
  for (uint32_t i = 0; i < vn; ++i) put(k++, uint32_t(text[ks + kn + 2 + i]));
}
// everything that is no member: the braces, the headers, what separates the groups, the FREQ part
template <class Put>
AVDB_HD void put_frame(const uint8_t* text, const Layout& Y, uint64_t fq_s, uint32_t fq_n, uint32_t alt_k, Put put) {
  put(0u, uint32_t('{'));
  auto group = [=](uint32_t g, uint32_t cnt, uint32_t len, uint32_t gm, uint32_t at, bool sep) {
    if (!cnt) return;
    if (sep) {
      put(at - 2, uint32_t(','));
      put(at - 1, uint32_t(' '));
    }
    const char* h = hdr_of(g);
    const uint32_t hn = hdr_len(g);
    for (uint32_t i = 0; i < hn; ++i) put(at + i, uint32_t(uint8_t(h[i])));
    uint32_t k = at + hn + len + 2u * (cnt - 1u);
    if (gm) {
      put(k++, uint32_t(','));
      put(k++, uint32_t(' '));
      for (uint32_t i = 0; i < kGmafN; ++i) put(k++, uint32_t(uint8_t(AVDB_VF_GMAF[i])));
      k += gm;
    }
    put(k, uint32_t('}'));
  };
  group(0, Y.cnt0, Y.len0, Y.F.gm0, Y.at0, false);
  group(1, Y.cnt1, Y.len1, Y.F.gm1, Y.at1, Y.cnt0 != 0);
  group(2, Y.cnt2, Y.len2, Y.F.gm2, Y.at2, (Y.cnt0 | Y.cnt1) != 0);
  if (fq_n) {
    const uint32_t g0 = Y.at0 + hdr_len(0) + Y.len0 + 2u * (Y.cnt0 - 1u) + 2u + kGmafN;
    const uint32_t g1 = Y.at1 + hdr_len(1) + Y.len1 + 2u * (Y.cnt1 - 1u) + 2u + kGmafN;
    const uint32_t g2 = Y.at2 + hdr_len(2) + Y.len2 + 2u * (Y.cnt2 - 1u) + 2u + kGmafN;
    const uint32_t tail_at = Y.tail_at;  // (by value: a layout whose address escapes lives in scratch memory)
    freq_part(text, fq_s, fq_n, alt_k, present_of(Y),
              [=](uint32_t g, uint32_t j, uint32_t c) { put((g == 0 ? g0 : g == 1 ? g1 : g2) + j, c); },
              [=](uint32_t j, uint32_t c) { put(tail_at + j, c); });
  }
  put(Y.total - 1, uint32_t('}'));
}

// the reasons the laid-out row adds: a gmaf of VEP's own where FREQ brings one
AVDB_HD uint32_t gmaf_clash(const Layout& Y, uint32_t gmaf_groups) {
  const uint32_t named = (Y.F.gm0 ? 1u : 0u) | (Y.F.gm1 ? 2u : 0u) | (Y.F.gm2 ? 4u : 0u);
  return (named & gmaf_groups) ? 1u << kGmaf : 0u;
}

// One row on the host: the walk of the chosen object [fs, fs + fn) (fn = 0: none) for ALT A, number
// alt_k from 1; the masks and the lanes are loops.  kWrite: its bytes through put(k, c).  Returns the
// length, or kBad | the reason.
template <bool kWrite, class Put>
inline uint32_t row_host(const uint8_t* text, uint64_t fs, uint32_t fn, const vrows::Alt& A, uint32_t alt_k,
                         uint64_t fq_s, uint32_t fq_n, Put put) {
  RowWalk st{};
  uint64_t key_at[kMaxMembers];
  for (uint32_t i = 0; i < kMaxMembers; ++i) key_at[i] = ~0ull;
  const uint64_t e = fs + fn;
  for (uint64_t b0 = fs; b0 < e; b0 += uint64_t(kWave)) {
    uint64_t rb[9] = {0};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      bool f[8];
      raw_of_byte(text[b0 + lane], f);
      for (int a = 0; a < 8; ++a) rb[a] |= uint64_t(f[a]) << lane;
      rb[8] |= 1ull << lane;
    }
    const Raw r{rb[0], rb[1], rb[2], rb[3], rb[4], rb[5], rb[6], rb[7], rb[8]};
    const Masks M = derive(r, st.c);
    uint64_t d[4] = {0};
    for (uint32_t lane = 0; lane < uint32_t(kWave) && b0 + lane < e; ++lane) {
      const int32_t dep = vep::depth_at(M.m, st.c.depth, lane);
      if (dep >= 1 && dep <= 3) d[dep] |= 1ull << lane;
    }
    step_depth(M, st.c);
    uint64_t am = 0, aobj = 0;
    for (uint64_t q = row_akey(M, d[1]); q; q &= q - 1) {
      const uint32_t lane = ctz(q);
      bool obj = false;
      if (allele_key_is(text + b0 + lane, e - (b0 + lane), text, A, &obj)) {
        am |= 1ull << lane;
        if (obj) aobj |= 1ull << lane;
      }
    }
    const RowMasks R = row_masks(r, M, d[1], d[2], d[3], am, aobj, st);
    for (uint32_t lane = 0; lane < kMaxMembers; ++lane) {
      const uint64_t at = lane_member(R, lane, b0);
      if (at != ~0ull) key_at[lane] = at;
    }
  }
  uint32_t why = st.why;
  if (st.n_match > 1) why |= 1u << kDupKey;
  if (st.n_mem > kMaxMembers) why |= 1u << kMembers;
  if (why) return kBad | ctz(why);
  Mem mem[kMaxMembers];
  Layout Y{};
  uint32_t gmaf_groups = 0;
  for (uint32_t i = 0; i < st.n_mem; ++i) {
    mem[i] = member_at(text, key_at[i], e);
    why |= mem[i].why;
    for (uint32_t j = 0; j < i; ++j)
      if (same_key(text, mem[i], mem[j].ks, mem[j].kn, mem[j].k8)) why |= 1u << kDupKey;
    if (mem[i].gmaf) gmaf_groups |= 1u << mem[i].grp;
    (mem[i].grp == 0 ? Y.cnt0 : mem[i].grp == 1 ? Y.cnt1 : Y.cnt2) += 1;
    (mem[i].grp == 0 ? Y.len0 : mem[i].grp == 1 ? Y.len1 : Y.len2) += mem_len(mem[i]);
  }
  if (why) return kBad | ctz(why);
  Y.F = freq_part(text, fq_s, fq_n, alt_k, present_of(Y), [](uint32_t, uint32_t, uint32_t) {}, [](uint32_t, uint32_t) {});
  why |= Y.F.why;
  why |= gmaf_clash(Y, gmaf_groups);
  if (why) return kBad | ctz(why);
  lay_out(Y);
  if (kWrite) {
    uint32_t rank[3] = {0, 0, 0}, before[3] = {0, 0, 0};
    for (uint32_t i = 0; i < st.n_mem; ++i) {
      put_member(text, Y, mem[i].grp, mem[i].ks, mem[i].kn, mem[i].vn, rank[mem[i].grp], before[mem[i].grp], put);
      ++rank[mem[i].grp];
      before[mem[i].grp] += mem_len(mem[i]);
    }
    put_frame(text, Y, fq_s, fq_n, alt_k, put);
  }
  return Y.total;
}

// ---- an update row with the column ---------------------------------------------------------------
using Freq = avdb_vep_freq_table;

inline const char* freq_error(const Freq* f, uint64_t table_rows) {
  if (!f || f->struct_size != sizeof(Freq)) return "null avdb_vep_freq_table, or one of another size";
  if (f->n_rows != table_rows) return "the frequency texts are not the table's rows'";
  if (f->n_rows && (!f->off || !f->len || (f->text_bytes && !f->text))) return "null frequency-text array";
  return nullptr;
}

// pk<TAB>chr<label><TAB> | frequencies | <TAB> | body | [<TAB> | cleaned text] | <TAB>alg_id[<TAB>true]<LF>
struct RowParts {
  vout::RowParts P;  // ok, head_n, label_n, body_n, body_s, clean_n, clean_s, tail_n, digits
  uint64_t fq_s;
  uint32_t fq_n;
  bool has_clean;
};
template <class TextAt>
AVDB_HD RowParts row_parts(const lof::UpdRow& row, const lof::Table& T, const Freq& Q, const vout::Cleaned* C,
                           uint64_t alg_id, uint32_t flags, TextAt text) {
  RowParts X{};
  vout::RowParts& P = X.P;
  X.has_clean = C != nullptr;
  if ((row.flags & AVDB_LOFUPD_BAD) || row.row < 0 || uint64_t(row.row) >= T.n_rows || uint64_t(row.row) >= Q.n_rows)
    return X;
  X.fq_s = Q.off[row.row];
  X.fq_n = Q.len[row.row];
  if (X.fq_s > Q.text_bytes || X.fq_n > Q.text_bytes - X.fq_s) return X;
  if (C) {
    const int32_t e = C->row_entry[row.row];
    if (e < 0 || uint64_t(e) >= C->n_entries) return X;
    P.clean_s = C->off[e];
    P.clean_n = C->len[e];
    if (P.clean_s > C->text_bytes || P.clean_n > C->text_bytes - P.clean_s) return X;
  }
  for (uint64_t p = row.start + row.pk_len + 1; P.label_n < row.out_len; ++p, ++P.label_n) {
    const uint32_t c = text(p);
    if (c == ':' || c == '\t' || c == '\n' || c == 0) break;
  }
  P.head_n = row.pk_len + 1 + 3 + P.label_n + 1;
  lof::json_span(T, uint64_t(row.row), &P.body_s, &P.body_n);
  P.digits = vrows::digits_of(alg_id);
  P.tail_n = vrows::tail_len(alg_id, flags) + 1;
  P.ok = uint64_t(P.head_n) + X.fq_n + 1 + P.body_n + (C ? 1ull + P.clean_n : 0ull) + P.tail_n == row.out_len;
  return X;
}

}  // namespace vfreq
}  // namespace avdb

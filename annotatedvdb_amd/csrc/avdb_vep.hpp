// K18a — the consequences of VEP's JSON lines, ranked and sorted (avdb_vep.hip): the code one
// line's pass is made of, compiled for both sides as avdb_rows.hpp and avdb_tables.hpp are.
//
// A line is read in blocks of 64 bytes.  The caller turns a block into 64-bit masks, one bit per
// byte (ballots on the device, a loop in the _host entries); everything that follows is this
// file's: word arithmetic on the masks that is the same for the whole block (derive, regions),
// and a step per byte position (depth_at, lane_kind, elem_init, lane_events), which the device
// runs in the position's lane and the host in a loop over the 64 positions.  The state that
// crosses a block edge is State; a line's consequences are collected in Elem[AVDB_VEP_MAX_CSQ]
// (LDS on the device) and ranked, grouped and placed from there (check_elem, leader_of, place).
#pragma once

#include "avdb_lines.hpp"

namespace avdb {
namespace vep {

constexpr uint32_t kMaxCsq = AVDB_VEP_MAX_CSQ;
constexpr int kMaxDepth = AVDB_VEP_MAX_DEPTH;
constexpr uint64_t kEven = 0x5555555555555555ull;
constexpr uint32_t kOrderMask = (1u << 30) - 1;
static_assert(kMaxCsq <= 1024, "a sort key holds a consequence's index in 10 bits");

// why a line is left to the host: bit numbers, in the order AVDB_VEP_COUNT_REASON0 counts them
enum : uint32_t { kWs = 0, kStruct, kDepth, kDupKey, kElem, kBytes, kRepeat, kEmpty, kTerm, kCombo, kCap };
static_assert(kCap + 1 == AVDB_VEP_N_REASONS, "reasons");

// what a position is to the pass (lane_kind)
enum : uint32_t { kNone = 0, kArr0 = 1, kTermsArr = 5, kAllele = 6, kInput = 7, kId = 8, kKey0 = 9, kTermStr = 13 };

struct Elem {
  uint64_t mask;       // the term ids; the sort key once the rows are written
  uint64_t al8;        // the allele's first 8 bytes (until check_elem: whether a term string was seen)
  uint32_t start, end;  // '{' and '}', from the line's start
  uint32_t al_start, al_len;
  uint32_t seen;        // variant_allele strings (low half) and consequence_terms arrays (high half)
  uint32_t type_order;  // type << 30 | order number
};

struct TableView {
  const uint64_t* term_words;  // every term zero-padded to whole words
  const uint32_t* term_off;    // in words
  const uint32_t* term_len;
  uint32_t n_terms;
  const uint64_t* slot_mask;
  const int32_t* slot_entry;
  uint32_t n_slots;
  const uint32_t* rank_order;
  uint32_t n_entries;
  uint64_t coding_mask;
};

inline TableView view_of(const avdb_vep_table* t) {
  return TableView{t->term_words, t->term_off, t->term_len, t->n_terms, t->slot_mask, t->slot_entry,
                   t->n_slots,    t->rank_order, t->n_entries, t->coding_mask};
}

inline const char* table_error(const avdb_vep_table* t) {
  if (!t || t->struct_size != sizeof(avdb_vep_table)) return "null table, or one of another size";
  if (t->n_terms > 64) return "more than 64 terms";
  if (t->n_terms && (!t->term_words || !t->term_off || !t->term_len)) return "null term arrays";
  if (!t->n_slots || (t->n_slots & (t->n_slots - 1)) || !t->slot_mask || !t->slot_entry) return "slots: a power of two";
  if (t->n_entries && !t->rank_order) return "null rank order";
  return nullptr;
}

AVDB_HD uint32_t slot_of(uint64_t mask, uint32_t n_slots) {
  return uint32_t((mask * 0x9E3779B97F4A7C15ull) >> 32) & (n_slots - 1);
}

// the ranking entry whose terms are exactly `mask`, or -1
AVDB_HD int32_t entry_of(const TableView& t, uint64_t mask) {
  uint32_t s = slot_of(mask, t.n_slots);
  for (uint32_t k = 0; k < t.n_slots; ++k, s = (s + 1) & (t.n_slots - 1)) {
    const int32_t e = t.slot_entry[s];
    if (e < 0) return -1;
    if (t.slot_mask[s] == mask) return uint32_t(e) < t.n_entries ? e : -1;
  }
  return -1;
}

// a word of a string has a backslash or a byte >= 0x80
AVDB_HD bool word_not_plain(uint64_t w) {
  const uint64_t x = w ^ 0x5C5C5C5C5C5C5C5Cull;
  return ((w | ((x - 0x0101010101010101ull) & ~x)) & 0x8080808080808080ull) != 0;
}
AVDB_HD bool span_not_plain(const Heap& h, uint64_t at, uint32_t len) {
  for (uint32_t k = 0; k < len; k += 8)
    if (word_not_plain(heap_u64(h, at + k) & low_bytes_mask(len - k))) return true;
  return false;
}

// the id of the term text[at, at + len), or -1
AVDB_HD int32_t term_id(const Heap& h, uint64_t at, uint32_t len, const TableView& t) {
  const uint64_t w0 = heap_u64(h, at) & low_bytes_mask(len);
  for (uint32_t id = 0; id < t.n_terms; ++id) {
    if (t.term_len[id] != len) continue;
    const uint64_t* tw = t.term_words + t.term_off[id];
    if (len && tw[0] != w0) continue;
    bool same = true;
    for (uint32_t k = 8; k < len && same; k += 8) same = (heap_u64(h, at + k) & low_bytes_mask(len - k)) == tw[k / 8];
    if (same) return int32_t(id);
  }
  return -1;
}

// text[pos - n, pos) is the literal, and the byte before it opens an object or follows a member
template <int N>
AVDB_HD bool lit_before(const Heap& h, uint64_t line_s, uint64_t pos, const char (&lit)[N]) {
  constexpr uint32_t n = N - 1;
  if (pos < line_s + n + 1) return false;
  const uint64_t at = pos - n;
#pragma unroll
  for (uint32_t k = 0; k < n; k += 8) {
    uint64_t lw = 0;
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b)
      if (k + b < n) lw |= uint64_t(uint8_t(lit[k + b])) << (8 * b);
    if ((heap_u64(h, at + k) & low_bytes_mask(n - k)) != lw) return false;
  }
  const uint8_t pc = uint8_t(heap_u64(h, at - 1));
  return pc == '{' || pc == ',';
}

AVDB_HD uint64_t prefix_xor(uint64_t x) {
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x ^= x << 16;
  x ^= x << 32;
  return x;
}
AVDB_HD uint64_t bits_lt(uint32_t p) { return (1ull << p) - 1; }                   // p in 0..63
AVDB_HD uint64_t bits_le(uint32_t p) { return p >= 63 ? ~0ull : (2ull << p) - 1; }
AVDB_HD uint64_t bits_range(uint32_t a, uint32_t b) { return bits_le(b) & ~bits_lt(a); }  // a <= b
AVDB_HD uint32_t popc(uint64_t x) { return uint32_t(__builtin_popcountll(x)); }
AVDB_HD uint32_t ctz(uint64_t x) { return uint32_t(__builtin_ctzll(x)); }
// the runs of ones of `runs` that begin at a bit of `heads` (a run that came in over the block's
// lower edge begins at bit 0): adding a head ripples through its run and no further
AVDB_HD uint64_t runs_from(uint64_t runs, uint64_t heads) { return ((runs + heads) ^ runs) & runs; }

struct Raw {  // a block's bytes, a bit each
  uint64_t bs, qt, lbrace, lbrack, rbrace, rbrack, comma, colon, ws, hi, valid;
};
AVDB_HD void raw_of_byte(uint8_t c, bool* f) {  // in Raw's order, without valid
  f[0] = c == '\\';
  f[1] = c == '"';
  f[2] = c == '{';
  f[3] = c == '[';
  f[4] = c == '}';
  f[5] = c == ']';
  f[6] = c == ',';
  f[7] = c == ':';
  f[8] = c == ' ' || c == '\t' || c == '\r' || c == '\n';
  f[9] = c >= 0x80;
}

struct Masks {
  uint64_t in_str;   // inside a string: its opening quote and its bytes, not its closing quote
  uint64_t quotes;   // the quotes no backslash escapes
  uint64_t sopen;    // the opening ones
  uint64_t outside;  // ~in_str
  uint64_t open, close;  // brackets and braces outside strings
};
struct Depths {  // positions by depth_at
  uint64_t d1, d2, d3, d4, bad;
};
struct Kinds {
  uint64_t arr[4], terms_arr, allele, input, id, key[4];
};
struct Regions {
  uint64_t csq[4];                 // inside the array of a <type>_consequences key, brackets included
  uint64_t elem_open, elem_close;  // its elements' braces
  uint64_t terms;                  // inside a consequence_terms array, from its '[' to before its ']'
  uint64_t term_open;              // the opening quotes of its strings
  uint32_t n0;                     // elements before this block
  int32_t pend_close;              // the position that closes the string the last block left open, or -1
  uint32_t pend_kind, pend_start, pend_len, pend_eidx;
};

struct State {
  uint64_t esc;     // bit 0: the next block's first byte is escaped
  uint64_t in_str;  // all ones: the next block begins inside a string
  int32_t depth;
  int32_t cur_type;  // the consequence array the next block begins in, or -1
  uint32_t prev_oc;  // the last byte was a '{' or a ',' outside a string
  uint32_t in_key, seg4, in_terms;
  uint32_t n_elems;
  uint32_t base[4];  // elements before the array of each type
  uint32_t n_arrays[4], n_keys[4], n_input, n_id;
  uint32_t pend_kind, pend_start, pend_eidx;
  uint64_t input_start, id_start;  // from the line's start
  int32_t input_len, id_len;       // -1: none
  uint32_t reasons;
};

AVDB_HD void init_state(State& st) {
  st = State{};
  st.cur_type = -1;
  st.input_len = st.id_len = -1;
}

// the bytes a backslash escapes: those behind a run of backslashes of odd length.  esc carries over
// the block edge (bit 0: the next block's first byte is escaped)
AVDB_HD uint64_t escaped_of(uint64_t bs, uint64_t& esc) {
  const uint64_t b = bs & ~esc;  // (an escaped backslash escapes nothing)
  const uint64_t starts = b & ~(b << 1);
  const uint64_t even_runs = (b + (starts & kEven)) ^ b;  // the runs that start on an even bit, and the bit past each
  const uint64_t follows = b << 1;
  const uint64_t escaped = (follows & even_runs & ~kEven) | (follows & ~even_runs & kEven) | esc;
  esc = (b >> 63) & ~(even_runs >> 63) & 1;  // a run to the edge that started on an odd bit: 64 - start is odd
  return escaped;
}

// the quotes that count, the string mask and the brackets outside strings; carries st over the edge
AVDB_HD Masks derive(const Raw& r, State& st) {
  const uint64_t escaped = escaped_of(r.bs, st.esc);
  Masks m;
  m.quotes = r.qt & ~escaped;
  m.in_str = prefix_xor(m.quotes) ^ st.in_str;
  st.in_str = (m.in_str >> 63) ? ~0ull : 0ull;
  m.sopen = m.quotes & m.in_str;
  m.outside = ~m.in_str;
  m.open = (r.lbrace | r.lbrack) & m.outside;
  m.close = (r.rbrace | r.rbrack) & m.outside;
  return m;
}

// the depth a position is at: an opening bracket counts from itself, a closing one until itself
AVDB_HD int32_t depth_at(const Masks& m, int32_t depth0, uint32_t lane) {
  return depth0 + int32_t(popc(m.open & bits_le(lane))) - int32_t(popc(m.close & bits_lt(lane)));
}

// what the byte at `pos` (bit `lane` of its block) is, read back from the bytes before it
AVDB_HD uint32_t lane_kind(const Heap& h, uint64_t line_s, uint64_t pos, uint32_t lane, const Raw& r, const Masks& m,
                           const Depths& d) {
  const uint64_t bit = 1ull << lane;
  if (m.open & r.lbrack & bit) {
    if (d.d2 & bit) {
      if (lit_before(h, line_s, pos, "\"transcript_consequences\":")) return kArr0;
      if (lit_before(h, line_s, pos, "\"regulatory_feature_consequences\":")) return kArr0 + 1;
      if (lit_before(h, line_s, pos, "\"motif_feature_consequences\":")) return kArr0 + 2;
      if (lit_before(h, line_s, pos, "\"intergenic_consequences\":")) return kArr0 + 3;
    } else if (d.d4 & bit) {
      if (lit_before(h, line_s, pos, "\"consequence_terms\":")) return kTermsArr;
    }
  } else if (m.sopen & bit) {
    if (d.d3 & bit) {
      if (lit_before(h, line_s, pos, "\"variant_allele\":")) return kAllele;
    } else if (d.d1 & bit) {
      if (lit_before(h, line_s, pos, "\"input\":")) return kInput;
      if (lit_before(h, line_s, pos, "\"id\":")) return kId;
    }
  } else if (r.colon & m.outside & d.d1 & bit) {
    if (lit_before(h, line_s, pos + 1, "\"transcript_consequences\":")) return kKey0;
    if (lit_before(h, line_s, pos + 1, "\"regulatory_feature_consequences\":")) return kKey0 + 1;
    if (lit_before(h, line_s, pos + 1, "\"motif_feature_consequences\":")) return kKey0 + 2;
    if (lit_before(h, line_s, pos + 1, "\"intergenic_consequences\":")) return kKey0 + 3;
  }
  return kNone;
}

AVDB_HD void top_string(State& st, uint32_t kind, uint64_t start, uint32_t len) {
  if (kind == kInput) {
    st.input_start = start;
    st.input_len = int32_t(len);
  } else {
    st.id_start = start;
    st.id_len = int32_t(len);
  }
}

// the block's regions and what it alone decides about the line; blk: the block's first byte from the line's start
AVDB_HD void regions(const Raw& r, const Masks& m, const Depths& d, Kinds& k, State& st, Regions& g, uint32_t blk) {
  uint32_t why = 0;
  // the string the last block left open
  g.pend_close = -1;
  g.pend_kind = 0;
  if (st.pend_kind && m.quotes) {
    const uint32_t c = ctz(m.quotes), len = blk + c - st.pend_start;
    if (st.pend_kind == kInput || st.pend_kind == kId) {
      top_string(st, st.pend_kind, st.pend_start, len);
    } else {
      g.pend_close = int32_t(c);
      g.pend_kind = st.pend_kind;
      g.pend_start = st.pend_start;
      g.pend_len = len;
      g.pend_eidx = st.pend_eidx;
    }
    st.pend_kind = 0;
  }
  // the consequence arrays: from a '[' behind one of the four keys to the bracket that closes depth 2
  const uint64_t arr_any = k.arr[0] | k.arr[1] | k.arr[2] | k.arr[3];
  int32_t cur = st.cur_type;
  uint32_t from = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) g.csq[t] = 0;
  for (uint64_t ev = arr_any | (m.close & d.d2); ev; ev &= ev - 1) {
    const uint32_t e = ctz(ev);
#pragma unroll
    for (int t = 0; t < 4; ++t)  // (no array is indexed by a value: they stay in registers)
      if (cur == t) g.csq[t] |= bits_range(from, e);
    if ((arr_any >> e) & 1) {
      cur = (k.arr[0] >> e) & 1 ? 0 : (k.arr[1] >> e) & 1 ? 1 : (k.arr[2] >> e) & 1 ? 2 : 3;
      from = e;
#pragma unroll
      for (int t = 0; t < 4; ++t) st.n_arrays[t] += cur == t;
    } else {
      cur = -1;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (cur == t) g.csq[t] |= bits_range(from, 63);
  st.cur_type = cur;
  const uint64_t in_csq = g.csq[0] | g.csq[1] | g.csq[2] | g.csq[3];
  g.elem_open = m.open & r.lbrace & d.d3 & in_csq;
  g.elem_close = m.close & r.rbrace & d.d3 & in_csq;
  g.n0 = st.n_elems;
  for (uint64_t a = arr_any; a; a &= a - 1) {
    const uint32_t e = ctz(a), before = st.n_elems + popc(g.elem_open & bits_lt(e));
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if ((k.arr[t] >> e) & 1) st.base[t] = before;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) st.n_keys[t] += popc(k.key[t]);
  // the consequence_terms arrays: the depth-4 containers that open at one of their brackets
  k.allele &= in_csq;
  k.terms_arr &= in_csq;
  const uint64_t o4 = m.open & d.d4, c4 = m.close & d.d4;
  const uint64_t seg = prefix_xor(o4 | c4) ^ (st.seg4 ? ~0ull : 0ull);
  g.terms = runs_from(seg, k.terms_arr | (st.in_terms & seg & 1));
  st.seg4 = uint32_t(seg >> 63);
  st.in_terms = uint32_t(g.terms >> 63);
  g.term_open = m.sopen & g.terms & d.d4;
  // the key strings: those that open behind a '{' or a ','
  const uint64_t oc = (m.open & r.lbrace) | (r.comma & m.outside);
  const uint64_t key_open = m.sopen & ((oc << 1) | st.prev_oc);
  st.prev_oc = uint32_t(oc >> 63);
  const uint64_t in_key = runs_from(m.in_str, key_open | (st.in_key & m.in_str & 1));
  st.in_key = uint32_t(in_key >> 63);
  // what is left to the host
  if (r.ws & m.outside) why |= 1u << kWs;
  if (d.bad) why |= 1u << kDepth;
  if ((r.bs | r.hi) & in_key & (d.d1 | (d.d3 & in_csq))) why |= 1u << kBytes;
  const uint64_t ok2 = r.comma | (m.open & r.lbrack) | (m.close & r.rbrack);
  if (in_csq & d.d2 & (m.in_str | ~ok2)) why |= 1u << kElem;  // an array holds objects only
  if (m.open & r.lbrack & d.d3 & in_csq) why |= 1u << kElem;
  if (g.terms & m.outside & ~(r.comma | r.qt | o4 | c4)) why |= 1u << kElem;  // a terms array holds strings only
  // input and id
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    const uint32_t kind = which ? kId : kInput;
    for (uint64_t q = which ? k.id : k.input; q; q &= q - 1) {
      const uint32_t p = ctz(q);
      ++(which ? st.n_id : st.n_input);
      const uint64_t cq = m.quotes & ~bits_le(p);
      if (cq) top_string(st, kind, blk + p + 1, ctz(cq) - p - 1);
    }
  }
  // the string this block leaves open
  if (st.in_str && m.sopen) {
    const uint32_t p = 63 - uint32_t(__builtin_clzll(m.sopen));
    const uint64_t bit = 1ull << p;
    st.pend_kind = k.allele & bit ? kAllele : g.term_open & bit ? kTermStr : k.input & bit ? kInput : k.id & bit ? kId : kNone;
    st.pend_start = blk + p + 1;
    st.pend_eidx = st.n_elems + popc(g.elem_open & bits_le(p)) - 1;
  }
  st.n_elems += popc(g.elem_open);
  st.reasons |= why;
}

// a position that opens an element starts its record
AVDB_HD void elem_init(uint32_t lane, const Regions& g, const State& st, uint32_t blk, Elem* el) {
  if (!((g.elem_open >> lane) & 1)) return;
  const uint32_t i = g.n0 + popc(g.elem_open & bits_lt(lane));
  if (i >= kMaxCsq) return;
  const bool t0 = (g.csq[0] >> lane) & 1, t1 = (g.csq[1] >> lane) & 1, t2 = (g.csq[2] >> lane) & 1;
  const uint32_t t = t0 ? 0 : t1 ? 1 : t2 ? 2 : 3, base = t0 ? st.base[0] : t1 ? st.base[1] : t2 ? st.base[2] : st.base[3];
  el[i] = Elem{0, 0, blk + lane, 0, 0, 0, 0, (t << 30) | ((i - base) & kOrderMask)};
}

template <class Ops>
AVDB_HD uint32_t close_string(const Heap& h, uint64_t line_s, const TableView& tab, uint32_t kind, uint32_t i,
                              uint32_t start, uint32_t len, Elem* el) {
  if (i >= kMaxCsq) return 0;
  if (kind == kAllele) {
    el[i].al_start = start;
    el[i].al_len = len;
    Ops::add(&el[i].seen, 1u);
    return 0;
  }
  Ops::or64(&el[i].al8, 1);  // (free until check_elem: the element has a term string)
  if (span_not_plain(h, line_s + start, len)) return 1u << kBytes;
  const int32_t id = term_id(h, line_s + start, len, tab);
  if (id < 0) return 1u << kTerm;
  const uint64_t bit = 1ull << id;
  return Ops::or64(&el[i].mask, bit) & bit ? 1u << kRepeat : 0u;
}

// what a position adds to its element's record; returns the reasons it found
template <class Ops>
AVDB_HD uint32_t lane_events(const Heap& h, uint64_t line_s, const TableView& tab, uint32_t lane, const Masks& m,
                             const Kinds& k, const Regions& g, uint32_t blk, Elem* el) {
  const uint64_t bit = 1ull << lane;
  const uint32_t i = g.n0 + popc(g.elem_open & bits_le(lane)) - 1;  // the element the position lies in
  uint32_t why = 0;
  if (int32_t(lane) == g.pend_close)
    why |= close_string<Ops>(h, line_s, tab, g.pend_kind, g.pend_eidx, g.pend_start, g.pend_len, el);
  if ((g.elem_close & bit) && i < kMaxCsq) el[i].end = blk + lane;
  if ((k.terms_arr & bit) && i < kMaxCsq) Ops::add(&el[i].seen, 0x10000u);
  if ((k.allele | g.term_open) & bit) {
    const uint64_t cq = m.quotes & ~bits_le(lane);
    if (cq)
      why |= close_string<Ops>(h, line_s, tab, k.allele & bit ? kAllele : kTermStr, i, blk + lane + 1,
                               ctz(cq) - lane - 1, el);
  }
  return why;
}

// what the line's end decides
AVDB_HD uint32_t end_reasons(const State& st) {
  uint32_t why = st.reasons;
  if (st.depth != 0 || st.in_str) why |= 1u << kStruct;
  if (st.n_input > 1 || st.n_id > 1) why |= 1u << kDupKey;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (st.n_keys[t] > 1) why |= 1u << kDupKey;
    if (st.n_keys[t] != st.n_arrays[t]) why |= 1u << kElem;  // a key whose value is no array
  }
  if (st.n_elems > kMaxCsq) why |= 1u << kCap;
  return why;
}

// the flags byte of a line: 0, or 1 + its first reason
AVDB_HD uint8_t flags_of(uint32_t why) { return why ? uint8_t(1 + ctz(why)) : uint8_t(0); }

// an element once its line is read: its allele's first bytes, its ranking entry; returns the reasons
AVDB_HD uint32_t check_elem(const Heap& h, uint64_t line_s, const TableView& tab, Elem& e, int32_t* entry) {
  *entry = -1;
  if (e.seen != 0x10001u) return 1u << kElem;
  const bool any_term = e.al8 != 0;
  if (span_not_plain(h, line_s + e.al_start, e.al_len)) return 1u << kBytes;
  e.al8 = heap_u64(h, line_s + e.al_start) & low_bytes_mask(e.al_len);
  if (!e.mask) return any_term ? 0u : 1u << kEmpty;  // (terms without a number: their position said why)
  *entry = entry_of(tab, e.mask);
  return *entry < 0 ? 1u << kCombo : 0u;
}

struct CsqOut {
  uint8_t* type;
  int32_t* order;
  uint64_t* el_start;
  uint32_t* el_len;
  uint64_t* al_start;
  uint32_t* al_len;
  uint64_t* mask;
  int32_t* entry;
  uint8_t* coding;
  int32_t* sorted;
  uint8_t* head;
};

// row `at` of a line the host answers: nothing, in text order
AVDB_HD void blank_row(const CsqOut& o, uint64_t at, uint32_t i) {
  o.type[at] = 0;
  o.order[at] = 0;
  o.el_start[at] = 0;
  o.el_len[at] = 0;
  o.al_start[at] = 0;
  o.al_len[at] = 0;
  o.mask[at] = 0;
  o.entry[at] = -1;
  o.coding[at] = 0;
  o.sorted[at] = int32_t(i);
  o.head[at] = 0;
}

AVDB_HD void write_row(const CsqOut& o, uint64_t at, uint64_t line_s, const TableView& tab, const Elem& e, int32_t entry) {
  o.type[at] = uint8_t(e.type_order >> 30);
  o.order[at] = int32_t(e.type_order & kOrderMask);
  o.el_start[at] = line_s + e.start;
  o.el_len[at] = e.end - e.start + 1;
  o.al_start[at] = line_s + e.al_start;
  o.al_len[at] = e.al_len;
  o.mask[at] = e.mask;
  o.entry[at] = entry;
  o.coding[at] = (e.mask & tab.coding_mask) != 0;
}

// the first element of i's type with i's allele (alleles: byte strings, the length included)
AVDB_HD uint32_t leader_of(const Heap& h, uint64_t line_s, const Elem* el, uint32_t i) {
  const Elem& e = el[i];
  for (uint32_t j = i - (e.type_order & kOrderMask); j < i; ++j) {
    const Elem& f = el[j];
    if (f.al_len == e.al_len && f.al8 == e.al8 &&
        (e.al_len <= 8 || heap_equal(h, line_s + e.al_start, line_s + f.al_start, e.al_len)))
      return j;
  }
  return i;
}

// type, then the allele's first appearance, then the rank's order, then the place in the text
AVDB_HD uint64_t sort_key(const Elem& e, uint32_t leader, uint32_t rank_order, uint32_t i) {
  return (uint64_t(e.type_order >> 30) << 58) | (uint64_t(leader) << 42) | (uint64_t(rank_order) << 10) | i;
}

// where element i comes among the line's n (keys in el[].mask), and whether it heads its (type, allele) group
AVDB_HD uint32_t place(const Elem* el, uint32_t n, uint32_t i, bool* head) {
  const uint64_t key = el[i].mask;
  uint32_t before = 0, in_group = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const uint64_t kj = el[j].mask;
    before += kj < key;
    in_group += kj < key && (kj >> 42) == (key >> 42);
  }
  *head = in_group == 0;
  return before;
}

}  // namespace vep
}  // namespace avdb

// K11 — BGZF member framing and the per-member DEFLATE decoder (RFC 1951 / RFC 1952,
// SAM specification §4.1), shared by k_bgzf_inflate (one 64-lane wave per member),
// avdb_bgzf_inflate_host, avdb_bgzf_index_host and tools/bgzf_sanitize.hip: one
// definition, compiled for both sides.
//
// The code is written for `Lanes{lane, n}` cooperating on one member: n = 64 on the
// device (the wave; every lane runs the bit reader and the symbol chain uniformly,
// the lanes split table fills, match copies, the CRC and the flush), n = 1 on the
// host.  A member is decoded into a 64 KiB window of its own (on the device: the
// wave's slot of the context's workspace in global memory, read back through L2; see
// avdb_bgzf.hip); its bytes reach the caller's buffer only after the CRC-32 matched,
// so a failed member writes nothing.
//
// Bounds, for any input bytes:
//   * input: every read goes through Bits (bytes of the member's own deflate extent;
//     the 4-byte load is assembled bytewise in the last 3 bytes; past the end it reads
//     zeros and overrun() turns true) or is a stored block's copy checked against it;
//   * output: every window store is checked against the member's ISIZE (<= 65536)
//     first; the flush writes exactly ISIZE bytes, which the caller checked against
//     its buffer;
//   * a distance greater than the bytes this member produced is an error;
//   * every loop consumes at least one input bit per trip (and overrun() ends it) or
//     has a trip count fixed before it starts.
#pragma once

#include "avdb_internal.hpp"

namespace avdb {
namespace inflate {

constexpr uint32_t kMaxOut = 65536;    // ISIZE of a BGZF member is at most this
constexpr uint32_t kCrcChunk = 1024;   // the CRC chunk of one lane (64 of them cover the window)
constexpr int kLitBits = 10, kDistBits = 9, kClBits = 7;  // primary table widths

struct Lanes {
  uint32_t lane, n;  // n <= 64
};

// all lanes' earlier window / table writes are visible to all lanes
AVDB_HD void sync(const Lanes&) {
#if defined(__HIP_DEVICE_COMPILE__)
  __syncthreads();  // (the workgroup is the one wave)
#endif
}
// the same between two steps of the symbol chain, without the barrier: the wave's window
// stores have completed (vmcnt) before any lane loads what another lane stored; the
// lanes of a workgroup share their CU's L1, so nothing is invalidated
AVDB_HD void order(const Lanes&) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
#endif
}

AVDB_HD uint32_t le16(const uint8_t* p) { return uint32_t(p[0]) | uint32_t(p[1]) << 8; }
AVDB_HD uint32_t le32(const uint8_t* p) { return le16(p) | le16(p + 2) << 16; }

// ---- framing ---------------------------------------------------------------------
struct Member {
  uint32_t hdr_bytes;    // 12 + XLEN: the deflate stream starts here
  uint32_t total_bytes;  // BSIZE + 1
  uint32_t isize, crc;   // the trailer
};
enum { kMemberOk = 0, kMemberIncomplete = 1, kMemberNotGzip = 2, kMemberNotBgzf = 3 };

// The member at p, of which `avail` bytes are there.  A BGZF member: magic 1f 8b, CM 8,
// FLG 4 (FEXTRA alone), a 'B' 'C' subfield of length 2 among the extra subfields,
// BSIZE + 1 >= header + trailer, ISIZE <= 65536.
AVDB_HD int parse_member(const uint8_t* p, size_t avail, Member* m) {
  if (avail >= 1 && p[0] != 0x1f) return kMemberNotGzip;
  if (avail >= 2 && p[1] != 0x8b) return kMemberNotGzip;
  if (avail >= 3 && p[2] != 8) return kMemberNotBgzf;
  if (avail >= 4 && p[3] != 4) return kMemberNotBgzf;
  if (avail < 12) return kMemberIncomplete;
  const uint32_t end = 12 + le16(p + 10);
  if (avail < end) return kMemberIncomplete;
  uint32_t q = 12, total = 0;
  while (q + 4 <= end) {  // (q grows by at least 4 per trip)
    const uint32_t slen = le16(p + q + 2);
    if (q + 4 + slen > end) return kMemberNotBgzf;
    if (p[q] == 'B' && p[q + 1] == 'C' && !total) {
      if (slen != 2) return kMemberNotBgzf;
      total = le16(p + q + 4) + 1;
    }
    q += 4 + slen;
  }
  if (q != end || !total || total < end + 8) return kMemberNotBgzf;
  if (avail < total) return kMemberIncomplete;
  m->hdr_bytes = end;
  m->total_bytes = total;
  m->crc = le32(p + total - 8);
  m->isize = le32(p + total - 4);
  return m->isize <= kMaxOut ? kMemberOk : kMemberNotBgzf;
}

// ---- bit reader -------------------------------------------------------------------
struct Bits {
  const uint8_t* p;  // the deflate stream
  uint32_t end;      // its bytes
  uint32_t pos;      // next byte to load (may run past end: those bytes read 0)
  uint32_t cnt;      // bits in buf
  uint64_t buf;
  uint32_t ahead;    // the 4 bytes at pos, loaded one refill early: the load's latency hides behind the
                     // symbols decoded meanwhile instead of standing in the chain
};

AVDB_HD uint32_t load32(const Bits& b) {
  if (b.pos + 4 <= b.end) return reinterpret_cast<const U32u*>(b.p + b.pos)->v;
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k)
    if (b.pos + k < b.end) v |= uint32_t(b.p[b.pos + k]) << (8 * k);
  return v;
}
// at least 33 bits afterwards
AVDB_HD void refill(Bits& b) {
  if (b.cnt <= 32) {
    b.buf |= uint64_t(b.ahead) << b.cnt;
    b.pos += 4;
    b.cnt += 32;
    b.ahead = load32(b);
  }
}
AVDB_HD uint32_t take(Bits& b, uint32_t n) {  // n <= 16, n <= cnt
  const uint32_t v = uint32_t(b.buf) & ((1u << n) - 1);
  b.buf >>= n;
  b.cnt -= n;
  return v;
}
// more bits taken than the stream has
AVDB_HD bool overrun(const Bits& b) { return uint64_t(b.pos) * 8 - b.cnt > uint64_t(b.end) * 8; }

// ---- canonical Huffman tables -------------------------------------------------------
// Codes of up to PBITS bits: one lookup in tab[] by the next PBITS bits.  Longer ones:
// one compare per length PBITS+1..15 of the bit-reversed peek against that length's
// code range (first[], count[]), then sorted[] (at most 5 trips, none for most files:
// zlib gives a 65,280-byte block of VCF text codes of 11 or more bits to rare bytes only).
template <int PBITS, int NSYM>
struct Huff {
  uint16_t tab[1 << PBITS];  // (symbol << 4) | length; 0: not the prefix of a short code
  uint16_t sorted[NSYM];     // symbols by (length, symbol)
  uint16_t count[16], first[16], offs[16], cur[16];
  uint32_t used, ok;
};

// zlib's inflate_table acceptance: an over-subscribed set is refused; an incomplete one
// too, unless it is a single code of length 1 (and never for the code-length code);
// a set with no code at all is accepted here and refused by the caller where zlib does.
template <int PBITS, int NSYM>
AVDB_HD bool huff_build(const Lanes& L, Huff<PBITS, NSYM>& h, const uint8_t* lens, uint32_t n, bool codes) {
  if (L.lane == 0) {
    for (int l = 0; l < 16; ++l) h.count[l] = 0;
    for (uint32_t s = 0; s < n; ++s) ++h.count[lens[s] & 15];
    const uint32_t used = n - h.count[0];
    int left = 1;
    bool ok = true;
    for (int l = 1; l < 16 && ok; ++l) {
      left = (left << 1) - int(h.count[l]);
      ok = left >= 0;
    }
    if (ok && left > 0 && used && (codes || !(used == 1 && h.count[1] == 1))) ok = false;
    if (ok) {
      uint32_t code = 0, off = 0;
      for (int l = 1; l < 16; ++l) {
        h.first[l] = uint16_t(code);
        h.offs[l] = h.cur[l] = uint16_t(off);
        code = (code + h.count[l]) << 1;
        off += h.count[l];
      }
      for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = lens[s] & 15;
        if (l) h.sorted[h.cur[l]++] = uint16_t(s);
      }
    }
    h.used = used;
    h.ok = ok;
  }
  for (uint32_t i = L.lane; i < (1u << PBITS); i += L.n) h.tab[i] = 0;
  sync(L);
  if (!h.ok) return false;
  const uint32_t used = h.used;
  for (uint32_t idx = L.lane; idx < used; idx += L.n) {
    const uint32_t s = h.sorted[idx], l = lens[s] & 15;
    if (l <= uint32_t(PBITS)) {
      const uint32_t code = h.first[l] + (idx - h.offs[l]);
      const uint32_t rev = __builtin_bitreverse32(code) >> (32 - l);
      for (uint32_t j = rev; j < (1u << PBITS); j += 1u << l) h.tab[j] = uint16_t(s << 4 | l);
    }
  }
  sync(L);
  return true;
}

// the symbol whose code starts the (at least 15 valid) bits of `bits`; *len = 0: none
template <int PBITS, int NSYM>
AVDB_HD uint32_t huff_decode(const Huff<PBITS, NSYM>& h, uint32_t bits, uint32_t* len) {
  const uint32_t e = h.tab[bits & ((1u << PBITS) - 1)];
  if (e) {
    *len = e & 15;
    return e >> 4;
  }
  const uint32_t v = __builtin_bitreverse32(bits) >> 17;  // the next 15 bits, first bit highest
  for (uint32_t l = PBITS + 1; l <= 15; ++l) {
    const uint32_t code = v >> (15 - l), f = h.first[l];
    if (code >= f && code - f < h.count[l]) {
      *len = l;
      return h.sorted[h.offs[l] + (code - f)];
    }
  }
  *len = 0;
  return 0;
}

// ---- CRC-32 (reflected 0xEDB88320), in chunks --------------------------------------
constexpr uint32_t kPoly = 0xEDB88320u;

AVDB_HD uint32_t crc_step(uint32_t crc, int bits) {
  for (int k = 0; k < bits; ++k) crc = (crc >> 1) ^ (kPoly & (0u - (crc & 1u)));
  return crc;
}
// the CRC register after window[from .. to), from 4-aligned (window is 16-aligned)
AVDB_HD uint32_t crc_run(const uint8_t* w, uint32_t from, uint32_t to, uint32_t crc) {
  uint32_t i = from;
  for (; i + 4 <= to; i += 4) crc = crc_step(crc ^ *reinterpret_cast<const uint32_t*>(w + i), 32);
  for (; i < to; ++i) crc = crc_step(crc ^ w[i], 8);
  return crc;
}
// a * b modulo the polynomial (bit 31 is x^0, as in zlib's multmodp)
AVDB_HD uint32_t mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int k = 0; k < 32; ++k) {
    p ^= b & (0u - ((a >> (31 - k)) & 1u));
    b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
  }
  return p;
}
// x^(8 m) modulo the polynomial, m <= 65536
AVDB_HD uint32_t xpow8(uint32_t m) {
  uint32_t r = 0x80000000u, base = 0x00800000u;  // x^0, x^8
  for (int k = 0; k < 17; ++k) {
    if ((m >> k) & 1u) r = mulmod(r, base);
    base = mulmod(base, base);
  }
  return r;
}

// ---- the state of one member --------------------------------------------------------
struct Window {  // (one per wave, in global memory, on the device; one for the call on the host)
  alignas(16) uint8_t b[kMaxOut + 32];  // (the flush reads whole words up to 19 bytes past the output)
};
struct State {  // (LDS on the device)
  Huff<kLitBits, 288> lit;
  Huff<kDistBits, 32> dist;
  Huff<kClBits, 19> cl;
  uint8_t lens[288 + 32];  // literal/length code lengths, then the distance code lengths
  uint8_t cl_lens[20];
  uint32_t crc[64];
};

// The register is linear in the message: after A then B it is reg(A) * x^(8 |B|) + reg0(B),
// reg0 the register started from 0.  Chunk c of 1 KiB is run by lane c (chunk 0 from
// 0xFFFFFFFF) and multiplied by x^(8 * bytes after it); the sum is the member's register.
AVDB_HD uint32_t crc32_window(const Lanes& L, State& S, const uint8_t* w, uint32_t n) {
  uint32_t acc = 0;
  for (uint32_t c = L.lane; c < 64; c += L.n) {
    const uint32_t from = c * kCrcChunk;
    if (c && from >= n) break;
    const uint32_t to = from + kCrcChunk < n ? from + kCrcChunk : n;
    acc ^= mulmod(crc_run(w, from, to, c ? 0u : 0xFFFFFFFFu), xpow8(n - to));
  }
  S.crc[L.lane] = acc;
  sync(L);
  uint32_t r = 0;
  for (uint32_t k = 0; k < L.n; ++k) r ^= S.crc[k];
  sync(L);
  return ~r;
}

// ---- DEFLATE -------------------------------------------------------------------------
// src[0 .. src_bytes): one member's deflate stream -> w[0 .. isize); AVDB_BGZF_*
AVDB_HD uint32_t inflate_stream(const Lanes& L, State& S, uint8_t* w, const uint8_t* src, uint32_t src_bytes,
                                uint32_t isize) {
  Bits b{src, src_bytes, 0, 0, 0, 0};
  b.ahead = load32(b);
  uint32_t o = 0;  // bytes produced
  for (;;) {       // one deflate block per trip: at least its 3 header bits
    refill(b);
    const uint32_t hdr = take(b, 3);
    if (overrun(b)) return AVDB_BGZF_OVERRUN;
    const uint32_t type = hdr >> 1;
    if (type == 3) return AVDB_BGZF_BAD_BTYPE;
    if (type == 0) {
      take(b, b.cnt & 7);  // to the byte boundary (pos * 8 - cnt bits are taken: cnt mod 8 are left in this byte)
      refill(b);
      const uint32_t len = take(b, 16), nlen = take(b, 16);
      if (overrun(b)) return AVDB_BGZF_OVERRUN;
      if ((len ^ nlen) != 0xFFFFu) return AVDB_BGZF_BAD_STORED;
      const uint32_t at = b.pos - (b.cnt >> 3);  // (no overrun: at <= end)
      if (len > b.end - at) return AVDB_BGZF_OVERRUN;
      if (len > isize - o) return AVDB_BGZF_OUT_LONG;
      for (uint32_t i = L.lane; i < len; i += L.n) w[o + i] = src[at + i];
      o += len;
      b.pos = at + len;
      b.cnt = 0;
      b.buf = 0;
      b.ahead = load32(b);
    } else {
      uint32_t nlit, ndist;
      sync(L);  // (the last block's tables are done with)
      if (type == 1) {
        // RFC 1951 §3.2.6; 32 distance codes of 5 bits make the set complete: 30 and 31,
        // like literal/length 286 and 287, are refused where they turn up
        nlit = 288, ndist = 32;
        for (uint32_t i = L.lane; i < 320; i += L.n)
          S.lens[i] = uint8_t(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
      } else {
        nlit = take(b, 5) + 257;
        ndist = take(b, 5) + 1;
        const uint32_t ncl = take(b, 4) + 4;
        if (overrun(b)) return AVDB_BGZF_OVERRUN;
        if (nlit > 286 || ndist > 30) return AVDB_BGZF_BAD_LENS;
        const uint8_t kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        for (uint32_t i = L.lane; i < 19; i += L.n) S.cl_lens[i] = 0;
        sync(L);
        for (uint32_t i = 0; i < ncl; ++i) {
          refill(b);
          const uint32_t v = take(b, 3);
          if (L.lane == 0) S.cl_lens[kOrder[i]] = uint8_t(v);
        }
        if (overrun(b)) return AVDB_BGZF_OVERRUN;
        sync(L);
        if (!huff_build(L, S.cl, S.cl_lens, 19, true) || !S.cl.used) return AVDB_BGZF_BAD_LENS;
        const uint32_t total = nlit + ndist;
        uint32_t i = 0, prev = 0;
        while (i < total) {  // at least one bit per trip
          refill(b);
          uint32_t l;
          const uint32_t sym = huff_decode(S.cl, uint32_t(b.buf), &l);
          if (!l) return AVDB_BGZF_BAD_LENS;
          take(b, l);
          if (sym < 16) {
            if (L.lane == 0) S.lens[i] = uint8_t(sym);
            prev = sym;
            ++i;
          } else {
            uint32_t rep, val = 0;
            if (sym == 16) {
              if (i == 0) return AVDB_BGZF_BAD_LENS;
              rep = 3 + take(b, 2);
              val = prev;
            } else if (sym == 17) {
              rep = 3 + take(b, 3);
            } else {
              rep = 11 + take(b, 7);
            }
            if (rep > total - i) return AVDB_BGZF_BAD_LENS;
            for (uint32_t k = L.lane; k < rep; k += L.n) S.lens[i + k] = uint8_t(val);
            i += rep;
            prev = val;
          }
          if (overrun(b)) return AVDB_BGZF_OVERRUN;
        }
      }
      sync(L);
      if (S.lens[256] == 0) return AVDB_BGZF_BAD_LENS;  // no end-of-block code
      if (!huff_build(L, S.lit, S.lens, nlit, false)) return AVDB_BGZF_BAD_LENS;
      if (!huff_build(L, S.dist, S.lens + nlit, ndist, false)) return AVDB_BGZF_BAD_LENS;
      for (;;) {  // one symbol per trip: at least one bit
        refill(b);
        uint32_t l;
        uint32_t sym = huff_decode(S.lit, uint32_t(b.buf), &l);
        if (!l) return overrun(b) ? AVDB_BGZF_OVERRUN : AVDB_BGZF_BAD_SYMBOL;
        take(b, l);
        if (sym < 256) {
          if (overrun(b)) return AVDB_BGZF_OVERRUN;
          if (o >= isize) return AVDB_BGZF_OUT_LONG;
          if (L.lane == 0) w[o] = uint8_t(sym);
          ++o;
          continue;
        }
        if (sym == 256) {
          if (overrun(b)) return AVDB_BGZF_OVERRUN;
          break;
        }
        if (sym > 285) return AVDB_BGZF_BAD_SYMBOL;
        sym -= 257;
        uint32_t len;
        if (sym < 8) {
          len = 3 + sym;
        } else if (sym == 28) {
          len = 258;
        } else {
          const uint32_t eb = (sym >> 2) - 1;
          len = 3 + ((4 + (sym & 3)) << eb) + take(b, eb);
        }
        refill(b);
        const uint32_t dsym = huff_decode(S.dist, uint32_t(b.buf), &l);
        if (!l) return overrun(b) ? AVDB_BGZF_OVERRUN : AVDB_BGZF_BAD_SYMBOL;
        take(b, l);
        if (dsym > 29) return AVDB_BGZF_BAD_SYMBOL;
        uint32_t d;
        if (dsym < 4) {
          d = 1 + dsym;
        } else {
          const uint32_t eb = (dsym >> 1) - 1;
          d = 1 + ((2 + (dsym & 1)) << eb) + take(b, eb);
        }
        if (overrun(b)) return AVDB_BGZF_OVERRUN;
        if (d > o) return AVDB_BGZF_DIST_FAR;  // there is no history before a member
        if (len > isize - o) return AVDB_BGZF_OUT_LONG;
        // All lanes copy.  Round r (bytes 64 r .. 64 r + 63 of the match) may read what
        // rounds before it wrote, never its own bytes: byte i comes from o - d + i when
        // d >= 64 (or the match does not overlap itself), else from the first period,
        // o - d + i mod d — a run of one byte when d = 1.
        order(L);
        const bool direct = d >= len || d >= 64;
        for (uint32_t i = L.lane; i < len; i += L.n) {
          w[o + i] = w[o - d + (direct ? i : i % d)];
          order(L);
        }
        o += len;
      }
    }
    if (hdr & 1) break;
  }
  if (o != isize) return AVDB_BGZF_OUT_SHORT;
  // the trailer follows the stream's last byte, or BSIZE is not this stream's
  if ((uint64_t(b.pos) * 8 - b.cnt + 7) / 8 != b.end) return AVDB_BGZF_BAD_HEADER;
  sync(L);
  return AVDB_BGZF_OK;
}

// w[0 .. n) -> dst: bytes up to dst's 16-byte boundary, 16-byte stores (each word
// funnelled from two aligned window words), the bytes left
AVDB_HD void flush(const Lanes& L, const uint8_t* win, uint8_t* dst, uint32_t n) {
  uint32_t head = uint32_t((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15);
  if (head > n) head = n;
  for (uint32_t i = L.lane; i < head; i += L.n) dst[i] = win[i];
  const uint32_t nvec = (n - head) / 16, sh = (head & 3) * 8;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(win) + (head >> 2);
  for (uint32_t j = L.lane; j < nvec; j += L.n) {
    const uint32_t* a = w + 4 * j;
    uint32_t x[5];
    for (int k = 0; k < 5; ++k) x[k] = a[k];
    u32x4 v;
    v.x = uint32_t((uint64_t(x[1]) << 32 | x[0]) >> sh);
    v.y = uint32_t((uint64_t(x[2]) << 32 | x[1]) >> sh);
    v.z = uint32_t((uint64_t(x[3]) << 32 | x[2]) >> sh);
    v.w = uint32_t((uint64_t(x[4]) << 32 | x[3]) >> sh);
    *reinterpret_cast<u32x4*>(dst + head + 16 * j) = v;
  }
  for (uint32_t i = head + 16 * nvec + L.lane; i < n; i += L.n) dst[i] = win[i];
}

// Member k of a chain: comp[in_off ..) -> out[out_lo .. out_hi) by way of the window w (a Window's bytes);
// AVDB_BGZF_*.  Nothing
// is taken on trust: the offsets are checked against comp_bytes and out_cap, the
// trailer's ISIZE against out_hi - out_lo.
AVDB_HD uint32_t inflate_member(const Lanes& L, State& S, uint8_t* w, const uint8_t* comp, size_t comp_bytes, uint64_t in_off,
                                uint64_t out_lo, uint64_t out_hi, uint8_t* out, size_t out_cap) {
  if (in_off > comp_bytes || out_lo > out_hi || out_hi > out_cap || out_hi - out_lo > kMaxOut)
    return AVDB_BGZF_BAD_HEADER;
  Member m;
  if (parse_member(comp + in_off, comp_bytes - in_off, &m) != kMemberOk || m.isize != out_hi - out_lo)
    return AVDB_BGZF_BAD_HEADER;
  const uint32_t st = inflate_stream(L, S, w, comp + in_off + m.hdr_bytes, m.total_bytes - m.hdr_bytes - 8, m.isize);
  if (st != AVDB_BGZF_OK) return st;
  if (crc32_window(L, S, w, m.isize) != m.crc) return AVDB_BGZF_BAD_CRC;
  flush(L, w, out + out_lo, m.isize);
  return AVDB_BGZF_OK;
}

}  // namespace inflate
}  // namespace avdb

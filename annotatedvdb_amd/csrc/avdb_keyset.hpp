// K6 — the hash, the insert and the text probe of the key set (avdb_keyset.hip), as code for
// both sides: the kernels of avdb_keyset.hip and of K16b (avdb_lof.hip) call it on the device,
// avdb_keyset_build_host and the _host entries of K16b on the host.  One definition, compiled for
// both sides, as avdb_existing.hpp is.
#pragma once

#include "avdb_internal.hpp"

namespace avdb {
namespace keyset {

AVDB_HD uint64_t mix(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// streaming hash of a byte sequence: bytes packed little-endian into 8-byte
// words, each completed word mixed in; the length closes it.  Keys and
// generated metaseq ids go through the same byte stream, so equal strings hash
// equal however they are assembled.
struct Hasher {
  uint64_t h = 0x9E3779B97F4A7C15ull, w = 0;
  uint32_t n = 0;
  AVDB_HD void put(uint32_t c) {
    w |= uint64_t(c & 0xFFu) << (8 * (n & 7));
    if ((++n & 7) == 0) { h = mix(h ^ w); w = 0; }
  }
  AVDB_HD uint64_t done() const {
    const uint64_t x = mix(h ^ w ^ (uint64_t(n) << 56));
    return x ? x : 1ull;  // 0 marks an empty slot
  }
};

// the slot a hash starts its linear probe at
AVDB_HD uint64_t first_slot(uint64_t h, uint64_t mask) { return mix(h ^ 0x5bd1e995ull) & mask; }

inline uint64_t slots(size_t n) {
  uint64_t s = 1024;
  while (s < 2ull * n) s <<= 1;
  return s;
}

// key i into the table: open addressing, the first of equal keys wins (= firstHitOnly).  On the
// device atomicCAS on the hash and atomicMin on the key index; on the host, where one thread
// inserts the keys in order, the same two steps in plain code.
AVDB_HD void insert(const uint8_t* keys, const uint64_t* key_off, size_t i, unsigned long long* tkey, uint32_t* tidx,
                    uint64_t mask) {
  Hasher hs;
  for (uint64_t b = key_off[i]; b < key_off[i + 1]; ++b) hs.put(keys[b]);
  const uint64_t h = hs.done();
  uint64_t slot = first_slot(h, mask);
  for (;;) {  // >= 2n slots: terminates
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long prev = atomicCAS(&tkey[slot], 0ull, (unsigned long long)h);
    if (prev == 0ull || prev == h) { atomicMin(&tidx[slot], uint32_t(i)); break; }
#else
    const unsigned long long prev = tkey[slot];
    if (prev == 0ull) tkey[slot] = h;
    if (prev == 0ull || prev == h) {
      if (uint32_t(i) < tidx[slot]) tidx[slot] = uint32_t(i);
      break;
    }
#endif
    slot = (slot + 1) & mask;
  }
}

template <class CP>
AVDB_HD bool str_equals(const uint8_t* a, uint64_t alen, CP b, uint64_t blen) {
  if (alen != blen) return false;
  for (uint64_t i = 0; i < alen; ++i)
    if (a[i] != b[i]) return false;
  return true;
}

// the index of the first key equal to s[0, len), or -1; *coll counts 64-bit hash collisions.
// CP: a byte pointer in the query's address space (host, global or an LDS stage).
template <class CP>
AVDB_HD int32_t probe_text(const uint8_t* keys, const uint64_t* key_off, size_t n_keys, const unsigned long long* tkey,
                           const uint32_t* tidx, uint64_t mask, CP s, uint64_t len, uint32_t* coll) {
  Hasher hs;
  for (uint64_t b = 0; b < len; ++b) hs.put(s[b]);
  const uint64_t h = hs.done();
  uint64_t slot = first_slot(h, mask);
  for (;;) {
    const unsigned long long t = tkey[slot];
    if (t == 0ull) return -1;
    if (t == h) break;
    slot = (slot + 1) & mask;
  }
  const uint32_t k = tidx[slot];
  if (k < n_keys && str_equals(keys + key_off[k], key_off[k + 1] - key_off[k], s, len)) return int32_t(k);
  // a different key with the same 64-bit hash (astronomically rare): exact scan
  ++*coll;
  for (size_t j = 0; j < n_keys; ++j)
    if (str_equals(keys + key_off[j], key_off[j + 1] - key_off[j], s, len)) return int32_t(j);
  return -1;
}

}  // namespace keyset
}  // namespace avdb

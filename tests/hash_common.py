"""Python restatements of the K3 / K6 hashes and builders of inputs that collide
under them (shared by test_hash_common_host.py and test_gpu_dedup_join_edges.py).

Written from the comments in csrc/avdb_keyset.hip and csrc/avdb_dedup.hip:

* one 64-bit mixer (``h ^= h >> 33; h *= C1; h ^= h >> 33; h *= C2; h ^= h >> 33``);
* K6 hashes a byte string as little-endian 8-byte words, ``h = mix(h ^ word)`` per
  completed word from ``IV``, closed by ``mix(h ^ partial_word ^ (len << 56))``
  (``len`` is 32-bit, so only its low byte survives the shift), 0 -> 1;
  home slot ``mix(h ^ 0x5bd1e995) & mask``;
* K3 fingerprints a record as ``mix((chrom << 32) ^ pos ^ IV)``, then ``ext``, then
  ``(ref_len << 32) | alt_len``, then the ref+alt bytes as little-endian words (the
  last one masked to the bytes left), each by ``h = mix(h ^ word)``, 0 -> 1;
  home slot ``mix(h) & mask``;
* both tables have 1,024 slots, doubled until ``>= 2 n``.

Every step is ``h = mix(h ^ word)`` with an invertible ``mix``, so two inputs that
differ in one word and compensate in the next (``w2' = w2 ^ mix(h ^ w1) ^ mix(h ^
w1')``) hash equal.  Nothing here proves the restatement matches the device: the
GPU tests do, through their asserts on the collision counter.
"""

from typing import Iterable, List, Optional, Sequence, Tuple

M64 = (1 << 64) - 1
IV = 0x9E3779B97F4A7C15
K6_SLOT_SALT = 0x5BD1E995

Record = Tuple[int, int, bytes, bytes, int]  # (chrom code, pos, ref, alt, ext_id)


def mix(x: int) -> int:
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def slots(n: int) -> int:
    s = 1024
    while s < 2 * n:
        s <<= 1
    return s


def _words(b: bytes) -> List[int]:
    """Little-endian 8-byte words of ``b``; the last one holds the bytes left (zero filled)."""
    return [int.from_bytes(b[k:k + 8], "little") for k in range(0, len(b), 8)]


# ---- K6 ---------------------------------------------------------------------
def k6_hash(s: bytes) -> int:
    h = IV
    full = len(s) // 8
    for k in range(full):
        h = mix(h ^ int.from_bytes(s[8 * k:8 * k + 8], "little"))
    w = int.from_bytes(s[8 * full:], "little")
    x = mix(h ^ w ^ (((len(s) & 0xFFFFFFFF) << 56) & M64))
    return x or 1


def k6_home(h: int, n_slots: int) -> int:
    return mix(h ^ K6_SLOT_SALT) & (n_slots - 1)


def colliding_strings(a: bytes, first: bytes, forbid: bytes = b":") -> bytes:
    """A string ``b`` of ``a``'s length with ``k6_hash(b) == k6_hash(a)``: its first
    word is ``first`` (8 bytes, other than ``a[:8]``), bytes 8..15 compensate, the rest
    is ``a``'s.  Raises ValueError where a computed byte is in ``forbid``."""
    if len(a) < 16 or len(first) != 8 or first == a[:8]:
        raise ValueError("need >= 16 bytes and another first word")
    w1, w1b = int.from_bytes(a[:8], "little"), int.from_bytes(first, "little")
    w2 = int.from_bytes(a[8:16], "little")
    w2b = w2 ^ mix(IV ^ w1) ^ mix(IV ^ w1b)
    mid = w2b.to_bytes(8, "little")
    if any(c in forbid for c in mid):
        raise ValueError("computed bytes hit a forbidden value")
    return first + mid + a[16:]


def colliding_metaseq_pairs(count: int, chrom: str = "1", pos0: int = 1000, alt: bytes = b"G",
                            ref_len: int = 10) -> List[Tuple[bytes, bytes]]:
    """``count`` pairs ``(A, B)`` of metaseq ids ``chrom:pos:REF:alt`` with equal K6
    hashes, one pair per position from ``pos0`` on.  A's REF is ACGT text; B's differs
    in its first base, and the 8 computed bytes lie inside REF (any value but ':', so
    that the ids still split into four fields)."""
    out = []
    pos = pos0
    while len(out) < count:
        pre = b"%s:%d:" % (chrom.encode(), pos)
        if len(pre) > 7 or len(pre) + ref_len < 16:
            raise ValueError("the second word must lie inside REF")
        ref = bytes(b"ACGT"[(pos + 3 * k) & 3] for k in range(ref_len))
        a = pre + ref + b":" + alt
        for c in b"CGTA":
            if c == ref[0]:
                continue
            first = (pre + bytes([c]) + ref[1:])[:8]
            try:
                b = colliding_strings(a, first)
            except ValueError:
                continue
            out.append((a, b))
            break
        pos += 1
    return out


def split_metaseq(s: bytes) -> Tuple[bytes, bytes, bytes, bytes]:
    c, p, r, a = s.split(b":")
    return c, p, r, a


def k6_keys_at_slot(slot: int, n_slots: int, want: int, limit: int = 20000,
                    fmt: bytes = b"1:%d:A:G") -> List[bytes]:
    """The first ``want`` keys ``fmt % pos`` (pos in 1..limit-1) whose home slot is ``slot``."""
    out = []
    for p in range(1, limit):
        k = fmt % p
        if k6_home(k6_hash(k), n_slots) == slot:
            out.append(k)
            if len(out) == want:
                break
    return out


def k6_predict_collisions(keys: Sequence[bytes], lookups: Iterable[bytes]) -> int:
    """Lookups whose hash is in the table but whose slot owner (the first key with
    that hash) is another string — what AVDB_CTR_HASH_COLLISIONS counts for K6."""
    owner = {}
    for i, k in enumerate(keys):
        owner.setdefault(k6_hash(k), i)
    n = 0
    for s in lookups:
        w = owner.get(k6_hash(s))
        if w is not None and keys[w] != s:
            n += 1
    return n


# ---- K3 ---------------------------------------------------------------------
def _k3_head(chrom: int, pos: int, ext: int, ref_len: int, alt_len: int) -> int:
    h = mix(((chrom << 32) ^ (pos & 0xFFFFFFFF) ^ IV) & M64)
    h = mix(h ^ (ext & M64))
    return mix(h ^ ((ref_len << 32) | alt_len))


def k3_fingerprint(rec: Record) -> int:
    c, p, ref, alt, e = rec
    h = _k3_head(c, p, e, len(ref), len(alt))
    for w in _words(ref + alt):
        h = mix(h ^ w)
    return h or 1


def k3_home(h: int, n_slots: int) -> int:
    return mix(h) & (n_slots - 1)


def colliding_record_by_alleles(rec: Record, first_byte: Optional[int] = None) -> Record:
    """A record with ``rec``'s (chrom, pos, ext, ref_len, alt_len) and fingerprint whose
    allele bytes differ: byte 0 changes, bytes 8..15 compensate."""
    c, p, ref, alt, e = rec
    body = ref + alt
    if len(body) < 16:
        raise ValueError("need ref_len + alt_len >= 16")
    h3 = _k3_head(c, p, e, len(ref), len(alt))
    nb = (body[0] ^ 0x06) if first_byte is None else first_byte  # 'A' <-> 'G', 'C' <-> 'E'
    if nb == body[0]:
        raise ValueError("the first byte must change")
    w1 = int.from_bytes(body[:8], "little")
    w1b = int.from_bytes(bytes([nb]) + body[1:8], "little")
    w2b = int.from_bytes(body[8:16], "little") ^ mix(h3 ^ w1) ^ mix(h3 ^ w1b)
    nbody = bytes([nb]) + body[1:8] + w2b.to_bytes(8, "little") + body[16:]
    return (c, p, nbody[:len(ref)], nbody[len(ref):], e)


def colliding_record_by_position(rec: Record, pos2: int) -> Record:
    """``rec``'s alleles at ``pos2`` with the ext id that gives ``rec``'s fingerprint
    (as a signed 64-bit value, the ext_id array's type)."""
    c, p, ref, alt, e = rec
    if pos2 == p:
        raise ValueError("need another position")
    e2 = (e & M64) ^ mix(((c << 32) ^ p ^ IV) & M64) ^ mix(((c << 32) ^ pos2 ^ IV) & M64)
    if e2 >= 1 << 63:
        e2 -= 1 << 64
    return (c, pos2, ref, alt, e2)


def k3_records_at_slot(slot: int, n_slots: int, want: int, limit: int = 20000) -> List[Record]:
    """The first ``want`` records (chrom 0, pos, "A", "G", ext 0) whose home slot is ``slot``."""
    out = []
    for p in range(1, limit):
        r = (0, p, b"A", b"G", 0)
        if k3_home(k3_fingerprint(r), n_slots) == slot:
            out.append(r)
            if len(out) == want:
                break
    return out


def k3_predict_collisions(recs: Sequence[Record]) -> int:
    """Records whose slot winner (the first record with their fingerprint) is another
    key — what AVDB_CTR_HASH_COLLISIONS counts for K3's hash path."""
    first = {}
    n = 0
    for i, r in enumerate(recs):
        w = first.setdefault(k3_fingerprint(r), i)
        if w != i and recs[w] != r:
            n += 1
    return n


def keep_first(recs: Sequence[Record]) -> List[int]:
    seen, keep = set(), []
    for r in recs:
        keep.append(0 if r in seen else 1)
        seen.add(r)
    return keep

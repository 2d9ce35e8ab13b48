"""K7 (primary keys + ltree paths as text: `k_record_keys_v2` / `key_tile` in
annotatedvdb_amd/csrc/avdb_keys.hip) at the edges `synth.alleles` / `synth.np_c1` do not reach: hand-built
records, an independent plain-Python reference and, per builder, a CPU computation of
the edges its records reach (shared by test_k7_common_host.py and test_gpu_k7_edges.py).

Nothing in this module calls K7 or the C library's formatter.  The reference restates
K7's documented conventions (include/avdb.h, "AVDB_KEY_*"; annotatedvdb_amd/csrc/avdb_keys.hip, the K7
header comment and `key_tile`):

* key  = ``"%s:%d:%s:%s" % (label, pos, ref, alt)`` plus ``":rs%d" % ext`` when ext != 0
  (primary_key_generator.py:106-122), or ``label:pos:<32 digest chars>`` (plus the same
  suffix) when ``len(ref) + len(alt) > max_len``;
* contig code >= 25 (no label) or ext bit 63 (an interned, non-rs id): state KEY_HOST
  and an EMPTY span; a contig code >= 25 has no path either;
* a long record without digests: KEY_NEED_DIGEST and an empty span; under
  AVDB_KEYS_DIGEST_DEFERRED: KEY_DIGEST_PENDING and a span of the normal size whose 32
  digest bytes come later (avdb_primary_keys_fill_digests);
* a short record with ':' or a byte >= 0x80 in ref / alt, or with
  ``off + r + a > heap_bytes``: KEY_HOST and a span of the NORMAL size (the span is
  reserved from the SoA either way; its bytes are read only when the state is KEY_OK);
* path = "chr" + label + ".L<l>.B<k>" per level (generate_bin_index_references.py:54,
  60-61,74), empty for BIN_NONE.

Constants restated here, with their definitions:

* TILE 64          kWave (annotatedvdb_amd/csrc/avdb_internal.hpp): records per write-pass tile
* CHUNK 16         flush_span32's store granule (annotatedvdb_amd/csrc/avdb_keys.hip)
* WIN_BYTES 56     8 * kWinWords: `wide = m + n > 56` in `key_tile`
* KEY_WAVE 2560    kKeyWave: a tile's keys are staged iff K + (g0 & 15) + 16 <= 2560
* PATH_WAVE 5632   kPathWave: the same for paths
* SMALL_GROUP_N    AVDB_K7_SMALL_GROUP_N = 4 * 2^20: 256-record groups from there on

What the flush cells mean.  A tile's span [g0, g1) of a stream falls in one category:

  empty    g0 == g1 (cell phase = g0 & 15; phase 0 stores nothing)
  aligned  both ends 16-aligned
  tail     g0 aligned, g1 not (cell phase = g1 & 15: the start phase is 0 by definition)
  head     g0 not aligned, g1 aligned
  inside   both unaligned, inside one chunk
  cross    both unaligned, one boundary between them and no full chunk
  general  both unaligned, with full chunks between head and tail

`aligned` and `tail` exist at start phase 0 only; a key has at least 5 bytes
("1:5::") and a path 4 ("chr1"), so `inside` exists for start phases 1..10 (keys) and
1..11 (paths) only, and a tile's key total is 0 or >= 5 (never 4).  Every other cell,
phases 1..15, is built.
"""

import functools
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from k4_common import B64URL, bases
from oracle import avdb_oracle as O

TILE = 64
CHUNK = 16
WIN_BYTES = 56
KEY_WAVE = 2560
PATH_WAVE = 5632
SMALL_GROUP_N = 4 << 20
OFF32_SPAN = 4096       # kOff32Span: one u64 base per 4,096 narrow offsets
N_CONTIGS = 25          # labelled contigs (chromosomes.py:9-38)
DIGEST_CHARS = 32       # AVDB_DIGEST_CHARS
BIN_NONE = 0xFFFFFFFF   # AVDB_BIN_NONE
INTERNED = 1 << 63      # ext bit 63: an interned (non-rs) external id
KEY_OK, KEY_HOST, KEY_NEED_DIGEST, KEY_OVERFLOW, KEY_DIGEST_PENDING = 0, 1, 2, 3, 4  # AVDB_KEY_*
LABELS = tuple(str(i) for i in range(1, 23)) + ("X", "Y", "M")
FILL = 0x3A             # the heap bytes between alleles: ':' (an over-read turns a key HOST)
KEY_STAGE_MAX = KEY_WAVE - CHUNK    # staged iff total + (g0 & 15) <= 2544
PATH_STAGE_MAX = PATH_WAVE - CHUNK  # ... <= 5616
CATEGORIES = ("empty", "aligned", "tail", "head", "inside", "cross", "general")


class Rec(NamedTuple):
    c: int                       # contig code
    pos: int                     # 0 .. 2^32 - 1
    ref: bytes
    alt: bytes
    ext: int = 0                 # 0 .. 2^64 - 1
    code: int = BIN_NONE         # bin code K7 is given for the path
    phase: Optional[int] = None  # (address of ref[0]) & 7, None: packed behind the record before
    over: int = 0                # the last `over` bytes of the record lie past the heap end


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def is_long(rec: Rec, max_len: int) -> bool:
    return len(rec.ref) + len(rec.alt) > max_len


def body_at(rec: Rec) -> int:
    """Bytes of "label:pos:"."""
    return len(LABELS[rec.c]) + 2 + len("%d" % rec.pos)


def path_text(c: int, code: int) -> bytes:
    if code == BIN_NONE or c >= N_CONTIGS:
        return b""
    return O.format_bin_path(LABELS[c], code).encode()


def expected(recs: Sequence[Rec], max_len: int, digests=None, defer: bool = False, over=None, codes=None):
    """(state[], key_bytes[], path_bytes[]) as K7 must leave them.  ``digests``: one
    32-byte row per record (None: K7 runs without); ``defer``: long keys laid out
    pending (their digest bytes are zeros here); ``over[i]``: record i reaches past the
    heap end (default: ``rec.over``); ``codes``: the bin codes K7 was given (default:
    ``rec.code``)."""
    state, keys, paths = [], [], []
    for i, rec in enumerate(recs):
        code = rec.code if codes is None else int(codes[i])
        paths.append(path_text(rec.c, code))
        if rec.c >= N_CONTIGS or rec.ext >> 63:
            state.append(KEY_HOST)
            keys.append(b"")
            continue
        head = b"%s:%d:" % (LABELS[rec.c].encode(), rec.pos)
        tail = b":rs%d" % rec.ext if rec.ext else b""
        if is_long(rec, max_len):
            if digests is not None:
                state.append(KEY_OK)
                keys.append(head + bytes(digests[i]) + tail)
            elif defer:
                state.append(KEY_DIGEST_PENDING)
                keys.append(head + bytes(DIGEST_CHARS) + tail)
            else:
                state.append(KEY_NEED_DIGEST)
                keys.append(b"")
            continue
        past = bool(rec.over) if over is None else bool(over[i])
        bad = any(x == 0x3A or x >= 0x80 for x in rec.ref + rec.alt)
        state.append(KEY_HOST if past or bad else KEY_OK)
        keys.append(head + rec.ref + b":" + rec.alt + tail)
    return state, keys, paths


def exemptions(recs: Sequence[Rec], state: Sequence[int], keys: Sequence[bytes]):
    """Per record the (lo, hi) byte range of its key span that is not compared: the whole
    span of a KEY_HOST record that has one, the 32 digest bytes of a pending key."""
    out = []
    for rec, st, k in zip(recs, state, keys):
        if st == KEY_HOST and k:
            out.append((0, len(k)))
        elif st == KEY_DIGEST_PENDING:
            out.append((body_at(rec), body_at(rec) + DIGEST_CHARS))
        else:
            out.append(None)
    return out


def exempt_share(recs, state, keys) -> Tuple[float, float]:
    """(share of the records, share of the key bytes) that `exemptions` waives."""
    ex = exemptions(recs, state, keys)
    n_ex = sum(1 for e in ex if e)
    b_ex = sum(e[1] - e[0] for e in ex if e)
    return n_ex / max(1, len(recs)), b_ex / max(1, sum(len(k) for k in keys))


def digest_rows(n: int, seed: int = 7) -> np.ndarray:
    """uint8[n, 32] of base64url characters: what K4 would hand K7 (any text will do)."""
    rng = np.random.default_rng(seed)
    return np.frombuffer(B64URL, dtype=np.uint8)[rng.integers(0, 64, (n, DIGEST_CHARS))].copy()


# ---------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------
@dataclass
class Batch:
    recs: Tuple[Rec, ...]
    chrom: np.ndarray       # uint8
    pos: np.ndarray         # int32 (the uint32 bits)
    allele_off: np.ndarray  # int64
    ref_len: np.ndarray     # int32
    alt_len: np.ndarray     # int32
    heap: np.ndarray        # uint8, exactly heap_bytes
    ext_id: np.ndarray      # int64 (the uint64 bits)
    code: np.ndarray        # int32 (the uint32 bits)
    over: np.ndarray        # bool: off + r + a > heap_bytes
    heap_shift: int         # the heap's address & 7 on the device

    @property
    def n(self) -> int:
        return len(self.recs)

    @property
    def heap_bytes(self) -> int:
        return int(self.heap.size)

    def phases(self) -> Tuple[np.ndarray, np.ndarray]:
        """(ref phase, alt phase): the address & 7 of each allele's first byte."""
        p = (self.allele_off + self.heap_shift) & 7
        return p, (p + self.ref_len) & 7


def batch(recs: Sequence[Rec], heap_shift: int = 0, pad: int = 0) -> Batch:
    """The SoA of ``recs`` from numpy arrays with every ``allele_off`` set here: a record
    with a ``phase`` starts at the next offset whose address (heap_shift + off) & 7 is
    that phase, the gap filled with ':'; the heap ends ``pad`` bytes behind the last
    allele byte (0: exactly there; an all-empty heap gets one byte).  A record with
    ``over`` (the last one) keeps that many of its bytes past the heap end."""
    recs = tuple(recs)
    n = len(recs)
    off = np.zeros(n, dtype=np.int64)
    chunks, cur = [], 0
    for i, r in enumerate(recs):
        if r.phase is not None:
            gap = (r.phase - heap_shift - cur) % 8
            chunks.append(bytes([FILL]) * gap)
            cur += gap
        off[i] = cur
        data = r.ref + r.alt
        if r.over:
            assert i == n - 1 and pad == 0 and 0 < r.over <= len(data)
            data = data[: len(data) - r.over]
        chunks.append(data)
        cur += len(data)
    heap = np.frombuffer(b"".join(chunks) + bytes([FILL]) * (pad if cur + pad else 1), dtype=np.uint8).copy()
    rl = np.array([len(r.ref) for r in recs], dtype=np.int32)
    al = np.array([len(r.alt) for r in recs], dtype=np.int32)
    return Batch(recs=recs, chrom=np.array([r.c for r in recs], dtype=np.uint8),
                 pos=np.array([r.pos for r in recs], dtype=np.uint32).view(np.int32), allele_off=off,
                 ref_len=rl, alt_len=al, heap=heap,
                 ext_id=np.array([r.ext for r in recs], dtype=np.uint64).view(np.int64),
                 code=np.array([r.code for r in recs], dtype=np.uint32).view(np.int32),
                 over=(off + rl + al) > heap.size, heap_shift=heap_shift)


def wide_lanes(b: Batch, max_len: int) -> np.ndarray:
    """`key_tile`'s `wide` per record: a short record one of whose alleles does not fit
    the 56-byte register window at its phase (m + n > 56)."""
    m1, m2 = b.phases()
    short = (b.ref_len.astype(np.int64) + b.alt_len) <= max_len
    return short & ((m1 + b.ref_len > WIN_BYTES) | (m2 + b.alt_len > WIN_BYTES))


# ---------------------------------------------------------------------------
# tiles, spans and staging (restated from key_tile / flush_span32)
# ---------------------------------------------------------------------------
def tile_spans(sizes: Sequence[int]) -> List[Tuple[int, int]]:
    """[g0, g1) of each 64-record tile of a stream whose records have these sizes."""
    out, g = [], 0
    for t in range(0, len(sizes), TILE):
        s = int(sum(sizes[t:t + TILE]))
        out.append((g, g + s))
        g += s
    return out


def span_cell(g0: int, g1: int) -> Tuple[str, int]:
    """(category, phase) of a tile's span (module docstring)."""
    p0, p1 = g0 % CHUNK, g1 % CHUNK
    if g0 == g1:
        return "empty", p0
    if p0 == 0:
        return ("aligned", 0) if p1 == 0 else ("tail", p1)
    if p1 == 0:
        return "head", p0
    f0, f1 = (g0 + CHUNK - 1) // CHUNK * CHUNK, g1 // CHUNK * CHUNK
    return ("inside" if f1 < f0 else "cross" if f1 == f0 else "general"), p0


def staged(g0: int, g1: int, wave: int) -> bool:
    """`kst` / `pst`: the span, from its 16-aligned start, and one more chunk fit the image."""
    return g1 - (g0 // CHUNK * CHUNK) + CHUNK <= wave


def feasible_cells(totals: Sequence[int]) -> set:
    """Every (category, phase) a tile with one of these totals can have."""
    return {span_cell(p, p + t) for p in range(CHUNK) for t in totals}


def stream_info(sizes: Sequence[int], wave: int) -> Dict:
    spans = tile_spans(sizes)
    return {"spans": spans, "cells": {span_cell(*s) for s in spans},
            "staged": [(s[0] % CHUNK, s[1] - s[0], staged(s[0], s[1], wave)) for s in spans]}


# ---------------------------------------------------------------------------
# small pieces
# ---------------------------------------------------------------------------
def make_code(level: int, l1: int, low: int = 0) -> int:
    """A fabricated bin code of ``level`` whose L1 bin number is ``l1 + 1``."""
    if level == 0:
        return 0
    return (level << 28) | (l1 << (level - 1)) | (low & ((1 << (level - 1)) - 1))


def leaf_code(pos: int) -> int:
    return (13 << 28) | (max(pos, 1) - 1) // 15625


def small_key(size: int, rng, lab: int = 0) -> Rec:
    """A clean short record on a one-character contig whose key has ``size`` >= 5 bytes."""
    assert size >= 5
    ext = int(rng.integers(1, 10)) if size >= 11 and rng.integers(0, 2) else 0
    body = size - 5 - (4 if ext else 0)
    r = int(rng.integers(0, body + 1))
    return Rec(lab % 9, int(rng.integers(0, 10)), bases(rng, r), bases(rng, body - r), ext)


def _empty(k: int) -> Rec:
    """A record with an empty key span and no path: unlabelled, or interned id + BIN_NONE."""
    if k % 2:
        return Rec(25 + k % 7, 100 + k, b"A", b"C", k % 5, leaf_code(100 + k))
    return Rec(k % N_CONTIGS, 100 + k, b"G", b"T", INTERNED | k)


@functools.lru_cache(maxsize=None)
def _path_pieces() -> Dict[int, Tuple[Tuple[int, int, int], ...]]:
    """total -> the fewest (contig, level, l1) pieces (at most 3) whose paths add up to it;
    one- and two-character labels, levels 0..13, L1 bins B1 and B10."""
    single = {}
    for c in (0, 9):
        for level in range(14):
            for l1 in ((0, 9) if level else (0,)):
                single.setdefault(len(path_text(c, make_code(level, l1))), (c, level, l1))
    best: Dict[int, Tuple] = {0: ()}
    for _ in range(3):
        for t, ps in list(best.items()):
            for s, p in single.items():
                if t + s not in best or len(best[t + s]) > len(ps) + 1:
                    best[t + s] = ps + (p,)
    return best


def _split_key(total: int) -> List[int]:
    """A key total as 1..3 key sizes of at least 5."""
    if total == 0:
        return []
    if total < 10:
        return [total]
    if total < 15:
        return [5, total - 5]
    a = 5 + (total - 15) // 3
    return [a, 5, total - 5 - a]


def _sparse_tile(k_total: int, p_total: int, rng, t: int) -> List[Rec]:
    """64 records, all with empty spans but 0..3 small live keys adding up to ``k_total``
    and 0..3 paths adding up to ``p_total``, on lanes of their own."""
    ks, ps = _split_key(k_total), _path_pieces()[p_total]
    lanes = [int(x) for x in rng.choice(TILE, size=len(ks) + len(ps), replace=False)]
    recs = [_empty(TILE * t + j) for j in range(TILE)]
    for lane, size in zip(lanes, ks):
        recs[lane] = small_key(size, rng, lane)  # (code BIN_NONE: no path)
    for lane, (c, level, l1) in zip(lanes[len(ks):], ps):
        recs[lane] = Rec(c, 7 + lane, b"T", b"G", INTERNED | lane, make_code(level, l1, int(rng.integers(0, 1 << 12))))
    return recs


# ---------------------------------------------------------------------------
# window_cases
# ---------------------------------------------------------------------------
WIN_LENS = (0, 1, 7, 8, 9, 15, 16, 17, 41, 48, 49, 50)
WIDE_LENS = (57, 64, 100, 120)
PHASE7_PAIRS = ((50, 0), (0, 50), (49, 1), (1, 49), (25, 25), (48, 2), (49, 0))


def window_lens(max_len: int) -> Tuple[int, ...]:
    return WIN_LENS + tuple(x for x in WIDE_LENS if x <= max_len)


@functools.lru_cache(maxsize=None)
def window_cases(max_len: int):
    """Every (r, a) of `window_lens` with r + a <= max_len at every ref phase 0..7 (the alt
    phase follows: (phase + r) & 7, so every alt phase x length occurs too), PHASE7_PAIRS
    with the ref and with the alt at phase 7, long records of max_len + 1 bytes at every
    phase; shuffled, so tiles mix lengths (the window loop's wave-uniform end) and `wide`
    with windowed lanes."""
    rng = np.random.default_rng(70 + max_len)
    shapes = [(ph, r, a) for ph in range(8) for r in window_lens(max_len) for a in window_lens(max_len)
              if r + a <= max_len]
    shapes += [(7, r, a) for r, a in PHASE7_PAIRS] + [((7 - r) % 8, r, a) for r, a in PHASE7_PAIRS]
    shapes += [(ph, max_len + 1 - k, k) for ph in range(8) for k in (0, 1, 25)]
    recs = []
    for i, (ph, r, a) in enumerate(shapes):
        pos = 1000 + 7919 * i
        recs.append(Rec(i % N_CONTIGS, pos, bases(rng, r), bases(rng, a), (i + 1) * 37 if i % 3 == 0 else 0,
                        leaf_code(pos), ph))
    recs = tuple(recs[int(i)] for i in rng.permutation(len(recs)))
    b = batch(recs)
    m1, m2 = b.phases()
    short = np.array([not is_long(r, max_len) for r in recs])
    wide = wide_lanes(b, max_len)
    mixed = [t for t in range(0, len(recs), TILE)
             if (wide[t:t + TILE] & short[t:t + TILE]).any() and (~wide[t:t + TILE] & short[t:t + TILE]).any()]
    info = {"ref_cells": {(int(m1[i]), len(r.ref)) for i, r in enumerate(recs) if short[i]},
            "alt_cells": {(int(m2[i]), len(r.alt)) for i, r in enumerate(recs) if short[i]},
            "pairs_at_7": {(len(r.ref), len(r.alt)) for i, r in enumerate(recs) if short[i] and m1[i] == 7},
            "pairs_alt_at_7": {(len(r.ref), len(r.alt)) for i, r in enumerate(recs) if short[i] and m2[i] == 7},
            "wide": int(wide.sum()), "mixed_tiles": len(mixed),
            "wide_cells": {(int(m1[i]), len(r.ref)) for i, r in enumerate(recs) if wide[i] and m1[i] + len(r.ref) > WIN_BYTES}
            | {(int(m2[i]), len(r.alt)) for i, r in enumerate(recs) if wide[i] and m2[i] + len(r.alt) > WIN_BYTES},
            "long_phases": {int(m1[i]) for i in range(len(recs)) if not short[i]},
            # the deepest window word a windowed allele reaches (kWinWords = 7)
            "max_word": max(int((m + n + 7) // 8) for m, n, w, s in
                            list(zip(m1, b.ref_len, wide, short)) + list(zip(m2, b.alt_len, wide, short)) if s and not w)}
    return recs, info


# ---------------------------------------------------------------------------
# bad_byte_cases
# ---------------------------------------------------------------------------
BAD_BYTES = (0x3A, 0x80, 0xC3, 0xFF)
NEAR_MISS = (0x39, 0x3B, 0x7F, 0x01)
CLEAN_PER_BAD = 8


def _with(data: bytes, at: int, value: int) -> bytes:
    return data[:at] + bytes([value]) + data[at + 1:]


@functools.lru_cache(maxsize=None)
def bad_byte_cases(max_len: int):
    """':' / 0x80 / 0xC3 / 0xFF at the first byte, the last byte and the 8 byte lanes of
    one word, in ref and in alt, of a windowed allele (20 bytes at an odd phase: every
    appended word is assembled across W[j] / W[j + 1], the last one masked) and of a
    `wide` one (100 bytes under max_len 120; 50 bytes at phase 7 under 50); 8 clean
    records of the same shape after each; then the near-miss bytes at every lane of a
    word, which must stay KEY_OK."""
    rng = np.random.default_rng(80 + max_len)
    wl, other, wph = (100, 10, 5) if max_len >= 110 else (50, 0, 7)
    # (allele length, the other allele's length, the bad allele's phase, positions)
    forms = [("win", 20, 20, 3, (0, 19) + tuple(range(8, 16))),
             ("wide", wl, other, wph, (0, wl - 1) + tuple(range(wl - 10, wl - 2)))]
    recs, n_bad, bad_at = [], 0, set()
    for kind, n, m, ph, positions in forms:
        for which in ("ref", "alt"):
            for at in positions:
                for v in BAD_BYTES:
                    i = len(recs)
                    pos, c = 50_000 + 13 * i, i % N_CONTIGS
                    for k in range(1 + CLEAN_PER_BAD):
                        x, y = bases(rng, n), bases(rng, m)
                        if k == 0:
                            x = _with(x, at, v)
                        ref, alt = (x, y) if which == "ref" else (y, x)
                        # the bad allele at phase ph: an alt starts len(ref) behind the ref
                        rph = ph if which == "ref" else (ph - len(ref)) % 8
                        recs.append(Rec(c, pos + k, ref, alt, 0 if k % 2 else 400 + k, leaf_code(pos), rph))
                    n_bad += 1
                    bad_at.add((kind, which, at, v))
    n_near = 0
    for v in NEAR_MISS:
        for which in ("ref", "alt"):
            for at in range(8, 16):
                x, y = _with(bases(rng, 24), at, v), bases(rng, 9)
                ref, alt = (x, y) if which == "ref" else (y, x)
                recs.append(Rec((at + v) % N_CONTIGS, 900 + at, ref, alt, 0, leaf_code(900), 3))
                n_near += 1
    recs = tuple(recs)
    b = batch(recs)
    wide = wide_lanes(b, max_len)
    st, _, _ = expected(recs, max_len, digests=digest_rows(len(recs)))
    info = {"bad": n_bad, "bad_at": bad_at, "near_miss": n_near,
            "host": sum(1 for s in st if s == KEY_HOST),
            "wide_host": sum(1 for s, w in zip(st, wide) if s == KEY_HOST and w),
            "win_host": sum(1 for s, w in zip(st, wide) if s == KEY_HOST and not w),
            "max_gap_clean": CLEAN_PER_BAD}
    return recs, info


# ---------------------------------------------------------------------------
# prefix_suffix_cases
# ---------------------------------------------------------------------------
PS_CONTIGS = (0, 8, 9, 21, 22, 23, 24, 25, 30)
PS_POS = tuple(sorted({0, 1} | {10 ** k - 1 for k in range(1, 10)} | {10 ** k for k in range(1, 10)}
                      | {1 << 31, (1 << 32) - 1}))
PS_EXT = (0, 1, 9, 10, 10 ** 9 - 1, 10 ** 9, (1 << 32) - 1, 1 << 32, 10 ** 10, 10 ** 18, (1 << 63) - 1,
          INTERNED | 5)
PS_LONG = (61, 60)  # long under max_len 50 and 120


def _width(c: int) -> int:
    """Label bytes of contig code c, 0 for an unlabelled one."""
    return len(LABELS[c]) if c < N_CONTIGS else 0


@functools.lru_cache(maxsize=None)
def prefix_suffix_cases():
    """Every (contig, POS, ext) of PS_CONTIGS x PS_POS x PS_EXT with a 1 + 1-byte body;
    with a long (digest) body every POS and every ext on a one-character, a two-character
    and an unlabelled contig, the third value taken in turn (a pending key's 32 digest
    bytes are not compared before the fill: they stay below 1/8 of the batch's bytes)."""
    rng = np.random.default_rng(90)
    recs = []
    for c in PS_CONTIGS:
        for p in PS_POS:
            for e in PS_EXT:
                k = int(rng.integers(0, 4))
                recs.append(Rec(c, p, b"ACGT"[k:k + 1], b"CGTA"[k:k + 1], e, leaf_code(p)))
    lr, la = PS_LONG
    # (PS_CONTIGS[0::2] and [1::2] each hold one- and two-character labels and an unlabelled contig)
    for j, p in enumerate(PS_POS):
        for c in PS_CONTIGS[j % 2::2]:
            recs.append(Rec(c, p, bases(rng, lr), bases(rng, la), PS_EXT[(j + c) % len(PS_EXT)], leaf_code(p)))
    for j, e in enumerate(PS_EXT):
        for c in PS_CONTIGS[(j + 1) % 2::2]:
            recs.append(Rec(c, PS_POS[(3 * j + c) % len(PS_POS)], bases(rng, lr), bases(rng, la), e, leaf_code(77)))
    recs = tuple(recs[int(i)] for i in rng.permutation(len(recs)))
    info = {"short": {(r.c, r.pos, r.ext) for r in recs if len(r.ref) == 1},
            "long_pos": {(_width(r.c), r.pos) for r in recs if len(r.ref) == lr},
            "long_ext": {(_width(r.c), r.ext) for r in recs if len(r.ref) == lr},
            "long_contigs": {r.c for r in recs if len(r.ref) == lr},
            "pos_digits": {len("%d" % r.pos) for r in recs},
            "ext_digits": {len("%d" % r.ext) for r in recs if r.ext and not r.ext >> 63},
            # "label:pos:" of a two-character label and a 10-digit POS: the second ':' at byte 13
            "colon_at": {body_at(r) - 1 for r in recs if r.c < N_CONTIGS}}
    return recs, info


# ---------------------------------------------------------------------------
# threshold_tiles
# ---------------------------------------------------------------------------
KEY_SWEEP = tuple(range(2520, 2571))
PATH_SWEEP = tuple(range(5590, 5633))


def _key_tile_of(total: int, rng, t: int) -> List[Rec]:
    """64 clean short records whose keys add up to ``total`` (bodies of about 31 bytes)."""
    fixed = []
    for j in range(TILE):
        c, pos = (0, 9, 22, 12)[(j + t) % 4], (5, 42, 777, 1234567)[(j // 4 + t) % 4]
        ext = 31 if j % 8 == 3 else 0
        fixed.append((c, pos, ext, len(LABELS[c]) + len("%d" % pos) + 3 + (5 if ext else 0)))
    body = total - sum(f[3] for f in fixed)
    recs = []
    for j, (c, pos, ext, _) in enumerate(fixed):
        n = body // TILE + (1 if j < body % TILE else 0)
        assert 0 <= n <= 50
        r = int(rng.integers(0, n + 1))
        recs.append(Rec(c, pos, bases(rng, r), bases(rng, n - r), ext))
    return recs


def _path_tile_of(n88: int, rng, t: int) -> List[Rec]:
    """64 records on two-character contigs with level-13 paths: ``n88`` of 88 bytes (L1 bins
    B10..B12), the others of 87 (B1..B9); a small key each."""
    lanes = set(int(x) for x in rng.choice(TILE, size=n88, replace=False))
    recs = []
    for j in range(TILE):
        l1 = 9 + (j + t) % 3 if j in lanes else (j + t) % 9
        recs.append(Rec(9 + (j + t) % 13, 3 + j, b"A", b"ACGT"[1 + j % 3:2 + j % 3], 0,
                        make_code(13, l1, int(rng.integers(0, 1 << 12)))))
    return recs


@functools.lru_cache(maxsize=None)
def threshold_tiles():
    """64-record tiles on both sides of both staging thresholds.  Keys: every total
    2520..2570, and at every start phase p the last staged total (2544 - p) and the first
    direct one (2545 - p); before each a sparse staged tile whose total brings the running
    offset to the wanted phase.  Paths: the same around 5616 - p with totals 5590..5632
    (64 paths of 87 or 88 bytes).  A wave that renders the tiles in order (grid 1) goes
    staged -> direct -> staged over one LDS image, in both streams."""
    rng = np.random.default_rng(100)
    pieces = _path_pieces()
    key_targets = [(i % CHUNK, k) for i, k in enumerate(KEY_SWEEP)]
    key_targets += [(p, KEY_STAGE_MAX - p + d) for p in range(CHUNK) for d in (0, 1)]
    path_targets = [((5 * i) % CHUNK, k) for i, k in enumerate(PATH_SWEEP)]
    path_targets += [(p, PATH_STAGE_MAX - p + d) for p in range(CHUNK) for d in (0, 1)]
    recs: List[Rec] = []
    ko = po = 0
    t = 0
    for p, total in key_targets:
        f = (p - ko) % CHUNK + CHUNK  # 16..31 bytes: a staged tile of two or three keys
        recs += _sparse_tile(f, 0, rng, t)
        recs += _key_tile_of(total, rng, t)
        ko += f + total
        t += 2
    for p, total in path_targets:
        f = next(x for x in range((p - po) % CHUNK or CHUNK, 200, CHUNK) if x in pieces)
        recs += _sparse_tile(0, f, rng, t)
        recs += _path_tile_of(total - 64 * 87, rng, t)
        po += f + total
        t += 2
    recs = tuple(recs)
    _, keys, paths = expected(recs, 50)
    info = {"keys": stream_info([len(k) for k in keys], KEY_WAVE),
            "paths": stream_info([len(p) for p in paths], PATH_WAVE)}
    return recs, info


# ---------------------------------------------------------------------------
# flush_tiles
# ---------------------------------------------------------------------------
FLUSH_KEY_TOTALS = (0,) + tuple(range(5, 41))


def flush_path_totals() -> Tuple[int, ...]:
    return tuple(sorted(t for t in _path_pieces() if t <= 104))


def _steer(need: set, phase: int, totals: Sequence[int], turn: int) -> int:
    """The next tile's total: one that fills a needed cell at this phase (taken in turn),
    else one that leads to a phase where a needed cell can be filled."""
    hit = [t for t in totals if span_cell(phase, phase + t) in need]
    if hit:
        return hit[turn % len(hit)]
    for t in totals[1:]:
        nxt = (phase + t) % CHUNK
        if any(span_cell(nxt, nxt + u) in need for u in totals):
            return t
    raise AssertionError("no total leads to a needed cell")


@functools.lru_cache(maxsize=None)
def flush_tiles():
    """Sparse 64-record tiles (0..3 small live keys, 0..3 short paths, every other record
    with empty spans) whose totals are steered so that each stream meets every feasible
    (category, phase) cell of `flush_span32`; an all-empty tile first, last and wherever
    the `empty` cells ask for one."""
    rng = np.random.default_rng(110)
    kt, pt = FLUSH_KEY_TOTALS, flush_path_totals()
    need_k, need_p = feasible_cells(kt), feasible_cells(pt)
    plan = [(0, 0)]
    ko = po = 0
    while need_k or need_p:
        assert len(plan) < 2000
        k = _steer(need_k, ko % CHUNK, kt, len(plan)) if need_k else kt[len(plan) % len(kt)]
        p = _steer(need_p, po % CHUNK, pt, len(plan)) if need_p else pt[len(plan) % len(pt)]
        need_k.discard(span_cell(ko, ko + k))
        need_p.discard(span_cell(po, po + p))
        plan.append((k, p))
        ko, po = ko + k, po + p
    for k in sorted(set(kt) - {x for x, _ in plan}):  # every key total 0, 5..40 at least once
        plan.append((k, pt[len(plan) % len(pt)]))
    plan.append((0, 0))  # (an all-empty last tile)
    recs: List[Rec] = []
    for t, (k, p) in enumerate(plan):
        recs += _sparse_tile(k, p, rng, t)
    recs = tuple(recs)
    _, keys, paths = expected(recs, 50)
    info = {"keys": stream_info([len(k) for k in keys], KEY_WAVE),
            "paths": stream_info([len(p) for p in paths], PATH_WAVE),
            "plan": plan, "levels": {r.code >> 28 for r in recs if r.code != BIN_NONE and r.c < N_CONTIGS}}
    return recs, info


# ---------------------------------------------------------------------------
# heap_edge_cases
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def heap_edge_cases():
    """Batches (records, heap_shift) whose heap is exactly their allele bytes: for every
    shift 0..7 one of 70 packed records (the first at heap byte 0, the last ending the
    heap, heap_bytes % 8 in 1..7) and one whose whole heap is shorter than 56 bytes; for
    shifts 0 and 5 one whose last record's final byte lies past the heap end (KEY_HOST)."""
    rng = np.random.default_rng(120)
    out = []

    def packed(n, last_mod):
        recs = []
        for j in range(n):
            r, a = int(rng.integers(0, 22)), int(rng.integers(0, 22))
            recs.append(Rec(j % N_CONTIGS, 10 + 977 * j, bases(rng, r), bases(rng, a), j % 4 * 11, leaf_code(10 + 977 * j)))
        used = sum(len(x.ref) + len(x.alt) for x in recs)
        last = recs[-1]
        grow = (last_mod - used) % 8
        recs[-1] = last._replace(alt=last.alt + bases(rng, grow + 8)[:grow])
        return recs

    for shift in range(8):
        out.append((tuple(packed(70, shift % 7 + 1)), shift))
    for shift in range(8):
        recs = [Rec(shift, 5 + shift, bases(rng, 3 + shift), bases(rng, 9), 0, leaf_code(5)),
                Rec(9 + shift, 123456, b"", bases(rng, 17 - shift), 3, leaf_code(123456)),
                Rec(22, 99, bases(rng, 11), b"", 0, leaf_code(99))]
        out.append((tuple(recs), shift))
    for shift in (0, 5):
        recs = packed(70, 3)
        recs[-1] = recs[-1]._replace(ref=bases(rng, 4), alt=bases(rng, 2), over=1)
        out.append((tuple(recs), shift))
    return tuple(out)


# ---------------------------------------------------------------------------
# the repeated pattern of the 256-record-group test
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pattern_records():
    """Every builder's records at max_len 50 behind one another (the heap-edge batches
    apart: their subject is the heap's end), trimmed so that the count is no multiple of
    256 and the heap length is odd."""
    recs = list(window_cases(50)[0] + bad_byte_cases(50)[0] + prefix_suffix_cases()[0] + threshold_tiles()[0]
                + flush_tiles()[0])
    while len(recs) % 256 == 0 or batch(recs).heap_bytes % 2 == 0:
        recs.pop()
    return tuple(recs)

"""K4 (long-allele VRS digest) at the edges random batches do not reach: builders of the
records and a restatement of the kernel's block arithmetic (shared by
test_k4_common_host.py and test_gpu_k4_edges.py).

Restated from csrc/avdb_internal.hpp (``long_bucket``) and csrc/avdb_digest.hip
(``sha_blocks``, ``allele_blocks``, ``ndigits``):

* the VRS Allele message is ``AL0 + <32 location digest chars> + AL1 + ALT + AL2``:
  68 bytes before the ALT and 54 after, 122 fixed bytes; SHA-512 padding adds one 0x80
  byte and a 16-byte length, 17 bytes, and a block holds 128, so an ``a``-byte ALT takes
  ``(122 + a + 17 + 127) // 128`` compressions;
* the compaction groups long records by that count in 32 buckets, the last of which
  (31) takes every larger count: ALTs from 3,702 bytes up share it;
* block 1 of the SequenceLocation message is read from a per-(contig, nE + nS) table,
  nE and nS the decimal digit counts of the interval's end and start, 2..20 in all.

The expected digests come from ``hashlib`` through the oracle's serialiser
(``O.vrs_allele_digest``), never from K4.  Nothing here proves the restatement matches
the device: the GPU tests do, by comparing digests at the lengths on both sides of
every boundary these functions name.
"""

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import avdb_oracle as O

AL_FIXED_BYTES = 122    # Allele message bytes around the ALT (68 before, 54 after)
SHA_PAD_BYTES = 17      # 0x80 and the 128-bit message length
CLAMP_BUCKET = 31       # kLongBuckets - 1: every block count >= 31
N_CONTIGS = 25          # labelled contigs (chromosomes.CHROM_NAMES); codes from 25 up get '?' * 32
MAX_LEN = 50            # maxSequenceLength of the tests: ref + alt above it is a long record
REF_LEN = 60            # REF of every ALT-length case: long for any ALT, a = 0 included
U32_MAX = (1 << 32) - 1
DIGIT_SUMS = tuple(range(2, 21))
B64URL = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_"
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

Record = Tuple[int, int, bytes, bytes]  # (chrom code, pos, ref, alt)


def blocks(a: int) -> int:
    """SHA-512 compressions of the Allele message of an ``a``-byte ALT."""
    return (AL_FIXED_BYTES + a + SHA_PAD_BYTES + 127) // 128


def bucket(a: int) -> int:
    return min(blocks(a), CLAMP_BUCKET)


def ndigits(x: int) -> int:
    return len("%d" % x)


def digit_sum(rec: Record) -> int:
    """nE + nS of the record's interbase interval (pos - 1, pos - 1 + len(ref)]."""
    s = rec[1] - 1
    return ndigits(s) + ndigits(s + len(rec[2]))


def is_long(rec: Record, max_len: int = MAX_LEN) -> bool:
    return len(rec[2]) + len(rec[3]) > max_len


def expected(digests: Sequence[str], recs: Sequence[Record], max_len: int = MAX_LEN,
             schema: str = "1.2") -> List[Optional[bytes]]:
    """What K4 writes per record: the 32 digest characters of a long record on a labelled
    contig, 32 question marks for a long record on any other, nothing (None) for a
    short one."""
    out: List[Optional[bytes]] = []
    for c, pos, ref, alt in recs:
        if len(ref) + len(alt) <= max_len:
            out.append(None)
        elif c >= N_CONTIGS:
            out.append(b"?" * 32)
        else:
            out.append(O.vrs_allele_digest(digests[c], pos, ref, alt, schema).encode())
    return out


def _seq_digests() -> Tuple[str, ...]:
    rng = np.random.default_rng(40)
    out: List[str] = []
    while len(out) < N_CONTIGS:
        ch = bytearray(B64URL[int(k)] for k in rng.integers(0, 64, 32))
        p, q = (int(x) for x in rng.choice(32, size=2, replace=False))
        ch[p], ch[q] = ord("-"), ord("_")
        s = ch.decode()
        if s not in out:
            out.append(s)
    return tuple(out)


# one refget-style digest per contig over the whole base64url alphabet
SEQ_DIGESTS = _seq_digests()


def bases(rng, n: int) -> bytes:
    """``n`` seeded ACGT bytes, none equal to the one before it: reading a byte too far
    or one byte off always reads another value."""
    if n == 0:
        return b""
    steps = np.concatenate(([int(rng.integers(0, 4))], rng.integers(1, 4, n - 1)))
    return ACGT[np.cumsum(steps) % 4].tobytes()


# ---- ALT lengths --------------------------------------------------------------
def alt_lengths() -> List[int]:
    """Every length 0..520 (all 128 residues, 2..5 blocks, the empty ALT); the last length
    of k blocks, ``128 k - 139``, and its neighbours for k = 3..44 (below the clamp
    bucket and through it); 10,000 and 65,537 (80 and 514 blocks)."""
    return (list(range(521)) + [128 * k - 139 + d for k in range(3, 45) for d in (-1, 0, 1)]
            + [10_000, 65_537])


@functools.lru_cache(maxsize=None)
def alt_length_records() -> Tuple[Record, ...]:
    rng = np.random.default_rng(41)
    return tuple((i % N_CONTIGS, 1000 + 37 * i, bases(rng, REF_LEN), bases(rng, a))
                 for i, a in enumerate(alt_lengths()))


# ---- positions ------------------------------------------------------------------
TOP_START = 4294967234  # with a 60-base REF the interval ends at 2^32 - 2: nE + nS = 20


def position_forms() -> Dict[int, List[Tuple[int, int]]]:
    """digit sum -> the (S, len(ref)) pairs with S in {10^k - 1, 10^k, 10^k - 30} and
    len(ref) in {1, 60}: the starts and ends around every power of ten, where nS and nE
    change, together and apart."""
    out: Dict[int, List[Tuple[int, int]]] = {}
    for k in range(10):
        for s in (10 ** k - 1, 10 ** k, 10 ** k - 30):
            for r in (1, 60):
                if s >= 0 and s + r <= U32_MAX:
                    out.setdefault(ndigits(s) + ndigits(s + r), []).append((s, r))
    out[20].append((TOP_START, 60))
    return out


@functools.lru_cache(maxsize=None)
def position_records() -> Tuple[Record, ...]:
    """For each contig one long record per digit sum 2..20, the form taken in turn from
    ``position_forms``, and one at ``TOP_START``.  pos >= 1 and the interval ends at or
    below 2^32 - 1: outside that the kernel's 32-bit arithmetic and the oracle's integers
    differ, and the result is undefined."""
    rng = np.random.default_rng(42)
    forms = position_forms()
    recs: List[Record] = []
    for c in range(N_CONTIGS):
        for ds in DIGIT_SUMS:
            s, r = forms[ds][(c + ds) % len(forms[ds])]
            # long either way: a 1-base REF takes an ALT of 50..119 bytes (2 and 3 blocks)
            a = 50 + (7 * c + 3 * ds) % 70 if r == 1 else (5 * c + ds) % 64
            recs.append((c, s + 1, bases(rng, r), bases(rng, a)))
        recs.append((c, TOP_START + 1, bases(rng, 60), bases(rng, c)))
    return tuple(recs)


# ---- the mix for the list kernels -------------------------------------------------
def _short(rng, k: int) -> Record:
    c, pos = k % N_CONTIGS, 500 + 11 * k
    if k % 3 == 0:  # SNV
        at = int(rng.integers(0, 4))
        return (c, pos, b"ACGT"[at:at + 1], b"CGTA"[at:at + 1])
    return (c, pos, bases(rng, 1 + k % 4), bases(rng, 1 + (k // 4) % 6))


@functools.lru_cache(maxsize=None)
def mix_records() -> Tuple[Record, ...]:
    """Both lists, a short record (SNV or small indel) after every second long one,
    long and short records on contig codes 25 and 200, shuffled; ``n % 4 == 3``, so the
    batch ends inside a group of four."""
    rng = np.random.default_rng(43)
    recs: List[Record] = []
    for i, rec in enumerate(alt_length_records() + position_records()):
        recs.append(rec)
        if i % 2 == 1:
            recs.append(_short(rng, i))
    recs += [(25, 12345, bases(rng, 60), bases(rng, 100)), (200, 1, bases(rng, 1), bases(rng, 300)),
             (25, TOP_START + 1, bases(rng, 60), bases(rng, 7)), (200, 99, bases(rng, 60), b""),
             (255, 1000000, bases(rng, 30), bases(rng, 4000)), (25, 77, bases(rng, 2), bases(rng, 117)),
             (25, 5, b"A", b"G"), (200, 7, b"AC", b"G")]
    while len(recs) % 4 != 3:
        recs.append(_short(rng, len(recs)))
    return tuple(recs[int(i)] for i in rng.permutation(len(recs)))

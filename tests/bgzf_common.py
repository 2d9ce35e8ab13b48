"""Shared by test_bgzf_host.py and test_gpu_bgzf.py: BGZF framing around Python's own
``zlib`` (the oracle is ``zlib`` / ``gzip``; no htslib), a small deflate bit reader
that reports what each fixture really contains (block types, longest code), the
fixture chain, and the corrupt members with the status each must get."""

import gzip
import random
import struct
import zlib

import numpy as np

from annotatedvdb_amd import _native as N

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


# ---- framing ---------------------------------------------------------------------
def raw_deflate(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def frame(raw: bytes, data: bytes = None, *, crc=None, isize=None, extra_before=b"", extra_after=b"",
          bsize=None) -> bytes:
    """One BGZF member around a raw deflate stream; ``crc`` / ``isize`` / ``bsize``
    override what the member states."""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    xlen = len(extra_before) + 6 + len(extra_after)
    total = 12 + xlen + len(raw) + 8
    bs = total - 1 if bsize is None else bsize
    hdr = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + extra_before + b"BC" + \
        struct.pack("<HH", 2, bs) + extra_after
    return hdr + raw + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def member(data: bytes, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, **kw) -> bytes:
    m = frame(raw_deflate(data, level, strategy, flush_at), data, **kw)
    assert len(m) <= 65536, len(m)
    return m


def bgzip(data: bytes, block=65280, level=6, eof=True) -> bytes:
    """``data`` as bgzip writes it: members of ``block`` input bytes, then the EOF member."""
    out = [member(data[i:i + block], level) for i in range(0, len(data), block)]
    return b"".join(out) + (EOF_MEMBER if eof else b"")


def walk(chain: bytes):
    """The helper's own framing walk: ``(in_off, out_off, consumed, out_bytes)`` over
    the complete members of ``chain``."""
    in_off, out_off, at, total = [], [0], 0, 0
    while at + 18 <= len(chain):
        assert chain[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", chain, at + 10)[0]
        if at + 12 + xlen > len(chain):
            break
        q, bsize = at + 12, None
        while q < at + 12 + xlen:
            si, slen = chain[q:q + 2], struct.unpack_from("<H", chain, q + 2)[0]
            if si == b"BC" and bsize is None:
                bsize = struct.unpack_from("<H", chain, q + 4)[0]
            q += 4 + slen
        if at + bsize + 1 > len(chain):
            break
        in_off.append(at)
        total += struct.unpack_from("<I", chain, at + bsize - 3)[0]
        out_off.append(total)
        at += bsize + 1
    return in_off, out_off, at, total


def deflate_of(m: bytes) -> bytes:
    """The raw deflate stream of one member."""
    xlen = struct.unpack_from("<H", m, 10)[0]
    return m[12 + xlen:len(m) - 8]


# ---- what a deflate stream contains -------------------------------------------------
class _Bits:
    def __init__(self, raw):
        self.raw, self.pos = raw, 0

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.raw[self.pos >> 3] >> (self.pos & 7)) & 1) << k
            self.pos += 1
        return v


def _codes(lens):
    """{(length, code): symbol} of a canonical code."""
    out, code = {}, 0
    for l in range(1, 16):
        for s, x in enumerate(lens):
            if x == l:
                out[(l, code)] = s
                code += 1
        code <<= 1
    return out


def _symbol(b, codes):
    code = 0
    for l in range(1, 16):
        code = code << 1 | b.take(1)
        if (l, code) in codes:
            return codes[(l, code)]
    raise ValueError("no code")


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
_FIXED = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8


def deflate_blocks(raw: bytes):
    """``[(btype, longest code length, [(length, distance)] of its matches, stored bytes)]``
    per deflate block of a valid stream."""
    b, out = _Bits(raw), []
    while True:
        final, btype = b.take(1), b.take(2)
        maxlen, matches, stored = 0, [], 0
        if btype == 0:
            b.pos = (b.pos + 7) & ~7
            stored = b.take(16)
            assert b.take(16) == stored ^ 0xFFFF
            b.pos += 8 * stored
        else:
            if btype == 1:
                lit, dist = _codes(_FIXED), _codes([5] * 30)
            else:
                nlit, ndist, ncl = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for k in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[:ncl]:
                    cl[k] = b.take(3)
                clc, lens = _codes(cl), []
                while len(lens) < nlit + ndist:
                    s = _symbol(b, clc)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + b.take(2))
                    else:
                        lens += [0] * ((3 + b.take(3)) if s == 17 else (11 + b.take(7)))
                maxlen = max(lens)
                lit, dist = _codes(lens[:nlit]), _codes(lens[nlit:])
            while True:
                s = _symbol(b, lit)
                if s == 256:
                    break
                if s > 256:
                    ln = _LBASE[s - 257] + b.take(_LEXT[s - 257])
                    d = _symbol(b, dist)
                    matches.append((ln, _DBASE[d] + b.take(_DEXT[d])))
        out.append((btype, maxlen, matches, stored))
        if final:
            return out


# ---- fixtures ------------------------------------------------------------------------
_cache = {}


def vcf_text(n_bytes: int) -> bytes:
    from annotatedvdb_amd import synth
    if "vcf" not in _cache:
        _cache["vcf"] = synth.vcf_text(1500, seed=11)
    t = _cache["vcf"]
    assert len(t) >= n_bytes
    return t[:n_bytes]


def fib_text() -> bytes:
    """Byte frequencies 1, 1, 2, 3, 5, ...: a Huffman code as deep as its alphabet, which
    zlib then limits to 15 bits."""
    f, data = [1, 1], bytearray()
    while len(f) < 22:
        f.append(f[-1] + f[-2])
    for k, n in enumerate(f):
        data += bytes([65 + k]) * n
    random.Random(3).shuffle(data)
    return bytes(data)


def fixtures():
    """``[(name, data, member)]``, in chain order."""
    if "fx" in _cache:
        return _cache["fx"]
    rng = random.Random(7)
    rnd60k = bytes(rng.getrandbits(8) for _ in range(60000))
    rnd32k = bytes(rng.randrange(64) for _ in range(32000))
    vcf = vcf_text(65280)
    fx = [
        ("vcf", vcf, member(vcf)),
        ("fixed", vcf[:300], member(vcf[:300], 6, zlib.Z_FIXED)),
        ("level0", vcf[:5000], member(vcf[:5000], 0)),
        ("stored_big", rnd60k, member(rnd60k, 6, zlib.Z_HUFFMAN_ONLY)),
        ("full_flush", vcf[:40000], member(vcf[:40000], 6, flush_at=17001)),
        ("run", b"A" * 65536, member(b"A" * 65536)),
        ("eof_mid", b"", EOF_MEMBER),
        ("fib", fib_text(), member(fib_text(), 6, zlib.Z_HUFFMAN_ONLY)),
        ("period3", b"xyz" * 100 + b"q", member(b"xyz" * 100 + b"q")),
        ("period7", b"abcdefg" * 60, member(b"abcdefg" * 60)),
        ("far", rnd32k + rnd32k[:1000], member(rnd32k + rnd32k[:1000], 9)),
        ("one", b"\n", member(b"\n")),
        ("two", b"ab", member(b"ab")),
        ("seven", b"1234567", member(b"1234567")),
        ("extra", vcf[300:900], member(vcf[300:900], extra_before=b"XY\x03\x00abc", extra_after=b"ZZ\x00\x00")),
        ("tail", vcf[1000:3001], member(vcf[1000:3001])),
        ("eof", b"", EOF_MEMBER),
    ]
    _cache["fx"] = fx
    return fx


def chain():
    """``(compressed chain, its text)`` of all fixtures."""
    fx = fixtures()
    return b"".join(m for _, _, m in fx), b"".join(d for _, d, _ in fx)


# ---- corrupt members --------------------------------------------------------------------
class _W:
    """Deflate bits, LSB first."""

    def __init__(self):
        self.bits = []

    def put(self, v, n):
        self.bits += [(v >> k) & 1 for k in range(n)]
        return self

    def code(self, code, n):  # a Huffman code: first bit highest
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def _fixed_lit(w, byte):
    return w.code(0x30 + byte, 8) if byte < 144 else w.code(0x190 + byte - 144, 9)


def _dyn_header(w, cl_lens, nlit=257, ndist=1):
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    w.put(1, 1).put(2, 2).put(nlit - 257, 5).put(ndist - 1, 5).put(19 - 4, 4)
    for k in order:
        w.put(cl_lens.get(k, 0), 3)
    return w


def corrupt_members():
    """``[(name, member, status)]``: each member alone is refused by ``gzip.decompress``
    (the callers check that), and must get ``status`` from K11 (None: the index refuses
    or stops, see the tests)."""
    good = b"0123456789" * 3
    out = []
    out.append(("btype3", frame(_W().put(1, 1).put(3, 2).bytes(), b""), N.BGZF_BAD_BTYPE))
    # HLIT field 30: 287 literal/length codes
    w = _dyn_header(_W(), {0: 1, 8: 1}, nlit=287)
    out.append(("hlit287", frame(w.bytes() + b"\0" * 40, b""), N.BGZF_BAD_LENS))
    # code-length code {1: len 1, 2: len 1}; three literal/length codes of length 1: over-subscribed
    # (code-length code: symbol 0 is '0', symbol 1 is '1'; literals 0, 1 and 256 get length 1)
    w = _dyn_header(_W(), {1: 1, 0: 1})
    w.code(1, 1).code(1, 1)
    for _ in range(254):
        w.code(0, 1)
    w.code(1, 1).code(0, 1)
    out.append(("oversubscribed", frame(w.bytes() + b"\0" * 8, b""), N.BGZF_BAD_LENS))
    # the first length symbol is a repeat (16) with nothing before it
    w = _dyn_header(_W(), {16: 1, 0: 1})  # (symbol 0 is '0', symbol 16 is '1')
    w.code(1, 1).put(0, 2)
    out.append(("repeat_first", frame(w.bytes() + b"\0" * 8, b""), N.BGZF_BAD_LENS))
    # fixed block: 'a', then a match of length 3 at distance 2
    w = _fixed_lit(_W().put(1, 1).put(1, 2), 97).code(1, 7).code(1, 5).code(0, 7)
    out.append(("dist_far", frame(w.bytes(), b"aaaa"), N.BGZF_DIST_FAR))
    raw = raw_deflate(good)
    out.append(("out_long", frame(raw, good, isize=len(good) - 1), N.BGZF_OUT_LONG))
    out.append(("out_short", frame(raw, good, isize=len(good) + 1), N.BGZF_OUT_SHORT))
    out.append(("stored_len", frame(b"\x01\x05\x00\xfa\xfe" + b"hello", b"hello"), N.BGZF_BAD_STORED))
    vcf = vcf_text(3000)
    raw = raw_deflate(vcf)
    out.append(("truncated", frame(raw[:len(raw) // 2], vcf), None))  # (BSIZE is the shorter member's)
    out.append(("crc", frame(raw, vcf, crc=zlib.crc32(vcf) ^ 0x00010000), N.BGZF_BAD_CRC))
    return out


def python_refuses(m: bytes) -> bool:
    try:
        gzip.decompress(m)
    except (OSError, EOFError, zlib.error):
        return True
    return False


def in_chain(bad: bytes):
    """A corrupt member between good neighbours: ``(chain, index of the bad member,
    [text of member k or None])``."""
    fx = fixtures()
    a, b = fx[1], fx[9]
    return a[2] + bad + b[2] + EOF_MEMBER, 1, [a[1], None, b[1], b""]


def as_u8(data: bytes) -> np.ndarray:
    return np.frombuffer(data, dtype=np.uint8)

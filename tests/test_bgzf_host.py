"""K11 (BGZF index + DEFLATE decoder) through the library's host entries
(avdb_bgzf_index_host / avdb_bgzf_inflate_host on an avdb_ctx_create(-1, ...) context):
the same per-member code the kernel runs, checked against Python's own zlib / gzip.
No GPU."""

import gzip
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
import torch

import bgzf_common as B
import cadd_common as C
from conftest import ROOT
from annotatedvdb_amd import _native as N
from annotatedvdb_amd import bgzf
from annotatedvdb_amd.cadd import CaddTable
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.load_vcf_file import iter_batches, read_text


@pytest.fixture(scope="module")
def host():
    eng = Engine("host")
    eng.poison = 0xA5
    return eng


def text_of(t) -> bytes:
    return t.cpu().numpy().tobytes()


def test_fixtures_cover_what_they_claim():
    """Block types, code lengths and match shapes of the fixture members, read back
    with the helper's own bit reader."""
    blocks = {name: B.deflate_blocks(B.deflate_of(m)) for name, _, m in B.fixtures()}
    types = {name: [b[0] for b in bl] for name, bl in blocks.items()}
    assert types["vcf"] == [2] and len(B.fixtures()[0][1]) == 65280
    assert types["fixed"] == [1]
    assert types["level0"] == [0]
    assert set(types["stored_big"]) == {0} and len(B.fixtures()[3][2]) == 60036
    assert types["full_flush"] == [2, 0, 2] and blocks["full_flush"][1][3] == 0
    assert (258, 1) in blocks["run"][0][2] and len(B.fixtures()[5][1]) == 65536
    assert B.fixtures()[6][2] == B.EOF_MEMBER == B.fixtures()[-1][2] and len(B.EOF_MEMBER) == 28
    assert max(b[1] for b in blocks["fib"]) == 15
    assert any(ln > d == 3 for b in blocks["period3"] for ln, d in b[2])
    assert any(ln > d == 7 for b in blocks["period7"] for ln, d in b[2])
    assert any(d >= 30000 for b in blocks["far"] for _, d in b[2])
    assert [len(B.fixtures()[k][1]) for k in (11, 12, 13)] == [1, 2, 7]
    assert B.fixtures()[14][2][12:14] == b"XY"  # another subfield ahead of BC
    in_off = B.walk(B.chain()[0])[0]
    assert any(o % 8 for o in in_off) and len({o % 8 for o in in_off}) >= 4
    chain, text = B.chain()
    assert gzip.decompress(chain) == text and len(text) < (1 << 20)


def test_every_member_and_the_chain_equal_gzip(host):
    for name, data, m in B.fixtures():
        assert text_of(host.bgzf_inflate(m)) == data == gzip.decompress(m), name
    chain, text = B.chain()
    out, status, counts = host.bgzf_inflate(chain, raise_on_error=False)
    assert text_of(out) == text
    assert not status.numpy().any() and counts.tolist() == [len(B.fixtures()), 0, 2 ** 64 - 1]


def test_index_equals_the_framing_walk(host):
    chain, text = B.chain()
    in_off, out_off, consumed, total = B.walk(chain)
    ix = host.bgzf_index(chain)
    assert ix.in_off.tolist() == in_off and ix.out_off.tolist() == out_off
    assert (ix.consumed, ix.out_bytes, ix.n_blocks) == (consumed, total, len(in_off)) == (len(chain), len(text), 17)
    # cut at every byte of the last member, and at every byte of the first
    for cut in list(range(in_off[-1], len(chain))) + list(range(0, in_off[1])):
        ix = host.bgzf_index(chain[:cut])
        w = B.walk(chain[:cut])
        assert (ix.in_off.tolist(), ix.out_off.tolist(), ix.consumed, ix.out_bytes) == w, cut
    # the raw entry: a capacity below the member count stops there, to be called again
    lib = N.load_library()
    a = B.as_u8(chain)
    import ctypes
    io, oo = np.zeros(5, np.uint64), np.zeros(6, np.uint64)
    n, c, ob = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
    assert lib.avdb_bgzf_index_host(a.ctypes.data, a.size, 5, io.ctypes.data, oo.ctypes.data, ctypes.byref(n),
                                    ctypes.byref(c), ctypes.byref(ob)) == 0
    assert (n.value, c.value, ob.value) == (5, in_off[5], out_off[5]) and oo.tolist() == out_off[:6]


def test_index_refusals(host):
    chain, _ = B.chain()
    with pytest.raises(bgzf.NotBgzf):
        host.bgzf_index(gzip.compress(b"hello\n"))
    with pytest.raises(bgzf.BgzfError) as e:
        host.bgzf_index(b"hello, world, this is no gzip at all")
    assert not isinstance(e.value, bgzf.NotBgzf)
    first = B.fixtures()[1][2]
    # a malformed member later in the chain names its offset
    with pytest.raises(bgzf.BgzfError, match="offset %d" % len(first)):
        host.bgzf_index(first + gzip.compress(b"x") + first)
    # ISIZE 65537: refused by the index, as gzip refuses the member
    big = B.frame(B.raw_deflate(b"abc"), b"abc", isize=65537)
    assert B.python_refuses(big)
    with pytest.raises(bgzf.BgzfError, match="offset %d" % len(first)):
        host.bgzf_index(first + big)
    # BSIZE pointing past the buffer: the index stops there.  A member cut short (gzip
    # refuses it: EOFError), and one whose BSIZE overstates it (gzip does not read BSIZE)
    cut = B.fixtures()[9][2][:-5]
    assert B.python_refuses(cut)
    long_ = B.frame(B.raw_deflate(b"abc"), b"abc", bsize=4000)
    for tail in (cut, long_):
        ix = host.bgzf_index(first + tail)
        assert (ix.n_blocks, ix.consumed) == (1, len(first))
        with pytest.raises(bgzf.BgzfError, match="truncated"):
            host.bgzf_inflate(first + tail)


@pytest.mark.parametrize("name,bad,want", B.corrupt_members(), ids=[c[0] for c in B.corrupt_members()])
def test_corrupt_member_fails_alone(host, name, bad, want):
    """Python's gzip refuses the member; K11 gives it its status, decodes its neighbours,
    and leaves the sentinel everywhere outside the OK members' ranges."""
    assert B.python_refuses(bad)
    chain, k, texts = B.in_chain(bad)
    ix = host.bgzf_index(chain)
    assert ix.n_blocks == len(texts)
    out, status, counts = host.bgzf_inflate(chain, ix, raise_on_error=False)
    status, out = status.numpy(), out.numpy()
    assert [int(s) for i, s in enumerate(status) if i != k] == [0] * (len(texts) - 1)
    assert status[k] != N.BGZF_OK and (want is None or status[k] == want), (name, int(status[k]))
    assert counts.tolist() == [len(texts) - 1, 1, k]
    for i, t in enumerate(texts):
        lo, hi = int(ix.out_off[i]), int(ix.out_off[i + 1])
        if t is None:
            assert (out[lo:hi] == 0xA5).all()
        else:
            assert out[lo:hi].tobytes() == t
    with pytest.raises(bgzf.BgzfError) as e:
        host.bgzf_inflate(chain)
    assert isinstance(e.value, OSError) and (e.value.block, e.value.offset, e.value.status) == \
        (k, int(ix.in_off[k]), int(status[k]))
    assert "block %d" % k in str(e.value) and "offset %d" % int(ix.in_off[k]) in str(e.value) and \
        N.BGZF_STATUS[int(status[k])] in str(e.value)


def test_untrusted_index_is_checked(host):
    """Offsets that point outside the buffers are refused in Python, and by the library
    itself when handed to it directly."""
    import ctypes
    m = B.fixtures()[1][2]
    ix = host.bgzf_index(m)
    with pytest.raises(ValueError):
        host.bgzf_inflate(m, bgzf.BgzfIndex(ix.in_off, np.array([0, 70000], np.uint64), ix.consumed, 70000))
    with pytest.raises(ValueError):
        host.bgzf_inflate(m, bgzf.BgzfIndex(np.array([len(m)], np.uint64), ix.out_off, ix.consumed, ix.out_bytes))
    lib, a = N.load_library(), B.as_u8(m)
    out, st, cnt = np.full(300, 0xA5, np.uint8), np.zeros(1, np.uint8), np.zeros(3, np.uint64)
    for in_off, out_off, cap in (([1 << 40], [0, 300], 300), ([0], [0, 300], 299), ([0], [300, 0], 300),
                                 ([0], [0, 299], 300), ([7], [0, 300], 300), ([len(m) - 3], [0, 300], 300)):
        io, oo = np.array(in_off, np.uint64), np.array(out_off, np.uint64)
        assert lib.avdb_bgzf_inflate_host(host.ctx, a.ctypes.data, a.size, io.ctypes.data, oo.ctypes.data, 1,
                                          out.ctypes.data, cap, st.ctypes.data, cnt.ctypes.data) == 0
        assert st[0] == N.BGZF_BAD_HEADER and (out == 0xA5).all() and cnt.tolist() == [0, 1, 0]


@pytest.mark.parametrize("chunk", [7, 29, 1000, 20000, 1 << 20])
def test_iter_text_splits_members_and_lines(host, tmp_path, chunk):
    vcf = B.vcf_text(90000)[:-7]  # (no final newline)
    data = b"".join(B.member(vcf[i:i + 9000]) for i in range(0, len(vcf), 9000)) + B.EOF_MEMBER
    p = tmp_path / "x.vcf.gz"
    p.write_bytes(data)
    assert bgzf.is_bgzf(str(p))
    pieces = [text_of(t) for t in bgzf.BgzfFile(str(p), host).iter_text(chunk)]
    assert b"".join(pieces) == gzip.open(p).read() == vcf
    assert all(x.endswith(b"\n") for x in pieces[:-1]) and not pieces[-1].endswith(b"\n")
    assert len(pieces) > 1 or chunk > len(data)
    p.write_bytes(data[:-40])
    with pytest.raises(bgzf.BgzfError, match="truncated"):
        list(bgzf.BgzfFile(str(p), host).iter_text(chunk))


def test_call_sites_read_bgzf_like_the_plain_file(host, tmp_path):
    vcf = B.vcf_text(150000)
    plain, gz, single = tmp_path / "a.vcf", tmp_path / "a.vcf.gz", tmp_path / "s.vcf.gz"
    plain.write_bytes(vcf)
    gz.write_bytes(B.bgzip(vcf))
    single.write_bytes(gzip.compress(vcf))
    assert bgzf.is_bgzf(str(gz)) and not bgzf.is_bgzf(str(single)) and not bgzf.is_bgzf(str(plain))
    assert read_text(str(gz), host) == read_text(str(plain)) == read_text(str(single), host) == vcf
    for bb in (64, 4000, 1 << 20):
        blocks = list(iter_batches(str(gz), bb, host))
        assert b"".join(blocks) == b"".join(iter_batches(str(plain), bb)) == vcf
        assert all(b.endswith(b"\n") for b in blocks[:-1])
        assert b"".join(iter_batches(str(single), bb, host)) == vcf  # the gzip fallback
    # a corrupt bgzip file keeps failing, as it does under gzip.open
    bad = bytearray(B.bgzip(vcf))
    bad[len(bad) // 2] ^= 0x10
    gz.write_bytes(bytes(bad))
    with pytest.raises((OSError, zlib.error)):
        gzip.open(gz).read()
    with pytest.raises(OSError):
        read_text(str(gz), host)
    with pytest.raises(OSError):
        list(iter_batches(str(gz), 1 << 20, host))


def test_cadd_from_file_reads_bgzf(host, tmp_path):
    snv = C.golden()[0]
    gz, single = tmp_path / "snv.tsv.gz", tmp_path / "single.tsv.gz"
    gz.write_bytes(B.bgzip(snv, block=20000))
    single.write_bytes(gzip.compress(snv))
    want = C.table_columns(CaddTable.from_text(snv, host).cols)
    t = CaddTable.from_file(str(gz), engine=host)
    C.assert_same_table(C.table_columns(t.cols), want, "bgzf")
    assert t.slab() == snv
    C.assert_same_table(C.table_columns(CaddTable.from_file(str(single), engine=host).cols), want, "gzip")
    part = CaddTable.from_file(str(gz), contigs=["21"], engine=host)  # (the host filter path)
    assert 0 < len(part) < len(t)


def test_crc_of_chunk_edges(host):
    """Sizes around the 1 KiB CRC chunks and the 16-byte flush words."""
    rng = np.random.default_rng(5)
    data = rng.integers(97, 113, 70000, dtype=np.uint8).tobytes()
    sizes = [0, 1, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 4097, 65535, 65536]
    chain = b"".join(B.member(data[s:s + n], 1) for s, n in enumerate(sizes))
    assert text_of(host.bgzf_inflate(chain)) == b"".join(data[s:s + n] for s, n in enumerate(sizes))


def test_sanitizer_program(tmp_path):
    """tools/bgzf_sanitize.hip (its own main around the shared per-member decoder, built
    for the host with AddressSanitizer and UBSan) over the fixture corpus and seeded
    single-byte flips and truncations of it ends clean."""
    if torch.cuda.is_available():
        pytest.skip("sanitizer builds run on CPU-only hosts")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path / "bgzf_sanitize"
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-I", os.path.join(ROOT, "include"),
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tools", "bgzf_sanitize.hip"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr.lower() or "sanitizer" in r.stderr.lower()):
        pytest.skip("sanitizer runtime missing: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-2000:]
    corpus = tmp_path / "corpus.bgzf"
    corpus.write_bytes(B.chain()[0] + b"".join(m for _, m, _ in B.corrupt_members()))
    r = subprocess.run([str(exe), str(corpus), "10000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "clean" in r.stdout and "17 of 27 members OK" in r.stdout, r.stdout

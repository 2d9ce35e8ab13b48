"""K12 (the --skipExisting key set's columns from an export) through the library's
host entries (avdb_existing_size_host / avdb_existing_write_host on an
avdb_ctx_create(-1, ...) context): the same per-line and per-row code the kernels
run, checked against a restatement of ExistingVariants.from_tsv's parse
(existing_common.restate).  No GPU."""

import ctypes

import numpy as np
import pytest

import existing_common as X
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine

SENTINEL = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def host():
    return Engine("host")


def test_h1_every_line_class(host):
    want = X.restate(X.H1)
    # the printable rule, counted here by hand: a build that flags every row fails
    assert want["counts"]["frag_host"] == X.H1_FRAG_HOST
    assert want["counts"]["noncanon"] == X.H1_NONCANON
    assert want["counts"]["rows"] == 34 and want["counts"]["skipped"] == 6 and len(X.H1_LINES) == 40
    got = X.columns(host, X.H1)
    X.assert_same(got, want)
    assert got["counts"]["frag_host"] == X.H1_FRAG_HOST and got["counts"]["lone_cr"] == 0
    # numpy and tensor input give the same
    import torch
    arr = np.frombuffer(X.H1, dtype=np.uint8)
    X.assert_same(X.columns(host, arr), want)
    X.assert_same(X.columns(host, torch.from_numpy(arr.copy())), want)


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_h2_workgroup_and_tile_edges(host, n_rows):
    text = X.h2(n_rows)
    want = X.restate(text)
    assert want["counts"]["rows"] == n_rows
    X.assert_same(X.columns(host, text), want)


def test_h2_empty_text(host):
    got = X.columns(host, b"")
    assert got["counts"]["rows"] == 0 and got["key_off"].tolist() == [0]
    X.assert_same(got, X.restate(b""))


def test_h3_long_lines(host):
    text = X.h3()
    want = X.restate(text)
    assert want["counts"]["rows"] == 701 and want["counts"]["frag_host"] == 1
    assert int(np.diff(want["key_off"]).max()) == X.LONG
    X.assert_same(X.columns(host, text), want)


@pytest.mark.parametrize("labels", [["22", "X"], ["other"], [], None])
def test_h4_contig_mask(host, labels):
    text = X.h4()
    got = X.columns(host, text, labels)
    want = X.restate(text if labels is None else X.filtered(text, labels))
    X.assert_same(got, want, counts=False)
    assert got["counts"]["rows"] == want["counts"]["rows"]
    # a masked row is a skipped line
    assert got["counts"]["rows"] + got["counts"]["skipped"] == X.restate(text)["counts"]["rows"] + \
        X.restate(text)["counts"]["skipped"]
    if labels == []:
        assert got["counts"]["rows"] == 0
    if labels == ["22", "X"]:
        assert got["counts"]["rows"] == sum(1 for i in range(600) if i % 28 in (21, 22))
    # an integer mask is taken as it is
    if labels == ["other"]:
        X.assert_same(X.columns(host, text, 1 << 31), want, counts=False)


# ---- H5: bounds and arguments, on the C entries ------------------------------------
def raw_build(host, text: bytes, short=None, patch=None):
    """The two host entries with sentinel-filled blobs of total + PAD bytes (short:
    (blob index, bytes) taken off one cap)."""
    lib, ctx = host.lib, host.ctx
    t = np.frombuffer(text, dtype=np.uint8)
    n_lines = text.count(b"\n") + (1 if text and not text.endswith(b"\n") else 0)
    m = max(1, n_lines)
    lens = [np.zeros(m, dtype=np.uint32) for _ in range(3)]
    flags, row_off = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint64)
    counts = np.zeros(N.EXIST_N_COUNTS, dtype=np.uint64)
    rc = lib.avdb_existing_size_host(ctx, t.ctypes.data, t.size, n_lines, N.EXIST_ALL_CONTIGS, lens[0].ctypes.data,
                                     lens[1].ctypes.data, lens[2].ctypes.data, flags.ctypes.data, row_off.ctypes.data,
                                     counts.ctypes.data)
    assert rc == 0
    cnt = dict(zip(N.EXIST_COUNTS, counts.tolist()))
    n = cnt["rows"]
    if patch:
        for r, v in patch.items():
            lens[2][r] = v
    caps = [int(lens[a][:n].sum()) for a in range(3)]
    blobs = [np.full(c + PAD, SENTINEL, dtype=np.uint8) for c in caps]
    if short:
        caps[short[0]] -= short[1]
    offs = [np.full(n + 1, 0x7777, dtype=np.uint64) for _ in range(3)]
    totals = np.zeros(4, dtype=np.uint64)
    rc = lib.avdb_existing_write_host(ctx, t.ctypes.data, t.size, n_lines, n, lens[0].ctypes.data, lens[1].ctypes.data,
                                      lens[2].ctypes.data, flags.ctypes.data, row_off.ctypes.data,
                                      blobs[0].ctypes.data, caps[0], offs[0].ctypes.data,
                                      blobs[1].ctypes.data, caps[1], offs[1].ctypes.data,
                                      blobs[2].ctypes.data, caps[2], offs[2].ctypes.data, totals.ctypes.data)
    return rc, cnt, lens, flags, blobs, offs, totals


def test_h5_sentinels_and_host_spans(host):
    rc, cnt, lens, flags, blobs, offs, totals = raw_build(host, X.H1)
    assert rc == 0 and totals[3] == 0
    want = X.restate(X.H1)
    for a, name in enumerate(("keys", "pks")):
        tot = int(totals[a])
        assert blobs[a][:tot].tobytes() == want[name]
        assert (blobs[a][tot:] == SENTINEL).all() and blobs[a].size == tot + PAD
    tot = int(totals[2])
    assert tot == cnt["frag_bytes"] and (blobs[2][tot:] == SENTINEL).all()
    n_host = 0
    for r in range(cnt["rows"]):
        a, b = int(offs[2][r]), int(offs[2][r + 1])
        if flags[r] & N.EXIST_FRAG_HOST:  # left for the caller: not a byte written
            assert (blobs[2][a:b] == SENTINEL).all() and b - a == lens[2][r] >= 36 + lens[1][r]
            n_host += 1
        else:
            w0, w1 = int(want["frag_off"][r]), int(want["frag_off"][r + 1])
            assert blobs[2][a:b].tobytes() == want["frag"][w0:w1]
    assert n_host == X.H1_FRAG_HOST
    # patched lengths move the later spans and leave the patched spans unwritten
    hr = [r for r in range(cnt["rows"]) if flags[r] & N.EXIST_FRAG_HOST]
    new = {r: int(want["frag_off"][r + 1] - want["frag_off"][r]) for r in hr}
    rc, cnt, lens, flags, blobs, offs, totals = raw_build(host, X.H1, patch=new)
    assert rc == 0 and np.array_equal(offs[2].astype(np.int64), want["frag_off"])
    got = blobs[2][:int(totals[2])].copy()
    for r in hr:
        a, b = int(offs[2][r]), int(offs[2][r + 1])
        assert (got[a:b] == SENTINEL).all()
        got[a:b] = np.frombuffer(want["frag"][a:b], dtype=np.uint8)
    assert got.tobytes() == want["frag"]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_h5_cap_one_byte_short(host, which):
    rc, cnt, lens, flags, blobs, offs, totals = raw_build(host, X.H1, short=(which, 1))
    assert rc == N.AVDB_ERANGE and totals[3] == 1
    assert all((b == SENTINEL).all() for b in blobs)  # nothing written


def test_h5_null_arguments(host):
    lib, ctx = host.lib, host.ctx
    t = np.frombuffer(b"1:1:A:C\tpk\tbin\n", dtype=np.uint8)
    a = np.zeros(8, dtype=np.uint64)
    p = a.ctypes.data
    assert lib.avdb_existing_size_host(None, t.ctypes.data, t.size, 1, 0xFFFFFFFF, p, p, p, p, p, p) == N.AVDB_EINVAL
    assert lib.avdb_existing_size_host(ctx, None, t.size, 1, 0xFFFFFFFF, p, p, p, p, p, p) == N.AVDB_EINVAL
    assert lib.avdb_existing_size_host(ctx, t.ctypes.data, t.size, 1, 0xFFFFFFFF, None, p, p, p, p, p) == N.AVDB_EINVAL
    assert lib.avdb_existing_size_host(ctx, t.ctypes.data, t.size, 1, 0xFFFFFFFF, p, p, p, None, p, p) == N.AVDB_EINVAL
    assert lib.avdb_existing_size_host(ctx, t.ctypes.data, t.size, 1, 0xFFFFFFFF, p, p, p, p, p, None) == N.AVDB_EINVAL
    assert lib.avdb_existing_size_host(ctx, None, 0, 0, 0xFFFFFFFF, None, None, None, None, None, p) == 0
    w = lib.avdb_existing_write_host
    assert w(None, t.ctypes.data, t.size, 1, 1, p, p, p, p, p, p, 8, p, p, 8, p, p, 8, p, p) == N.AVDB_EINVAL
    assert w(ctx, t.ctypes.data, t.size, 1, 1, None, p, p, p, p, p, 8, p, p, 8, p, p, 8, p, p) == N.AVDB_EINVAL
    assert w(ctx, t.ctypes.data, t.size, 1, 1, p, p, p, p, None, p, 8, p, p, 8, p, p, 8, p, p) == N.AVDB_EINVAL
    assert w(ctx, t.ctypes.data, t.size, 1, 1, p, p, p, p, p, None, 8, p, p, 8, p, p, 8, p, p) == N.AVDB_EINVAL
    assert w(ctx, t.ctypes.data, t.size, 1, 1, p, p, p, p, p, p, 8, None, p, 8, p, p, 8, p, p) == N.AVDB_EINVAL
    assert w(ctx, t.ctypes.data, t.size, 1, 2, p, p, p, p, p, p, 8, p, p, 8, p, p, 8, p, p) == N.AVDB_EINVAL  # rows > lines
    # the device entries refuse the same before any GPU work (no stream, no workspace is reached)
    assert lib.avdb_existing_size(None, t.ctypes.data, t.size, 1, 0xFFFFFFFF, p, p, p, p, p, p, None, 0,
                                  None) == N.AVDB_EINVAL
    assert lib.avdb_existing_size(ctx, t.ctypes.data, t.size, 1, 0xFFFFFFFF, p, p, None, p, p, p, None, 0,
                                  None) == N.AVDB_EINVAL
    assert lib.avdb_existing_size(ctx, t.ctypes.data, t.size, 1, 0xFFFFFFFF, p, p, p, p, p, p, None, 0,
                                  None) == N.AVDB_ERANGE  # no workspace
    sz = ctypes.c_size_t()
    assert lib.avdb_existing_workspace_size(1 << 20, 1000, ctypes.byref(sz)) == 0 and sz.value >= 40 * 1000
    assert lib.avdb_existing_workspace_size(0, 0, None) == N.AVDB_EINVAL


@pytest.mark.parametrize("text,n", [(b"1:1:A:C\tpk\rx\tbin\n", 1), (b"1:1:A:C\tpk\tbin\r\r\n", 1),
                                    (b"a\rb\n1:1:A:C\tpk\tbin\r", 2)])
def test_h5_lone_cr_raises(host, text, n):
    with pytest.raises(ValueError, match="%d carriage return" % n) as ei:
        host.existing_table_build(text)
    assert "from_tsv" in str(ei.value)

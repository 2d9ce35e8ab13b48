"""K10 (CADD table build + allele join) through the library's host entries
(avdb_cadd_table_build_host / avdb_cadd_match_host on an avdb_ctx_create(-1, ...)
context): the same per-line and per-record code the kernels run, checked against
the reference's own CADDUpdater output (tests/golden/make_golden_cadd.py).  No GPU."""

import ctypes
import random

import numpy as np
import pytest
import torch

import cadd_common as C
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.cadd import CaddTable, CADDUpdater
from annotatedvdb_amd.engine import Engine

HEADER = b"## CADD\n#Chrom\tPos\tRef\tAlt\tRawScore\tPHRED\n"


@pytest.fixture(scope="module")
def host():
    return Engine("host")


@pytest.fixture(scope="module")
def tables(host):
    snv, indel, _, _ = C.golden()
    return CaddTable.from_text(snv, host), CaddTable.from_text(indel, host)


def test_restatement_reproduces_the_reference():
    """The in-test restatement of match / buffer_variant is pinned to what the
    reference's CADDUpdater buffered, tuple for tuple."""
    snv, indel, recs, counters = C.golden()
    got, ctr = C.ref_buffer(C.parse_table(snv), C.parse_table(indel), recs)
    assert got == [r["expected"] for r in recs if r["expected"] is not None]
    assert ctr == counters
    classes = {}
    for r in recs:
        classes[r["cls"]] = classes.get(r["cls"], 0) + 1
    assert len(classes) == 18 and min(classes.values()) >= 100


def test_t1_golden_tuples_and_counters(host, tables):
    snv_t, indel_t = tables
    snv, indel, recs, counters = C.golden()
    assert snv_t.counts["score_host"] == 0 and indel_t.counts["score_host"] == 0
    assert snv_t.counts["bad"] == 0 and indel_t.counts["bad"] == 0
    assert snv_t.counts["rows"] == sum(len(v) for v in C.parse_table(snv).values())
    assert indel_t.counts["rows"] == sum(len(v) for v in C.parse_table(indel).values())
    # no fixture variant may lean on the host fallback
    ids = [r["metaseq_id"] for r in recs]
    ctr = host.new_cadd_counters()
    row, kind, raw, phred = host.cadd_match(snv_t.cols, indel_t.cols, C.batch_of(ids), ctr)
    assert not (kind.numpy() == N.CADD_HOST).any()
    erow, ekind, eraw, ephred = C.expect_arrays(snv, indel, ids)
    assert np.array_equal(row.numpy(), erow) and np.array_equal(kind.numpy(), ekind)
    assert np.array_equal(C.bits(raw.numpy()), C.bits(eraw)) and np.array_equal(C.bits(phred.numpy()), C.bits(ephred))
    assert ctr.tolist() == [int((ekind == N.CADD_SNV).sum()), int((ekind == N.CADD_INDEL).sum()),
                            int((ekind == N.CADD_NONE).sum())]
    # the tuples and the five counters, through CADDUpdater (JSON compared as text)
    got, gctr = C.run_updater(CADDUpdater(snv_t, indel_t, host), recs)
    assert got == [r["expected"] for r in recs if r["expected"] is not None]
    assert gctr == counters


def _score_table(host, pairs):
    text = HEADER + b"".join(b"1\t%d\tA\tC\t%s\t%s\n" % (i + 1, a, b) for i, (a, b) in enumerate(pairs))
    return text, host.cadd_table_build(text)


def test_t2_scores_bit_exact_against_float(host):
    hand = [b"0", b"-0.000000", b"0.1", b"12.345", b"-7.250000", b"123456789.012345", b"0.0000000123456789012345",
            b"-0", b"000012.5", b"999999999999999", b"0.000000", b"0.0000000000000000000001"]
    rng = random.Random(11)
    seeded = [(b"%.6f" % rng.uniform(-10, 40), b"%.3f" % rng.uniform(0, 99)) for _ in range(20000)]
    pairs = [(s, hand[(i + 1) % len(hand)]) for i, s in enumerate(hand)] + seeded
    _, cols = _score_table(host, pairs)
    assert cols.n_rows == len(pairs) and int(cols.counts[N.CADD_COUNT_SCORE_HOST]) == 0
    assert not cols.flags.numpy().any()
    assert np.array_equal(C.bits(cols.raw.numpy()), C.bits([float(a) for a, _ in pairs]))
    assert np.array_equal(C.bits(cols.phred.numpy()), C.bits([float(b) for _, b in pairs]))
    assert C.bits(cols.raw.numpy())[1] == np.int64(-2 ** 63)  # -0.0 keeps its sign


def test_t2_scores_left_to_the_host(host):
    odd = [b"1234567890.123456", b"1e-05", b".5", b"3.2\r", b"nan", b"5.", b"+1.5", b"1234567890123456",
           b"0.00000000000000000000001"]
    pairs = [(s, b"1.5") for s in odd] + [(b"2.5", s) for s in odd]
    text, cols = _score_table(host, pairs)
    assert (cols.flags.numpy() == N.CADD_ROW_SCORE_HOST).all()
    assert int(cols.counts[N.CADD_COUNT_SCORE_HOST]) == len(pairs)
    t = CaddTable.from_text(text, host)  # the wrapper's one-time patch
    want_raw, want_phred = [float(a) for a, _ in pairs], [float(b) for _, b in pairs]
    assert np.array_equal(C.bits(t.cols.raw.numpy()), C.bits(want_raw))
    assert np.array_equal(C.bits(t.cols.phred.numpy()), C.bits(want_phred))
    with pytest.raises(ValueError):
        CaddTable.from_text(HEADER + b"1\t5\tA\tC\t\t1.0\n", host)  # an empty score: float('') raises there too


def test_t3_text_edge_cases(host):
    assert host.cadd_table_build(HEADER).n_rows == 0
    assert host.cadd_table_build(b"").n_rows == 0
    assert len(CaddTable.from_text(b"", host)) == 0
    line = b"1\t100\tA\tC\t0.5\t1.5"
    for text in (HEADER + line, HEADER + line + b"\n", line, b"\n" + line + b"\n\n"):
        cols = host.cadd_table_build(text)
        assert cols.n_rows == 1 and cols.pos.tolist() == [100] and cols.raw.tolist() == [0.5]
        s = text.index(b"100\t") + 4
        assert (cols.ref_off.tolist(), cols.ref_len.tolist(), cols.alt_off.tolist(), cols.alt_len.tolist()) == \
               ([s], [1], [s + 2], [1])
        assert cols.first_row[0].item() == 0 and cols.end_row[0].item() == 1
    # a 5-field line and unusable positions are BAD and never match
    text = HEADER + b"1\t100\tA\tC\t0.5\n1\t100\tA\tC\t0.25\t2.5\textra\tcolumns\n1\t0\tA\tC\t1\t1\n" \
                    b"1\t4294967296\tA\tC\t1\t1\n1\t1e3\tA\tC\t1\t1\n1\t\tA\tC\t1\t1\n1\t4294967295\tG\tT\t1\t1\n"
    cols = host.cadd_table_build(text)
    assert cols.flags.tolist() == [N.CADD_ROW_BAD, 0, N.CADD_ROW_BAD, N.CADD_ROW_BAD, N.CADD_ROW_BAD,
                                   N.CADD_ROW_BAD, 0]
    assert int(cols.counts[N.CADD_COUNT_BAD]) == 5 and int(cols.counts[N.CADD_COUNT_ORDER_VIOLATIONS]) == 0
    t = CaddTable.from_text(text, host)
    row, kind, raw, phred = CADDUpdater(t, None, host).match_batch(["1:100:A:C", "1:4294967295:T:G", "1:0:A:C"])
    assert row.tolist() == [1, 6, -1] and kind.tolist() == [N.CADD_SNV, N.CADD_SNV, N.CADD_NONE]
    assert raw[0] == 0.25 and phred[0] == 2.5
    # contig labels: MT is the project's M; an unknown contig is 255 and resolved by name on the host
    text = HEADER + b"22\t5\tA\tC\t1\t1\nX\t5\tA\tC\t1\t1\nY\t5\tA\tC\t1\t1\nMT\t5\tA\tC\t1\t1\n" \
                    b"GL000009.2\t5\tA\tC\t0.75\t1\n23\t5\tA\tC\t1\t1\nM\t5\tA\tC\t1\t1\n0\t5\tA\tC\t1\t1\n"
    t = CaddTable.from_text(text, host)
    assert t.cols.chrom.tolist() == [21, 22, 23, 24, 255, 255, 255, 255]
    assert t.cols.first_row[24].item() == 3 and t.cols.end_row[24].item() == 4
    u = CADDUpdater(t, None, host)
    row, kind, raw, _ = u.match_batch(["M:5:A:C", "MT:5:C:A", "GL000009.2:5:A:C", "GL000009.2:6:A:C", "chr1:5:A:C"])
    assert row.tolist() == [3, 3, 4, -1, -1]
    assert kind.tolist() == [N.CADD_SNV, N.CADD_SNV, N.CADD_SNV, N.CADD_NONE, N.CADD_NONE] and raw[2] == 0.75
    # tabix order: a contig in two runs, a position that decreases
    for bad in (b"1\t5\tA\tC\t1\t1\n2\t5\tA\tC\t1\t1\n1\t6\tA\tC\t1\t1\n", b"1\t6\tA\tC\t1\t1\n1\t5\tA\tC\t1\t1\n"):
        assert int(host.cadd_table_build(HEADER + bad).counts[N.CADD_COUNT_ORDER_VIOLATIONS]) == 1
        with pytest.raises(ValueError):
            CaddTable.from_text(HEADER + bad, host)
    ok = b"2\t5\tA\tC\t1\t1\n2\t5\tA\tG\t1\t1\n1\t1\tA\tC\t1\t1\n"  # contigs in any order, equal positions
    assert int(host.cadd_table_build(HEADER + ok).counts[N.CADD_COUNT_ORDER_VIOLATIONS]) == 0


def test_t3_from_file_reads_gzip_and_filters_contigs(host, tmp_path):
    import gzip
    import os
    from conftest import GOLDEN
    snv, _, _, _ = C.golden()
    whole = CaddTable.from_file(os.path.join(GOLDEN, "cadd_snv.tsv.gz"), engine=host)
    assert len(whole) == sum(len(v) for v in C.parse_table(snv).values())
    part = CaddTable.from_file(os.path.join(GOLDEN, "cadd_snv.tsv.gz"), contigs=["chr21", "M"], engine=host)
    rows = C.parse_table(snv)
    assert len(part) == len(rows["21"]) + len(rows["MT"])
    assert sorted(set(part.cols.chrom.tolist())) == [20, 24]
    plain = tmp_path / "t.tsv"
    plain.write_bytes(snv)
    assert len(CaddTable.from_file(str(plain), engine=host)) == len(whole)
    two = tmp_path / "two.tsv.gz"  # bgzip: several gzip members in one file
    cut = snv.index(b"\n", len(snv) // 2) + 1
    two.write_bytes(gzip.compress(snv[:cut]) + gzip.compress(snv[cut:]))
    assert len(CaddTable.from_file(str(two), engine=host)) == len(whole)


def test_t4_argument_checks(host, tables):
    lib, ctx = host.lib, host.ctx
    text = HEADER + b"1\t100\tA\tC\t0.5\t1.5\n"
    buf = ctypes.create_string_buffer(text, len(text))
    cols = [np.zeros(4, dt) for dt in (np.uint8, np.uint32, np.uint64, np.uint32, np.uint64, np.uint32, np.float64,
                                       np.float64, np.uint8)]
    first, end, counts = np.zeros(25, np.uint32), np.zeros(25, np.uint32), np.zeros(4, np.uint64)
    ptrs = [c.ctypes.data for c in cols]
    tail = [first.ctypes.data, end.ctypes.data, counts.ctypes.data]
    addr = ctypes.addressof(buf)
    assert lib.avdb_cadd_table_build_host(ctx, addr, len(text), 3, *ptrs, *tail) == 0 and counts[0] == 1
    assert lib.avdb_cadd_table_build_host(None, addr, len(text), 3, *ptrs, *tail) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build_host(ctx, None, len(text), 3, *ptrs, *tail) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build_host(ctx, addr, len(text), 3, *([None] + ptrs[1:]), *tail) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build_host(ctx, addr, len(text), 3, *ptrs, None, *tail[1:]) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build_host(ctx, addr, len(text), 3, *ptrs, *tail[:2], None) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build_host(ctx, None, 0, 0, *([None] * 9), *tail) == 0 and counts[0] == 0
    # the device entries refuse the same before any GPU work (this context has no GPU)
    assert lib.avdb_cadd_table_build(None, addr, len(text), 3, *ptrs, *tail, None, 0, None) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build(ctx, addr, len(text), 3, *ptrs, None, *tail[1:], None, 0, None) == N.AVDB_EINVAL
    assert lib.avdb_cadd_table_build(ctx, addr, len(text), 3, *ptrs, *tail, None, 0, None) == N.AVDB_ERANGE
    sz = ctypes.c_size_t()
    assert lib.avdb_cadd_workspace_size(len(text), 3, None) == N.AVDB_EINVAL
    assert lib.avdb_cadd_workspace_size(len(text), 3, ctypes.byref(sz)) == 0 and sz.value >= 32768 + 8 * 7

    snv_t, indel_t = tables
    vs, vi = snv_t.cols.view(), indel_t.cols.view()
    b = C.batch_of(["1:100:A:C", "1:100:AT:C"])
    n = 2
    row, kind = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    raw, phred, ctr = np.zeros(n), np.zeros(n), np.zeros(3, np.uint64)
    rec = [N.ptr(b.chrom), N.ptr(b.pos), N.ptr(b.allele_off), N.ptr(b.ref_len), N.ptr(b.alt_len), N.ptr(b.heap),
           b.heap.numel()]
    outs = [row.ctypes.data, kind.ctypes.data, raw.ctypes.data, phred.ctypes.data]
    f = lib.avdb_cadd_match_host
    assert f(ctx, ctypes.byref(vs), ctypes.byref(vi), *rec, n, *outs, ctr.ctypes.data) == 0
    assert f(None, ctypes.byref(vs), ctypes.byref(vi), *rec, n, *outs, None) == N.AVDB_EINVAL
    assert f(ctx, ctypes.byref(vs), ctypes.byref(vi), None, *rec[1:], n, *outs, None) == N.AVDB_EINVAL
    assert f(ctx, ctypes.byref(vs), ctypes.byref(vi), *rec, n, None, *outs[1:], None) == N.AVDB_EINVAL
    assert lib.avdb_cadd_match(ctx, ctypes.byref(vs), ctypes.byref(vi), *rec, n, None, *outs[1:], None, None) == \
        N.AVDB_EINVAL
    wrong = snv_t.cols.view()
    wrong.struct_size = 8
    assert f(ctx, ctypes.byref(wrong), None, *rec, n, *outs, None) == N.AVDB_EINVAL
    assert b"struct_size" in lib.avdb_last_error()
    assert f(ctx, ctypes.byref(vs), ctypes.byref(vi), *([None] * 6), 0, 0, *([None] * 4), None) == 0  # n == 0
    # both tables empty (or absent): every record NONE, all of them counted not_matched
    empty = N.CaddTableView()
    for a, c in ((None, None), (ctypes.byref(empty), ctypes.byref(empty))):
        row[:], kind[:], ctr[:] = 7, 7, 0
        assert f(ctx, a, c, *rec, n, *outs, ctr.ctypes.data) == 0
        assert row.tolist() == [-1, -1] and kind.tolist() == [N.CADD_NONE] * 2 and ctr.tolist() == [0, 0, n]
    u = CADDUpdater(None, None, host)
    assert u.match_batch(["1:100:A:C"])[1].tolist() == [N.CADD_NONE] and u.match_batch([])[0].size == 0
    assert torch.equal(host.new_cadd_counters(), torch.zeros(3, dtype=torch.int64))


# ---- the header's restatement (cadd_common.expect_table / expect_match) ----------
def _check_table(host, text, what):
    want = C.expect_table(text)
    C.assert_same_table(C.table_columns(host.cadd_table_build(text)), want, what)
    return want


def _window_slab_and_odd():
    import test_gpu_cadd as G
    odd = HEADER + b"1\t5\tA\tC\t1e-05\t1.5\n1\t6\tA\n\n1\tx\tA\tC\t1\t1\n1\t7\tAT\tA\t-0.000000\t.5\r\n" \
                   b"GL1\t7\tA\tC\t1\t2\n2\t9\tA\tC\t1\t2\n1\t9\tA\tC\t1234567890.123456\t2\n2\t8\tA\tC\t1\t2"
    return G.window_slab(), odd


def test_t5_expect_table_equals_the_host_entry(host):
    """expect_table is written from avdb.h, not from avdb_cadd.hpp: every column
    (doubles as bits) and all four counts, on the suite's texts and a seeded fuzz."""
    snv, indel, _, _ = C.golden()
    slab, odd = _window_slab_and_odd()
    for what, text in (("snv", snv), ("indel", indel), ("window_slab", slab), ("odd", odd), ("empty", b""),
                       ("header", HEADER), ("blank", b"\n\n")):
        _check_table(host, text, what)
    cols, counts = C.expect_table(odd)
    assert counts == [8, 3, 2, 2] and cols["pos"].tolist() == [5, 5, 5, 7, 7, 9, 9, 8]
    rng = random.Random(2024)
    seen = [0, 0, 0, 0]
    for k in range(400):
        text = C.fuzz_table(rng)
        _, counts = _check_table(host, text, "fuzz %d: %r" % (k, text))
        seen = [a + (b > 0) for a, b in zip(seen, counts)]
    assert min(seen) >= 100  # the fuzz reaches rows, host-left scores, BAD rows and violations


def test_t5_a_long_allele_and_long_lines(host):
    rng = random.Random(5)
    big = "".join(rng.choice("ACGT") for _ in range(24000)).encode()
    text = b"1\t5\tA\tC\t0.5\t1.5\n1\t6\tA\t" + big + b"\t0.25\t2.5\textra\n1\t7\t" + big + b"\tA\t1\t2"
    cols, counts = _check_table(host, text, "24 kB allele")
    assert counts == [3, 0, 0, 0] and cols["alt_len"].tolist() == [1, 24000, 1]


BAD = b"1\tx\tA\tC\t1\t1\n"


def _bad_run_texts(n):
    g = lambda c, p: b"%d\t%d\tA\tC\t0.5\t1.5\n" % (c, p)
    return {"top": BAD * n + g(1, 5) + g(1, 6),
            "mid": g(1, 5) + g(1, 6) + BAD * n + g(1, 7) + g(1, 8),
            "mid, pos decreases": g(1, 5) + g(1, 6) + BAD * n + g(1, 4),
            "boundary": g(1, 5) + g(1, 6) + BAD * n + g(2, 1) + g(2, 2),
            "end": g(1, 5) + g(1, 6) + BAD * n,
            "end, no newline": (g(1, 5) + g(1, 6) + BAD * n)[:-1],
            "far down": g(3, 1) * 100 + g(1, 6) + BAD * n + g(1, 7)}


@pytest.mark.parametrize("n", [63, 64, 65, 200])
def test_t5_bad_runs_at_the_bound(host, n):
    """avdb.h: *more than* 64 BAD rows in a row are a violation, wherever they stand."""
    texts = _bad_run_texts(n)
    got = {}
    for what, text in texts.items():
        cols, counts = _check_table(host, HEADER + text, "%d BAD rows, %s" % (n, what))
        assert counts[0] == text.count(b"\n") + (not text.endswith(b"\n")) and counts[2] == n
        got[what] = (cols, counts[3])
    if n <= 64:
        assert [v for _, v in got.values()] == [0, 0, 1, 0, 0, 0, 0]
        cols = got["mid"][0]
        assert cols["first_row"][0] == 0 and cols["end_row"][0] == n + 4  # one run: the row after is no start
        assert cols["pos"].tolist() == [5] + [6] * (n + 1) + [7, 8]
        assert got["top"][0]["pos"].tolist() == [0] * n + [5, 6]
        cols = got["boundary"][0]
        assert (cols["first_row"][:2].tolist(), cols["end_row"][:2].tolist()) == ([0, n + 2], [2, n + 4])
    else:
        assert all(v > 0 for what, (_, v) in got.items() if not what.startswith("end")), got
        assert got["top"][1] == n - 64  # rows 65 .. n see no usable row among the 65 before them
        assert got["end"][1] == n - 65
        # the 65th BAD row of the run still reaches the good row 65 rows up; the 66th does not
        assert got["mid"][0]["pos"][2:2 + n].tolist() == [6] * 65 + [0] * (n - 65)
        with pytest.raises(ValueError):
            CaddTable.from_text(HEADER + texts["mid"], host)
    if n == 64:
        assert len(CaddTable.from_text(HEADER + texts["mid"], host)) == 68


def test_t6_expect_match_equals_the_host_join(host):
    snv, indel, recs, _ = C.golden()
    ids = [r["metaseq_id"] for r in recs]
    want = C.expect_arrays(snv, indel, ids)
    for a, b in zip(C.expect_match(snv, indel, ids), want):  # the two restatements agree where both apply
        assert np.array_equal(C.bits(a), C.bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
    rng = random.Random(77)
    kinds, hits, n = set(), 0, 0
    for k in range(120):
        s, i, ids = C.join_case(rng, edge=k % 4 == 0)
        erow, ekind = C.check_join(host, s, i, ids, "case %d" % k)
        kinds |= set(ekind.tolist())
        hits += int((erow >= 0).sum())
        n += len(ids)
    assert kinds == {N.CADD_NONE, N.CADD_SNV, N.CADD_INDEL, N.CADD_HOST} and hits > n // 5 and n > 20000


def test_t6_join_edges_by_hand(host):
    """The cases the fuzz is built around, with the answers written out."""
    P = 2 ** 32 - 1
    snv = HEADER + b"1\t2147483648\tA\tC\t0.5\t1.5\n1\t2147483648\tA\t1\n1\t2147483648x\tG\tT\t9\t9\n" \
                   b"1\t2147483648\tG\tT\t0.25\t2.5\n1\t%d\tA\tA\t1.5\t3.5\n2\t%d\tC\tG\t2.5\t4.5\n" % (P, P)
    ids = ["1:2147483648:A:C", "1:2147483648:T:G", "1:2147483648::", "1:%d:A:A" % P, "1:%d:C:G" % P, "2:%d:G:C" % P,
           "1:2147483647:A:C", "1:0:A:C", "3:%d:C:G" % P, "GL1:5:A:C"]
    erow, ekind = C.check_join(host, snv, HEADER, ids, "by hand")
    assert erow.tolist() == [0, 3, -1, 4, -1, 5, -1, -1, -1, -1]
    assert ekind.tolist() == [1, 1, 0, 1, 0, 1, 0, 0, 0, N.CADD_HOST]

"""K13 (CADD update rows rendered from an export) through the library's host entries
(avdb_cadd_update_size_host / avdb_cadd_update_write_host / avdb_cadd_score_text_host on
an avdb_ctx_create(-1, ...) context): the same per-line code the kernels run, checked
against the reference's own CADDUpdater output (tests/golden/cadd_expected.tsv.gz), a
restatement of the reference's loop, and CADDUpdater.buffer_variants.  No GPU."""

import ctypes
import gzip
import json
import logging
import os
import random
import re

import numpy as np
import pytest

import cadd_common as C
import cadd_update_common as U
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.cadd import CaddTable, CADDUpdater
from annotatedvdb_amd.engine import Engine

HEADER = b"## CADD\n#Chrom\tPos\tRef\tAlt\tRawScore\tPHRED\n"
COUNTERS = ("snv", "indel", "not_matched", "update", "skipped")


@pytest.fixture(scope="module")
def host():
    return Engine("host")


@pytest.fixture(scope="module")
def tables(host):
    snv, indel, _, _ = C.golden()
    return CaddTable.from_text(snv, host), CaddTable.from_text(indel, host)


# ---- 1: the golden ------------------------------------------------------------------
def test_u1_golden_text_tuples_and_counters(host, tables):
    _, _, recs, counters = C.golden()
    u = CADDUpdater(tables[0], tables[1], host)
    settings = []
    for chromosome, text, part in U.golden_exports():
        if chromosome:
            u.set_chromosome(chromosome)
        rows = host.cadd_update_rows(text, tables[0], tables[1], chromosome=u.get_chromosome())
        assert rows.counts["host_rows"] == 0 and rows.counts["bad"] == 0  # nothing leans on the fallback
        assert rows.counts["skipped_lines"] == 0 and rows.counts["rows"] + rows.counts["skipped"] == len(part)
        assert u.buffer_export(text) == rows.n == sum(r["expected"] is not None for r in part)
        settings.append((chromosome, len(part)))
    assert settings == [(None, 2231), ("chr1", 825), ("chr21", 784)]
    assert u.update_buffer(sizeOnly=True) == sum(r["expected"] is not None for r in recs)
    assert u.update_text() == U.golden_text()
    assert u.update_buffer() == [r["expected"] for r in recs if r["expected"] is not None]
    assert u.update_text() == U.golden_text()  # (from the tuples now)
    assert {k: u.get_count(k) for k in COUNTERS} == counters
    rows = U.golden_text().decode().split("\n")[:-1]  # 39 rows in exponent form, 434 with a score of -0.0
    assert sum("e-" in r for r in rows) == 39 and sum(bool(re.search(r"-0\.0[,}]", r)) for r in rows) == 434
    u.reset_update_buffer()
    assert u.update_buffer() == [] and u.update_text() == b""


def test_u1_export_rows_keep_their_place_among_tuples(host, tables):
    """buffer_variants before and after a buffer_export: one buffer, in call order."""
    _, _, recs, _ = C.golden()
    part = [r for r in recs if not r["chromosome"]][:60]
    want, _ = C.run_updater(CADDUpdater(tables[0], tables[1], host), part)
    u = CADDUpdater(tables[0], tables[1], host)
    u.buffer_variants(part[:20])
    u.buffer_export(b"".join(U.export_line(r["record_primary_key"], r["metaseq_id"], r["cadd_scores"]) + b"\n"
                             for r in part[20:40]))
    u.buffer_variants(part[40:])
    assert u.update_buffer(sizeOnly=True) == len(want)
    assert u.update_text() == U.rows_text(want)
    assert u.update_buffer() == want


# ---- 2: the score text --------------------------------------------------------------
def _score_text(s: bytes):
    out, ln = np.zeros(N.CADDUPD_SCORE_MAX, np.uint8), ctypes.c_size_t()
    src = np.frombuffer(s, dtype=np.uint8).copy() if s else None
    rc = N.call("avdb_cadd_score_text_host", src, len(s), out, out.size, ctypes.byref(ln))
    assert (rc == 1 and 0 < ln.value <= 21) or (rc == 0 and ln.value == 0)
    return out[:ln.value].tobytes().decode() if rc else None


def _seeded_scores(n):
    """-?digits[.digits] with 1-15 digits behind optional zeros and 0-22 fractional digits."""
    rng = random.Random(412003)
    for _ in range(n):
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 15)))
        if rng.random() < 0.3:
            digits = digits.rstrip("0") + "0" * rng.randint(0, 3)  # trailing zeros
            digits = digits[:15] or "0"
        frac = rng.randint(0, 22)
        s = digits.rjust(frac + 1, "0") if frac else digits  # at least one digit before the point
        s = "0" * rng.randint(0, 3) + s
        if frac:
            s = s[:-frac] + "." + s[-frac:]
        yield ("-" if rng.random() < 0.5 else "") + s


def test_u2_score_text_is_json_dumps_of_float():
    hand = [b"0", b"-0.000000", b"0.1", b"12.345", b"-7.250000", b"123456789.012345", b"0.0000000123456789012345",
            b"-0", b"000012.5", b"999999999999999", b"0.000000", b"0.0000000000000000000001"]  # test_cadd_host.py
    grid = [b"%.6f" % (k / 7919.0) for k in range(-3000, 3000)] + [b"%.3f" % (k / 97.0) for k in range(-3000, 3000)] + \
           [b"%.6f" % (k * 1e-6) for k in range(-2000, 2000)] + [b"%.3f" % (k * 1e-3) for k in range(-2000, 2000)]
    n = 0
    for s in [x.encode() for x in _seeded_scores(400000)] + grid + hand:
        assert _score_text(s) == json.dumps(float(s)), s
        n += 1
    assert n >= 400000 + len(grid) + len(hand)
    for s in (b"0.0001", b"0.00001", b"-0.00001230", b"1000000000000000"[:15], b"100", b"0.5"):
        assert _score_text(s) == json.dumps(float(s)), s
    assert (_score_text(b"0.00001"), _score_text(b"-0.0"), _score_text(b"100")) == ("1e-05", "-0.0", "100.0")


def test_u2_score_text_refuses_what_parse_score_refuses(host):
    odd = [b"1234567890.123456", b"1e-05", b".5", b"3.2\r", b"nan", b"5.", b"+1.5", b"1234567890123456",
           b"0.00000000000000000000001"]  # test_cadd_host.py's list
    text = HEADER + b"".join(b"1\t%d\tA\tC\t%s\t1.5\n" % (i + 1, s) for i, s in enumerate(odd))
    assert (host.cadd_table_build(text).flags.numpy() == N.CADD_ROW_SCORE_HOST).all()
    for s in odd + [b"", b"-", b"1.2.3", b"1,5", b" 1", b"0x10", b"1e5", b"--1", b"inf"]:
        assert _score_text(s) is None, s
    out, ln = np.zeros(8, np.uint8), ctypes.c_size_t()
    assert N.call("avdb_cadd_score_text_host", np.zeros(1, np.uint8), 1, out, 8, ctypes.byref(ln), check=False) == \
        N.AVDB_EINVAL  # an output shorter than AVDB_CADDUPD_SCORE_MAX


# ---- 3: the line classes ------------------------------------------------------------
SNV3 = HEADER + b"1\t12\tA\tC\t0.5\t1.25\n1\t100\tA\tC\t-0.000010\t0.001\n1\t100\tA\tG\t12\t3.0\n" \
                b"1\t4294967295\tG\tT\t1.5\t2.5\n2\t5\tA\tC\t0.25\t9.75\nMT\t7\tG\tA\t-1.5\t0.000\n"
INDEL3 = HEADER + b"1\t100\tAT\tA\t2.5\t22.0\n2\t5\tA\tACC\t0.000001\t10\n"


def _both(host, tabs, text, **kw):
    """The engine's rows as tuples and its counts, checked against the restatement."""
    want, ctr = U.ref_export(SNV3, INDEL3, text, **kw)
    rows = host.cadd_update_rows(text, tabs[0], tabs[1], **kw)
    assert rows.text.numpy().tobytes() == U.rows_text(want), (text, rows.text.numpy().tobytes(), want)
    assert {k: rows.counts[k] for k in ctr} == ctr, (text, rows.counts, ctr)
    off = rows.row_off.numpy()
    assert off[0] == 0 and off[-1] == len(U.rows_text(want)) and len(off) == len(want) + 1
    assert [len("\t".join(r)) + 1 for r in want] == np.diff(off).tolist()
    return want, rows


def test_u3_line_classes(host):
    tabs = CaddTable.from_text(SNV3, host), CaddTable.from_text(INDEL3, host)
    L = U.export_line
    # line ends, empty lines, the header, NULL in its three spellings, extra columns
    for text in (L("1:100:A:C", "1:100:A:C"), L("1:100:A:C", "1:100:A:C") + b"\n",
                 L("1:100:A:C", "1:100:A:C") + b"\r\n" + L("1:100:AT:A", "1:100:AT:A") + b"\r\n",
                 b"\n\n" + L("1:100:A:G", "1:100:A:G") + b"\n\n", U.HEADER_LINE + b"\n" + L("2:5:A:C", "2:5:A:C"),
                 b"2:5:A:C\t2:5:A:C\n2:5:A:ACC\t2:5:A:ACC\t\n2:5:A:T\t2:5:A:T\t\\N\textra\tcolumns\n",
                 b"lonely\n\nalone\r\n", b""):
        want, rows = _both(host, tabs, text)
    w, r = _both(host, tabs, L("1:100:A:C", "1:100:A:C", {"CADD_raw_score": 1.0, "CADD_phred": 2.0}) + b"\n" +
                 L("1:12:A:C", "1:12:A:C", {}) + b"\n" + L("1:12:A:C", "1:12:A:C"))
    assert r.counts["skipped"] == 2 and w == [("1:12:A:C", "chr1", '{"CADD_raw_score": 0.5, "CADD_phred": 1.25}')]
    w, r = _both(host, tabs, L("1:100:A:C", "1:100:A:C", {"CADD_raw_score": 1.0, "CADD_phred": 2.0}) + b"\n",
                 skip_existing=False)
    assert r.counts["skipped"] == 0 and w == [("1:100:A:C", "chr1", '{"CADD_raw_score": -1e-05, "CADD_phred": 0.001}')]
    # the primary key: with an rsid, without a ':', empty; with and without a chromosome set
    text = b"\n".join(L(pk, "1:100:A:G") for pk in ("1:100:A:G:rs12", "rs12", "", "X:1:A:G", "chr9:1"))
    w, _ = _both(host, tabs, text)
    assert [x[1] for x in w] == ["chr1", "chrrs12", "chr", "chrX", "chrchr9"]
    for chromosome in ("chr1", "1", "chrX", "GL000009.2"):
        w, _ = _both(host, tabs, text, chromosome=chromosome)
        assert {x[1] for x in w} == {"chr" + chromosome.replace("chr", "")}
    # M and MT both reach the table's MT rows; a switched row matches
    w, r = _both(host, tabs, L("a", "M:7:G:A") + b"\n" + L("b", "MT:7:A:G") + b"\n" + L("c", "M:8:G:A"))
    assert [x[2] == "{}" for x in w] == [False, False, True] and r.counts["host_rows"] == 0
    # positions
    ids = ["1:0012:A:C", "1:0:A:C", "1:4294967295:G:T", "1:4294967296:G:T", "1:00004294967295:G:T", "1:+12:A:C",
           "1: 12:A:C", "1:12 :A:C", "1:0000000012:A:C", "1:1_2:A:C", "1:00000000012:A:C"]  # (the last: 11 digits)
    w, r = _both(host, tabs, b"\n".join(L(m, m) for m in ids))
    assert [x[2] != "{}" for x in w] == [True, False, True, False, True, True, True, True, True, True, True]
    assert r.counts["host_rows"] == 7 and r.flags.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 1]
    assert r.kind.tolist() == [N.CADD_SNV, 0, N.CADD_SNV, 0, N.CADD_SNV, N.CADD_SNV, N.CADD_SNV, N.CADD_SNV,
                               N.CADD_SNV, N.CADD_SNV, N.CADD_SNV]
    # a chr1 label is no contig of the table
    w, r = _both(host, tabs, L("1:100:A:C", "chr1:100:A:C"))
    assert w == [("1:100:A:C", "chr1", "{}")] and r.counts["host_rows"] == 1 and r.counts["not_matched"] == 1
    # metaseq ids with two and with four ':' (and with none)
    for m in ("1:100:A", "1:100:A:C:T", "rs5", ""):
        text = L("1:12:A:C", "1:12:A:C") + b"\n\n" + L("k", m) + b"\n"
        with pytest.raises(ValueError, match="line 3"):
            host.cadd_update_rows(text, tabs[0], tabs[1])
        with pytest.raises(ValueError):
            U.ref_export(SNV3, INDEL3, text)
    assert host.cadd_update_rows(L("k", "1:100:A", {}) + b"\n", tabs[0], tabs[1]).counts["skipped"] == 1  # skipped first
    with pytest.raises(ValueError, match="carriage return"):
        host.cadd_update_rows(b"1:12:A:C\t1:12\r:A:C\n", tabs[0], tabs[1])
    # the contig mask over a whole-table export
    text = b"\n".join(L(m, m) for m in ("1:100:A:C", "2:5:A:C", "M:7:G:A", "MT:7:G:A", "GL9:5:A:C", "2:5:A:ACC")) + b"\n"
    for contigs, n in ((["1"], 1), (["2"], 2), (["M"], 1), (["1", "2"], 3), (["GL9"], 2), (None, 6), ([], 0)):
        w, r = _both(host, tabs, text, contigs=contigs)
        assert len(w) == n and r.counts["skipped_lines"] == 6 - n
    # no tables at all
    rows = host.cadd_update_rows(L("1:100:A:C", "1:100:A:C"), None, None)
    assert rows.text.numpy().tobytes() == b"1:100:A:C\tchr1\t{}\n" and rows.counts["not_matched"] == 1


def test_u3_long_alleles(host):
    rng = random.Random(3)
    big, big2 = C._bases(rng, 40000), C._bases(rng, 40000)
    indel = HEADER + b"1\t100\tAT\tA\t2.5\t22.0\n1\t100\t%s\tA\t0.125\t3.5\n1\t100\t%s\t%s\t7\t8\n" % (
        big.encode(), big.encode(), big2.encode())
    tabs = CaddTable.from_text(SNV3, host), CaddTable.from_text(indel, host)
    ids = ["1:100:%s:A" % big, "1:100:A:%s" % big, "1:100:%s:%s" % (big, big2), "1:100:%s:%s" % (big2, big2),
           "1:100:%sA:A" % big[:-1], "1:100:AT:A"]
    text = b"\n".join(U.export_line("pk%d" % i, m) for i, m in enumerate(ids))
    want, _ = U.ref_export(SNV3, indel, text)
    rows = host.cadd_update_rows(text, tabs[0], tabs[1])
    assert rows.text.numpy().tobytes() == U.rows_text(want)
    assert [w[2] != "{}" for w in want] == [True, True, True, True, big[-1] == "A", True]


# ---- 4: rows left to the host ---------------------------------------------------------
HOST_SNV = HEADER + b"1\t10\tA\tC\t1e-05\t1.5\n1\t11\tA\tC\t0.5\t1234567890123456\n1\t12\tA\tC\tnan\t2\n" \
                    b"1\t13\tA\tC\t0.25\t4.0\nGL9\t5\tA\tC\t0.75\t1.0\nGL9\t6\tAT\tA\t9\t9\n"
HOST_IDS = ["1:10:A:C", "1:11:C:A", "1:12:A:C", "1:13:A:C", "GL9:5:A:C", "GL9:5:A:G", "GL9:6:AT:A", "1:14:A:C",
            "HLA-A:7:A:C", "1: 13:A:C"]


def check_host_rows(eng):
    snv_t = CaddTable.from_text(HOST_SNV, eng)
    indel_t = CaddTable.from_text(HEADER + b"GL9\t6\tAT\tA\t3.5\t0.0625\n", eng)
    recs = [{"record_primary_key": "%s:rs%d" % (m, i), "metaseq_id": m} for i, m in enumerate(HOST_IDS)]
    for chromosome in (None, "chr1"):
        b = CADDUpdater(snv_t, indel_t, eng)
        u = CADDUpdater(snv_t, indel_t, eng)
        if chromosome:
            b.set_chromosome(chromosome)
            u.set_chromosome(chromosome)
        b.buffer_variants(recs)
        text = b"".join(U.export_line(r["record_primary_key"], r["metaseq_id"]) + b"\n" for r in recs)
        rows = eng.cadd_update_rows(text, snv_t, indel_t, chromosome=u.get_chromosome())
        # three scores the device does not parse, four records on contigs without a code, one position with a space
        assert rows.counts["host_rows"] == 8 and rows.flags.tolist() == [1, 1, 1, 0, 1, 1, 1, 0, 1, 1]
        assert rows.kind.tolist() == [1, 1, 1, 1, 1, 0, 2, 0, 0, 1]
        assert u.buffer_export(text) == len(recs)
        assert u.update_text() == U.rows_text(b.update_buffer())
        assert u.update_buffer() == b.update_buffer()
        assert '"CADD_raw_score": 1e-05' in b.update_buffer()[0][2] and "NaN" in b.update_buffer()[2][2]
        for k in COUNTERS:
            assert u.get_count(k) == b.get_count(k), k
        assert u.get_count("snv") == 6 and u.get_count("indel") == 1 and u.get_count("not_matched") == 3


def test_u4_host_rows(host):
    check_host_rows(host)


# ---- 5: buffer_export is buffer_variants ----------------------------------------------
def check_equivalence(eng, seeds):
    for seed in seeds:
        rng = random.Random(seed)
        snv, indel, ids = C.join_case(rng, edge=seed % 8 == 0)
        snv_t, indel_t = CaddTable.from_text(snv, eng), CaddTable.from_text(indel, eng)
        recs = [{"record_primary_key": rng.choice((m, m + ":rs%d" % i, "rs%d" % i)), "metaseq_id": m,
                 "cadd_scores": rng.choice((None, None, None, {}, {"CADD_raw_score": 1.0, "CADD_phred": 2.0}))}
                for i, m in enumerate(ids)]
        text = b"".join(U.export_line(r["record_primary_key"], r["metaseq_id"], r["cadd_scores"]) + b"\n"
                        for r in recs)
        for chromosome, skip in ((None, True), ("chr7", False)):
            b, u = CADDUpdater(snv_t, indel_t, eng), CADDUpdater(snv_t, indel_t, eng)
            if chromosome:
                b.set_chromosome(chromosome)
                u.set_chromosome(chromosome)
            n = b.buffer_variants(recs, skip_existing=skip)
            assert u.buffer_export(text, skip_existing=skip) == n, seed
            assert u.update_text() == U.rows_text(b.update_buffer()), seed
            assert u.update_buffer() == b.update_buffer(), seed
            assert [u.get_count(k) for k in COUNTERS] == [b.get_count(k) for k in COUNTERS], seed


def test_u5_buffer_export_equals_buffer_variants(host):
    check_equivalence(host, range(200))


# ---- 6: capacity and sentinels --------------------------------------------------------
def check_capacity(eng, tabs):
    _, text, _ = U.golden_exports()[1]
    rc, cnt, out, totals, cap = U.raw_passes(eng, text, tabs[0], tabs[1], chrom=b"chr1")
    assert rc == 0 and totals == [cap, 0] and cap == cnt["out_bytes"] > 10000
    assert (out[cap:] == 0xA5).all() and out[cap - 1] == 10
    want = U.rows_text(r["expected"] for r in U.golden_exports()[1][2] if r["expected"] is not None)
    assert out[:cap].tobytes() == want
    for short in (cap - 1, cap // 2, 0):
        rc, _, out, totals, _ = U.raw_passes(eng, text, tabs[0], tabs[1], chrom=b"chr1", cap=short)
        # (the device entry does not wait for its own scan: it reports through totals)
        assert rc == (N.AVDB_ERANGE if eng.host_only else 0) and totals == [cap, 1]
        assert (out == 0xA5).all()  # nothing is written at all
    rc, _, out, totals, _ = U.raw_passes(eng, text, tabs[0], tabs[1], chrom=b"chr1", cap=cap + 8)
    assert rc == 0 and totals == [cap, 0] and (out[cap:] == 0xA5).all() and out[:cap].tobytes() == want
    with pytest.raises(N.NativeError, match="AVDB_CADDUPD_CHROM_MAX"):
        U.raw_passes(eng, text, tabs[0], tabs[1], chrom=b"c" * 65)


def test_u6_capacity_and_sentinels(host, tables):
    check_capacity(host, tables)
    sz = ctypes.c_size_t()
    assert host.lib.avdb_cadd_update_workspace_size(100, 3, None) == N.AVDB_EINVAL
    assert host.lib.avdb_cadd_update_workspace_size(100, 3, ctypes.byref(sz)) == 0 and sz.value % 256 == 0
    # the device entries refuse bad arguments before any GPU work (this context has no GPU)
    assert N.call("avdb_cadd_update_size", host.ctx, None, 5, 1, None, None, None, 0, 0, 0, *([None] * 7), None, 0,
                  None, check=False) == N.AVDB_EINVAL
    assert N.call("avdb_cadd_update_size_host", None, None, 0, 0, None, None, None, 0, 0, 0, *([None] * 7),
                  check=False) == N.AVDB_EINVAL


# ---- 7: the driver ----------------------------------------------------------------------
def test_u7_driver(host, tmp_path, caplog):
    from annotatedvdb_amd import load_cadd_scores as D
    snv, indel, recs, _ = C.golden()
    db = tmp_path / "cadd"
    db.mkdir()
    (db / D.SNV_FILE).write_bytes(gzip.compress(snv))
    (db / D.INDEL_FILE).write_bytes(gzip.compress(indel))
    export = tmp_path / "variants.tsv.gz"
    lines = [U.HEADER_LINE] + [U.export_line(r["record_primary_key"], r["metaseq_id"], r["cadd_scores"]) for r in recs]
    export.write_bytes(gzip.compress(b"\n".join(lines) + b"\n"))
    out = tmp_path / "out"
    with caplog.at_level(logging.INFO, logger="load_cadd_scores"):
        got = D.main(["-d", str(db), "--export", str(export), "--chr", "1,chr21,M,Y", "--skipExisting", "--outDir",
                      str(out)], engine=host)
    snv_rows, indel_rows = C.parse_table(snv), C.parse_table(indel)
    for c in ("1", "21", "M", "Y"):
        part = [dict(r, chromosome="chr" + c) for r in recs if r["metaseq_id"].split(":")[0] == c]
        want, ctr = C.ref_buffer(snv_rows, indel_rows, part)
        assert (out / ("chr%s.cadd_update.tsv" % c)).read_bytes() == U.rows_text(want), c
        assert got[c] == {"records": len(part), "rows": len(want), "snv": ctr["snv"], "indel": ctr["indel"],
                          "not_matched": ctr["not_matched"], "skipped": ctr["skipped"]}
        line = "Updated {:,} variants - SNVS: {:,} - INDELs: {:,} - No match {:,} - Skipped {:,}".format(
            len(part), ctr["snv"], ctr["indel"], ctr["not_matched"], ctr["skipped"])
        assert any(line in rec.getMessage() and "chr%s:" % c in rec.getMessage() for rec in caplog.records), line
    assert got["1"]["records"] > 800 and got["1"]["snv"] > 0 and got["1"]["skipped"] > 0
    assert sorted(os.listdir(out)) == ["chr1.cadd_update.tsv", "chr21.cadd_update.tsv", "chrM.cadd_update.tsv",
                                       "chrY.cadd_update.tsv"]
    assert len(D.chromosome_list("all")) == 25 and D.chromosome_list("autosome") == [str(i) for i in range(1, 23)]
    # a missing table file: every record of the kind goes unmatched; --vcfFile is refused
    os.remove(db / D.INDEL_FILE)
    got = D.main(["-d", str(db), "--export", str(export), "--chr", "21", "--outDir", str(out)], engine=host)
    assert got["21"]["indel"] == 0 and got["21"]["snv"] > 0
    with pytest.raises(SystemExit):
        D.main(["-d", str(db), "--vcfFile", "x.vcf", "--outDir", str(out)], engine=host)
    with pytest.raises(SystemExit):
        D.main(["-d", str(db), "--outDir", str(out)], engine=host)

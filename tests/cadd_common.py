"""Shared by test_cadd_host.py, test_gpu_cadd.py and test_gpu_cadd_edges.py: the
CADD golden (written by tests/golden/make_golden_cadd.py from the reference's own
CADDUpdater), a pure-Python restatement of the reference's ``match`` and
``buffer_variant`` (Util/lib/python/loaders/cadd_updater.py:175-221), which
test_cadd_host.py pins to that golden before any test leans on it, and a
restatement of the K10 table and join written from the K10 comment of
include/avdb.h (``expect_table`` / ``expect_match``), pinned there to the
library's host entries."""

import gzip
import json
import os
import re

import numpy as np
import torch

from conftest import GOLDEN
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import RecordBatch

_cache = {}


def golden():
    """``(snv_text, indel_text, records, counters)``; a record is a dict of the
    expected file's columns (``expected``: the buffered tuple, or None if skipped)."""
    if "g" not in _cache:
        snv = gzip.open(os.path.join(GOLDEN, "cadd_snv.tsv.gz"), "rb").read()
        indel = gzip.open(os.path.join(GOLDEN, "cadd_indel.tsv.gz"), "rb").read()
        recs, counters = [], None
        for line in gzip.open(os.path.join(GOLDEN, "cadd_expected.tsv.gz"), "rt"):
            f = line.rstrip("\n").split("\t")
            if f[0] == "#counters":
                counters = json.loads(f[1])
                continue
            recs.append({"cls": f[0], "chromosome": f[1], "metaseq_id": f[2], "record_primary_key": f[3],
                         "cadd_scores": json.loads(f[4]) if f[4] else None,
                         "expected": None if f[4] else (f[5], f[6], f[7])})
        _cache["g"] = (snv, indel, recs, counters)
    return _cache["g"]


# ---- the restatement ---------------------------------------------------------
def parse_table(text: bytes):
    """{contig: [fields]} in file order — what a TabixFile over the text serves."""
    rows = {}
    for line in text.decode().split("\n"):
        if line and not line.startswith("#"):
            f = line.split("\t")
            rows.setdefault(f[0], []).append(f)
    return rows


def ref_match(snv, indel, metaseq_id):
    """cadd_updater.py:188-214: ``(table name or None, matched row fields or None)``."""
    chrm, position, ref, alt = metaseq_id.split(":")
    is_indel = len(ref) > 1 or len(alt) > 1
    table = indel if is_indel else snv
    cadd_chr = "MT" if chrm == "M" else chrm
    for row in table.get(cadd_chr, ()):  # (a missing contig: pysam's ValueError -> [])
        if int(row[1]) == int(position) and ref in (row[2], row[3]) and alt in (row[2], row[3]):
            return ("indel" if is_indel else "snv"), row
    return None, None


def ref_buffer(snv, indel, records):
    """load_cadd_scores.py:109-120 + buffer_variant over records carrying the
    golden's ``chromosome`` setting: ``(tuples, counters)``."""
    out, ctr = [], {"snv": 0, "indel": 0, "not_matched": 0, "update": 0, "skipped": 0}
    for r in records:
        if r["cadd_scores"] is not None:
            ctr["skipped"] += 1
            continue
        which, row = ref_match(snv, indel, r["metaseq_id"])
        if row is None:
            evidence = {}
            ctr["not_matched"] += 1
        else:
            evidence = {"CADD_raw_score": float(row[4]), "CADD_phred": float(row[5])}
            ctr[which] += 1
            ctr["update"] += 1
        pk = r["record_primary_key"]
        chrm = r.get("chromosome") or "chr" + pk.split(":")[0]
        out.append((pk, chrm, json.dumps(evidence)))
    return out, ctr


# ---- helpers over the package --------------------------------------------------
def run_updater(updater, records):
    """Feed the golden's records to a package CADDUpdater the way the reference's
    driver would: one buffer_variants call per chromosome setting."""
    i = 0
    while i < len(records):
        j = i
        while j < len(records) and records[j]["chromosome"] == records[i]["chromosome"]:
            j += 1
        if records[i]["chromosome"]:
            updater.set_chromosome(records[i]["chromosome"])
        updater.buffer_variants(records[i:j])
        i = j
    return list(updater.update_buffer()), {k: updater.get_count(k)
                                            for k in ("snv", "indel", "not_matched", "update", "skipped")}


CODE = {str(i + 1): i for i in range(22)}
CODE.update({"X": 22, "Y": 23, "M": 24, "MT": 24})


def batch_of(metaseq_ids, residue=None):
    """A CPU RecordBatch of ``chrom:pos:ref:alt`` ids; with ``residue``, junk bytes
    in front of record i's alleles put its heap offset at ``residue[i]`` mod 8."""
    chrom, pos, off, rl, al, heap = [], [], [], [], [], bytearray()
    for i, m in enumerate(metaseq_ids):
        c, p, r, a = m.split(":")
        while residue is not None and len(heap) % 8 != residue[i]:
            heap += b"#"
        chrom.append(CODE.get(c, 255))
        pos.append(int(p))
        off.append(len(heap))
        rl.append(len(r))
        al.append(len(a))
        heap += (r + a).encode()
    heap = bytes(heap) or b"\0"
    pos = torch.from_numpy(np.array(pos, dtype=np.uint32).view(np.int32))  # 2^31 and above: the same bits
    return RecordBatch(chrom=torch.tensor(chrom, dtype=torch.uint8), pos=pos,
                       allele_off=torch.tensor(off, dtype=torch.int64), ref_len=torch.tensor(rl, dtype=torch.int32),
                       alt_len=torch.tensor(al, dtype=torch.int32),
                       heap=torch.from_numpy(np.frombuffer(heap, dtype=np.uint8).copy()))


def expect_arrays(snv_text, indel_text, metaseq_ids):
    """What cadd_match must give for these ids, by the restatement: row index in
    its table (-1), kind, raw and phred (NaN where unmatched)."""
    tabs = {"snv": parse_table(snv_text), "indel": parse_table(indel_text)}
    index = {}
    for name, t in tabs.items():
        k = 0
        for line in (snv_text if name == "snv" else indel_text).decode().split("\n"):
            if line and not line.startswith("#"):
                index.setdefault((name, line), k)  # the first of identical lines
                k += 1
    n = len(metaseq_ids)
    row, kind = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    raw, phred = np.full(n, np.nan), np.full(n, np.nan)
    for i, m in enumerate(metaseq_ids):
        which, r = ref_match(tabs["snv"], tabs["indel"], m)
        if r is not None:
            row[i] = index[(which, "\t".join(r))]
            kind[i] = N.CADD_SNV if which == "snv" else N.CADD_INDEL
            raw[i], phred[i] = float(r[4]), float(r[5])
    return row, kind, raw, phred


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---- the table and the join, restated from include/avdb.h (K10) ------------------
LABEL = {str(i + 1): i for i in range(22)}  # CADD's own contig labels only
LABEL.update({"X": 22, "Y": 23, "MT": 24})
N_CONTIGS = 25
BAD_RUN = 64  # avdb.h: more than 64 BAD rows in a row are an order violation
_POS_RE = re.compile(rb"[0-9]+")
_SCORE_RE = re.compile(rb"-?([0-9]+)(?:\.([0-9]+))?")
TABLE_COLUMNS = (("chrom", np.uint8), ("pos", np.uint32), ("ref_off", np.uint64), ("ref_len", np.uint32),
                 ("alt_off", np.uint64), ("alt_len", np.uint32), ("raw", np.float64), ("phred", np.float64),
                 ("flags", np.uint8))


def data_lines(text: bytes):
    """``[(offset, line)]`` of the data lines (not empty, not '#'), in file order."""
    out, off = [], 0
    for line in text.split(b"\n"):
        if line and not line.startswith(b"#"):
            out.append((off, line))
        off += len(line) + 1
    return out


def expect_score(field: bytes):
    """``(value, left to the host)`` of one score field."""
    m = _SCORE_RE.fullmatch(field)
    if m:
        frac = m.group(2) or b""
        if len((m.group(1) + frac).lstrip(b"0")) <= 15 and len(frac) <= 22:
            return float(field), False
    return 0.0, True


def expect_row(off: int, line: bytes):
    """One data line's row, before the index pass: the TABLE_COLUMNS as a tuple
    (a BAD row's pos is 0 here)."""
    f = line.split(b"\t")
    pos = int(f[1]) if len(f) >= 6 and _POS_RE.fullmatch(f[1]) else 0
    if not 1 <= pos < 2 ** 32:
        return (255, 0, off, 0, off, 0, 0.0, 0.0, N.CADD_ROW_BAD)
    ref_off = off + len(f[0]) + 1 + len(f[1]) + 1
    (raw, h0), (phred, h1) = expect_score(f[4]), expect_score(f[5])
    return (LABEL.get(f[0].decode("latin-1"), 255), pos, ref_off, len(f[2]), ref_off + len(f[2]) + 1, len(f[3]),
            raw, phred, N.CADD_ROW_SCORE_HOST if h0 or h1 else 0)


def expect_table(text: bytes):
    """``(columns, counts)`` avdb_cadd_table_build must give for ``text``: a dict of
    numpy columns (TABLE_COLUMNS, ``first_row``, ``end_row``) and
    ``[rows, score_host, bad, order violations]``."""
    rows = [expect_row(off, line) for off, line in data_lines(text)]
    n = len(rows)
    cols = {name: np.array([r[k] for r in rows], dtype=dt) for k, (name, dt) in enumerate(TABLE_COLUMNS)}
    bad = (cols["flags"] & N.CADD_ROW_BAD) != 0
    chrom, pos = cols["chrom"], cols["pos"]
    # the nearest non-BAD row on either side, across at most BAD_RUN BAD rows (-1: none)
    before, after = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    last = -1
    for i in range(n):
        if last >= 0 and i - last - 1 <= BAD_RUN:
            before[i] = last
        if not bad[i]:
            last = i
    last = -1
    for i in range(n - 1, -1, -1):
        if last >= 0 and last - i - 1 <= BAD_RUN:
            after[i] = last
        if not bad[i]:
            last = i
    first_row, end_row = np.full(N_CONTIGS, 0xFFFFFFFF, np.uint32), np.zeros(N_CONTIGS, np.uint32)
    starts = [0] * N_CONTIGS
    violations = 0
    for i in range(n):
        if i > BAD_RUN and not (~bad[i - BAD_RUN - 1:i]).any():
            violations += 1  # no usable row among the 65 before it
        if bad[i]:
            pos[i] = pos[before[i]] if before[i] >= 0 else 0
            continue
        c = int(chrom[i])
        if c >= N_CONTIGS:
            continue
        if before[i] < 0 or chrom[before[i]] != c:
            starts[c] += 1
            violations += starts[c] > 1
            first_row[c] = min(first_row[c], i)
        elif pos[i] < pos[before[i]]:
            violations += 1
        if after[i] < 0 or chrom[after[i]] != c:
            end_row[c] = max(end_row[c], i + 1)
    cols["first_row"], cols["end_row"] = first_row, end_row
    counts = [n, int(((cols["flags"] & N.CADD_ROW_SCORE_HOST) != 0).sum()), int(bad.sum()), violations]
    return cols, counts


def table_columns(t):
    """A CaddColumns (host or device) as ``(columns, counts)`` in expect_table's form."""
    cols = {name: getattr(t, name).cpu().numpy().view(dt) for name, dt in TABLE_COLUMNS}
    cols["first_row"] = t.first_row.cpu().numpy().view(np.uint32)
    cols["end_row"] = t.end_row.cpu().numpy().view(np.uint32)
    return cols, [int(x) for x in t.counts]


def assert_same_table(got, want, what=""):
    """Two ``(columns, counts)``: every column entry for entry (doubles as bits), all four counts."""
    (gc, gn), (wc, wn) = got, want
    assert list(gn) == list(wn), (what, "counts", gn, wn)
    for name in wc:
        x, y = gc[name], wc[name]
        assert x.dtype == y.dtype and x.shape == y.shape, (what, name, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        if not np.array_equal(x, y):
            k = int(np.nonzero(x != y)[0][0])
            raise AssertionError("%s: column %s differs first at %d: %r != %r" % (what, name, k, x[k], y[k]))


def expect_match(snv_text, indel_text, metaseq_ids):
    """What avdb_cadd_match must give for these ids over tables without order
    violations: ``(row, kind, raw, phred)`` as expect_arrays, with BAD rows (they
    keep their row number and never match) and POS compared as an integer.  A
    record on a contig without a code is ``CADD_HOST``."""
    tabs = []
    for text in (snv_text, indel_text):
        by_contig = {}
        for k, (_, line) in enumerate(data_lines(text)):
            f = line.split(b"\t")
            if len(f) < 6 or not _POS_RE.fullmatch(f[1]) or not 1 <= int(f[1]) < 2 ** 32:
                continue
            c = LABEL.get(f[0].decode("latin-1"))
            if c is not None:
                by_contig.setdefault(c, []).append((int(f[1]), f[2], f[3], k, f[4], f[5]))
        tabs.append(by_contig)
    n = len(metaseq_ids)
    row, kind = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    raw, phred = np.full(n, np.nan), np.full(n, np.nan)
    for i, m in enumerate(metaseq_ids):
        c, p, r, a = m.split(":")
        if c not in CODE:
            kind[i] = N.CADD_HOST
            continue
        r, a, p = r.encode(), a.encode(), int(p)
        is_indel = len(r) > 1 or len(a) > 1
        for tp, tr, ta, k, x, y in tabs[is_indel].get(CODE[c], ()):
            if tp == p and r in (tr, ta) and a in (tr, ta):
                row[i], kind[i] = k, N.CADD_INDEL if is_indel else N.CADD_SNV
                raw[i], phred[i] = float(x), float(y)
                break
    return row, kind, raw, phred



def check_join(eng, snv, indel, ids, what):
    """cadd_match on ``eng`` over the two texts' tables against expect_match: rows,
    kinds, score bits and the three counters; returns the expected ``(row, kind)``."""
    from annotatedvdb_amd.cadd import CaddTable
    snv_t, indel_t = CaddTable.from_text(snv, eng), CaddTable.from_text(indel, eng)  # (raises on a violation)
    ctr = eng.new_cadd_counters()
    row, kind, raw, phred = eng.cadd_match(snv_t.cols, indel_t.cols, batch_of(ids), ctr)
    erow, ekind, eraw, ephred = expect_match(snv, indel, ids)
    row, kind = row.cpu().numpy(), kind.cpu().numpy()
    bad = np.nonzero((row != erow) | (kind != ekind))[0]
    assert not len(bad), (what, ids[bad[0]], int(row[bad[0]]), int(erow[bad[0]]), int(kind[bad[0]]))
    assert np.array_equal(bits(raw.cpu().numpy()), bits(eraw)), what
    assert np.array_equal(bits(phred.cpu().numpy()), bits(ephred)), what
    assert ctr.tolist() == [int((ekind == k).sum()) for k in (N.CADD_SNV, N.CADD_INDEL, N.CADD_NONE)]
    return erow, ekind


# ---- seeded inputs shared by the host and the device tests ----------------------
_SCORES_OK = (b"0.5", b"-1.25", b"12", b"000.75", b"3.141593", b"-0", b"0.000001", b"27.9")
_SCORES_HOST = (b"1e-05", b".5", b"nan", b"1234567890123456", b"5.", b"+1", b"")
_BAD_LINES = (b"1\t5\tA", b"1\tx\tA\tC\t1\t1", b"2\t0\tA\tC\t1\t1", b"1\t4294967296\tA\tC\t1\t1", b"3\t\tA\tC\t1\t1",
              b"junk", b"1\t7\tA\tC\t0.5", b"\t")


def fuzz_table(rng):
    """A small table text with everything the build tells apart: comments, blank
    lines, BAD rows (now and then a run around the 64-row bound), unknown contigs,
    positions that decrease, contigs that come back, extra columns, scores left to
    the host, CRLF, a last line with or without its newline."""
    contigs = rng.sample(["1", "2", "3", "10", "22", "X", "Y", "MT", "GL1", "23", "M", "01"], rng.randint(1, 5))
    lines, pos, c = [], rng.randint(1, 50), contigs[0]
    for _ in range(rng.randint(0, 60)):
        k = rng.random()
        if k < 0.08:
            lines.append(rng.choice((b"", b"#", b"## a comment\twith\ttabs\t1\t2\t3", b"#1\t5\tA\tC\t1\t1")))
        elif k < 0.2:
            lines.append(rng.choice(_BAD_LINES))
        elif k < 0.23:
            lines += [rng.choice(_BAD_LINES)] * rng.randint(60, 70)
        else:
            if rng.random() < 0.12:
                c = rng.choice(contigs)
            pos = max(1, pos + rng.choice((0, 0, 1, 1, 2, 7, 1000, -1, -3)))
            if rng.random() < 0.03:
                pos = rng.choice((2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1))
            ref = "".join(rng.choice("ACGT") for _ in range(rng.choice((1, 1, 1, 2, 5, 0))))
            alt = "".join(rng.choice("ACGT") for _ in range(rng.choice((1, 1, 1, 3, 9, 0))))
            score = [rng.choice(_SCORES_HOST if rng.random() < 0.1 else _SCORES_OK) for _ in range(2)]
            line = b"\t".join([c.encode(), b"%d" % pos, ref.encode(), alt.encode()] + score)
            if rng.random() < 0.15:
                line += rng.choice((b"\textra", b"\t", b"\t1\t2\t3\t\t", b"\r"))
            lines.append(line)
    text = b"\n".join(lines)
    return text + rng.choice((b"", b"\n", b"\n\n")) if lines else text


def _bases(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def join_case(rng, edge=False):
    """``(snv_text, indel_text, ids)``: two tables without order violations and
    queries aimed at them.  Rows: many at one position, ``ref == alt``, empty
    alleles, BAD rows inside a same-position group (one with the group's own
    alleles in its unusable line), positions 2^31 and 2^32 - 1, neighbouring
    positions.  Queries per sampled row: as written, switched, ``ref == alt``,
    another ALT, the positions beside it, another contig, a contig without a code,
    and empty alleles (what a BAD row's zero-length alleles would equal).
    ``edge``: also a 300-row group whose only match is its last row, with a BAD row
    in it, and a query at a contig's last position whose alleles stand only in the
    next contig's first row at that position."""
    texts, ids = [], []
    for indel in (False, True):
        contigs = rng.sample(["1", "2", "7", "19", "22", "X", "Y", "MT", "GL9"], rng.randint(2, 5))
        nxt = contigs.pop(1 if contigs[1] != "GL9" else 0) if edge else None
        if edge and contigs[0] == "GL9":
            contigs[0] = "3"
        lines, good = [b"## CADD", b"#Chrom\tPos\tRef\tAlt\tRawScore\tPHRED"], []
        for ci, c in enumerate(contigs):
            pos = rng.randint(1, 30)
            if rng.random() < 0.2:
                lines.append(rng.choice(_BAD_LINES))  # a BAD row between two contigs
            for g in range(rng.randint(1, 12)):
                pos += rng.choice((1, 1, 2, 50))
                if g >= 8 and rng.random() < 0.5:
                    pos = max(pos, rng.choice((2 ** 31, 2 ** 32 - 1)))
                for _ in range(rng.choice((1, 1, 2, 4, 9))):
                    if indel:
                        ref, alt = _bases(rng, rng.choice((1, 1, 2, 4))), _bases(rng, rng.choice((1, 2, 3, 17, 0)))
                    else:
                        ref, alt = _bases(rng, rng.choice((1, 1, 1, 1, 0))), _bases(rng, 1)
                    if rng.random() < 0.1:
                        alt = ref
                    if rng.random() < 0.15:  # unusable lines carrying the alleles of the row that follows them
                        lines.append(b"%s\t%dx\t%s\t%s\t1\t1" % (c.encode(), pos, ref.encode(), alt.encode()))
                        lines.append(b"%s\t%d\t%s\t%s\t1" % (c.encode(), pos, ref.encode(), alt.encode()))
                    score = b"%.6f\t%.3f" % (rng.uniform(-5, 30), rng.uniform(0, 60))
                    lines.append(b"%s\t%d\t%s\t%s\t%s" % (c.encode(), pos, ref.encode(), alt.encode(), score))
                    good.append((c, pos, ref, alt))
                if pos >= 2 ** 32 - 1:
                    break
            if edge and ci == 0:
                # 300 rows at one position; only the last carries the queried pair, and the
                # BAD row among them carries it too
                pos = min(pos + 3, 2 ** 32 - 1)
                ref, alt = ("ACG", "A") if indel else ("A", "C")
                other = ("ACG", "AC") if indel else ("A", "G")
                for k in range(299):
                    if k == 150:
                        lines.append(b"%s\t-%d\t%s\t%s\t1\t1" % (c.encode(), pos, ref.encode(), alt.encode()))
                    lines.append(b"%s\t%d\t%s\t%s\t%d.5\t1" % (c.encode(), pos, other[0].encode(), other[1].encode(),
                                                                k))
                lines.append(b"%s\t%d\t%s\t%s\t-7.125\t9.75" % (c.encode(), pos, ref.encode(), alt.encode()))
                ids += ["%s:%d:%s:%s" % (c, pos, ref, alt), "%s:%d:%s:%s" % (c, pos, alt, ref),
                        "%s:%d:%s:%s" % (c, pos, other[0], other[1]), "%s:%d::" % (c, pos)]
                # the contig ends at `pos`; the next one starts at the same position with other alleles
                only = ("T", "TGG") if indel else ("T", "G")
                lines.append(b"%s\t%d\t%s\t%s\t2.5\t3.5" % (nxt.encode(), pos, only[0].encode(), only[1].encode()))
                lines.append(b"%s\t%d\t%s\t%s\t4.5\t5.5" % (nxt.encode(), min(pos + 1, 2 ** 32 - 1), ref.encode(),
                                                              alt.encode()))
                ids += ["%s:%d:%s:%s" % (c, pos, only[0], only[1]), "%s:%d:%s:%s" % (nxt, pos, only[0], only[1]),
                        "%s:%d:%s:%s" % (nxt, pos, ref, alt)]
        texts.append(b"\n".join(lines) + rng.choice((b"", b"\n")))
        others = ["1", "2", "7", "19", "22", "X", "Y", "M"]
        for c, pos, ref, alt in rng.sample(good, min(len(good), 40)):
            q = "M" if c == "MT" else c
            wrong = _bases(rng, len(alt) or 1)
            ids += ["%s:%d:%s:%s" % (q, pos, ref, alt), "%s:%d:%s:%s" % (q, pos, alt, ref),
                    "%s:%d:%s:%s" % (q, pos, ref, ref), "%s:%d:%s:%s" % (q, pos, alt, alt),
                    "%s:%d:%s:%s" % (q, pos, ref, wrong), "%s:%d:%s:%s" % (q, max(pos - 1, 0), ref, alt),
                    "%s:%d:%s:%s" % (q, min(pos + 1, 2 ** 32 - 1), ref, alt),
                    "%s:%d:%s:%s" % (rng.choice(others), pos, ref, alt), "GL9:%d:%s:%s" % (pos, ref, alt),
                    "%s:%d::" % (q, pos), "%s:%d:%s:" % (q, pos, ref)]
    return texts[0], texts[1], ids

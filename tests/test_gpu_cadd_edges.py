"""K10 on the device where the golden does not reach: the table build against the
restatement written from include/avdb.h (cadd_common.expect_table) *and* the
library's host entry, at k_cadd_parse's own geometry (256 lines per trip staged in
16 KiB of LDS, or parsed from global memory when the trip's span does not fit), on
unaligned slabs, with rows != lines, across workgroups in k_cadd_index, on a second
grid-stride trip; scores parsed and patched on the device; the join's edges."""

import random

import numpy as np
import pytest
import torch

import cadd_common as C
import test_gpu_cadd as G
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.cadd import CaddTable
from annotatedvdb_amd.engine import Engine

pytestmark = pytest.mark.gpu

HEADER = G.HEADER
TRIP = 256          # lines per k_cadd_parse trip (one workgroup)
STAGE = 16 * 1024   # its LDS stage: a trip is staged when its span, counted from the
#                     16-byte floor of its first line's address, is at most this
GRID = 4096         # workgroups at most: line 4096 * 256 is workgroup 0's second trip
ODD = HEADER + b"1\t5\tA\tC\t1e-05\t1.5\n1\t6\tA\n\n1\tx\tA\tC\t1\t1\n1\t7\tAT\tA\t-0.000000\t.5\r\n" \
               b"GL1\t7\tA\tC\t1\t2\n2\t9\tA\tC\t1\t2\n1\t9\tA\tC\t1234567890.123456\t2\n2\t8\tA\tC\t1\t2"


@pytest.fixture(scope="module")
def host():
    return Engine("host")


def check_table(engine, host, text, what, slab=None):
    """The device table of ``text`` (or of ``slab``, a device tensor holding it)
    against the restatement and the host entry; returns the expected table."""
    want = C.expect_table(text)
    ref = C.table_columns(host.cadd_table_build(text))
    dev = C.table_columns(engine.cadd_table_build(text if slab is None else slab))
    C.assert_same_table(ref, want, what + ": host entry against the restatement")
    C.assert_same_table(dev, want, what + ": device against the restatement")
    C.assert_same_table(dev, ref, what + ": device against the host entry")
    return want


def trip_spans(text, residue=0):
    """Per trip of 256 lines (no line is skipped before the trips are cut: headers
    and blank lines are lines too), the bytes k_cadd_parse would stage for a slab
    whose address is ``residue`` mod 16."""
    a = np.frombuffer(text, dtype=np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(a == 10) + 1))
    if starts[-1] == len(text):
        starts = starts[:-1]  # the text ends in its last line's newline
    s0 = starts[::TRIP]
    s1 = np.concatenate((s0[1:], [len(text)]))
    return (s1 + residue) - ((s0 + residue) & ~np.int64(15))


def test_e1_restatement_on_the_device(engine, host):
    snv, indel, _, _ = C.golden()
    for what, text in (("snv", snv), ("indel", indel), ("window_slab", G.window_slab()), ("odd", ODD)):
        check_table(engine, host, text, what)


# ---- e2 / e3: the stage's fit boundary ------------------------------------------
LONG = "long"  # a trip holding one line with a 20,000-byte ALT


def fit_line(i, fill):
    """Data line i + a 7th column of ``fill`` bytes (-1: no 7th column)."""
    line = b"1\t%07d\t%c\t%c\t%d.%02d\t%d.5" % (1000000 + i, b"ACGT"[i % 4], b"CGTA"[i % 4], i % 10, i % 100, i % 10)
    return line + (b"\t" + b"f" * fill if fill >= 0 else b"") + b"\n"


FIT0 = len(fit_line(0, 0))  # a line with an empty 7th column


def fit_text(spans, residue=0, tail_lines=100):
    """Header-less text whose trip k stages exactly ``spans[k]`` bytes on a slab at
    ``residue`` mod 16, then ``tail_lines`` plain lines, the last without newline."""
    out, at, i = [], 0, 0
    for span in spans:
        if span == LONG:
            lines = [fit_line(i + k, k % 3 - 1) for k in range(TRIP)]
            big = bytes(b"ACGT"[(k * 7 + k // 5) % 4] for k in range(20000))
            lines[100] = b"1\t%07d\tA\t%s\t0.25\t2.5\tx\n" % (1000000 + i + 100, big)
        else:
            # every 4th line ends at its PHRED; the others share the bytes left as 7th-column filler
            room = span - ((at + residue) - ((at + residue) & ~15)) - (TRIP * FIT0 - TRIP // 4)
            assert room >= 0
            q, r = divmod(room, TRIP - TRIP // 4)
            lines = [fit_line(i + k, -1 if k % 4 == 3 else q + (k - k // 4 < r)) for k in range(TRIP)]
        out += lines
        at += sum(len(ln) for ln in lines)
        i += TRIP
    out += [fit_line(i + k, k % 5 - 1) for k in range(tail_lines)]
    return b"".join(out)[:-1]


def fit_plan(first):
    """Trip 0 at ``first`` bytes, then fitting and non-fitting trips in turn."""
    rest = [16385, 16384, LONG, 16368, 16400] if first <= STAGE else [16384, 16385, 16368, LONG, 16384, 16400]
    return [first] + rest


def check_fit_plan(text, plan, residue=0):
    spans = trip_spans(text, residue).tolist()
    assert len(spans) == len(plan) + 1 and spans[-1] < STAGE
    assert [s for s, p in zip(spans, plan) if p != LONG] == [p for p in plan if p != LONG], spans
    assert all(s > 20000 for s, p in zip(spans, plan) if p == LONG)
    fits = [s <= STAGE for s in spans]
    assert all(a != b for a, b in zip(fits, fits[1:])), fits  # staged and unstaged trips alternate
    return fits


@pytest.mark.parametrize("first", [16368, 16384, 16385, 16400])
def test_e2_stage_fit_boundary(engine, host, first):
    """Trip 0 stages 16,368 / 16,384 bytes (the last that fits) or is parsed from
    global memory at 16,385 / 16,400; the trips after it alternate, one of them
    holds a line longer than the whole stage, the last line has no newline."""
    plan = fit_plan(first)
    text = fit_text(plan)
    fits = check_fit_plan(text, plan)
    assert fits[0] == (first <= STAGE) and not text.endswith(b"\n")
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(engine.device)
    assert slab.data_ptr() % 16 == 0
    cols, counts = check_table(engine, host, text, "first trip %d" % first, slab)
    assert counts == [len(plan) * TRIP + 100, 0, 0, 0] and cols["alt_len"].max() == 20000


JUNK = b"\n1\t1\tA\tC\t9\t9\n"


def unaligned(engine, text, k):
    """``text`` on the device ``k`` bytes into an allocation, junk lines before and
    after it: a read outside the slice shows as a row that should not be there."""
    tail = JUNK * 8
    whole = (JUNK * 2)[-k:] + text + tail
    assert len(tail) >= 64
    dev = torch.from_numpy(np.frombuffer(whole, dtype=np.uint8).copy()).to(engine.device)
    assert dev.data_ptr() % 16 == 0
    slab = dev[k:k + len(text)]
    assert slab.is_contiguous() and slab.data_ptr() % 16 == k
    return slab


@pytest.mark.parametrize("k", [1, 7, 8, 15])
def test_e3_unaligned_slab(engine, host, k):
    """The slab ``k`` bytes off 16-byte alignment: the stage's first word starts
    before the text, and the fit boundary moves with the address — the e2 text is
    built for this residue, so 16,384 / 16,385 are again exact."""
    plan = fit_plan(16384 if k % 2 else 16385)
    text = fit_text(plan, residue=k)
    check_fit_plan(text, plan, residue=k)
    check_table(engine, host, text, "fit text at +%d" % k, unaligned(engine, text, k))
    snv, _, _, _ = C.golden()
    for what, t in (("snv", snv), ("snv without its last newline", snv[:-1])):
        check_table(engine, host, t, "%s at +%d" % (what, k), unaligned(engine, t, k))


# ---- e4: rows != lines ----------------------------------------------------------
def sparse_text():
    """About 2,000 lines with '#' and empty lines throughout (runs of them too),
    trip 2 nothing but comments, a data line in the last lane of trip 0 and the
    first of trip 1, a few CRLF lines."""
    lines, pos, crlf = [], 10, 0
    for i in range(2000):
        trip, lane = divmod(i, TRIP)
        data = b"%d\t%d\t%c\t%c\t%d.25\t%d.5" % (1 + i // 700, pos, b"ACGT"[i % 4], b"TGCA"[i % 4], i % 50, i % 40)
        if trip == 2:
            line = b"#" + b"c" * (i % 90)
        elif (trip, lane) in ((0, TRIP - 1), (1, 0)):
            line = data
        elif i % 7 == 3 or 900 <= i < 910:
            line = b"## comment %d\twith\ttabs\t1\t2\t3" % i
        elif i % 11 == 5 or 1300 <= i < 1304 or i < 2:
            line = b""
        elif i % 97 == 50:
            line, crlf = data + b"\r", crlf + 1
        else:
            line = data
        if line is data or line.endswith(b"\r"):
            pos += i % 3
        lines.append(line)
    return lines, crlf


def test_e4_rows_are_not_lines(engine, host):
    lines, crlf = sparse_text()
    is_data = [bool(ln) and not ln.startswith(b"#") for ln in lines]
    assert is_data[TRIP - 1] and is_data[TRIP] and not any(is_data[2 * TRIP:3 * TRIP]) and not any(is_data[:2])
    assert b"\n\n\n\n" in b"\n".join(lines) and crlf >= 10
    for what, text in (("newline at the end", b"\n".join(lines) + b"\n"), ("no newline at the end", b"\n".join(lines)),
                       ("blank lines at the end", b"\n".join(lines) + b"\n\n\n")):
        cols, counts = check_table(engine, host, text, "sparse text, " + what)
        assert counts == [sum(is_data), crlf, 0, 0]  # a CRLF line's PHRED is the host's; the row stays good
        assert int((cols["flags"] == N.CADD_ROW_SCORE_HOST).sum()) == crlf


# ---- e5: the index across workgroups -----------------------------------------------
BAD_LINE = b"4\tx\tA\tC\t1\t1"
LABELS = [str(i + 1) for i in range(22)] + ["X", "Y", "MT"]


def index_rows():
    """``[label or None (BAD), pos]`` per row (no header: row == line).  Contig
    boundaries at rows 255|256, 256|257 (contig 2 is one row) and 511|512; contig 4
    spans rows 512..1711; BAD runs of 64 and 63 inside contig 4 across rows 768 and
    1024, of 63 and 64 between two contigs across rows 1792 and 2048, single BAD
    rows in the last lane (2303) and the first lane (2560) of a workgroup, both
    between two contigs; row 0 and the last row are BAD."""
    rows = [[None, 0]]
    def good(label, n):
        rows.extend([label, 100 + 3 * k // 2] for k in range(n))
    def bad(n):
        rows.extend([None, 0] for _ in range(n))
    good("1", 255), good("2", 1), good("3", 255), good("4", 1200)
    for at, n in ((736, 64), (993, 63)):
        for r in range(at, at + n):
            rows[r][0] = None
    good("5", 48), bad(63), good("6", 193), bad(64), good("7", 223), bad(1), good("8", 256), bad(1)
    for label in LABELS[8:]:
        good(label, 25)
    bad(1)
    return rows


def index_text(rows):
    return b"\n".join(BAD_LINE if label is None else b"%s\t%d\tA\tC\t0.5\t1.5" % (label.encode(), pos)
                      for label, pos in rows) + b"\n"


def bad_runs(rows):
    runs, r = [], 0
    while r < len(rows):
        e = r
        while e < len(rows) and rows[e][0] is None:
            e += 1
        if e > r:
            runs.append((r, e - r))
        r = max(e, r + 1)
    return runs


def test_e5_index_across_workgroups(engine, host):
    rows = index_rows()
    n = len(rows)
    label = [r[0] for r in rows]
    assert (label[255], label[256], label[257], label[511], label[512], label[1711], label[1712]) == \
           ("1", "2", "3", "3", "4", "4", "5")
    assert bad_runs(rows) == [(0, 1), (736, 64), (993, 63), (1760, 63), (2016, 64), (2303, 1), (2560, 1), (n - 1, 1)]
    assert (label[1759], label[1823], label[2015], label[2080], label[2302], label[2304], label[2559], label[2561]) == \
           ("5", "6", "6", "7", "7", "8", "8", "9")
    cols, counts = check_table(engine, host, index_text(rows), "index table")
    assert counts == [n, 0, 64 + 63 + 63 + 64 + 4, 0] and 2900 < n < 3100
    first, end = cols["first_row"].tolist(), cols["end_row"].tolist()
    assert first[:9] == [1, 256, 257, 512, 1712, 1823, 2080, 2304, 2561]
    assert end[:9] == [256, 257, 512, 1712, 1760, 2016, 2303, 2560, 2586] and end[24] == n - 1
    assert all(e - f == 25 for f, e in zip(first[8:], end[8:]))

    def variant(what, edit, violations):
        v = [list(r) for r in rows]
        edit(v)
        _, c = check_table(engine, host, index_text(v), what)
        assert c[3] == violations, (what, c)

    def run_of_65(v):
        v[800][0] = None  # 736 .. 800: row 801 sees no usable row, and contig 4 starts again there
    def second_run_far_away(v):
        v[2700][0] = "1"  # contig 1 comes back nine workgroups later, splitting that contig in two
    def decrease_at_an_edge(v):
        v[1280][1] = v[1279][1] - 1
        v[1281][1] = v[1279][1]
    def decrease_across_a_bad_row(v):
        v[1400][0] = None
        v[1401][1] = v[1399][1] - 1
    def unknown_contig_inside_a_run(v):
        v[1500][0] = "GL7"

    variant("a BAD run of 65", run_of_65, 2)
    variant("a second run far away", second_run_far_away, 2)
    variant("pos decreases across a 256-row edge", decrease_at_an_edge, 1)
    variant("pos decreases across a BAD row", decrease_across_a_bad_row, 1)
    variant("an unknown contig inside a run", unknown_contig_inside_a_run, 1)


# ---- e6: a second grid-stride trip ---------------------------------------------
def big_text():
    """4096 * 256 + 300 lines: a block of 16 trips 256 times over, then a tail of
    300 lines.  The block's byte length is a multiple of 16, so every copy stages
    alike: its trip 0 fits the stage and its trip 1 does not; the tail's first 256
    lines (workgroup 0's second trip) do not fit, its last 44 (workgroup 1's) do."""
    def line(i, fill):
        if i % 61 == 17:
            return b"#c%d\n" % (i % 1000)
        if i % 509 == 100:
            return b"1\t\tA\tC\t1\t1\n"  # BAD
        seventh = b"\t" + b"f" * fill if fill else b""
        return b"%d\t%d\t%c\t%c\t%d.%03d\t%d.5%s\n" % (1 + i // 1500 % 3, 1000 + i, b"ACGT"[i % 4], b"GTAC"[i % 4],
                                                  i % 7, i % 1000, i % 30, seventh)
    # (a long trip: every other line with a 7th column, the rest ending at their PHRED)
    block = [line(i, 128 * (i % 2) if i // TRIP in (1, 6, 11) else 0) for i in range(16 * TRIP)]
    pad = -sum(len(ln) for ln in block) % 16
    block[5] = block[5][:-1] + b"\t" + b"p" * (pad + 15) + b"\n"
    block = b"".join(block)
    assert len(block) % 16 == 0
    tail = b"".join([line(i, 140 * (i % 2)) for i in range(TRIP)] + [line(i, 0) for i in range(300 - TRIP)])
    return block * (GRID * TRIP // (16 * TRIP)) + tail


def test_e6_second_grid_stride_trip(engine, host):
    text = big_text()
    a = np.frombuffer(text, dtype=np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(a == 10) + 1))[:-1]
    n_lines = len(starts)
    assert n_lines == GRID * TRIP + 300 and len(text) < 48 << 20
    fits = trip_spans(text) <= STAGE
    # workgroup 0: trips 0 and 4096; workgroup 1: trips 1 and 4097
    assert (fits[0], fits[GRID], fits[1], fits[GRID + 1]) == (True, False, False, True) and len(fits) == GRID + 2
    dev, ref = engine.cadd_table_build(text), host.cadd_table_build(text)
    G.same_table(dev, ref)  # every row, every column, the four counts
    got, _ = C.table_columns(dev)
    ends = np.concatenate((starts[1:] - 1, [len(text) - 1]))
    is_data = (ends > starts) & (a[starts] != ord("#"))
    row_of = np.cumsum(is_data) - is_data
    assert dev.n_rows == int(is_data.sum()) < n_lines and int(ref.counts[N.CADD_COUNT_BAD]) > 2000
    rng = np.random.default_rng(6)
    picked = np.unique(np.concatenate((np.arange(600), np.arange(GRID * TRIP - 300, GRID * TRIP + 300),
                                       rng.integers(0, n_lines, 2000))))
    checked = 0
    for li in picked[is_data[picked]].tolist():
        s, r = int(starts[li]), int(row_of[li])
        want = C.expect_row(s, text[s:int(ends[li])])
        for k, (name, _) in enumerate(C.TABLE_COLUMNS):
            if name == "pos" and want[8] & N.CADD_ROW_BAD:
                continue  # (a BAD row's pos is the index pass's: the host entry's, above)
            x = got[name][r]
            assert (C.bits(x) == C.bits(want[k])) if name in ("raw", "phred") else (int(x) == want[k]), (li, r, name)
        checked += 1
    assert checked > 3000
    del dev, ref, got

    # the join's second trip: 4096 * 256 + 65 records
    n = GRID * TRIP + 65
    snv_t, indel_t = CaddTable.from_text(G.SMALL_SNV, engine), CaddTable.from_text(G.SMALL_INDEL, engine)
    b = C.batch_of(G.SMALL_QUERIES)
    q = len(G.SMALL_QUERIES)
    reps = -(-n // q)
    big = type(b)(chrom=b.chrom.repeat(reps)[:n], pos=b.pos.repeat(reps)[:n], allele_off=b.allele_off.repeat(reps)[:n],
                  ref_len=b.ref_len.repeat(reps)[:n], alt_len=b.alt_len.repeat(reps)[:n], heap=b.heap)
    d = engine.device
    out = (torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device=d),
           torch.full((n + 16,), 0x5A, dtype=torch.uint8, device=d),
           torch.full((n + 16,), -12345.5, dtype=torch.float64, device=d),
           torch.full((n + 16,), -12345.5, dtype=torch.float64, device=d))
    ctr = engine.new_cadd_counters()
    row, kind, raw, phred = engine.cadd_match(snv_t.cols, indel_t.cols, big, ctr, out=out)
    erow, ekind, eraw, ephred = (np.tile(x, reps)[:n] for x in C.expect_arrays(G.SMALL_SNV, G.SMALL_INDEL,
                                                                             G.SMALL_QUERIES))
    assert np.array_equal(row.cpu().numpy(), erow) and np.array_equal(kind.cpu().numpy(), ekind)
    hit = erow >= 0
    for x, want in ((raw, eraw), (phred, ephred)):
        x = x.cpu().numpy()
        assert np.array_equal(C.bits(x[hit]), C.bits(want[hit])) and (x[~hit] == -12345.5).all()
    assert (out[0][n:] == 0x5A5A5A5A).all() and (out[1][n:] == 0x5A).all()
    assert (out[2][n:] == -12345.5).all() and (out[3][n:] == -12345.5).all()
    assert ctr.tolist() == [int((ekind == k).sum()) for k in (N.CADD_SNV, N.CADD_INDEL, N.CADD_NONE)]
    assert min(ctr.tolist()) > 0 and sum(ctr.tolist()) == n


# ---- e7 / e8: scores ------------------------------------------------------------
def score_texts():
    """The pairs of test_cadd_host.test_t2_scores_bit_exact_against_float, then what
    the grammar allows at its edges: 15 significant digits with 0 .. 22 fractional
    digits, integers up to 2^53's neighbourhood, leading zeros, every form of -0."""
    hand = [b"0", b"-0.000000", b"0.1", b"12.345", b"-7.250000", b"123456789.012345", b"0.0000000123456789012345",
            b"-0", b"000012.5", b"999999999999999", b"0.000000", b"0.0000000000000000000001"]
    rng = random.Random(11)
    seeded = [(b"%.6f" % rng.uniform(-10, 40), b"%.3f" % rng.uniform(0, 99)) for _ in range(20000)]
    pairs = [(s, hand[(i + 1) % len(hand)]) for i, s in enumerate(hand)] + seeded
    assert len(pairs) == 20012
    edge = [b"999999999999999", b"0.0000000999999999999999", b"9007199254740.99", b"0", b"-0", b"-0.0", b"-00.000",
            b"-0.0000000000000000000000", b"0.0000000000000000000000", b"0000000000000000000000000000001.5",
            b"0.0000000000000000000001", b"000.0000000123456789012345", b"100000000000000", b"1.00000000000000",
            b"56294995342131.5", b"4503599627370.49", b"0.3", b"0.7", b"2.675", b"1.005", b"8.41", b"0.1",
            b"123456789012345"]
    rng = random.Random(7)
    digits = [b"999999999999999", b"100000000000001", b"123456789012345", b"900719925474099", b"450359962737049"]
    digits += [b"%015d" % rng.randrange(10 ** 14, 10 ** 15) for _ in range(40)]
    for d in digits:
        for frac in range(23):
            s = d[:15 - frac] + b"." + d[15 - frac:] if 0 < frac < 15 else d if frac == 0 else \
                b"0." + b"0" * (frac - 15) + d
            edge.append(s)
    edge += [b"-" + s for s in edge if not s.startswith(b"-")]
    return pairs + [(s, edge[-1 - i]) for i, s in enumerate(edge)]


def test_e7_scores_on_the_device(engine):
    """The one f64 division per score, on gfx950, against float() bit for bit."""
    pairs = score_texts()
    assert len(pairs) > 22000 and all(not C.expect_score(s)[1] for p in pairs for s in p)
    text = HEADER + b"".join(b"1\t%d\tA\tC\t%s\t%s\n" % (i + 1, x, y) for i, (x, y) in enumerate(pairs))
    cols = engine.cadd_table_build(text)
    assert cols.n_rows == len(pairs) and [int(x) for x in cols.counts] == [len(pairs), 0, 0, 0]
    assert not cols.flags.cpu().numpy().any()
    raw, phred = C.bits(cols.raw.cpu().numpy()), C.bits(cols.phred.cpu().numpy())
    want_raw, want_phred = C.bits([float(x) for x, _ in pairs]), C.bits([float(y) for _, y in pairs])
    for got, want, k in ((raw, want_raw, 0), (phred, want_phred, 1)):
        bad = np.nonzero(got != want)[0]
        assert not len(bad), (pairs[bad[0]][k], len(bad))
    assert raw[1] == np.int64(-2 ** 63) and int((want_raw == np.int64(-2 ** 63)).sum()) >= 5  # -0.0 keeps its sign


def test_e8_host_left_scores_patched_on_the_device(engine):
    odd = [b"1234567890.123456", b"1e-05", b".5", b"3.2\r", b"nan", b"5.", b"+1.5", b"1234567890123456",
           b"0.00000000000000000000001"]
    pairs = []
    for i, s in enumerate(odd):
        pairs += [(s, b"1.5"), (b"%d.25" % i, b"%d.5" % i), (b"2.5", s), (b"-%d.125" % i, b"0.75")]
    text = HEADER + b"".join(b"1\t%d\tA\tC\t%s\t%s\n" % (i + 1, x, y) for i, (x, y) in enumerate(pairs))
    plain = engine.cadd_table_build(text)  # before the patch: the flagged rows' scores are 0.0
    flagged = np.arange(len(pairs)) % 2 == 0
    assert np.array_equal(plain.flags.cpu().numpy(), np.where(flagged, N.CADD_ROW_SCORE_HOST, 0).astype(np.uint8))
    assert not plain.raw.cpu().numpy()[0::4].any() and not plain.phred.cpu().numpy()[2::4].any()
    t = CaddTable.from_text(text, engine)
    assert t.counts["score_host"] == 2 * len(odd) and t.counts["rows"] == len(pairs)
    assert t.cols.raw.device == plain.raw.device  # patched where the columns live
    want_raw, want_phred = [float(x) for x, _ in pairs], [float(y) for _, y in pairs]
    for got, before, want in ((t.cols.raw, plain.raw, want_raw), (t.cols.phred, plain.phred, want_phred)):
        got = got.cpu().numpy()
        assert np.array_equal(C.bits(got), C.bits(want))
        assert np.array_equal(C.bits(got[~flagged]), C.bits(before.cpu().numpy()[~flagged]))  # the others: untouched
    ids = ["1:%d:A:C" % (i + 1) for i in range(len(pairs))]
    row, kind, raw, phred = engine.cadd_match(t.cols, None, C.batch_of(ids))
    assert row.cpu().numpy().tolist() == list(range(len(pairs))) and (kind == N.CADD_SNV).all()
    assert np.array_equal(C.bits(raw.cpu().numpy()), C.bits(want_raw))  # (nan's bits included)
    assert np.array_equal(C.bits(phred.cpu().numpy()), C.bits(want_phred))


# ---- e9: the join's edges ---------------------------------------------------------
def test_e9_join_edges_on_the_device(engine):
    """The host tests' seeded join cases (test_cadd_host.test_t6_*) on the device."""
    rng = random.Random(99)
    n, hits, kinds = 0, 0, set()
    for k in range(12):
        snv, indel, ids = C.join_case(rng, edge=k % 2 == 0)
        erow, ekind = C.check_join(engine, snv, indel, ids, "case %d" % k)
        n, hits, kinds = n + len(ids), hits + int((erow >= 0).sum()), kinds | set(ekind.tolist())
    assert n > 3000 and hits > n // 5 and kinds == {N.CADD_NONE, N.CADD_SNV, N.CADD_INDEL, N.CADD_HOST}
    P = 2 ** 32 - 1
    snv = HEADER + b"1\t2147483648\tA\tC\t0.5\t1.5\n1\t2147483648\tA\t1\n1\t2147483648x\tG\tT\t9\t9\n" \
                   b"1\t2147483648\tG\tT\t0.25\t2.5\n1\t%d\tA\tA\t1.5\t3.5\n2\t%d\tC\tG\t2.5\t4.5\n" % (P, P)
    ids = ["1:2147483648:A:C", "1:2147483648:T:G", "1:2147483648::", "1:%d:A:A" % P, "1:%d:C:G" % P, "2:%d:G:C" % P,
           "1:2147483647:A:C", "1:0:A:C", "3:%d:C:G" % P, "GL1:5:A:C"]
    erow, ekind = C.check_join(engine, snv, HEADER, ids, "by hand")
    assert erow.tolist() == [0, 3, -1, 4, -1, 5, -1, -1, -1, -1]
    assert ekind.tolist() == [1, 1, 0, 1, 0, 1, 0, 0, 0, N.CADD_HOST]

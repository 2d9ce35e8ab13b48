"""Shared by the K12 tests (test_existing_host.py, test_gpu_existing_export.py): a
restatement of ExistingVariants.from_tsv's parse over bytes, the slabs H1-H4 and the
comparison of an engine's columns with it."""

import io

import numpy as np

from annotatedvdb_amd import _native as N
from annotatedvdb_amd.chromosomes import CHROM_NAMES

LONG = 40000  # longer than any LDS stage of the kernels


def printable_rule(s: str) -> bool:
    """True when repr() renders s verbatim inside single quotes."""
    return all(0x20 <= ord(c) <= 0x7E and c not in "'\\" for c in s)


def label_of(metaseq: str) -> str:
    return metaseq.split(":")[0]


def parse(text: bytes):
    """from_tsv's rows: text mode with universal newlines, rstrip, split, the two skips."""
    rows, n_lines = [], 0
    for line in io.TextIOWrapper(io.BytesIO(text), encoding="utf-8", newline=None):
        n_lines += 1
        f = line.rstrip("\n").split("\t")
        if len(f) < 3 or f[0] == "metaseq_id":
            continue
        rows.append((f[0], f[1], f[2]))
    return rows, n_lines


def restate(text: bytes) -> dict:
    rows, n_lines = parse(text)
    keys = [r[0].encode() for r in rows]
    pks = [r[1].encode() for r in rows]
    frags = [repr({"primary_key": r[1], "bin_index": r[2]}).encode() for r in rows]
    flags = np.array([(0 if printable_rule(r[1]) and printable_rule(r[2]) else N.EXIST_FRAG_HOST) |
                      (0 if label_of(r[0]) in CHROM_NAMES else N.EXIST_NONCANON) for r in rows], dtype=np.uint8)

    def blob(parts):
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(p) for p in parts], out=off[1:])
        return b"".join(parts), off

    out = {"flags": flags}
    out["keys"], out["key_off"] = blob(keys)
    out["pks"], out["pk_off"] = blob(pks)
    out["frag"], out["frag_off"] = blob(frags)
    out["counts"] = {"rows": len(rows), "skipped": n_lines - len(rows),
                     "frag_host": int(((flags & N.EXIST_FRAG_HOST) != 0).sum()),
                     "noncanon": int(((flags & N.EXIST_NONCANON) != 0).sum()), "lone_cr": 0,
                     "key_bytes": len(out["keys"]), "pk_bytes": len(out["pks"]),
                     "frag_bytes": sum(36 + len(r[1].encode()) + len(r[2].encode()) for r in rows)}
    return out


def columns(engine, text: bytes, contigs=None) -> dict:
    """existing_table_build's result as host bytes / arrays, shaped like restate()."""
    c = engine.existing_table_build(text, contigs)

    def b(t, n):
        return t.cpu().numpy().tobytes()[:n]

    out = {"flags": c.flags.cpu().numpy(), "counts": dict(c.counts)}
    for name, off in (("keys", "key_off"), ("pks", "pk_off"), ("frag", "frag_off")):
        o = getattr(c, off).cpu().numpy()
        assert o.shape == (c.n_rows + 1,) and o[0] == 0
        out[off] = o
        out[name] = b(getattr(c, name), int(o[-1]))
    return out


def assert_same(got: dict, want: dict, counts=True):
    for k in ("key_off", "pk_off", "frag_off", "flags"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("keys", "pks", "frag"):
        assert got[k] == want[k], k
    if counts:
        assert got["counts"] == want["counts"]


def filtered(text: bytes, labels) -> bytes:
    """The text without the rows whose contig label the mask drops (lines that are no
    row stay: they are skipped either way)."""
    keep_other = any(c not in CHROM_NAMES for c in labels)
    out = []
    for ln in text.split(b"\n"):
        f = ln.rstrip(b"\r").split(b"\t")
        if len(f) >= 3 and f[0] != b"metaseq_id":
            lab = f[0].split(b":")[0].decode()
            if not (lab in labels if lab in CHROM_NAMES else keep_other):
                continue
        out.append(ln)
    return b"\n".join(out)


# ---- slabs ---------------------------------------------------------------------
BIN = "chr1.L1.B1.L2.B1.L3.B2.L4.B3.L5.B6.L6.B12.L7.B23.L8.B46.L9.B91.L10.B182.L11.B364.L12.B727.L13.B1453"

H1_LINES = [
    b"metaseq_id\trecord_primary_key\tbin_index\n",                    # header
    b"1:1000:A:G\t1:1000:A:G:rs12\t" + BIN.encode() + b"\n",
    b"\n",                                                              # empty line
    b"onefield\n",
    b"two\tfields\n",
    b"2:2000:AT:A\t2:2000:AT:A\tchr2.L1.B1\textra\n",                   # 4 fields
    b"3:3000:G:C\t3:3000:G:C\tchr3.L1.B1\ta\tb\t\td\n",                 # 7 fields
    b"\tpk_for_empty_metaseq\tchr4.L1.B1\n",                            # empty metaseq
    b"4:4000:T:C\t\tchr4.L1.B2\n",                                      # empty pk
    b"5:5000:T:C\t5:5000:T:C\t\n",                                      # empty bin
    b"\t\t\n",                                                          # all three empty
    b"6:6000:C:T\t6:6000:C:T:rs6\tchr6.L1.B1\r\n",                      # \r\n
    b"short\tline\r\n",                                                 # \r\n on a skipped line
    b"7:7000:C:T\t7:7000:C:T\tchr7.L1.B1\twith\textras\r\n",
    b"1:1000:A:G\tdup:first\tchr1.L1.B1\n",                             # duplicate keys
    b"1:1000:A:G\tdup:second\tchr1.L1.B1\n",
    b"8:8000:A:T\tpk\"quoted\"\tchr8.L1.B1\n",                          # '"': verbatim
    b"9:9000:A:T\tit's\tchr9.L1.B1\n",                                  # FRAG_HOST from here
    b"10:100:A:T\tback\\slash\tchr10.L1.B1\n",
    b"11:110:A:T\tctl\x01byte\tchr11.L1.B1\n",
    b"12:120:A:T\tdel\x7fbyte\tchr12.L1.B1\n",
    b"13:130:A:T\tcaf\xc3\xa9\tchr13.L1.B1\n",
    b"14:140:A:T\t14:140:A:T\tbin'quote\n",                             # FRAG_HOST by the bin
    b"15:150:A:T\tboth'\"quotes\tchr15.L1.B1\n",
    b"16:160:A:T\t16:160:A:T\tbin with space\n",                        # a space: verbatim
    b"HSCHR1_RANDOM:5:A:T\tHSCHR1_RANDOM:5:A:T\tchrUn.L1.B1\n",         # NONCANON
    b"chr1:5:A:T\tchr1:5:A:T\tchr1.L1.B1\n",
    b":5:A:T\tempty-label\tchr1.L1.B1\n",
    b"nocolon\tnocolon-pk\tchr1.L1.B1\n",
    b"23:5:A:T\ttwenty-three\tchr1.L1.B1\n",
    b"0:5:A:T\tzero\tchr1.L1.B1\n",
    b"MT:5:A:T\tmt-label\tchrM.L1.B1\n",
    b"X:5:A:T\tX:5:A:T\tchrX.L1.B1\n",                                  # canonical again
    b"Y:5:A:T\tY:5:A:T\tchrY.L1.B1\n",
    b"M:5:A:T\tM:5:A:T\tchrM.L1.B1\n",
    b"22:5:A:T\t22:5:A:T\tchr22.L1.B1\n",
    b"metaseq_id\n",
    b"metaseq_idx\tnot-a-header\tchr1.L1.B1\n",
    b"HSCHR1_RANDOM:7:A:T\tnoncanon'and-host\tchrUn.L1.B1\r\n",
    b"19:190:G:GA\t19:190:G:GA:rs19\tchr19.L1.B1",                      # last line, no \n
]
H1 = b"".join(H1_LINES)
H1_FRAG_HOST = 8   # it's, back\slash, \x01, \x7f, é, bin'quote, both quotes, noncanon'and-host
H1_NONCANON = 11   # empty metaseq x2, HSCHR1_RANDOM x2, chr1, empty label, nocolon, 23, 0, MT, metaseq_idx


def h2(n_rows: int) -> bytes:
    """n_rows rows with a skipped line first, last and at every 256th line."""
    out, r, li = [], 0, 0
    while r < n_rows:
        if li % 256 == 0:
            out.append(b"skipped\tline %d\n" % li)
        else:
            out.append(b"%d:%d:A:G\t%d:%d:A:G:rs%d\tchr%d.L1.B1.L2.B%d\n" % (r % 22 + 1, 1000 + r, r % 22 + 1,
                                                                           1000 + r, r, r % 22 + 1, r % 7))
            r += 1
        li += 1
    out.append(b"metaseq_id\tx\ty\n")
    return b"".join(out)


def h3() -> bytes:
    """A 40,000-byte metaseq id as the first, the last and a middle line of a trip of
    both passes (256 lines, 128 rows), and as the file's last line without a newline;
    a 100-byte pk and a 2,000-byte bin."""
    def row(i):
        return b"%d:%d:C:T\t%d:%d:C:T\tchr%d.L1.B%d\n" % (i % 22 + 1, i, i % 22 + 1, i, i % 22 + 1, i)

    def long_row(i):
        head = b"%d:%d:" % (i % 22 + 1, i)
        return head + b"A" * (LONG - len(head) - 2) + b":T\tlong%d\tchr1.L1.B%d\n" % (i, i)

    lines = [row(i) for i in range(700)]
    for i in (0, 127, 255, 256, 400, 511):
        lines[i] = long_row(i)
    lines[50] = b"3:50:C:T\t" + b"p" * 100 + b"\t" + b"b" * 2000 + b"\n"
    lines[60] = b"3:60:C:T\t" + b"q'" * 50 + b"\t" + b"b" * 2000 + b"\n"   # FRAG_HOST and long
    lines.append(long_row(700).rstrip(b"\n"))
    return b"".join(lines)


def h4() -> bytes:
    out = [b"metaseq_id\trecord_primary_key\tbin_index\n"]
    labels = CHROM_NAMES + ["HSCHR1_RANDOM", "chr22", ""]
    for i in range(600):
        lab = labels[i % len(labels)].encode()
        out.append(lab + b":%d:A:G\t" % i + lab + b":%d:A:G\tchr.L1.B%d\n" % (i, i))
        if i % 97 == 0:
            out.append(b"junk\n")
    return b"".join(out)


# ---- texts on the size pass's stage fit boundary -------------------------------
TRIP = 256          # lines per k_exist_lines trip (one workgroup); a skipped line is a line
STAGE = 48 * 1024   # its LDS stage: a trip is staged when its span, counted from the
#                     16-byte floor of its first line's address, is at most this
LONG_TRIP = "long"  # a trip holding one line with a 60,000-byte metaseq id
JUNK = b"~\t~\t~\n"   # a row of three fields in 6 bytes, of a byte no text here has


def fit_line(i, fill=0):
    """Row i with ``fill`` more bytes in its bin; every 4th row has further columns,
    every 9th ends in "\\r\\n", every 50th has a primary key repr() escapes in."""
    pk = b"it's:%d" % i if i % 50 == 7 else b"%d:%d:A:G:rs%d" % (i % 22 + 1, 1000 + i, i)
    return b"%d:%d:A:G\t%s\tchr%d.L1.B%d%s%s%s\n" % (i % 22 + 1, 1000 + i, pk, i % 22 + 1, i % 9, b"f" * fill,
                                                b"\tmore\tcolumns" if i % 4 == 1 else b"", b"\r" if i % 9 == 4 else b"")


def fit_text(spans, residue=0, tail_lines=100):
    """Text whose trip k stages exactly ``spans[k]`` bytes on a slab at ``residue``
    mod 16, then ``tail_lines`` plain rows, the last without newline.  A skipped line
    is the first line of every odd trip and the last line of every even one."""
    out, at, i = [], 0, 0
    for t, span in enumerate(spans):
        lines = [fit_line(i + k) for k in range(TRIP)]
        lines[0 if t % 2 else TRIP - 1] = b"metaseq_id\trecord_primary_key\tbin_index\n" if t % 4 < 2 else b"two\tfields\n"
        if span == LONG_TRIP:
            lines[100] = b"1:%d:%s:T\tlong%d\tchr1.L1.B1\n" % (i + 100, b"ACGT" * 15000, i)
        else:
            room = span - ((at + residue) & 15) - sum(len(ln) for ln in lines)
            assert room >= 0
            q, r = divmod(room, TRIP - 2)  # shared by the lines between the first and the last
            for k in range(1, TRIP - 1):
                lines[k] = fit_line(i + k, q + (k <= r))
        out += lines
        at += sum(len(ln) for ln in lines)
        i += TRIP
    out += [fit_line(i + k, k % 5) for k in range(tail_lines)]
    return b"".join(out)[:-1]


def fit_plan(first):
    """Trip 0 at ``first`` bytes, then fitting and non-fitting trips in turn."""
    rest = [STAGE + 1, STAGE, LONG_TRIP, STAGE - 16, STAGE + 16] if first <= STAGE else \
        [STAGE, STAGE + 1, STAGE - 16, LONG_TRIP, STAGE, STAGE + 16]
    return [first] + rest


def trip_spans(text, residue=0):
    """Per trip of 256 lines, the bytes k_exist_lines would stage for a slab whose
    address is ``residue`` mod 16, computed from the text alone."""
    a = np.frombuffer(text, dtype=np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(a == 10) + 1))
    if starts[-1] == len(text):
        starts = starts[:-1]  # the text ends in its last line's newline
    s0 = starts[::TRIP]
    s1 = np.concatenate((s0[1:], [len(text)]))
    return (s1 + residue) - ((s0 + residue) & ~np.int64(15))


def check_fit_plan(text, plan, residue=0):
    spans = trip_spans(text, residue).tolist()
    assert len(spans) == len(plan) + 1 and spans[-1] < STAGE
    assert [s for s, p in zip(spans, plan) if p != LONG_TRIP] == [p for p in plan if p != LONG_TRIP], spans
    assert all(s > 60000 for s, p in zip(spans, plan) if p == LONG_TRIP)
    fits = [s <= STAGE for s in spans]
    assert all(a != b for a, b in zip(fits, fits[1:])), fits  # staged and unstaged trips alternate
    lines = text.split(b"\n")
    skipped = [ln.count(b"\t") < 2 or ln.startswith(b"metaseq_id\t") for ln in lines]
    assert all(skipped[t * TRIP + (0 if t % 2 else TRIP - 1)] for t in range(len(plan))) and not text.endswith(b"\n")
    return fits

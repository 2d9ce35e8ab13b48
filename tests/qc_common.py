"""Shared by test_qc_update_host.py and test_gpu_qc_update.py (K17, the ADSP QC pVCF update rows):
the golden fixture, a pure-Python restatement of the reference's loop
(Load/bin/update_from_qc_pvcf_file.py:34-58,117-149,226-258 with VcfEntryParser.parse_entry /
get_variant and vcf_variant_loader.py:172-219) over a VCF text and an export text, a seeded fuzz of
both texts, the engine's outputs as numpy arrays, and the four library entries called directly."""

import ctypes
import gzip
import json
import os

from annotatedvdb_amd import _native as N
from lof_common import (BASES, CANON, _bases, _call, _runner, assert_same, export_lines, table_arrays,  # noqa: F401
                        table_rows, text_lines, to_numeric, xstr)

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ["chrom", "pos", "id", "ref", "alt", "qual", "filter", "info", "format"]
_GOLDEN = None


def golden():
    """``{"vcf", "export", "version", "host_lines", "data_lines", "tuples": {0: [...], 1: [...]},
    "skipped": {0: n, 1: n}, "missing": [...], "cases": [(case, exception or None, line bytes, ids,
    True | None, json)]}`` of adsp_qc.tsv.gz."""
    global _GOLDEN
    if _GOLDEN is not None:
        return _GOLDEN
    with gzip.open(os.path.join(HERE, "golden", "adsp_qc.tsv.gz"), "rb") as fh:
        raw = fh.read()
    g = {"tuples": {0: [], 1: []}, "skipped": {}, "missing": [], "cases": []}
    flag = {"true": True, "\\N": None, "": None}
    at = 0
    while at < len(raw):
        e = raw.index(b"\n", at)
        f = raw[at:e].decode().split("\t")
        at = e + 1
        if f[0] in ("V", "X"):
            g["vcf" if f[0] == "V" else "export"] = raw[at:at + int(f[1])]
            at += int(f[1]) + 1
        elif f[0] == "R":
            g["version"] = f[1]
        elif f[0] == "H":
            g["host_lines"], g["data_lines"] = int(f[1]), int(f[2])
        elif f[0] == "U":
            g["tuples"][int(f[1])].append((f[2], f[3], flag[f[4]], f[5]))
        elif f[0] == "S":
            g["skipped"][int(f[1])] = int(f[2])
        elif f[0] == "M":
            g["missing"].append(f[1])
        elif f[0] == "E":
            n = int(f[3])
            g["cases"].append((f[1], None if f[2] == "-" else f[2], raw[at:at + n], f[4].split(",") if f[4] else [],
                               flag[f[5]], f[6]))
            at += n + 1
        else:
            raise ValueError(f[0])
    _GOLDEN = g
    return g


# ---- the reference's loop, restated --------------------------------------------------------
def ref_line(raw: bytes, release: str):
    """One line by the reference: ``"comment"`` or ``(ids, json, True | None)``; raises what the
    reference raises."""
    line = raw.decode("utf-8").rstrip()
    if line.startswith("#"):
        return "comment"
    values = line.split("\t")
    entry = {f: to_numeric(values[i]) for i, f in enumerate(FIELDS)}  # IndexError
    try:
        info_str = entry["info"].replace("\\x2c", ",").replace("\\x59", "/").replace("#", ":")
    except AttributeError as err:
        raise ImportError(str(err))
    info = dict(item.split("=", 1) if "=" in item else [item, True] for item in info_str.split(";"))
    info = {k: to_numeric(v) if isinstance(v, str) else v for k, v in info.items()}
    chrom = xstr(entry["chrom"])
    if chrom == "MT":
        chrom = "M"
    alts = entry["alt"].split(",")
    vid = entry["id"]
    if vid == "." or vid.startswith("rs"):
        pass
    if "rs" in entry["id"]:
        pass
    ids = [":".join((chrom.replace("chr", ""), xstr(int(entry["pos"])), entry["ref"], alt)) for alt in alts]
    text = json.dumps({release: {"info": info, "filter": entry["filter"], "qual": entry["qual"],
                                 "format": entry["format"]}})
    if "Infinity" in text:
        raise ValueError("Infinity found among QC scores")
    return ids, text, True if entry["filter"] == "PASS" else None


def ref_table(vcf: bytes, release: str):
    """``(rows, counters)``: rows are ``(id, json, True | None, line index)`` per ALT allele of every
    data line, in file order.  An exception carries ``line`` (1-based)."""
    rows, ctr = [], {"lines": 0, "comment_lines": 0}
    for no, raw in enumerate(text_lines(vcf)):
        ctr["lines"] += 1
        try:
            r = ref_line(raw, release)
        except Exception as err:
            err.line = no + 1
            raise
        if r == "comment":
            ctr["comment_lines"] += 1
        else:
            rows += [(i, r[1], r[2], no) for i in r[0]]
    ctr["rows"] = len(rows)
    return rows, ctr


def copy_unescape(s: str) -> str:
    out, i = [], 0
    while i < len(s):
        if s[i] == "\\" and i + 1 < len(s):
            i += 1
            out.append({"t": "\t", "n": "\n", "r": "\r", "b": "\b", "f": "\f", "v": "\v"}.get(s[i], s[i]))
        else:
            out.append(s[i])
        i += 1
    return "".join(out)


def ref_update(vcf: bytes, export: bytes, release: str, update_existing=False, contigs=None):
    """The reference's pass with the export for a database: ``(rows, counters, unmatched ids)``;
    rows are the ``(pk, 'chr' + label, True | None, json)`` tuples in export order, one per export
    row whose metaseq id the QC file holds (the last record of an id answers)."""
    table, _ = ref_table(vcf, release)
    last = {}
    for i, js, flag, _ in table:
        last[i] = (flag, js)
    hit = set()
    rows, ctr = [], {"rows": 0, "skipped_lines": 0, "skipped": 0, "not_in_vcf": 0}
    keep = None if contigs is None else {c if c in CANON else None for c in contigs}
    for line in export_lines(export):
        f = line.split(b"\t")
        if len(f) < 2 or f[0] == b"record_primary_key":
            ctr["skipped_lines"] += 1
            continue
        pk, m = f[0].decode(), f[1].decode()
        label = m.split(":")[0]
        if keep is not None and (label if label in CANON else None) not in keep:
            ctr["skipped_lines"] += 1
            continue
        if len(m.split(":")) != 4:
            raise ValueError("metaseq id")
        if m not in last:
            ctr["not_in_vcf"] += 1
            continue
        hit.add(m)
        qc = None if len(f) < 3 or f[2] in (b"", b"\\N") else json.loads(copy_unescape(f[2].decode()))
        has = qc is not None and release in qc  # load():49
        if has and not update_existing:  # {'update': False}: counted skipped
            ctr["skipped"] += 1
            continue
        rows.append((pk, "chr" + label) + last[m])
    ctr["rows"] = len(rows)
    return rows, ctr, [i for i in last if i not in hit]


def rows_text(rows) -> bytes:
    return "".join("\t".join((r[0], r[1], "true" if r[2] else "\\N", r[3])) + "\n" for r in rows).encode()


# ---- fuzz ------------------------------------------------------------------------------------
PLAIN_VALUES = ["5", "-5", "007", "-0", "0.0", "-0.0", "0.00", ".5", "5.", ".", "0.00001", "-0.000012", "0.5,0.25",
                "123456789012345678901234567890", "0.123456789012345", "10000000000000000.0", "MQ", "a b", "G#1",
                "1234.5", "-12.50", "60.00", "3.0103", "1,2"]
HOST_VALUES = ["1e-5", "+5", "0.1234567890123456", "nan", "1_0", " 5", "-", "", "A\\x2cB", "A\\x59B", "q\"q",
               "café", "5 "]


def fuzz_vcf(rng, n_lines, multi_alt=0.3, host=0.05, long_allele=None, positions=400, samples=0.2):
    """A QC-like pVCF of exactly ``n_lines`` lines and the lookup ids of its data lines: comments,
    data lines with ``chr`` prefixes and MT, multi-alt lines, sample columns, flags, empty items,
    every FILTER / QUAL form, trailing blanks and CRLF, and a ``host`` share of lines outside the
    device subset that the reference still accepts."""
    lines, ids = [], []
    for _ in range(n_lines):
        if rng.random() < 0.03:
            lines.append(rng.choice((b"#comment", b"##x=1;y", b"#")))
            continue
        c = rng.choice(["1", "2", "10", "22", "X", "Y", "M"])
        pos = rng.randint(1, positions)
        ref = _bases(rng, long_allele if long_allele and rng.random() < 0.02 else rng.choice((1, 1, 1, 2, 5)))
        alts = [_bases(rng, rng.choice((1, 1, 3))) for _ in range(rng.randint(2, 4) if rng.random() < multi_alt else 1)]
        if rng.random() < 0.05:
            alts[-1] = rng.choice(("*", ".", "NAN") if len(alts) > 1 else ("*", "."))
        odd = rng.random() < host
        chrom = c
        if rng.random() < 0.2:
            chrom = "chr" + c
        elif c == "M" and rng.random() < 0.5:
            chrom = "MT"
        if odd and rng.random() < 0.2:
            chrom = rng.choice(("chrMT", "0" + c if c.isdigit() else c, c))
        posv = ("0" * rng.choice((0, 0, 0, 2))) + str(pos)
        vid = rng.choice((".", "rs%d" % rng.randint(1, 999), "%s:%d:%s:%s" % (c, pos, ref, alts[0])))
        info = []
        for k in range(rng.choice((1, 3, 8, 12, 14))):
            r = rng.random()
            if r < 0.15:
                info.append("F%d" % k)
            elif r < 0.2:
                info.append("")
            else:
                info.append("K%d%s=%s" % (k, rng.choice(("", "", "#x")), rng.choice(PLAIN_VALUES)))
        if odd:
            kind = rng.randrange(3)
            if kind == 0:
                info.append("H=" + rng.choice(HOST_VALUES))
            elif kind == 1 and info:
                info.append(rng.choice(info).split("=")[0] + "=2")
            else:
                info.insert(0, "H=" + rng.choice(HOST_VALUES))
        qual = rng.choice((".", "50", "1234.56", "0.00", "-1")) if not odd else rng.choice((".", "1e3", "+5"))
        filt = rng.choice(("PASS", "PASS", ".", "VQSRTrancheSNP99.80to100.00", "q10;s50", "pass"))
        fields = [chrom, posv, vid, ref, ",".join(alts), qual, filt, ";".join(info) or "DB", rng.choice(("GT", "GT:AD:DP", "."))]
        if rng.random() < samples:
            fields += ["0/1:1,2:3"] * rng.randint(1, 5)
        line = ("\t".join(fields) + rng.choice(("", "", "", "\r", " ", "\t", " \t"))).encode()
        r = ref_line(line, "r1")
        ids += r[0]
        lines.append(line)
    if not lines:
        return b"", ids
    text = b"\n".join(lines)
    return (text + b"\n" if lines[-1].strip() == b"" or text.endswith(b"\r") or rng.random() < 0.5 else text), ids


def qc_columns(release: str):
    """adsp_qc columns of an export, as COPY writes them: NULLs, this release at depth 1, at depth
    2 only, as a string value, as a prefix of a longer key, and columns with a backslash."""
    r = release
    esc = lambda v: json.dumps(v).replace("\\", "\\\\").encode()  # noqa: E731
    return [b"\t\\N", b"\t\\N", b"\t\\N", b"\t", b"", b"\t\\N\textra\t\tcolumns", b"\tnull",
            b"\t" + json.dumps({r: {"info": {}}}).encode(),
            b"\t" + json.dumps({"r0": {"info": {"a": [1, {"b": 2}]}}, r: {}}).encode() + b"\tmore",
            b"\t" + json.dumps({"r0": {r: 1, "x": {r: 2}}}).encode(),
            b"\t" + json.dumps({"r0": r, "label": r}).encode(),
            b"\t" + json.dumps({r + "x": 1, "x" + r: 2, "k": [r, {r: 1}]}).encode(),
            b"\t{}", b'\t{"' + r.encode() + b'" : 1}',
            b"\t" + esc({"r0": {"note": 'say "' + r + '": 1'}}),
            b"\t" + esc({r: {"note": "a\\b"}}),
            b"\t" + esc({"r0": {"note": "tab\there"}})]


def fuzz_export(rng, ids, n_lines, release="r1", long_allele=None):
    """An export of exactly ``n_lines`` lines: about half of the ids drawn from ``ids``, every column
    of :func:`qc_columns`, two primary keys of one id, headers, empty and one-field lines, CRLF."""
    lines = []
    pool = list(ids) or ["1:1:A:C"]
    cols = qc_columns(release)
    for _ in range(n_lines):
        if rng.random() < 0.04:
            lines.append(rng.choice((b"", b"record_primary_key\tmetaseq_id\tadsp_qc", b"one field", b"\r")))
            continue
        if rng.random() < 0.6:
            m = rng.choice(pool)
        else:
            m = "%s:%d:%s:%s" % (rng.choice(["1", "2", "X", "M", "GL000219.1"]), rng.randint(1, 400),
                                 _bases(rng, long_allele if long_allele and rng.random() < 0.05 else 1), _bases(rng, 1))
        pk = rng.choice((m, m + ":rs%d" % rng.randint(1, 10 ** 9), "rs%d" % rng.randint(1, 999), ""))
        line = pk.encode() + b"\t" + m.encode() + rng.choice(cols)
        if rng.random() < 0.1:
            line += b"\r"
        lines.append(line)
    if not lines:
        return b""
    text = b"\n".join(lines)
    return text + b"\n" if lines[-1] in (b"", b"\r") or text.endswith(b"\r") or rng.random() < 0.5 else text


# ---- the engine's outputs --------------------------------------------------------------------
def table_tuples(t):
    """``[(id, json, True | None)]`` of a QcTable."""
    flags = t.flags.cpu().numpy()
    return [(i, js, True if flags[r] & N.QC_PASS else None) for r, (i, js) in enumerate(table_rows(t))]


def rows_arrays(rows):
    return {"text": rows.text.cpu().numpy().copy(), "row_off": rows.row_off.cpu().numpy().copy(),
            "match": rows.match.cpu().numpy().copy(), "flags": rows.flags.cpu().numpy().copy(),
            "counts": dict(rows.counts), "n": rows.n}


def raw_table_passes(eng, text, release=b"r1", key_cap=None, json_cap=None, pad=64, sentinel=0xA5):
    """avdb_qc_table_size / _write called directly on ``eng`` (host lines are left blank), every
    output ``pad`` entries longer than asked for and filled with ``sentinel``: ``(rc of the write
    pass, counts, {name: numpy array with its padding}, totals)``."""
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    suffix, tail = _runner(eng, "qc_table", "avdb_qc_table_workspace_size", nb, n_lines)
    full = lambda n, dt: torch.full(((n + pad) * torch.empty(0, dtype=dt).element_size(),), sentinel,  # noqa: E731
                                    dtype=torch.uint8, device=eng.device).view(dt)
    ents = [full(m, torch.int64)] + [full(m, torch.int32) for _ in range(3)] + [full(m, torch.uint8)]
    counts = eng.empty(N.QC_N_COUNTS, torch.int64)
    tp = t if nb else None
    rc = _call(eng, "avdb_qc_table_size" + suffix, tp, nb, n_lines, release, len(release), *ents, counts, *tail)
    assert rc == 0, N.last_error()
    cnt = dict(zip(N.QC_COUNTS, counts.cpu().tolist()))
    ne, n = cnt["entries"], cnt["rows"]
    key_cap = cnt["key_bytes"] if key_cap is None else key_cap
    json_cap = cnt["json_bytes"] if json_cap is None else json_cap
    out = {"keys": full((key_cap + 7) & ~7, torch.uint8), "key_off": full(n + 1, torch.int64),
           "json": full((json_cap + 7) & ~7, torch.uint8), "json_off": full(n, torch.int64),
           "json_len": full(n, torch.int32), "line_start": full(n, torch.int64), "flags": full(n, torch.uint8)}
    totals = eng.empty(4, torch.int64)
    rc = _call(eng, "avdb_qc_table_write" + suffix, tp, nb, n_lines, ne, n, release, len(release), *ents, out["keys"],
               key_cap, out["key_off"], out["json"], json_cap, out["json_off"], out["json_len"], out["line_start"],
               out["flags"], totals, *tail)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update({"ent_%d" % i: e.cpu().numpy() for i, e in enumerate(ents)})
    return rc, cnt, res, totals.cpu().tolist()


def raw_update_passes(eng, text, table, mask=N.EXIST_ALL_CONTIGS, flags=0, cap=None, pad=64, sentinel=0xA5):
    """avdb_qc_update_size / _write called directly (host rows are written as update rows): ``(rc of
    the write pass, counts, out buffer with its padding, totals, cap)``."""
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    suffix, tail = _runner(eng, "qc_update", "avdb_qc_update_workspace_size", nb, n_lines)
    view = table.view()
    vp = ctypes.byref(view)
    row_start = eng.empty(m, torch.int64)
    pk_len, match, out_len = (eng.empty(m, torch.int32) for _ in range(3))
    fl = eng.empty(m, torch.uint8)
    counts = eng.empty(N.QCUPD_N_COUNTS, torch.int64)
    tp = t if nb else None
    rc = _call(eng, "avdb_qc_update_size" + suffix, tp, nb, n_lines, vp, mask, flags, row_start, pk_len, match,
               out_len, fl, counts, *tail)
    assert rc == 0, N.last_error()
    cnt = dict(zip(N.QCUPD_COUNTS, counts.cpu().tolist()))
    cap = cnt["out_bytes"] if cap is None else cap
    out = torch.full((cap + pad,), sentinel, dtype=torch.uint8, device=eng.device)
    row_off = eng.empty(cnt["rows"] + 1, torch.int64)
    totals = eng.empty(2, torch.int64)
    rc = _call(eng, "avdb_qc_update_write" + suffix, tp, nb, n_lines, cnt["rows"], vp, row_start, pk_len, match,
               out_len, fl, out, cap, row_off, totals, *tail)
    return rc, cnt, out.cpu().numpy(), totals.cpu().tolist(), cap

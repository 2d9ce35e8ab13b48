"""Shared by test_lof_update_host.py and test_gpu_lof_update.py (K16, the SnpEff LOF/NMD update
rows): the golden fixture, a pure-Python restatement of the reference's loop
(Load/bin/load_snpeff_lof.py:112-173,250-288 with VcfEntryParser.parse_entry / get_variant and
vcf_variant_loader.py:197-217) over a VCF text and an export text, a seeded fuzz of both texts,
the engine's outputs as numpy arrays, and the four library entries called directly."""

import ctypes
import gzip
import json
import os

import numpy as np

from annotatedvdb_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = ["chrom", "pos", "id", "ref", "alt", "qual", "filter", "info"]
CANON = {str(i + 1) for i in range(22)} | {"X", "Y", "M"}
BASES = "ACGT"
_GOLDEN = None


def golden():
    """``{"vcf", "export", "host_lines", "tuples": {0: [...], 1: [...]}, "missing": [...],
    "cases": [(case, exception or None, line bytes, ids, json)]}`` of snpeff_lof.tsv.gz."""
    global _GOLDEN
    if _GOLDEN is not None:
        return _GOLDEN
    with gzip.open(os.path.join(HERE, "golden", "snpeff_lof.tsv.gz"), "rb") as fh:
        raw = fh.read()
    g = {"tuples": {0: [], 1: []}, "missing": [], "cases": []}
    at = 0
    while at < len(raw):
        e = raw.index(b"\n", at)
        f = raw[at:e].decode().split("\t")
        at = e + 1
        if f[0] in ("V", "X"):
            g["vcf" if f[0] == "V" else "export"] = raw[at:at + int(f[1])]
            at += int(f[1]) + 1
        elif f[0] == "H":
            g["host_lines"] = int(f[1])
        elif f[0] == "U":
            g["tuples"][int(f[1])].append(tuple(f[2:5]))
        elif f[0] == "M":
            g["missing"].append(f[1])
        elif f[0] == "E":
            n = int(f[3])
            g["cases"].append((f[1], None if f[2] == "-" else f[2], raw[at:at + n], f[4].split(",") if f[4] else [],
                               f[5]))
            at += n + 1
        else:
            raise ValueError(f[0])
    _GOLDEN = g
    return g


# ---- the reference's loop, restated --------------------------------------------------------
def to_numeric(value):
    try:
        return int(value)
    except (ValueError, TypeError):
        try:
            return float(value)
        except (ValueError, TypeError):
            return value


def xstr(v):
    return "" if v is None else str(v)


def parse_annotation_string(valueStr):
    if valueStr is None:
        return None
    out = []
    for a in valueStr.split(","):
        values = a.replace("(", "").replace(")", "").split("|")
        out.append({"gene_symbol": values[0], "gene_id": values[1], "num_transcripts": int(values[2]),
                    "fraction_affected_transcripts": float(values[3])})
    return out


def ref_line(raw: bytes):
    """One line by the reference: ``"comment"``, ``"unannotated"``, or ``(ids, json or None)``
    (None: neither value); raises what the reference raises."""
    line = raw.decode("utf-8").rstrip()
    if line.startswith("#"):
        return "comment"
    if ';LOF=' not in line and ';NMD=' not in line:
        return "unannotated"
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
    lof = parse_annotation_string(info.get("LOF"))
    nmd = parse_annotation_string(info.get("NMD"))
    if lof is None and nmd is None:
        return ids, None
    v = {}
    if lof is not None:
        v["LOF"] = lof
    if nmd is not None:
        v["NMD"] = nmd
    return ids, json.dumps(v)


def text_lines(text: bytes):
    lines = text.split(b"\n")
    return lines[:-1] if lines[-1] == b"" else lines


def ref_table(vcf: bytes):
    """``(rows, counters)``: rows are ``(id, json, line index)`` per ALT allele of every line with
    values, in file order.  An exception carries ``line`` (1-based)."""
    rows, ctr = [], {"lines": 0, "comment_lines": 0, "unannotated_lines": 0, "no_values": 0}
    for no, raw in enumerate(text_lines(vcf)):
        ctr["lines"] += 1
        try:
            r = ref_line(raw)
        except Exception as err:
            err.line = no + 1
            raise
        if r == "comment":
            ctr["comment_lines"] += 1
        elif r == "unannotated":
            ctr["unannotated_lines"] += 1
        elif r[1] is None:
            ctr["no_values"] += 1
        else:
            rows += [(i, r[1], no) for i in r[0]]
    ctr["rows"] = len(rows)
    return rows, ctr


def export_lines(text: bytes):
    """The export's lines as K13 takes them: one '\\r' before a '\\n' stripped."""
    lines = text.split(b"\n")
    ended = [True] * (len(lines) - 1) + [False]
    if lines[-1] == b"":
        lines, ended = lines[:-1], ended[:-1]
    return [ln[:-1] if nl and ln.endswith(b"\r") else ln for ln, nl in zip(lines, ended)]


def ref_update(vcf: bytes, export: bytes, update_existing=False, contigs=None):
    """The reference's pass with the export for a database: ``(rows, counters, unmatched ids)``;
    rows are the ``(pk, 'chr' + label, json)`` tuples in export order, one per export row whose
    metaseq id is annotated (the last annotated record of an id answers)."""
    table, _ = ref_table(vcf)
    last = {}
    for i, js, _ in table:
        last[i] = js
    hit = set()
    rows, ctr = [], {"rows": 0, "skipped_lines": 0, "skipped": 0, "not_annotated": 0}
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
        if m not in last:  # the lookup of the annotated ids never returns this row
            ctr["not_annotated"] += 1
            continue
        hit.add(m)
        existing = None if len(f) < 3 or f[2] in (b"", b"\\N") else f[2]
        if existing is not None and not update_existing:  # {'update': False}: counted skipped
            ctr["skipped"] += 1
            continue
        rows.append((pk, "chr" + label, last[m]))
    ctr["rows"] = len(rows)
    return rows, ctr, [i for i in last if i not in hit]


def rows_text(rows) -> bytes:
    return "".join("\t".join(r) + "\n" for r in rows).encode()


# ---- fuzz ------------------------------------------------------------------------------------
def _bases(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def _group(rng, odd):
    frac = rng.choice(["0.17", "1.00", "0.50", "0", "12", "0.00001", "0.000123", "0.333333333333"])
    count = str(rng.randint(0, 99))
    if odd:
        frac = rng.choice([".5", "1e-5", "nan", "5.", "0.1234567890123456789"]) if rng.random() < 0.5 else frac
        count = rng.choice([" 3 ", "+7", "1_0"]) if rng.random() < 0.5 else count
    return "(%s|ENSG%05d|%s|%s%s)" % (rng.choice(["SFI1", "PRAME", "A-B", "x y", "G'1"]), rng.randint(0, 99999),
                                      count.rjust(rng.choice([0, 0, 3]), "0") if count.isdigit() else count, frac,
                                      rng.choice(["", "", "|x|y"]))


def fuzz_vcf(rng, n_lines, annotated=0.3, multi_alt=0.3, host=0.05, long_allele=None, positions=400):
    """A SnpEff-like VCF of exactly ``n_lines`` lines and the lookup ids of its annotated lines:
    comments, empty lines, lines without values, annotated lines (LOF, NMD, both, repeated keys,
    INFO beginning with a key, the key only in a sample column), ``chr`` prefixes and MT, multi-alt
    lines, trailing blanks and CRLF, and a ``host`` share of annotated lines outside the device
    subset that the reference still accepts."""
    lines, ids = [], []
    for _ in range(n_lines):
        k = rng.random()
        if k < 0.03:
            lines.append(rng.choice((b"", b"#comment;LOF=(a|b|1|1)", b"##x", b"  ")))
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
        if odd and rng.random() < 0.3:
            chrom = rng.choice(("chrMT", "0" + c if c.isdigit() else c, c))
        posv = ("0" * rng.choice((0, 0, 0, 2))) + str(pos)
        vid = rng.choice((".", "rs%d" % rng.randint(1, 999), "%s:%d:%s:%s" % (c, pos, ref, alts[0])))
        info = ["AC=%d" % rng.randint(1, 9), "ANN=%s|x" % alts[0]]
        if rng.random() < annotated:
            kind = rng.randrange(6)
            vals = lambda: ",".join(_group(rng, odd) for _ in range(rng.choice((1, 1, 2, 3))))  # noqa: E731
            if kind in (0, 2):
                info.append("LOF=" + vals())
            if kind in (1, 2):
                info.append("NMD=" + vals())
            if kind == 3:
                info += ["LOF=" + vals(), "NMD=" + vals(), "LOF=" + vals()]
            if kind == 4:
                info = ["LOF=" + vals(), "DP=3", "NMD=" + vals()]
            if kind == 5:
                info += ["LOF", "X=1", "LOF=" + vals()]
            if odd and rng.random() < 0.3:
                info.append("NMD=(A\\x59B#2|\"q\"|1|0.5)")
        fields = [chrom, posv, vid, ref, ",".join(alts), ".", "PASS", ";".join(info)]
        if rng.random() < 0.1:
            fields += ["GT", "0/1" + rng.choice(("", ";LOF=1", ";NMD=."))]
        line = "\t".join(fields) + rng.choice(("", "", "", "\r", " ", "\t", " \t"))
        r = ref_line(line.encode())
        if isinstance(r, tuple) and r[1] is not None:
            ids += r[0]
        lines.append(line.encode())
    if not lines:
        return b"", ids
    text = b"\n".join(lines)
    return (text + b"\n" if lines[-1].strip() == b"" or text.endswith(b"\r") or rng.random() < 0.5 else text), ids


def fuzz_export(rng, ids, n_lines, long_allele=None):
    """An export of exactly ``n_lines`` lines: about half of the ids drawn from ``ids``, NULL as
    ``\\N``, empty and missing, records with values, extra columns, two primary keys of one id,
    headers, empty and one-field lines, CRLF."""
    lines = []
    pool = list(ids) or ["1:1:A:C"]
    for _ in range(n_lines):
        k = rng.random()
        if k < 0.04:
            lines.append(rng.choice((b"", b"record_primary_key\tmetaseq_id\tloss_of_function", b"one field", b"\r")))
            continue
        if rng.random() < 0.6:
            m = rng.choice(pool)
        else:
            m = "%s:%d:%s:%s" % (rng.choice(["1", "2", "X", "M", "GL000219.1"]), rng.randint(1, 400),
                                 _bases(rng, long_allele if long_allele and rng.random() < 0.05 else 1), _bases(rng, 1))
        pk = rng.choice((m, m + ":rs%d" % rng.randint(1, 10 ** 9), "rs%d" % rng.randint(1, 999), ""))
        third = rng.choice((b"\t\\N", b"\t\\N", b"\t\\N", b"\t", b"", b"\t\\N\textra\t\tcolumns", b"\t\t{}",
                            b'\t{"LOF": []}'))
        line = pk.encode() + b"\t" + m.encode() + third
        if rng.random() < 0.1:
            line += b"\r"
        lines.append(line)
    if not lines:
        return b""
    text = b"\n".join(lines)
    return text + b"\n" if lines[-1] in (b"", b"\r") or text.endswith(b"\r") or rng.random() < 0.5 else text


# ---- the engine's outputs --------------------------------------------------------------------
def table_arrays(t):
    """A LofTable (host or device) as numpy."""
    out = {name: getattr(t, name).cpu().numpy().copy()
           for name in ("keys", "key_off", "json", "json_off", "json_len", "line_start", "flags", "hit")}
    out["counts"], out["n_rows"] = dict(t.counts), t.n_rows
    return out


def table_rows(t):
    """``[(id, json)]`` of a LofTable."""
    a = table_arrays(t)
    keys, js = a["keys"].tobytes(), a["json"].tobytes()
    return [(keys[a["key_off"][r]:a["key_off"][r + 1]].decode(),
             js[a["json_off"][r]:a["json_off"][r] + a["json_len"][r]].decode()) for r in range(t.n_rows)]


def rows_arrays(rows):
    return {"text": rows.text.cpu().numpy().copy(), "row_off": rows.row_off.cpu().numpy().copy(),
            "match": rows.match.cpu().numpy().copy(), "counts": dict(rows.counts), "n": rows.n}


def assert_same(got, want, what=""):
    for name in want:
        x, y = got[name], want[name]
        if not isinstance(y, np.ndarray):
            assert x == y, (what, name, x, y)
            continue
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        if not np.array_equal(x, y):
            k = int(np.nonzero(x != y)[0][0])
            raise AssertionError("%s: %s differs first at %d: %r != %r" % (what, name, k, x[k], y[k]))


def _runner(eng, scratch, size_entry, nb, n_lines):
    if eng.host_only:
        return "_host", ()
    ws = eng.scratch(scratch, N.size(size_entry, nb, n_lines))
    return "", (ws, ws.numel())


def _call(eng, name, *args):
    return N.call(name, eng.ctx, *args, check=False) if eng.host_only else \
        N.call(name, eng.ctx, *args, eng._stream(), check=False)


def raw_table_passes(eng, text, key_cap=None, json_cap=None, pad=64, sentinel=0xA5):
    """avdb_lof_table_size / _write called directly on ``eng`` (host lines are left blank), every
    output ``pad`` entries longer than asked for and filled with ``sentinel``: ``(rc of the write
    pass, counts, {name: numpy array with its padding}, totals)``."""
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    suffix, tail = _runner(eng, "lof_table", "avdb_lof_table_workspace_size", nb, n_lines)
    full = lambda n, dt: torch.full(((n + pad) * torch.empty(0, dtype=dt).element_size(),), sentinel,  # noqa: E731
                                    dtype=torch.uint8, device=eng.device).view(dt)
    ents = [full(m, torch.int64)] + [full(m, torch.int32) for _ in range(3)] + [full(m, torch.uint8)]
    counts = eng.empty(N.LOF_N_COUNTS, torch.int64)
    tp = t if nb else None
    rc = _call(eng, "avdb_lof_table_size" + suffix, tp, nb, n_lines, *ents, counts, *tail)
    assert rc == 0, N.last_error()
    cnt = dict(zip(N.LOF_COUNTS, counts.cpu().tolist()))
    ne, n = cnt["entries"], cnt["rows"]
    key_cap = cnt["key_bytes"] if key_cap is None else key_cap
    json_cap = cnt["json_bytes"] if json_cap is None else json_cap
    out = {"keys": full((key_cap + 7) & ~7, torch.uint8), "key_off": full(n + 1, torch.int64),
           "json": full((json_cap + 7) & ~7, torch.uint8), "json_off": full(n, torch.int64),
           "json_len": full(n, torch.int32), "line_start": full(n, torch.int64), "flags": full(n, torch.uint8)}
    totals = eng.empty(4, torch.int64)
    rc = _call(eng, "avdb_lof_table_write" + suffix, tp, nb, n_lines, ne, n, *ents, out["keys"], key_cap,
               out["key_off"], out["json"], json_cap, out["json_off"], out["json_len"], out["line_start"],
               out["flags"], totals, *tail)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update({"ent_%d" % i: e.cpu().numpy() for i, e in enumerate(ents)})
    return rc, cnt, res, totals.cpu().tolist()


def raw_update_passes(eng, text, table, mask=N.EXIST_ALL_CONTIGS, flags=0, cap=None, pad=64, sentinel=0xA5):
    """avdb_lof_update_size / _write called directly: ``(rc of the write pass, counts, out buffer
    with its padding, totals, cap)``."""
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    suffix, tail = _runner(eng, "lof_update", "avdb_lof_update_workspace_size", nb, n_lines)
    view = table.view()
    vp = ctypes.byref(view)
    row_start = eng.empty(m, torch.int64)
    pk_len, match, out_len = (eng.empty(m, torch.int32) for _ in range(3))
    fl = eng.empty(m, torch.uint8)
    counts = eng.empty(N.LOFUPD_N_COUNTS, torch.int64)
    tp = t if nb else None
    rc = _call(eng, "avdb_lof_update_size" + suffix, tp, nb, n_lines, vp, mask, flags, row_start, pk_len, match,
               out_len, fl, counts, *tail)
    assert rc == 0, N.last_error()
    cnt = dict(zip(N.LOFUPD_COUNTS, counts.cpu().tolist()))
    cap = cnt["out_bytes"] if cap is None else cap
    out = torch.full((cap + pad,), sentinel, dtype=torch.uint8, device=eng.device)
    row_off = eng.empty(cnt["rows"] + 1, torch.int64)
    totals = eng.empty(2, torch.int64)
    rc = _call(eng, "avdb_lof_update_write" + suffix, tp, nb, n_lines, cnt["rows"], vp, row_start, pk_len, match,
               out_len, fl, out, cap, row_off, totals, *tail)
    return rc, cnt, out.cpu().numpy(), totals.cpu().tolist(), cap

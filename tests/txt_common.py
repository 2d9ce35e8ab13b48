"""K19's test helpers: the golden (tests/golden/make_golden_txt.py), a plain-Python restatement of
the generic annotation update (csv.DictReader, set_current_variant, __buffer_update_values), fuzzers,
and the library's entries called on poisoned buffers."""

import csv
import ctypes
import functools
import gzip
import json
import os

import numpy as np
import torch

from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import existing_contig_mask
from annotatedvdb_amd.slab_passes import SlabPass
from annotatedvdb_amd.text_update import read_header

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_update.tsv.gz")
ID_TYPES = ("METASEQ", "REFSNP", "PRIMARY_KEY")
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def golden():
    """{'export', 'files': {idtype: bytes}, 'host': {idtype: (host, data)}, 'tuples': {(idtype,
    datasource): [(line, tuple)]}, 'missing': {idtype: [id]}, 'cases': [(case, idtype, exc or None,
    text, [tuple])], 'sql': [(header fields, datasource, legacy, statement)]}"""
    raw = gzip.open(GOLDEN, "rb").read()
    g = {"files": {}, "host": {}, "tuples": {}, "missing": {t: [] for t in ID_TYPES}, "cases": [], "sql": []}
    at = 0
    while at < len(raw):
        nl = raw.index(b"\n", at)
        f = raw[at:nl].decode("utf-8").split("\t")
        at = nl + 1
        if f[0] == "X":
            g["export"] = raw[at:at + int(f[1])]
            at += int(f[1]) + 1
        elif f[0] == "F":
            g["files"][f[1]] = raw[at:at + int(f[2])]
            at += int(f[2]) + 1
        elif f[0] == "H":
            g["host"][f[1]] = (int(f[2]), int(f[3]))
        elif f[0] == "U":
            t = tuple(json.loads(f[4]))
            g["tuples"].setdefault((f[1], f[2]), []).append((int(f[3]), t))
        elif f[0] == "M":
            g["missing"][f[1]].append(f[2])
        elif f[0] == "Q":
            g["sql"].append((json.loads(f[1]), f[2], bool(int(f[3])), f[4]))
        elif f[0] == "E":
            n = int(f[4])
            g["cases"].append((f[1], f[2], None if f[3] == "-" else f[3], raw[at:at + n],
                               [tuple(t) for t in json.loads(f[5])]))
            at += n + 1
        else:
            raise AssertionError(f)
    return g


# ---- the restatement -------------------------------------------------------------------------
def text_lines(text: bytes):
    """The slab's lines as the passes number them, each without its line end."""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def ref_records(text: bytes, id_type: str):
    """Per data line (file order): (line number, looked-up id, chromosome label or None, values
    with None for NULL).  csv reads every line by itself, as the passes do."""
    lines = [ln[:-1] if ln.endswith(b"\r") else ln for ln in text_lines(text)]
    fields = next(csv.reader([lines[0].decode("utf-8")], delimiter="\t"))
    update = list(fields)
    update.remove("variant")
    out = []
    for no, ln in enumerate(lines[1:], 2):
        row = next(csv.reader([ln.decode("utf-8")], delimiter="\t"), [])
        if not row:
            continue
        rec = dict(zip(fields, row))
        for f in fields[len(row):]:
            rec[f] = None
        variant = rec["variant"]
        label = variant.split(":")[0] if ":" in variant else None
        look = rec["ref_snp_id"] if id_type == "REFSNP" else variant
        out.append((no, look, label, [None if rec[f] == "NULL" else rec[f] for f in update]))
    return out


def body_of(label, values) -> bytes:
    return ((label or "") + "\t" + "\t".join("\\N" if v is None else v for v in values)).encode("utf-8")


def ref_table(text: bytes, id_type: str):
    """[(key, body)] per data line, and the counts the restatement knows."""
    recs = ref_records(text, id_type)
    n_lines = len(text_lines(text))
    return ([(look.encode("utf-8"), body_of(label, values)) for _, look, label, values in recs],
            {"lines": n_lines, "entries": len(recs), "rows": len(recs), "skipped_lines": n_lines - len(recs)})


def row_tuple(pk, label, values, adsp):
    chrom = "chr" + (label if label is not None else pk.split(":")[0])
    return (pk, chrom) + tuple(values) + ((True,) if adsp else ())


def contig_label(metaseq: str):
    return metaseq.split(":")[0]


def ref_update(text: bytes, export: bytes, id_type: str, adsp=False, contigs=None):
    """(tuples in export order, counts, ids of the file without an export row in file order)"""
    recs = ref_records(text, id_type)
    last = {}
    for r in recs:
        last[r[1]] = r  # the last line of a repeated id answers
    hit, rows = set(), []
    ctr = {"rows": 0, "not_in_file": 0, "skipped_lines": 0}
    for ln in text_lines(export):
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        f = ln.decode("utf-8").split("\t")
        if len(f) < 2 or f[0] == "record_primary_key":
            ctr["skipped_lines"] += 1
            continue
        lab = contig_label(f[1])
        if contigs is not None and lab not in contigs:
            ctr["skipped_lines"] += 1
            continue
        if id_type == "METASEQ":
            look = f[1]
        else:
            look = f[2] if len(f) > 2 and f[2] not in ("", "\\N") else None
        r = last.get(look) if look else None
        if r is None:
            ctr["not_in_file"] += 1
            continue
        hit.add(look)
        rows.append(row_tuple(f[0], r[2], r[3], adsp))
        ctr["rows"] += 1
    return rows, ctr, [k for k in last if k not in hit]


def ref_repeated(text: bytes, id_type: str):
    """The looked-up ids the file holds more than once, in file order of their first line."""
    seen = {}
    for _, look, _, _ in ref_records(text, id_type):
        seen[look] = seen.get(look, 0) + 1
    return [k for k, c in seen.items() if c > 1]


def ref_direct(text: bytes, adsp=False):
    return [row_tuple(look, label, values, adsp) for _, look, label, values in ref_records(text, "PRIMARY_KEY")]


def rows_text(rows) -> bytes:
    return b"".join(("\t".join("\\N" if v is None else "true" if v is True else v for v in t) + "\n").encode("utf-8")
                    for t in rows)


def golden_expected(id_type: str, datasource: str):
    """The reference's tuples with this project's two deviations applied: of a
    repeated id the last line's tuples only; compared as a sorted list, the order being the export's."""
    g = golden()
    tuples = g["tuples"][(id_type, datasource)]
    if id_type == "PRIMARY_KEY":
        return [t for _, t in tuples]
    last = {}
    for no, look, _, _ in ref_records(g["files"][id_type], id_type):
        last[look] = no
    keep = set(last.values())
    return sorted((t for no, t in tuples if no in keep), key=repr)


def table_rows(t):
    keys, off = t.keys.cpu().numpy().tobytes(), t.key_off.cpu().tolist()
    body, boff, blen = t.json.cpu().numpy().tobytes(), t.json_off.cpu().tolist(), t.json_len.cpu().tolist()
    return [(keys[off[r]:off[r + 1]], body[boff[r]:boff[r] + blen[r]]) for r in range(t.n_rows)]


# ---- fuzzers ----------------------------------------------------------------------------------
COLUMNS = ["gwas_flags", "other_annotation", "allele_frequencies", "is_adsp_variant", "is_multi_allelic",
           "adsp_qc", "cadd_scores", "loss_of_function", "vep_output", "display_attributes", "bin_index",
           "position", "chromosome", "metaseq_id", "row_algorithm_id", "adsp_most_severe_consequence",
           "adsp_ranked_consequences", "record_primary_key"] + ["extra_%d" % i for i in range(16)]
BASES = "ACGT"


def fuzz_value(rng, host):
    r = rng.random()
    if r < host:
        return rng.choice(['"quoted"', '"a ""b"""', "café", '"NULL"', '""', '"x"y'])
    if r < .2:
        return rng.choice(["NULL", "NULLx", "null", "", "xNULL", "NUL", "\\n", "N", "\\NN"])
    return "".join(rng.choice("abcdefgh{}:,. 0123456789\"\\") for _ in range(rng.choice([1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65])))\
        .lstrip('"') or "v"


def fuzz_file(rng, n, id_type="METASEQ", n_cols=None, id_pos=None, host=0.03, crlf=0.2, final_newline=None):
    """(text, [(looked-up id, metaseq id, rs id)]) of n data lines: column counts 2 .. 32, `variant`
    anywhere, short and long rows, NULL beside its look-alikes, quoting and non-ASCII, CRLF, empty
    lines, repeated ids, ids with and without ':'."""
    n_cols = n_cols or rng.randint(3 if id_type == "REFSNP" else 2, 32)
    cols = COLUMNS[:n_cols - 1 - (id_type == "REFSNP")]
    rng.shuffle(cols)
    id_pos = rng.randrange(len(cols) + 1) if id_pos is None else min(id_pos, len(cols))
    cols.insert(id_pos, "variant")
    if id_type == "REFSNP":
        cols.insert(rng.randrange(len(cols) + 1), "ref_snp_id")
    need = max(cols.index("variant"), cols.index("ref_snp_id") if id_type == "REFSNP" else 0) + 1
    lines, ids = ["\t".join(cols)], []
    for k in range(n):
        metaseq = "%s:%d:%s:%s" % (rng.choice(["1", "2", "10", "22", "X", "M"]), rng.randint(1, 10 ** rng.randint(1, 8)),
                                   rng.choice(BASES), "".join(rng.choice(BASES) for _ in range(rng.choice([1, 1, 2, 9]))))
        rs = "rs%d" % rng.randint(1, 10 ** 7)
        if ids and rng.random() < .05:
            _, metaseq, rs = rng.choice(ids)
        rec = {c: fuzz_value(rng, host) for c in cols}
        if id_type == "METASEQ":
            rec["variant"] = look = metaseq
        elif id_type == "REFSNP":
            rec["variant"], rec["ref_snp_id"] = rng.choice([metaseq, rs]), rs
            look = rs
        else:
            rec["variant"] = look = rng.choice([metaseq + ":" + rs, metaseq, rs])
        fields = [rec[c] for c in cols]
        r = rng.random()
        if r < .1:
            fields = fields[:rng.randint(need, len(fields))]
        elif r < .2:
            fields += ["more"] * rng.randint(1, 3)
        lines.append("\t".join(fields) + ("\r" if rng.random() < crlf else ""))
        ids.append((look, metaseq, rs))
        if rng.random() < .03:
            lines.append(rng.choice(["", "\r"]))
    final_newline = rng.random() < .7 if final_newline is None else final_newline
    final_newline = final_newline or lines[-1] in ("", "\r")
    if not final_newline:
        lines[-1] = lines[-1].rstrip("\r")  # (a '\r' no '\n' follows is no line end)
    text = "\n".join(lines) + ("\n" if final_newline else "")
    return text.encode("utf-8"), ids


def fuzz_export(rng, ids, n, hit=0.7):
    rows = ["record_primary_key\tmetaseq_id\tref_snp_id"] if rng.random() < .5 else []
    for _ in range(n):
        if ids and rng.random() < hit:
            _, metaseq, rs = rng.choice(ids)
        else:
            metaseq = "%s:%d:%s:%s" % (rng.choice(["1", "7", "Y", "GL1"]), rng.randint(1, 10 ** 6), rng.choice(BASES),
                                       rng.choice(BASES))
            rs = "rs%d" % rng.randint(1, 10 ** 7)
        r = rng.random()
        third = ["\t" + rs, "\t\\N", "\t", "", "\t" + rs + "\textra"][0 if r < .7 else rng.randint(1, 4)]
        pk = metaseq + rng.choice(["", ":" + rs, "_x"])
        rows.append(pk + "\t" + metaseq + third + ("\r" if rng.random() < .1 else ""))
        if rng.random() < .03:
            rows.append(rng.choice(["", "short", "\r"]))
    return ("\n".join(rows) + ("\n" if rows else "")).encode("utf-8")


# ---- the entries on poisoned buffers -----------------------------------------------------------
def poisoned(engine, n, dtype):
    item = torch.empty(0, dtype=dtype).element_size()
    return torch.full((max(1, n) * item,), POISON, dtype=torch.uint8, device=engine.device).view(dtype)


def host_arrays(d):
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def shape_of(text: bytes, id_type="METASEQ"):
    h = read_header(text[:1 << 16], id_type, len(text))
    return h.extra()


def raw_table_passes(engine, text: bytes, shape, key_cap=None, body_cap=None):
    """avdb_txt_table_size / _write as they are, no host rendering: (rc, counts, arrays, totals)"""
    sp = SlabPass(engine, text, "txt_table", "avdb_txt_table_workspace_size")
    ents = [poisoned(engine, sp.m, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
    counts = poisoned(engine, N.TXT_N_COUNTS, torch.int64)
    sp.call("avdb_txt_table_size", sp.tp, sp.nb, sp.n_lines, *shape, *ents, counts)
    cnt = sp.counts(counts, N.TXT_COUNTS)
    ne, n, kb, bb = cnt["entries"], cnt["rows"], cnt["key_bytes"], cnt["json_bytes"]
    kc, bc = (kb if key_cap is None else key_cap), (bb if body_cap is None else body_cap)
    out = {"keys": poisoned(engine, kb + 16, torch.uint8), "body": poisoned(engine, bb + 16, torch.uint8),
           "key_off": poisoned(engine, n + 3, torch.int64), "body_off": poisoned(engine, n + 2, torch.int64),
           "body_len": poisoned(engine, n + 2, torch.int32), "line_start": poisoned(engine, n + 2, torch.int64),
           "flags": poisoned(engine, n + 2, torch.uint8)}
    totals = poisoned(engine, 4, torch.int64)
    try:
        rc = sp.call("avdb_txt_table_write", sp.tp, sp.nb, sp.n_lines, ne, n, *shape, *ents, out["keys"], kc,
                     out["key_off"], out["body"], bc, out["body_off"], out["body_len"], out["line_start"],
                     out["flags"], totals)
    except N.NativeError as e:
        rc = e.rc
    out.update(zip(("ent_start", "ent_alts", "ent_key", "ent_body", "ent_flags"), (e[:max(ne, 0)] for e in ents)))
    return rc, cnt, host_arrays(out), totals.cpu().tolist()


def raw_update_passes(engine, export: bytes, table, key_col=1, adsp=False, contigs=None, cap=None):
    view = table.view()
    vp = ctypes.byref(view)
    fl = N.TXT_ADSP if adsp else 0
    sp = SlabPass(engine, export, "txt_update", "avdb_txt_update_workspace_size")
    cols = [poisoned(engine, sp.m, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
    counts = poisoned(engine, N.TXTUPD_N_COUNTS, torch.int64)
    sp.call("avdb_txt_update_size", sp.tp, sp.nb, sp.n_lines, vp, existing_contig_mask(contigs), key_col, fl, *cols,
            counts)
    cnt = sp.counts(counts, N.TXTUPD_COUNTS)
    n, nbytes = cnt["rows"], cnt["out_bytes"]
    out = {"text": poisoned(engine, nbytes + 16, torch.uint8), "row_off": poisoned(engine, n + 3, torch.int64)}
    totals = poisoned(engine, 2, torch.int64)
    try:
        rc = sp.call("avdb_txt_update_write", sp.tp, sp.nb, sp.n_lines, n, vp, fl, *cols, out["text"],
                     nbytes if cap is None else cap, out["row_off"], totals)
    except N.NativeError as e:
        rc = e.rc
    out.update(zip(("row_start", "pk_len", "match", "out_len", "flags"), (c[:n] for c in cols)))
    out["hit"] = table.hit.clone()
    return rc, cnt, host_arrays(out), totals.cpu().tolist()


def raw_direct_passes(engine, text: bytes, shape, adsp=False, cap=None):
    args = (shape[0], shape[1], shape[2], N.TXT_ADSP if adsp else 0)
    sp = SlabPass(engine, text, "txt_direct", "avdb_txt_direct_workspace_size")
    cols = [poisoned(engine, sp.m, dt) for dt in (torch.int64, torch.int32, torch.uint8)]
    counts = poisoned(engine, N.TXTDIR_N_COUNTS, torch.int64)
    sp.call("avdb_txt_direct_size", sp.tp, sp.nb, sp.n_lines, *args, *cols, counts)
    cnt = sp.counts(counts, N.TXTDIR_COUNTS)
    n, nbytes = cnt["rows"], cnt["out_bytes"]
    out = {"text": poisoned(engine, nbytes + 16, torch.uint8), "row_off": poisoned(engine, n + 3, torch.int64)}
    totals = poisoned(engine, 2, torch.int64)
    try:
        rc = sp.call("avdb_txt_direct_write", sp.tp, sp.nb, sp.n_lines, n, *args, *cols, out["text"],
                     nbytes if cap is None else cap, out["row_off"], totals)
    except N.NativeError as e:
        rc = e.rc
    out.update(zip(("row_start", "out_len", "flags"), (c[:n] for c in cols)))
    return rc, cnt, host_arrays(out), totals.cpu().tolist()


def same_arrays(a, b, what=""):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and (a[k] == b[k]).all(), (what, k)


def table_arrays(t):
    """Every array of a TxtTable, on the host (the key set's slots aside: where colliding keys land
    depends on the order the device's lanes insert them in; the probes' answers are compared)."""
    d = {name: getattr(t, name) for name in ("keys", "key_off", "rkeys", "rkey_off", "json", "json_off",
                                             "json_len", "line_start", "flags", "hit")}
    out = host_arrays(d)
    out["counts"] = np.array([t.counts[k] for k in N.TXT_COUNTS], dtype=np.int64)
    return out


def rows_arrays(r, names):
    out = host_arrays({"text": r.text, "row_off": r.row_off})
    if r.match is not None:
        out["match"] = r.match.cpu().numpy()
    out["counts"] = np.array([r.counts[k] for k in names], dtype=np.int64)
    return out

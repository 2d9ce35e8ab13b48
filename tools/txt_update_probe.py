"""K19 probe: the table of a tab-delimited annotation file (Engine.txt_table_build), the update rows
streamed from an export (Engine.txt_update_rows) and the rows of the same file read as primary keys
(Engine.txt_direct_rows), beside K16's two whole calls on K16's own probe inputs, a torch.clone of
each text and the pure-Python restatement of the reference's loop over a sample, all in one run.

Workload, synthesised on the device (it is input, not part of the timing): the export of the K13
probe (tools/cadd_update_probe.py: ``--rows`` lines ``22:PPPPPPPP:R:A:rsNNNNNNNNN<TAB>22:PPPPPPPP:R:A<TAB>\\N``)
and a file of as many lines with four update columns, one of them a 60-byte JSON value,
``22:PPPPPPPP:R:A<TAB>{"NG00000":{"p_value":"0.0e-00","is_gws":false,"pmid":0000}}<TAB>true<TAB>NULL<TAB>0.0000``,
line j carrying the id of the export's SNV formula for row j (seven export rows in eight are SNVs;
positions repeat, so the file holds repeated ids).

Timed: each whole Engine call through its final sync by the host clock, and the library entries
alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/txt_update_probe.py [--rows 1e7] [--host-sample 1e6] [--out profiles/txt_update_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
import torch

import cadd_update_probe as K13
import lof_update_probe as K16
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine

HEADER = b"variant\tgwas_flags\tis_adsp_variant\tother_annotation\tallele_frequencies\n"
VALUE = b'{"NG00000":{"p_value":"0.0e-00","is_gws":false,"pmid":0000}}'
LINE = b"22:00000000:A:C\t" + VALUE + b"\ttrue\tNULL\t0.0000\n"
assert len(VALUE) == 60
SHAPE = (1, 5, 0, 0)  # skip_lines, n_fields, id_col, key_col


def file_text(rows: int, positions: int, device) -> torch.Tensor:
    acgt = K13._bytes(K13.ACGT, device)
    body = torch.empty((rows, len(LINE)), dtype=torch.uint8, device=device)
    body[:] = K13._bytes(LINE, device)
    span = positions + positions // 10
    chunk = 1 << 21
    v = 16  # where the JSON value begins
    for a in range(0, rows, chunk):
        i = torch.arange(a, min(rows, a + chunk), dtype=torch.int64, device=device)
        dst = body[a:a + i.numel()]
        h = (i * 6364136223846793005 >> 17) & 0x7FFFFFFF
        p = K13.LO + i * span // rows
        ref = K13._ref(p)
        K13._digits(dst, 3, p, 8)
        dst[:, 12] = acgt[ref]
        dst[:, 14] = acgt[(ref + 1 + h % 3) & 3]
        K13._digits(dst, v + 4, h % 100000, 5)
        K13._digits(dst, v + 54, h % 10000, 4)
        K13._digits(dst, len(LINE) - 5, h % 10000, 4)
    return torch.cat([K13._bytes(HEADER, device), body.reshape(-1)])


def restated_loop(text: bytes):
    """update_annotation's loop and what parse_variant does per row for a file of primary keys, as the
    reference has them: a DictReader row, the id's split and SimpleNamespace, the loop over the update
    fields with its NULL test, the tuple.  No lookup is made."""
    import csv
    import io
    from types import SimpleNamespace
    reader = csv.DictReader(io.StringIO(text.decode("utf-8"), newline=None), delimiter="\t")
    fields = list(reader.fieldnames)
    fields.remove("variant")
    out = []
    for record in reader:
        variantId = record["variant"]
        info = {"id": variantId, "record_primary_key": variantId}
        parts = variantId.split(":") if ":" in variantId else None
        if parts is not None:
            info["chromosome"] = "chr" + str(parts[0])
        current = SimpleNamespace(**info)
        values = [current.record_primary_key]
        values.append(current.chromosome if hasattr(current, "chromosome") else "chr" + variantId.split(":")[0])
        for f in fields:
            v = record[f]
            values.append(v if v != "NULL" else None)
        out.append(tuple(values))
    return out


def rows_text(rows) -> bytes:
    """Tuples as the passes' row text: tab-joined, None as \\N."""
    return b"".join(("\t".join("\\N" if v is None else v for v in t) + "\n").encode("utf-8") for t in rows)


def table_passes(eng, text, n_lines, reps):
    nb = text.numel()
    ents = [eng.empty(n_lines, torch.int64)] + [eng.empty(n_lines, torch.int32) for _ in range(3)] + \
        [eng.empty(n_lines, torch.uint8)]
    counts = eng.empty(N.TXT_N_COUNTS, torch.int64)
    ws = eng.scratch("txt_table", N.size("avdb_txt_table_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_txt_table_size", text, nb, n_lines, *SHAPE, *ents, counts, ws, ws.numel())  # noqa: E731
    size()
    c = dict(zip(N.TXT_COUNTS, counts.cpu().tolist()))
    n = c["rows"]
    keys, body = eng.empty(max(8, c["key_bytes"]), torch.uint8), eng.empty(max(8, c["json_bytes"]), torch.uint8)
    key_off, body_off, line_start = (eng.empty(n + 1, torch.int64) for _ in range(3))
    body_len, flags, totals = eng.empty(n + 1, torch.int32), eng.empty(n + 1, torch.uint8), eng.empty(4, torch.int64)
    write = lambda: eng._launch("avdb_txt_table_write", text, nb, n_lines, c["entries"], n, *SHAPE, *ents, keys,  # noqa: E731
                                c["key_bytes"], key_off, body, c["json_bytes"], body_off, body_len, line_start, flags,
                                totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [c["key_bytes"], c["json_bytes"], n, 0]
    return t


def update_passes(eng, text, n_lines, table, reps):
    nb = text.numel()
    view = table.view()
    vp = ctypes.byref(view)
    row_start = eng.empty(n_lines, torch.int64)
    pk_len, match, out_len = (eng.empty(n_lines, torch.int32) for _ in range(3))
    flags, counts = eng.empty(n_lines, torch.uint8), eng.empty(N.TXTUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("txt_update", N.size("avdb_txt_update_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_txt_update_size", text, nb, n_lines, vp, N.EXIST_ALL_CONTIGS, 1, 0, row_start,  # noqa: E731
                               pk_len, match, out_len, flags, counts, ws, ws.numel())
    size()
    c = dict(zip(N.TXTUPD_COUNTS, counts.cpu().tolist()))
    out, row_off, totals = eng.empty(max(8, c["out_bytes"]), torch.uint8), eng.empty(c["rows"] + 1, torch.int64), \
        eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_txt_update_write", text, nb, n_lines, c["rows"], vp, 0, row_start, pk_len,  # noqa: E731
                                match, out_len, flags, out, c["out_bytes"], row_off, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [c["out_bytes"], 0]
    return t


def direct_passes(eng, text, n_lines, reps):
    nb = text.numel()
    row_start, out_len, flags = eng.empty(n_lines, torch.int64), eng.empty(n_lines, torch.int32), \
        eng.empty(n_lines, torch.uint8)
    counts = eng.empty(N.TXTDIR_N_COUNTS, torch.int64)
    ws = eng.scratch("txt_direct", N.size("avdb_txt_direct_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_txt_direct_size", text, nb, n_lines, *SHAPE[:3], 0, row_start, out_len, flags,  # noqa: E731
                               counts, ws, ws.numel())
    size()
    c = dict(zip(N.TXTDIR_COUNTS, counts.cpu().tolist()))
    out, row_off, totals = eng.empty(max(8, c["out_bytes"]), torch.uint8), eng.empty(c["rows"] + 1, torch.int64), \
        eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_txt_direct_write", text, nb, n_lines, c["rows"], *SHAPE[:3], 0, row_start,  # noqa: E731
                                out_len, flags, out, c["out_bytes"], row_off, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [c["out_bytes"], 0]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--positions", type=float, default=4e6)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/txt_update_probe.json")
    a = ap.parse_args()
    rows, positions, reps = int(a.rows) // 400 * 400, int(a.positions), max(5, a.reps)
    eng = Engine(0)
    export = K13.export_text(rows, positions, eng.device)
    text = file_text(rows, positions, eng.device)
    torch.cuda.synchronize()
    stats, timed = K13.stats, K16.timed
    got = {}

    def build():
        got.pop("table", None)
        got["table"] = eng.txt_table_build(text)

    t_build = timed(build, reps)
    table = got["table"]
    c = table.counts
    assert c["host_lines"] == 0 and c["entries"] == rows == table.n_rows and c["lines"] == rows + 1

    def update():
        got.pop("rows", None)
        got["rows"] = eng.txt_update_rows(export, table)

    t_update = timed(update, reps)
    r = got.pop("rows")
    assert r.counts["rows"] + r.counts["not_in_file"] == rows and r.n > rows // 2
    upd = {"rows": r.n, "out_bytes": r.counts["out_bytes"], "not_in_file": r.counts["not_in_file"]}
    del r

    def direct():
        got.pop("direct", None)
        got["direct"] = eng.txt_direct_rows(text)

    t_direct = timed(direct, reps)
    d = got.pop("direct")
    assert d.n == rows and d.counts["host_rows"] == 0
    direct_out = d.counts["out_bytes"]
    del d
    t_ts, t_tw = table_passes(eng, text, rows + 1, reps)
    t_us, t_uw = update_passes(eng, export, rows, table, reps)
    t_ds, t_dw = direct_passes(eng, text, rows + 1, reps)
    t_cf, t_ce = K16.events([lambda: text.clone(), lambda: export.clone()], reps)
    # update_annotation's loop restated (restated_loop: no database lookup is in it) over the first
    # lines of the file
    n_s = min(int(a.host_sample), rows)
    s_text = text[:len(HEADER) + n_s * len(LINE)].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    want = restated_loop(s_text)
    host_s = time.perf_counter() - t0
    assert eng.txt_direct_rows(s_text).text.cpu().numpy().tobytes() == rows_text(want) and len(want) == n_s
    del want
    # the driver's reporting: the ids no export row matched and the ids the file repeats, picked on
    # the device (every key probed in the table's own key set); the lists themselves are host strings
    from annotatedvdb_amd.text_update import TextUpdater
    upd_er = TextUpdater(text, "METASEQ", engine=eng)
    upd_er.buffer_export(export)
    upd_er.reset_update_buffer()
    report = {}
    t_groups, = K16.events([lambda: upd_er._id_groups()], reps)
    t_unm = timed(lambda: report.__setitem__("unmatched", len(upd_er.unmatched())), reps)
    t_rep = timed(lambda: report.__setitem__("repeated", len(upd_er.repeated_ids())), reps)
    del upd_er
    # K16's two whole calls and its size pass on K16's own probe inputs, in the same run
    got.clear()
    del table
    vcf = K16.vcf_text(rows, positions, eng.device)
    torch.cuda.synchronize()

    def k16_build():
        got.pop("lof", None)
        got["lof"] = eng.lof_table_build(vcf)

    t_k16a = timed(k16_build, reps)
    lof = got["lof"]

    def k16_update():
        got.pop("lof_rows", None)
        got["lof_rows"] = eng.lof_update_rows(export, lof)

    t_k16b = timed(k16_update, reps)
    got.pop("lof_rows")
    t_k16s, _ = K16.table_passes(eng, vcf, rows, reps)
    t_cv, = K16.events([lambda: vcf.clone()], reps)
    bt, bu, bd = stats(t_build), stats(t_update), stats(t_direct)
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "file_bytes": text.numel(), "export_bytes": export.numel(),
        "k16_vcf_bytes": vcf.numel(), "table_rows": rows, "table_key_bytes": c["key_bytes"],
        "table_body_bytes": c["json_bytes"], "update_rows": upd["rows"], "update_out_bytes": upd["out_bytes"],
        "not_in_file": upd["not_in_file"], "direct_out_bytes": direct_out, "reps": reps,
        "txt_table_build_call_ms": bt, "txt_table_size_pass_ms": stats(t_ts), "txt_table_write_pass_ms": stats(t_tw),
        "txt_update_rows_call_ms": bu, "txt_update_size_pass_ms": stats(t_us), "txt_update_write_pass_ms": stats(t_uw),
        "txt_direct_rows_call_ms": bd, "txt_direct_size_pass_ms": stats(t_ds), "txt_direct_write_pass_ms": stats(t_dw),
        "lof_table_build_call_ms": stats(t_k16a), "lof_update_rows_call_ms": stats(t_k16b),
        "lof_table_size_pass_ms": stats(t_k16s),
        "unmatched_ids": report["unmatched"], "repeated_ids": report["repeated"],
        "id_groups_device_ms": stats(t_groups), "unmatched_call_ms": stats(t_unm), "repeated_ids_call_ms": stats(t_rep),
        "clone_file_ms": stats(t_cf), "clone_export_ms": stats(t_ce), "clone_k16_vcf_ms": stats(t_cv),
        "txt_table_size_pass_GBps_median": round(text.numel() / stats(t_ts)["median"] / 1e6, 1),
        "lof_table_size_pass_GBps_median": round(vcf.numel() / stats(t_k16s)["median"] / 1e6, 1),
        "txt_direct_size_pass_GBps_median": round(text.numel() / stats(t_ds)["median"] / 1e6, 1),
        "txt_update_size_pass_GBps_median": round(export.numel() / stats(t_us)["median"] / 1e6, 1),
        "restatement_sample_rows": n_s, "restatement_s": round(host_s, 3),
        "restatement_lines_per_s": round(n_s / host_s),
        "device_direct_lines_per_s_median": round(rows / bd["median"] * 1e3),
        "device_lines_per_s_table_and_update_calls_median": round(2 * rows / (bt["median"] + bu["median"]) * 1e3),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

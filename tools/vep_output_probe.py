"""K18c probe: the table build with and without the cleaned result (Engine.vep_rows_table_build,
``vep_output``), the two new library entries (avdb_vep_output_size / _write), the wave-per-row update
write (avdb_vep_output_update_write) beside K18b's lane-per-row avdb_vep_rows_update_write on the same
table and export, a torch.clone of the rows (the floor), K18b's table write on the same text (its
k_vr_body is the reader the cleaned-text pass is held against), and ``vep_output_line`` (the reference's
steps in Python) on the templates, all in one run.

Workload (it is input, not part of the timing): tools/vep_rows_probe.py's, with eight fields and a
dbSNP-like INFO in ``input`` (tests/vep_output_common.py's generator).

Timed: the whole Engine calls through their final sync by the host clock, and the library entries
alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/vep_output_probe.py [--lines 2e5] [--out profiles/vep_output_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, "tests")
import torch

import cadd_update_probe as K13
import lof_update_probe as K16
import vep_common as V
import vep_output_common as O
import vep_rows_probe as K18B
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine, existing_contig_mask
from annotatedvdb_amd.vep_consequences import ConsequenceRanking
from annotatedvdb_amd.vep_rows import vep_output_line

POS0, ALG_ID = K18B.POS0, K18B.ALG_ID


def template_lines(n: int, max_csq: int):
    """(lines, where POS stands in each): the K18c generator's lines, members in VEP's order, POS0 for POS."""
    gen = O.OutputLineGenerator(V.combos_of(V.read_ranking_rows()), 18)
    lines, pos_at = [], []
    for _ in range(n):
        o = gen.obj(n_csq=1 + gen.rng.randrange(max_csq))
        f = o["input"].split("\t")
        f[1] = str(POS0)
        assert len(f) >= 8
        o["input"] = "\t".join(f)
        line = V.dumps(o)
        pos_at.append(line.index('\\t%d\\t' % POS0) + 2)
        lines.append(line)
    return lines, pos_at


def output_entries(eng, text, n_lines, table, reps):
    """K18c's size and write entries alone, by device events, on the arrays the table's build kept."""
    csq, blob, rank_off, el_rlen = table._keep
    view = N.VepRowsIn(len(table.ranking.ranks), csq.counts["consequences"], N.ptr(blob), blob.numel(), N.ptr(rank_off),
                       *[N.ptr(getattr(csq, a)) for a in ("flags", "n_csq", "csq_off", "input_start", "input_len", "type",
                                                          "order", "el_start", "el_len", "al_start", "al_len", "entry",
                                                          "coding", "sorted")], N.ptr(el_rlen))
    vp = ctypes.byref(view)
    nb = text.numel()
    ent_flags = torch.zeros(n_lines, dtype=torch.uint8, device=eng.device)  # (no line is K18b's host's: asserted by the caller)
    cols = [eng.empty(n_lines, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
    counts = eng.empty(N.VEPOUT_N_COUNTS, torch.int64)
    ws = eng.scratch("vep_output", N.size("avdb_vep_output_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_vep_output_size", text, nb, n_lines, vp, ent_flags, 0, *cols, counts, ws, ws.numel())  # noqa: E731
    size()
    c = dict(zip(N.VEPOUT_COUNTS, counts.cpu().tolist()))
    assert c["host_lines"] == 0 and c["lines"] == n_lines, c
    lens = cols[1].long()
    off = torch.cumsum(lens, 0) - lens
    total = c["out_bytes"]
    out, totals = eng.empty(total, torch.uint8), eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_vep_output_write", text, nb, n_lines, vp, 0, off, *cols[1:], out, total, totals, ws,  # noqa: E731
                                ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [total, 0]
    assert torch.equal(out, table.cleaned)
    return t, c


def wide_update_write(eng, export, n_lines, table, reps):
    """The update write with the extra column alone, by device events, behind K18b's size entry."""
    view, cleaned = table.view(), table.cleaned_view()
    nb = export.numel()
    cols = [eng.empty(n_lines, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
    counts = eng.empty(N.LOFUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("vep_rows_update", N.size("avdb_vep_rows_update_workspace_size", nb, n_lines))
    eng._launch("avdb_vep_rows_update_size", export, nb, n_lines, ctypes.byref(view), existing_contig_mask(None), 0, ALG_ID,
                *cols, counts, ws, ws.numel())
    c = dict(zip(N.LOFUPD_COUNTS, counts.cpu().tolist()))
    n = c["rows"]
    add = 1 + table.cleaned_len[table.row_entry[cols[2][:n].long()].long()]
    cols[3][:n] += add
    ob = c["out_bytes"] + int(add.sum())
    out, row_off, totals = eng.empty(ob, torch.uint8), eng.empty(n + 1, torch.int64), eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_vep_output_update_write", export, nb, n_lines, n, ctypes.byref(view),  # noqa: E731
                                ctypes.byref(cleaned), 0, ALG_ID, *cols, out, ob, row_off, totals, ws, ws.numel())
    (t,) = K16.events([write], reps)
    assert totals.cpu().tolist() == [ob, 0]
    return t, ob, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=float, default=2e5)
    ap.add_argument("--templates", type=int, default=251)
    ap.add_argument("--max-csq", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/vep_output_probe.json")
    a = ap.parse_args()
    reps = max(5, a.reps)
    eng = Engine(0)
    ranking = ConsequenceRanking(V.RANKING_FILE)
    templates, pos_at = template_lines(a.templates, a.max_csq)
    tiles = max(1, int(a.lines) // a.templates)
    n_lines = tiles * a.templates
    text = K18B.tiled_text(eng, templates, pos_at, tiles)
    torch.cuda.synchronize()
    stats, timed, events = K13.stats, K16.timed, K16.events
    got = {}

    def build(vep_output):
        got.pop("table", None)
        got["table"] = eng.vep_rows_table_build(text, ranking, vep_output=vep_output)

    t_plain = timed(lambda: build(False), reps)
    t_build = timed(lambda: build(True), reps)
    table = got.pop("table")
    assert table.counts["host_lines"] == 0 and table.cleaned_counts["host_lines"] == 0, (table.counts, table.cleaned_counts)
    # the first block of templates against the host path, text for text
    first = text[:len(V.slab(templates))].cpu().numpy().tobytes().decode("ascii").splitlines()
    t0 = time.perf_counter()
    want = [vep_output_line(line, False) for line in first]
    host_s = time.perf_counter() - t0
    assert O.cleaned_texts(eng.vep_rows_table_build(V.slab(first), ranking, vep_output=True)) == want
    (t_os, t_ow), c = output_entries(eng, text, n_lines, table, reps)
    # an export of every id, in table order
    ko = table.key_off.cpu().numpy()
    keys = table.keys.cpu().numpy().tobytes()
    export = eng._as_text("".join("pk%d\t%s\t\\N\n" % (r, keys[ko[r]:ko[r + 1]].decode("ascii"))
                                  for r in range(table.n_rows)).encode("ascii"))
    n_records = table.n_rows

    def update():
        got.pop("rows", None)
        got["rows"] = eng.vep_update_rows(export, table, ALG_ID)

    t_upd = timed(update, reps)
    rows = got.pop("rows")
    assert rows.n == n_records and rows.counts["not_annotated"] == 0, rows.counts
    t_wide, wide_bytes, wide_out = wide_update_write(eng, export, n_records, table, reps)
    assert torch.equal(wide_out, rows.text)
    head = rows.text[:int(rows.row_off[1])].cpu().numpy().tobytes().decode("ascii").split("\t")
    assert head[0] == "pk0" and head[4] == want[0] and head[5] == "%d\n" % ALG_ID
    (t_clone_rows,) = events([lambda: rows.text.clone()], reps)
    del rows, wide_out
    (t_us, t_uw), cu, narrow_out = K18B.update_entries(eng, export, n_records, table, reps)  # K18b's write, same table
    narrow_bytes = narrow_out.numel()
    del narrow_out
    cleaned_bytes, body_bytes = table.cleaned.numel(), table.json.numel()
    del table, got
    torch.cuda.empty_cache()
    (t_ts, t_tw), c2, el_bytes = K18B.table_entries(eng, text, n_lines, ranking, reps)  # K18b's k_vr_body, same text
    (t_clone,) = events([lambda: text.clone()], reps)
    text_bytes = text.numel()
    med = lambda t: stats(t)["median"]  # noqa: E731
    out = {
        "device": torch.cuda.get_device_name(0), "lines": n_lines, "text_bytes": text_bytes, "templates": a.templates,
        "mean_line_bytes": round(text_bytes / n_lines, 1), "table_rows": c2["rows"], "body_bytes": body_bytes,
        "element_bytes": el_bytes, "cleaned_bytes": cleaned_bytes, "mean_cleaned_bytes": round(cleaned_bytes / n_lines, 1),
        "export_records": n_records, "export_bytes": export.numel(), "update_out_bytes_with_vep_output": wide_bytes,
        "update_out_bytes_k18b": narrow_bytes, "reps": reps,
        "vep_rows_table_build_call_ms": stats(t_plain), "vep_rows_table_build_vep_output_call_ms": stats(t_build),
        "vep_update_rows_vep_output_call_ms": stats(t_upd),
        "vep_output_size_ms": stats(t_os), "vep_output_write_ms": stats(t_ow),
        "vep_output_update_write_ms": stats(t_wide), "vep_rows_update_size_ms": stats(t_us),
        "vep_rows_update_write_ms": stats(t_uw), "vep_rows_table_size_ms": stats(t_ts),
        "vep_rows_table_write_ms": stats(t_tw), "clone_text_ms": stats(t_clone), "clone_rows_ms": stats(t_clone_rows),
        "update_written_GBps_vep_output_update_write_median": round(wide_bytes / med(t_wide) / 1e6, 1),
        "update_written_GBps_vep_rows_update_write_median": round(narrow_bytes / med(t_uw) / 1e6, 1),
        "clone_rows_GBps_median": round(wide_bytes / med(t_clone_rows) / 1e6, 1),
        "text_read_GBps_vep_output_size_median": round(text_bytes / med(t_os) / 1e6, 1),
        "text_read_GBps_vep_output_write_median": round(text_bytes / med(t_ow) / 1e6, 1),
        "element_read_GBps_vep_rows_table_write_median": round(el_bytes / med(t_tw) / 1e6, 1),
        "vep_output_line_sample_lines": len(first), "vep_output_line_s": round(host_s, 3),
        "vep_output_line_lines_per_s": round(len(first) / host_s),
        "device_lines_per_s_table_build_call_median": round(n_lines / med(t_plain) * 1e3),
        "device_lines_per_s_table_build_vep_output_call_median": round(n_lines / med(t_build) * 1e3),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

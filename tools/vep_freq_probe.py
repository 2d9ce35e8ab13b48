"""K18d probe: the table build with and without the allele_frequencies column (Engine.vep_rows_table_build,
``allele_frequencies``, beside ``vep_output`` alone), the two new library entries (avdb_vep_freq_size / _write),
the update write with the column (avdb_vep_freq_update_write) beside K18c's avdb_vep_output_update_write on
the same table and export, K18c's size and write entries on the same text (they read it with the same
per-block chain: the yardsticks), and ``allele_frequencies_line`` (the reference's steps in Python) on the
templates, all in one run.

Workload (it is input, not part of the timing): tools/vep_output_probe.py's, with ``colocated_variants``
frequencies and a ``FREQ`` item in INFO (tests/vep_freq_common.py's generator).  Not measured: real VEP
output (its allele objects hold some thirty members, the generator's one to sixteen), and host lines at scale
(no line of the workload is the host's).

Timed: the whole Engine calls through their final sync by the host clock, and the library entries alone by
device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/vep_freq_probe.py [--lines 2e5] [--out profiles/vep_freq_probe.json]
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
import vep_freq_common as F
import vep_output_probe as K18C
import vep_rows_probe as K18B
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine, existing_contig_mask
from annotatedvdb_amd.vep_consequences import ConsequenceRanking
from annotatedvdb_amd.vep_rows import allele_frequencies_line

POS0, ALG_ID = K18B.POS0, K18B.ALG_ID


def template_lines(n: int, max_csq: int):
    """(lines, where POS stands in each): the K18d generator's lines, POS0 for POS."""
    gen = F.FreqLineGenerator(V.combos_of(V.read_ranking_rows()), 18)
    lines, pos_at = [], []
    for _ in range(n):
        o = gen.obj(n_csq=1 + gen.rng.randrange(max_csq))
        f = o["input"].split("\t")
        f[1] = str(POS0)
        o["input"] = "\t".join(f)
        line = V.dumps(o)
        pos_at.append(line.index('\\t%d\\t' % POS0) + 2)
        lines.append(line)
    return lines, pos_at


def freq_entries(eng, text, n_lines, table, reps):
    """K18d's size and write entries alone, by device events, on the arrays the table's build kept."""
    csq, blob, rank_off, el_rlen = table._keep
    view = N.VepRowsIn(len(table.ranking.ranks), csq.counts["consequences"], N.ptr(blob), blob.numel(), N.ptr(rank_off),
                       *[N.ptr(getattr(csq, a)) for a in ("flags", "n_csq", "csq_off", "input_start", "input_len", "type",
                                                          "order", "el_start", "el_len", "al_start", "al_len", "entry",
                                                          "coding", "sorted")], N.ptr(el_rlen))
    vp = ctypes.byref(view)
    nb, n_rows = text.numel(), table.n_rows
    # (no line is the host's: asserted by the caller; every line has rows, so the rows' line starts give the entries)
    ent_start, alts = torch.unique_consecutive(table.line_start, return_counts=True)
    assert ent_start.numel() == n_lines
    ent_alts = alts.to(torch.int32)
    row0 = torch.cumsum(alts, 0) - alts
    ent_flags = torch.zeros(n_lines, dtype=torch.uint8, device=eng.device)
    cols = [eng.empty(n_lines, dt) for dt in (torch.int64, torch.int32, torch.int64, torch.int32, torch.uint8)]
    freq_len = eng.empty(n_rows, torch.int32)
    counts = eng.empty(N.VEPFREQ_N_COUNTS, torch.int64)
    fl = (N.VEPFREQ_IDENTITY_ONLY if table.identity_only else 0) | (N.VEPFREQ_MATCH_REFSNP if table.match_refsnp else 0)
    ws = eng.scratch("vep_freq", N.size("avdb_vep_freq_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_vep_freq_size", text, nb, n_lines, n_rows, vp, ent_start, ent_alts, ent_flags, row0, fl,  # noqa: E731
                               *cols, freq_len, counts, ws, ws.numel())
    size()
    c = dict(zip(N.VEPFREQ_COUNTS, counts.cpu().tolist()))
    assert c["host_lines"] == 0 and c["lines"] == n_lines and c["rows"] == n_rows, c
    lens = freq_len.long()
    off = torch.cumsum(lens, 0) - lens
    total = c["out_bytes"]
    out, totals = eng.empty(total, torch.uint8), eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_vep_freq_write", text, nb, n_lines, n_rows, vp, ent_alts, row0, *cols, off, freq_len, out,  # noqa: E731
                                total, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [total, 0]
    assert torch.equal(out, table.freq)
    span_bytes = int(cols[1].long().sum())  # the chosen objects: what the row walks read (once per ALT)
    return t, c, span_bytes


def freq_update_write(eng, export, n_lines, table, reps):
    """The update write with the column (and vep_output) alone, by device events, behind K18b's size entry."""
    view, cleaned, freq = table.view(), table.cleaned_view(), table.freq_view()
    nb = export.numel()
    cols = [eng.empty(n_lines, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
    counts = eng.empty(N.LOFUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("vep_rows_update", N.size("avdb_vep_rows_update_workspace_size", nb, n_lines))
    eng._launch("avdb_vep_rows_update_size", export, nb, n_lines, ctypes.byref(view), existing_contig_mask(None), 0, ALG_ID,
                *cols, counts, ws, ws.numel())
    c = dict(zip(N.LOFUPD_COUNTS, counts.cpu().tolist()))
    n = c["rows"]
    rows = cols[2][:n].long()
    add = 2 + table.cleaned_len[table.row_entry[rows].long()] + table.freq_len[rows]
    cols[3][:n] += add
    ob = c["out_bytes"] + int(add.sum())
    out, row_off, totals = eng.empty(ob, torch.uint8), eng.empty(n + 1, torch.int64), eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_vep_freq_update_write", export, nb, n_lines, n, ctypes.byref(view), ctypes.byref(freq),  # noqa: E731
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
    ap.add_argument("--out", default="profiles/vep_freq_probe.json")
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

    def build(**kw):
        got.pop("table", None)
        got["table"] = eng.vep_rows_table_build(text, ranking, **kw)

    t_plain = timed(lambda: build(), reps)
    t_vo = timed(lambda: build(vep_output=True), reps)
    t_fq = timed(lambda: build(allele_frequencies=True, match_refsnp=True), reps)
    t_both = timed(lambda: build(vep_output=True, allele_frequencies=True, match_refsnp=True), reps)
    table = got.pop("table")
    assert table.counts["host_lines"] == 0 and table.cleaned_counts["host_lines"] == 0 and \
        table.freq_counts["host_lines"] == 0, (table.counts, table.cleaned_counts, table.freq_counts)
    # the first block of templates against the host path, text for text
    first = text[:len(V.slab(templates))].cpu().numpy().tobytes().decode("ascii").splitlines()
    t0 = time.perf_counter()
    want = [t for line in first for _, t in allele_frequencies_line(line, False, True)]
    host_s = time.perf_counter() - t0
    assert F.freq_texts(eng.vep_rows_table_build(V.slab(first), ranking, allele_frequencies=True, match_refsnp=True)) == want
    (t_fs, t_fw), c, span_bytes = freq_entries(eng, text, n_lines, table, reps)
    (t_os, t_ow), _ = K18C.output_entries(eng, text, n_lines, table, reps)  # K18c's passes, same text
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
    t_full, full_bytes, full_out = freq_update_write(eng, export, n_records, table, reps)
    assert torch.equal(full_out, rows.text)
    head = rows.text[:int(rows.row_off[1])].cpu().numpy().tobytes().decode("ascii").split("\t")
    assert head[0] == "pk0" and head[2] == want[0] and head[6] == "%d\n" % ALG_ID
    (t_clone_rows,) = events([lambda: rows.text.clone()], reps)
    del rows, full_out
    t_wide, wide_bytes, wide_out = K18C.wide_update_write(eng, export, n_records, table, reps)  # K18c's write, same table
    del wide_out
    (t_clone,) = events([lambda: text.clone()], reps)
    text_bytes, freq_bytes, n_rows = text.numel(), table.freq.numel(), table.n_rows
    med = lambda t: stats(t)["median"]  # noqa: E731
    out = {
        "device": torch.cuda.get_device_name(0), "lines": n_lines, "text_bytes": text_bytes, "templates": a.templates,
        "mean_line_bytes": round(text_bytes / n_lines, 1), "table_rows": n_rows, "freq_bytes": freq_bytes,
        "mean_freq_bytes_per_row": round(freq_bytes / n_rows, 1), "chosen_object_bytes": span_bytes,
        "export_records": n_records, "export_bytes": export.numel(), "update_out_bytes_full_tuple": full_bytes,
        "update_out_bytes_k18c": wide_bytes, "reps": reps,
        "vep_rows_table_build_call_ms": stats(t_plain), "vep_rows_table_build_vep_output_call_ms": stats(t_vo),
        "vep_rows_table_build_allele_frequencies_call_ms": stats(t_fq),
        "vep_rows_table_build_both_call_ms": stats(t_both), "vep_update_rows_full_tuple_call_ms": stats(t_upd),
        "vep_freq_size_ms": stats(t_fs), "vep_freq_write_ms": stats(t_fw), "vep_output_size_ms": stats(t_os),
        "vep_output_write_ms": stats(t_ow), "vep_freq_update_write_ms": stats(t_full),
        "vep_output_update_write_ms": stats(t_wide), "clone_text_ms": stats(t_clone), "clone_rows_ms": stats(t_clone_rows),
        "ratio_vep_freq_size_to_vep_output_size_median": round(med(t_fs) / med(t_os), 2),
        "ratio_vep_freq_write_to_vep_output_write_median": round(med(t_fw) / med(t_ow), 2),
        "ratio_build_both_to_build_vep_output_median": round(med(t_both) / med(t_vo), 3),
        "text_read_GBps_vep_freq_size_median": round(text_bytes / med(t_fs) / 1e6, 1),
        "text_read_GBps_vep_output_size_median": round(text_bytes / med(t_os) / 1e6, 1),
        "update_written_GBps_vep_freq_update_write_median": round(full_bytes / med(t_full) / 1e6, 1),
        "update_written_GBps_vep_output_update_write_median": round(wide_bytes / med(t_wide) / 1e6, 1),
        "clone_rows_GBps_median": round(full_bytes / med(t_clone_rows) / 1e6, 1),
        "allele_frequencies_line_sample_lines": len(first), "allele_frequencies_line_s": round(host_s, 3),
        "allele_frequencies_line_lines_per_s": round(len(first) / host_s),
        "device_lines_per_s_table_build_both_call_median": round(n_lines / med(t_both) * 1e3),
        "not_measured": ["real VEP output", "host lines at scale"],
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

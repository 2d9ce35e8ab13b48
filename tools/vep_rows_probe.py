"""K18b probe: the table build over VEP JSON lines (Engine.vep_rows_table_build) and the export join
(Engine.vep_update_rows) with their four library entries, beside the K18a call they sit on, a
torch.clone of the text and of the rows (the floor), and ``vep_rows_line`` (the reference's pass
over a line, in Python) on the templates, all in one run.

Workload (it is input, not part of the timing): tools/vep_consequence_probe.py's, with ``input`` made
consistent with the alleles (tests/vep_rows_common.py's generator): ``--templates`` synthetic lines,
every line with all its consequences in one array of 1 to ``--max-csq`` elements, tiled on the
device to ``--lines`` lines; POS is a nine-digit field rewritten on the device so that every line
has metaseq ids of its own.  The export holds every id of the table once, ``vep_output`` NULL.

Timed: the whole Engine calls through their final sync by the host clock, and the library entries
alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/vep_rows_probe.py [--lines 2e5] [--out profiles/vep_rows_probe.json]
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
import numpy as np
import torch

import cadd_update_probe as K13
import lof_update_probe as K16
import vep_common as V
import vep_rows_common as R
from annotatedvdb_amd import _native as N
from annotatedvdb_amd import slab_passes
from annotatedvdb_amd.engine import Engine, existing_contig_mask
from annotatedvdb_amd.vep_consequences import ConsequenceRanking
from annotatedvdb_amd.vep_rows import vep_rows_line

POS0 = 100000000  # nine digits, and so is POS0 + any line number of the probe
ALG_ID = 4242


def template_lines(n: int, max_csq: int):
    """(lines, where POS stands in each): the generator's lines with POS0 for POS."""
    gen = R.RowsLineGenerator(V.combos_of(V.read_ranking_rows()), 18)
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


def tiled_text(eng, templates, pos_at, tiles: int):
    block = eng._as_text(V.slab(templates))
    text = block.repeat(tiles)
    starts = np.concatenate([[0], np.cumsum([len(t) + 1 for t in templates])[:-1]])
    at = torch.from_numpy(starts + np.array(pos_at)).to(eng.device)  # per template
    line = torch.arange(tiles * len(templates), device=eng.device)
    where = (line // len(templates)) * block.numel() + at[line % len(templates)]
    value = POS0 + line
    for d in range(9):
        text[where + (8 - d)] = (48 + (value // 10 ** d) % 10).to(torch.uint8)
    return text


def table_entries(eng, text, n_lines, ranking, reps):
    """K18b's two table entries alone, by device events, on K18a's arrays of the text."""
    csq = eng.vep_consequences(text, ranking)
    rank_text = [json.dumps(r).encode("ascii") for r in ranking.ranks]
    off = np.zeros(len(rank_text) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(t) for t in rank_text])
    blob = eng._as_text(b"".join(rank_text))
    rank_off = torch.from_numpy(off.view(np.int32)).to(eng.device)
    total = csq.counts["consequences"]
    el_rlen = eng.empty(max(1, total), torch.int32)
    view = N.VepRowsIn(len(rank_text), total, N.ptr(blob), int(off[-1]), N.ptr(rank_off),
                       *[N.ptr(getattr(csq, a)) for a in ("flags", "n_csq", "csq_off", "input_start", "input_len", "type",
                                                          "order", "el_start", "el_len", "al_start", "al_len", "entry",
                                                          "coding", "sorted")], N.ptr(el_rlen))
    vp = ctypes.byref(view)
    nb = text.numel()
    ents = [eng.empty(n_lines, torch.int64)] + [eng.empty(n_lines, torch.int32) for _ in range(3)] + \
        [eng.empty(n_lines, torch.uint8)]
    counts = eng.empty(N.VEPROWS_N_COUNTS, torch.int64)
    ws = eng.scratch("vep_rows_table", N.size("avdb_vep_rows_table_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_vep_rows_table_size", text, nb, n_lines, vp, *ents, counts, ws, ws.numel())  # noqa: E731
    size()
    c = dict(zip(N.VEPROWS_COUNTS, counts.cpu().tolist()))
    assert c["host_lines"] == 0 and c["entries"] == n_lines, c
    n, kb, jb = c["rows"], c["key_bytes"], c["json_bytes"]
    keys, body = eng.empty(kb, torch.uint8), eng.empty(jb, torch.uint8)
    key_off = eng.empty(n + 1, torch.int64)
    rows = [eng.empty(n, dt) for dt in (torch.int64, torch.int32, torch.int64, torch.uint8)]
    totals = eng.empty(4, torch.int64)
    write = lambda: eng._launch("avdb_vep_rows_table_write", text, nb, n_lines, n_lines, n, vp, *ents, keys, kb, key_off,  # noqa: E731
                                body, jb, *rows, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [kb, jb, n, 0]
    el_bytes = int(csq.el_len.long().sum())
    return t, c, el_bytes


def update_entries(eng, export, n_lines, table, reps):
    view = table.view()
    vp = ctypes.byref(view)
    nb = export.numel()
    cols = [eng.empty(n_lines, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
    counts = eng.empty(N.LOFUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("vep_rows_update", N.size("avdb_vep_rows_update_workspace_size", nb, n_lines))
    mask = existing_contig_mask(None)
    size = lambda: eng._launch("avdb_vep_rows_update_size", export, nb, n_lines, vp, mask, 0, ALG_ID, *cols, counts, ws,  # noqa: E731
                               ws.numel())
    size()
    c = dict(zip(N.LOFUPD_COUNTS, counts.cpu().tolist()))
    n, ob = c["rows"], c["out_bytes"]
    out, row_off, totals = eng.empty(ob, torch.uint8), eng.empty(n + 1, torch.int64), eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_vep_rows_update_write", export, nb, n_lines, n, vp, 0, ALG_ID, *cols, out, ob,  # noqa: E731
                                row_off, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [ob, 0]
    return t, c, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=float, default=2e5)
    ap.add_argument("--templates", type=int, default=251)
    ap.add_argument("--max-csq", type=int, default=60)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/vep_rows_probe.json")
    a = ap.parse_args()
    reps = max(5, a.reps)
    eng = Engine(0)
    ranking = ConsequenceRanking(V.RANKING_FILE)
    templates, pos_at = template_lines(a.templates, a.max_csq)
    tiles = max(1, int(a.lines) // a.templates)
    n_lines = tiles * a.templates
    text = tiled_text(eng, templates, pos_at, tiles)
    torch.cuda.synchronize()
    stats, timed, events = K13.stats, K16.timed, K16.events
    got = {}

    def consequences():
        got.pop("csq", None)
        got["csq"] = eng.vep_consequences(text, ranking)

    t_csq = timed(consequences, reps)
    got.clear()

    def build():
        got.pop("table", None)
        got["table"] = eng.vep_rows_table_build(text, ranking)

    t_build = timed(build, reps)
    table = got["table"]
    c = table.counts
    assert c["lines"] == n_lines and c["host_lines"] == 0, c
    # the first block of templates against the host path, row for row
    first = text[:len(V.slab(templates))].cpu().numpy().tobytes().decode("ascii").splitlines()
    t0 = time.perf_counter()
    want = [tuple(r) for line in first for r in vep_rows_line(line, ranking)]
    host_s = time.perf_counter() - t0
    small = eng.vep_rows_table_build(V.slab(first), ranking)
    assert R.table_rows(small) == want
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
    out_bytes = rows.text.numel()
    head = rows.text[:int(rows.row_off[1])].cpu().numpy().tobytes().decode("ascii")
    assert head == "pk0\tchr%s\t%s\t%s\t%d\n" % (want[0][0].split(":")[0], want[0][1], want[0][2], ALG_ID)
    (t_us, t_uw), cu, _ = update_entries(eng, export, n_records, table, reps)
    (t_clone_rows,) = events([lambda: rows.text.clone()], reps)
    del rows
    body_bytes, key_bytes = table.json.numel(), table.keys.numel()
    del table, got
    torch.cuda.empty_cache()
    (t_ts, t_tw), c2, el_bytes = table_entries(eng, text, n_lines, ranking, reps)
    assert c2 == c
    (t_clone,) = events([lambda: text.clone()], reps)
    text_bytes = text.numel()
    tw, uw = stats(t_tw)["median"], stats(t_uw)["median"]
    out = {
        "device": torch.cuda.get_device_name(0), "lines": n_lines, "text_bytes": text_bytes, "templates": a.templates,
        "mean_line_bytes": round(text_bytes / n_lines, 1), "table_rows": c["rows"], "key_bytes": key_bytes,
        "body_bytes": body_bytes, "element_bytes": el_bytes, "export_records": n_records, "export_bytes": export.numel(),
        "update_out_bytes": out_bytes, "reps": reps,
        "vep_consequences_call_ms": stats(t_csq), "vep_rows_table_build_call_ms": stats(t_build),
        "vep_update_rows_call_ms": stats(t_upd),
        "vep_rows_table_size_ms": stats(t_ts), "vep_rows_table_write_ms": stats(t_tw),
        "vep_rows_update_size_ms": stats(t_us), "vep_rows_update_write_ms": stats(t_uw),
        "clone_text_ms": stats(t_clone), "clone_rows_ms": stats(t_clone_rows),
        "render_read_GBps_table_write_median": round(el_bytes / tw / 1e6, 1),
        "render_written_GBps_table_write_median": round(body_bytes / tw / 1e6, 1),
        "update_written_GBps_update_write_median": round(out_bytes / uw / 1e6, 1),
        "vep_rows_line_sample_lines": len(first), "vep_rows_line_s": round(host_s, 3),
        "vep_rows_line_lines_per_s": round(len(first) / host_s),
        "device_lines_per_s_table_build_call_median": round(n_lines / stats(t_build)["median"] * 1e3),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

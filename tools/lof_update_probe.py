"""K16 probe: the SnpEff LOF/NMD table (Engine.lof_table_build) and the update rows streamed
from an export (Engine.lof_update_rows), beside K13's whole call on the same export, a
torch.clone of each text and the pure-Python restatement of the reference's loop over a sample,
all in one run.

Workload, synthesised on the device (it is input, not part of the timing): the export of the K13
probe (tools/cadd_update_probe.py: ``--rows`` lines ``22:PPPPPPPP:R:A:rsNNNNNNNNN<TAB>22:PPPPPPPP:R:A<TAB>\\N``)
and a SnpEff-like VCF of as many lines, ``22<TAB>PPPPPPPP<TAB>.<TAB>R<TAB>A<TAB>.<TAB>.<TAB>ANN=...;AC=1``
with the alleles of the export's row of the same number, one line in 50 carrying
``;LOF=(GENE|ENSG...|NN|0.NN)``.  Three quarters of the annotated lines name an id the export holds.

Timed: each whole Engine call through its final sync by the host clock, and the library entries
alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/lof_update_probe.py [--rows 1e7] [--host-sample 1e6] [--out profiles/lof_update_probe.json]
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
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.cadd import CaddTable
from annotatedvdb_amd.engine import Engine

PLAIN = b"22\t00000000\t.\tA\tC\t.\t.\tANN=C|missense_variant|MODERATE|GENE0000|ENSG00000000000;AC=1\n"
LOF = b"22\t00000000\t.\tA\tC\t.\t.\tANN=C|stop_gained|HIGH|GENE0000|ENSG00000000000;AC=1;LOF=(GENE0000|ENSG00000000000|12|0.25)\n"
EVERY = 50
GROUP = (EVERY - 1) * len(PLAIN) + len(LOF)


def vcf_text(rows: int, positions: int, device) -> torch.Tensor:
    """``rows`` lines (a multiple of 50), line 25 of every 50 annotated; line j carries the position
    and alleles of the export's row j (its SNV formula)."""
    assert rows % EVERY == 0
    acgt = K13._bytes(K13.ACGT, device)
    out = torch.empty((rows // EVERY, GROUP), dtype=torch.uint8, device=device)
    out[:] = K13._bytes(PLAIN * 25 + LOF + PLAIN * 24, device)
    span = positions + positions // 10
    chunk = 1 << 16
    for a in range(0, rows // EVERY, chunk):
        g = torch.arange(a, min(rows // EVERY, a + chunk), dtype=torch.int64, device=device)
        dst = out[a:a + g.numel()]
        for k in range(EVERY):
            i = EVERY * g + k
            at = k * len(PLAIN) + (len(LOF) - len(PLAIN) if k > 25 else 0)
            h = (i * 6364136223846793005 >> 17) & 0x7FFFFFFF
            p = K13.LO + i * span // rows
            ref = K13._ref(p)
            K13._digits(dst, at + 3, p, 8)
            dst[:, at + 14] = acgt[ref]
            dst[:, at + 16] = acgt[(ref + 1 + h % 3) & 3]
            if k == 25:
                K13._digits(dst, at + len(LOF) - 9, h % 100, 2)   # the count
                K13._digits(dst, at + len(LOF) - 4, h % 97, 2)    # the fraction's digits
    return out.reshape(-1)


def timed(f, reps):
    f()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def events(steps, reps):
    """``steps``: callables that enqueue; per step the device times of ``reps`` runs after a warm-up."""
    out = [[] for _ in steps]
    for r in range(reps + 1):
        for k, f in enumerate(steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            if r:
                out[k].append(a.elapsed_time(b))
    return out


def table_passes(eng, text, n_lines, reps):
    nb = text.numel()
    ents = [eng.empty(n_lines, torch.int64)] + [eng.empty(n_lines, torch.int32) for _ in range(3)] + \
        [eng.empty(n_lines, torch.uint8)]
    counts = eng.empty(N.LOF_N_COUNTS, torch.int64)
    ws = eng.scratch("lof_table", N.size("avdb_lof_table_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_lof_table_size", text, nb, n_lines, *ents, counts, ws, ws.numel())  # noqa: E731
    size()
    c = dict(zip(N.LOF_COUNTS, counts.cpu().tolist()))
    n = c["rows"]
    keys, js = eng.empty(max(8, c["key_bytes"]), torch.uint8), eng.empty(max(8, c["json_bytes"]), torch.uint8)
    key_off, json_off, line_start = (eng.empty(n + 1, torch.int64) for _ in range(3))
    json_len, flags, totals = eng.empty(n + 1, torch.int32), eng.empty(n + 1, torch.uint8), eng.empty(4, torch.int64)
    write = lambda: eng._launch("avdb_lof_table_write", text, nb, n_lines, c["entries"], n, *ents, keys,  # noqa: E731
                                c["key_bytes"], key_off, js, c["json_bytes"], json_off, json_len, line_start, flags,
                                totals, ws, ws.numel())
    t = events([size, write], reps)
    assert totals.cpu().tolist() == [c["key_bytes"], c["json_bytes"], n, 0]
    return t


def update_passes(eng, text, n_lines, table, reps):
    nb = text.numel()
    view = table.view()
    vp = ctypes.byref(view)
    row_start = eng.empty(n_lines, torch.int64)
    pk_len, match, out_len = (eng.empty(n_lines, torch.int32) for _ in range(3))
    flags, counts = eng.empty(n_lines, torch.uint8), eng.empty(N.LOFUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("lof_update", N.size("avdb_lof_update_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_lof_update_size", text, nb, n_lines, vp, N.EXIST_ALL_CONTIGS, 0, row_start,  # noqa: E731
                               pk_len, match, out_len, flags, counts, ws, ws.numel())
    size()
    c = dict(zip(N.LOFUPD_COUNTS, counts.cpu().tolist()))
    out, row_off, totals = eng.empty(max(8, c["out_bytes"]), torch.uint8), eng.empty(c["rows"] + 1, torch.int64), \
        eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_lof_update_write", text, nb, n_lines, c["rows"], vp, row_start, pk_len,  # noqa: E731
                                match, out_len, flags, out, c["out_bytes"], row_off, totals, ws, ws.numel())
    t = events([size, write], reps)
    assert totals.cpu().tolist() == [c["out_bytes"], 0]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--positions", type=float, default=4e6)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/lof_update_probe.json")
    a = ap.parse_args()
    rows, positions, reps = int(a.rows) // 400 * 400, int(a.positions), max(5, a.reps)
    eng = Engine(0)
    export = K13.export_text(rows, positions, eng.device)
    vcf = vcf_text(rows, positions, eng.device)
    torch.cuda.synchronize()
    stats = K13.stats
    got = {}

    def build():
        got.pop("table", None)
        got["table"] = eng.lof_table_build(vcf)

    t_build = timed(build, reps)
    table = got["table"]
    c = table.counts
    assert c["host_lines"] == 0 and c["entries"] == rows // EVERY == table.n_rows and c["lines"] == rows

    def update():
        got.pop("rows", None)
        got["rows"] = eng.lof_update_rows(export, table)

    t_update = timed(update, reps)
    r = got["rows"]
    assert r.counts["rows"] + r.counts["not_annotated"] == rows and r.n > rows // 400
    t_ts, t_tw = table_passes(eng, vcf, rows, reps)
    t_us, t_uw = update_passes(eng, export, rows, table, reps)
    # K13's whole call on the same export, in the same run
    tabs = [CaddTable(eng.cadd_table_build(f(positions, eng.device)), eng) for f in (K13.snv_table, K13.indel_table)]

    def k13():
        got.pop("k13", None)
        got["k13"] = eng.cadd_update_rows(export, tabs[0], tabs[1], chromosome="chr22")

    t_k13 = timed(k13, reps)
    k13_out = got.pop("k13").counts["out_bytes"]
    t_cv, t_ce = events([lambda: vcf.clone(), lambda: export.clone()], reps)
    # the reference's loop, restated (tests/lof_common.py), over the first lines of both texts
    import lof_common as L
    n_s = min(int(a.host_sample), rows) // 400 * 400
    s_vcf = vcf[:n_s // EVERY * GROUP].cpu().numpy().tobytes()
    s_exp = export[:n_s // 8 * K13.GROUP].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    want, _, _ = L.ref_update(s_vcf, s_exp)
    host_s = time.perf_counter() - t0
    sample_t = eng.lof_table_build(s_vcf)
    assert eng.lof_update_rows(s_exp, sample_t).text.cpu().numpy().tobytes() == L.rows_text(want) and len(want) > 100
    bu, bk = stats(t_update), stats(t_k13)
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "vcf_bytes": vcf.numel(), "export_bytes": export.numel(),
        "table_rows": table.n_rows, "table_key_bytes": c["key_bytes"], "table_json_bytes": c["json_bytes"],
        "update_rows": r.n, "update_out_bytes": r.counts["out_bytes"], "not_annotated": r.counts["not_annotated"],
        "reps": reps,
        "lof_table_build_call_ms": stats(t_build), "lof_table_size_pass_ms": stats(t_ts),
        "lof_table_write_pass_ms": stats(t_tw),
        "lof_update_rows_call_ms": bu, "lof_update_size_pass_ms": stats(t_us), "lof_update_write_pass_ms": stats(t_uw),
        "cadd_update_rows_call_ms": bk, "cadd_update_out_bytes": k13_out,
        "clone_vcf_ms": stats(t_cv), "clone_export_ms": stats(t_ce),
        "vcf_GBps_size_pass_median": round(vcf.numel() / stats(t_ts)["median"] / 1e6, 1),
        "export_GBps_size_pass_median": round(export.numel() / stats(t_us)["median"] / 1e6, 1),
        "update_call_over_k13_call_median": round(bu["median"] / bk["median"], 3),
        "restatement_sample_rows": n_s, "restatement_s": round(host_s, 3),
        "restatement_lines_per_s": round(2 * n_s / host_s),
        "device_lines_per_s_both_calls_median": round(2 * rows / (stats(t_build)["median"] + bu["median"]) * 1e3),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

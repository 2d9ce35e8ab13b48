"""K13 probe: the CADD update rows rendered from an export of AnnotatedVDB.Variant
(rows/s, GB/s) beside the unchanged CADDUpdater.buffer_variants over a sample of the
same export, in the same run.

Workload, synthesised on the device (it is input, not part of the timing): one
chromosome's SNV table as CADD's whole-genome file has it (three rows per position,
32-byte lines), an indel table with a deletion at every 16th position, and an export of
``--rows`` lines in position order, ``22:PPPPPPPP:R:A:rsNNNNNNNNN<TAB>22:PPPPPPPP:R:A<TAB>\\N``
(47 bytes), every eighth line an indel; the export runs 10 % past the tables' span, so
about one row in eleven finds no match.  No line carries cadd_scores: the first
annotation pass over a chromosome, the case that costs most.

Timed: the whole Engine.cadd_update_rows call through its final sync (line count, size
pass, allocation of the output, write pass) by the host clock, and the two library
entries alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum
and maximum.  Algorithmic bytes: the export read once by each pass's front end, the
matched table lines' scores read twice, the rows written once, 29 bytes of row columns
written and read, the offsets written.  The baseline is buffer_variants over the first
``--host-sample`` records as dicts (what a database cursor delivers; building them is
not timed), K10 join on the same GPU included; its rows must equal K13's.

    python tools/cadd_update_probe.py [--rows 1e7] [--host-sample 1e6] [--out profiles/cadd_update_probe.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from annotatedvdb_amd import _native as N
from annotatedvdb_amd.cadd import CADDUpdater, CaddTable
from annotatedvdb_amd.engine import Engine

LO = 16_000_000  # 8-digit positions
HBM_TBPS = 8.0
ACGT = b"ACGT"


def _digits(dst, col, v, n):
    for k in range(n):
        dst[..., col + k] = ((v // 10 ** (n - 1 - k)) % 10 + 48).to(torch.uint8)


def _ref(p):
    return (p * 2654435761 >> 9) & 3


def _bytes(s, device):
    return torch.tensor(list(s), dtype=torch.uint8, device=device)


def snv_table(positions: int, device) -> torch.Tensor:
    """3 rows for each position: ``22<TAB>PPPPPPPP<TAB>R<TAB>A<TAB>d.dddddd<TAB>dd.ddd``."""
    acgt = _bytes(ACGT, device)
    out = torch.empty((positions, 3, 32), dtype=torch.uint8, device=device)
    out[:] = _bytes(b"22\t00000000\tA\tC\t0.000000\t00.000\n", device)
    chunk = 1 << 22
    for a in range(0, positions, chunk):
        p = torch.arange(LO + a, LO + min(positions, a + chunk), dtype=torch.int64, device=device)
        dst = out[a:a + p.numel()]
        _digits(dst, 3, p[:, None], 8)
        ref = _ref(p)
        dst[:, :, 12] = acgt[ref][:, None]
        for j in range(3):
            dst[:, j, 14] = acgt[(ref + 1 + j) & 3]
            h = ((p * 3 + j) * 6364136223846793005 >> 20) & 0xFFFFFFFF
            for k, col in enumerate((16, 18, 19, 20, 21, 22, 23, 25, 26, 28, 29, 30)):
                dst[:, j, col] = ((h >> (2 * k)) % 10 + 48).to(torch.uint8)
    return out.reshape(-1)


def indel_table(positions: int, device) -> torch.Tensor:
    """A deletion ``RT -> R`` at every 16th position: ``22<TAB>PPPPPPPP<TAB>RT<TAB>R<TAB>-d.dddddd<TAB>d.ddd``."""
    acgt = _bytes(ACGT, device)
    p = torch.arange(LO, LO + positions, 16, dtype=torch.int64, device=device)
    out = torch.empty((p.numel(), 33), dtype=torch.uint8, device=device)
    out[:] = _bytes(b"22\t00000000\tAT\tA\t-0.000000\t0.000\n", device)
    _digits(out, 3, p, 8)
    out[:, 12] = acgt[_ref(p)]
    out[:, 15] = acgt[_ref(p)]
    h = (p * 6364136223846793005 >> 20) & 0xFFFFFFFF
    for k, col in enumerate((18, 20, 21, 22, 23, 24, 25, 27, 29, 30, 31)):
        out[:, col] = ((h >> (2 * k)) % 10 + 48).to(torch.uint8)
    return out.reshape(-1)


SNV_LINE = b"22:00000000:A:C:rs000000000\t22:00000000:A:C\t\\N\n"      # 47 bytes
INDEL_LINE = b"22:00000000:AT:A:rs000000000\t22:00000000:AT:A\t\\N\n"  # 49 bytes
GROUP = 7 * len(SNV_LINE) + len(INDEL_LINE)


def export_text(rows: int, positions: int, device) -> torch.Tensor:
    """``rows`` lines (a multiple of 8) in groups of seven SNVs and one deletion, in position order."""
    assert rows % 8 == 0
    acgt = _bytes(ACGT, device)
    out = torch.empty((rows // 8, GROUP), dtype=torch.uint8, device=device)
    out[:] = _bytes(SNV_LINE * 7 + INDEL_LINE, device)
    span = positions + positions // 10
    chunk = 1 << 19
    for a in range(0, rows // 8, chunk):
        g = torch.arange(a, min(rows // 8, a + chunk), dtype=torch.int64, device=device)
        dst = out[a:a + g.numel()]
        for k in range(8):
            i = 8 * g + k
            at = k * len(SNV_LINE)
            h = (i * 6364136223846793005 >> 17) & 0x7FFFFFFF
            if k < 7:
                p = LO + i * span // rows
                ref = _ref(p)
                alt = acgt[(ref + 1 + h % 3) & 3]
                cols = ((3, 31), (12, 40), (14, 42), 18)
            else:
                p = LO + (i * span // rows) // 16 * 16 + 8 * (h % 2)  # a deletion of the table, or no row at all
                ref = _ref(p)
                alt = acgt[ref]
                cols = ((3, 32), (12, 41), (15, 44), 19)
            for c in cols[0]:
                _digits(dst, at + c, p, 8)
            for c in cols[1]:
                dst[:, at + c] = acgt[ref]
            for c in cols[2]:
                dst[:, at + c] = alt
            _digits(dst, at + cols[3], h % 1_000_000_000, 9)
    return out.reshape(-1)


def stats(ts):
    return {"median": round(float(np.median(ts)), 3), "min": round(float(min(ts)), 3), "max": round(float(max(ts)), 3)}


def passes(eng, text, n_lines, tabs, reps):
    """The two library entries alone, by device events: (size ms, write ms) lists."""
    import ctypes
    views = [t.cols.view() for t in tabs]
    shared = (ctypes.byref(views[0]), ctypes.byref(views[1]), b"chr22", 5)
    nb = text.numel()
    row_start = eng.empty(n_lines, torch.int64)
    pk_len, out_len, match = (eng.empty(n_lines, torch.int32) for _ in range(3))
    kind, flags = eng.empty(n_lines, torch.uint8), eng.empty(n_lines, torch.uint8)
    counts = eng.empty(N.CADDUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("cadd_update", N.size("avdb_cadd_update_workspace_size", nb, n_lines))
    out = row_off = None
    totals = eng.empty(2, torch.int64)
    ts, tw = [], []
    for r in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        eng._launch("avdb_cadd_update_size", text, nb, n_lines, *shared, N.EXIST_ALL_CONTIGS, N.CADDUPD_SKIP_EXISTING,
                    row_start, pk_len, kind, match, out_len, flags, counts, ws, ws.numel())
        e[1].record()
        if out is None:
            cnt = dict(zip(N.CADDUPD_COUNTS, counts.cpu().tolist()))
            out = eng.empty(cnt["out_bytes"], torch.uint8)
            row_off = eng.empty(cnt["rows"] + 1, torch.int64)
        e[2].record()
        eng._launch("avdb_cadd_update_write", text, nb, n_lines, cnt["rows"], *shared, row_start, pk_len, kind, match,
                    out_len, flags, out, out.numel(), row_off, totals, ws, ws.numel())
        e[3].record()
        torch.cuda.synchronize()
        if r:
            ts.append(e[0].elapsed_time(e[1]))
            tw.append(e[2].elapsed_time(e[3]))
    assert totals.cpu().tolist() == [cnt["out_bytes"], 0]
    return ts, tw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--positions", type=float, default=4e6)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/cadd_update_probe.json")
    a = ap.parse_args()
    rows, positions, reps = int(a.rows) // 8 * 8, int(a.positions), max(5, a.reps)
    eng = Engine(0)
    tabs = [CaddTable(eng.cadd_table_build(f(positions, eng.device)), eng) for f in (snv_table, indel_table)]
    assert all(t.counts["score_host"] == 0 and t.counts["bad"] == 0 for t in tabs)
    text = export_text(rows, positions, eng.device)
    torch.cuda.synchronize()
    got = {}

    def run():
        got.clear()  # (the output of the run before is freed first)
        got["rows"] = eng.cadd_update_rows(text, tabs[0], tabs[1], chromosome="chr22")

    run()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        ts.append((time.perf_counter() - t0) * 1e3)
    r = got["rows"]
    c = r.counts
    assert r.n == rows and c["host_rows"] == 0 and c["skipped"] == 0 and c["skipped_lines"] == 0
    assert min(c["snv"], c["indel"], c["not_matched"]) > rows // 40
    t_size, t_write = passes(eng, text, rows, tabs, reps)
    matched = c["snv"] + c["indel"]
    alg = 2 * text.numel() + 2 * 16 * matched + c["out_bytes"] + 2 * 29 * rows + 8 * (rows + 1)
    # the baseline: buffer_variants over the first records of the same export
    n_s = min(int(a.host_sample), rows) // 8 * 8
    sample = text[:n_s // 8 * GROUP].cpu().numpy().tobytes()
    recs = []
    for line in sample.decode().split("\n")[:-1]:
        pk, m, _ = line.split("\t")
        recs.append({"record_primary_key": pk, "metaseq_id": m, "cadd_scores": None})
    u = CADDUpdater(tabs[0], tabs[1], eng)
    u.set_chromosome("chr22")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u.buffer_variants(recs)
    host_s = time.perf_counter() - t0
    assert u.update_text() == r.text[:int(r.row_off[n_s])].cpu().numpy().tobytes()
    b = stats(ts)
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "text_bytes": text.numel(),
        "table_rows": [len(t) for t in tabs], "out_bytes": c["out_bytes"],
        "counts": {k: c[k] for k in ("snv", "indel", "not_matched", "skipped", "host_rows")}, "reps": reps,
        "call_ms": b, "call_ms_all": [round(t, 3) for t in ts],
        "call_rows_per_s": {k: round(rows / v * 1e3) for k, v in b.items()},
        "size_pass_ms": stats(t_size), "write_pass_ms": stats(t_write),
        "algorithmic_bytes": alg,
        "algorithmic_GBps_call_median": round(alg / b["median"] / 1e6, 2),
        "algorithmic_GBps_passes_median": round(alg / (stats(t_size)["median"] + stats(t_write)["median"]) / 1e6, 2),
        "share_of_8TBps_passes_median": round(alg / (stats(t_size)["median"] + stats(t_write)["median"]) / 1e6
                                              / (HBM_TBPS * 1e3), 4),
        "buffer_variants_sample_rows": n_s, "buffer_variants_s": round(host_s, 4),
        "buffer_variants_rows_per_s": round(n_s / host_s),
        "ratio_call_median_over_buffer_variants": round((rows / b["median"] * 1e3) / (n_s / host_s), 1),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

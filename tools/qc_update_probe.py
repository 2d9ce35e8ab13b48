"""K17 probe: the ADSP QC table (Engine.qc_table_build) and the update rows streamed from an
export (Engine.qc_update_rows), beside K16's two calls on K16's probe inputs, a torch.clone of each
text and the pure-Python restatement of the reference's loop over a sample, all in one run.

Workload, synthesised on the device (it is input, not part of the timing): the export of the K13
probe (tools/cadd_update_probe.py: ``--rows`` lines ``22:PPPPPPPP:R:A:rsNNNNNNNNN<TAB>22:PPPPPPPP:R:A<TAB>\\N``)
and a QC-like VCF of as many lines without sample columns, twelve INFO items a line,
``22<TAB>PPPPPPPP<TAB>.<TAB>R<TAB>A<TAB>QUAL<TAB>FILTER<TAB>AC=..;AF=..;...;culprit=MQ<TAB>GT:AD:DP``,
with the alleles of the export's row of the same number (seven in eight name an id the export holds)
and FILTER alternating between PASS and a tranche name.

Timed: each whole Engine call through its final sync by the host clock, and the library entries
alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/qc_update_probe.py [--rows 1e7] [--host-sample 1e6] [--out profiles/qc_update_probe.json]
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
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine

HEAD = b"22\t00000000\t.\tA\tC\t"
INFO = (b"AC=00;AF=0.00000;AN=16240;BaseQRankSum=-1.234;DP=123456;ExcessHet=3.0103;FS=0.000;MQ=60.00;QD=25.36;"
        b"SOR=1.609;VQSLOD=-12.34;culprit=MQ\tGT:AD:DP\n")
LINES = (HEAD + b"1234.56\tPASS\t" + INFO, HEAD + b"98.7\tVQSRTrancheSNP99.80to100.00\t" + INFO)
GROUP = len(LINES[0]) + len(LINES[1])
VERSION = "17K"


def vcf_text(rows: int, positions: int, device) -> torch.Tensor:
    """``rows`` lines (a multiple of 2); line j carries the position and alleles of the export's row
    j by its SNV formula, and digits of its own in AC and AF."""
    assert rows % 2 == 0
    acgt = K13._bytes(K13.ACGT, device)
    out = torch.empty((rows // 2, GROUP), dtype=torch.uint8, device=device)
    out[:] = K13._bytes(LINES[0] + LINES[1], device)
    span = positions + positions // 10
    chunk = 1 << 20
    for a in range(0, rows // 2, chunk):
        g = torch.arange(a, min(rows // 2, a + chunk), dtype=torch.int64, device=device)
        dst = out[a:a + g.numel()]
        for k in range(2):
            i = 2 * g + k
            at = k * len(LINES[0])
            info = at + len(LINES[k]) - len(INFO)
            h = (i * 6364136223846793005 >> 17) & 0x7FFFFFFF
            p = K13.LO + i * span // rows
            ref = K13._ref(p)
            K13._digits(dst, at + 3, p, 8)
            dst[:, at + 14] = acgt[ref]
            dst[:, at + 16] = acgt[(ref + 1 + h % 3) & 3]
            K13._digits(dst, info + 3, h % 100, 2)        # AC
            K13._digits(dst, info + 11, h % 99991, 5)     # AF's fraction
    return out.reshape(-1)


def table_passes(eng, text, n_lines, release, reps):
    nb = text.numel()
    ents = [eng.empty(n_lines, torch.int64)] + [eng.empty(n_lines, torch.int32) for _ in range(3)] + \
        [eng.empty(n_lines, torch.uint8)]
    counts = eng.empty(N.QC_N_COUNTS, torch.int64)
    ws = eng.scratch("qc_table", N.size("avdb_qc_table_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_qc_table_size", text, nb, n_lines, release, len(release), *ents, counts, ws,  # noqa: E731
                               ws.numel())
    size()
    c = dict(zip(N.QC_COUNTS, counts.cpu().tolist()))
    n = c["rows"]
    keys, js = eng.empty(max(8, c["key_bytes"]), torch.uint8), eng.empty(max(8, c["json_bytes"]), torch.uint8)
    key_off, json_off, line_start = (eng.empty(n + 1, torch.int64) for _ in range(3))
    json_len, flags, totals = eng.empty(n + 1, torch.int32), eng.empty(n + 1, torch.uint8), eng.empty(4, torch.int64)
    write = lambda: eng._launch("avdb_qc_table_write", text, nb, n_lines, c["entries"], n, release, len(release),  # noqa: E731
                                *ents, keys, c["key_bytes"], key_off, js, c["json_bytes"], json_off, json_len,
                                line_start, flags, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [c["key_bytes"], c["json_bytes"], n, 0]
    return t


def update_passes(eng, text, n_lines, table, reps):
    nb = text.numel()
    view = table.view()
    vp = ctypes.byref(view)
    row_start = eng.empty(n_lines, torch.int64)
    pk_len, match, out_len = (eng.empty(n_lines, torch.int32) for _ in range(3))
    flags, counts = eng.empty(n_lines, torch.uint8), eng.empty(N.QCUPD_N_COUNTS, torch.int64)
    ws = eng.scratch("qc_update", N.size("avdb_qc_update_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_qc_update_size", text, nb, n_lines, vp, N.EXIST_ALL_CONTIGS, 0, row_start,  # noqa: E731
                               pk_len, match, out_len, flags, counts, ws, ws.numel())
    size()
    c = dict(zip(N.QCUPD_COUNTS, counts.cpu().tolist()))
    out, row_off, totals = eng.empty(max(8, c["out_bytes"]), torch.uint8), eng.empty(c["rows"] + 1, torch.int64), \
        eng.empty(2, torch.int64)
    write = lambda: eng._launch("avdb_qc_update_write", text, nb, n_lines, c["rows"], vp, row_start, pk_len,  # noqa: E731
                                match, out_len, flags, out, c["out_bytes"], row_off, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [c["out_bytes"], 0]
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--positions", type=float, default=4e6)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/qc_update_probe.json")
    a = ap.parse_args()
    rows, positions, reps = int(a.rows) // 400 * 400, int(a.positions), max(5, a.reps)
    eng = Engine(0)
    export = K13.export_text(rows, positions, eng.device)
    vcf = vcf_text(rows, positions, eng.device)
    torch.cuda.synchronize()
    stats, timed, events = K13.stats, K16.timed, K16.events
    got = {}

    def build():
        got.pop("table", None)
        got["table"] = eng.qc_table_build(vcf, VERSION)

    t_build = timed(build, reps)
    table = got["table"]
    c = table.counts
    assert c["host_lines"] == 0 and c["entries"] == rows == table.n_rows and c["pass"] == rows // 2

    def update():
        got.pop("rows", None)
        got["rows"] = eng.qc_update_rows(export, table)

    t_update = timed(update, reps)
    r = got["rows"]
    assert r.counts["rows"] + r.counts["not_in_vcf"] == rows and r.n > rows // 2 and r.counts["host_rows"] == 0
    t_ts, t_tw = table_passes(eng, vcf, rows, table.release, reps)
    t_us, t_uw = update_passes(eng, export, rows, table, reps)
    t_cv, t_ce = events([lambda: vcf.clone(), lambda: export.clone()], reps)
    out_bytes, json_bytes, key_bytes, n_upd, n_miss = r.counts["out_bytes"], c["json_bytes"], c["key_bytes"], r.n, \
        r.counts["not_in_vcf"]
    # the reference's loop, restated (tests/qc_common.py), over the first lines of both texts
    import qc_common as Q
    n_s = min(int(a.host_sample), rows) // 400 * 400
    s_vcf = vcf[:n_s // 2 * GROUP].cpu().numpy().tobytes()
    s_exp = export[:n_s // 8 * K13.GROUP].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    want, _, _ = Q.ref_update(s_vcf, s_exp, VERSION.lower())
    host_s = time.perf_counter() - t0
    sample_t = eng.qc_table_build(s_vcf, VERSION)
    assert eng.qc_update_rows(s_exp, sample_t).text.cpu().numpy().tobytes() == Q.rows_text(want) and len(want) > 100
    vcf_bytes = vcf.numel()
    del got["table"], got["rows"], table, r, sample_t, vcf
    torch.cuda.empty_cache()
    # K16's two calls on K16's probe inputs, in the same run
    lof_vcf = K16.vcf_text(rows, positions, eng.device)

    def lof_build():
        got.pop("lof", None)
        got["lof"] = eng.lof_table_build(lof_vcf)

    t_lb = timed(lof_build, reps)

    def lof_update():
        got.pop("lof_rows", None)
        got["lof_rows"] = eng.lof_update_rows(export, got["lof"])

    t_lu = timed(lof_update, reps)
    bb, bu = stats(t_build), stats(t_update)
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "vcf_bytes": vcf_bytes, "export_bytes": export.numel(),
        "info_items_per_line": 12, "table_rows": rows, "table_key_bytes": key_bytes, "table_json_bytes": json_bytes,
        "update_rows": n_upd, "update_out_bytes": out_bytes, "not_in_vcf": n_miss, "reps": reps,
        "qc_table_build_call_ms": bb, "qc_table_size_pass_ms": stats(t_ts), "qc_table_write_pass_ms": stats(t_tw),
        "qc_update_rows_call_ms": bu, "qc_update_size_pass_ms": stats(t_us), "qc_update_write_pass_ms": stats(t_uw),
        "lof_table_build_call_ms": stats(t_lb), "lof_update_rows_call_ms": stats(t_lu), "lof_vcf_bytes": lof_vcf.numel(),
        "clone_vcf_ms": stats(t_cv), "clone_export_ms": stats(t_ce),
        "vcf_GBps_size_pass_median": round(vcf_bytes / stats(t_ts)["median"] / 1e6, 1),
        "json_GBps_write_pass_median": round((json_bytes + key_bytes) / stats(t_tw)["median"] / 1e6, 1),
        "export_GBps_size_pass_median": round(export.numel() / stats(t_us)["median"] / 1e6, 1),
        "out_GBps_update_write_pass_median": round(out_bytes / stats(t_uw)["median"] / 1e6, 1),
        "restatement_sample_rows": n_s, "restatement_s": round(host_s, 3),
        "restatement_lines_per_s": round(2 * n_s / host_s),
        "device_lines_per_s_both_calls_median": round(2 * rows / (bb["median"] + bu["median"]) * 1e3),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""K14 probe: the VCF files of an export of AnnotatedVDB.Variant written on the GPU
(rows/s, GB/s), beside K13's cadd_update_rows over the same text and the reference
loop's restatement over a sample of it, in the same run.

Workload, synthesised on the device (it is input, not part of the timing): K13's probe
export (tools/cadd_update_probe.py) — ``--rows`` lines of the dbSNP mix in position order,
``22:PPPPPPPP:R:A:rsNNNNNNNNN<TAB>22:PPPPPPPP:R:A<TAB>\\N`` (47 bytes), every eighth line
a deletion — whose third column reads as a NULL row_algorithm_id here; every 64th
line's alt becomes ``N``, so the invalid stream is exercised too.
No key repeats: the normal case, in which no row text comes to the host.

Timed: the whole Engine.export_vcf call through its final sync (line count, size pass,
the sort that looks for repeated keys, allocation of the outputs, the two write passes)
by the host clock, and by device events the size entry, the two write entries and the
torch.sort of the key hashes alone.  K13's whole call on the same text and tables, timed
the same way, alternating with K14's.  One warm-up, then ``--reps`` repeats: median,
minimum and maximum.  Algorithmic bytes: the export read once by each pass's front end,
the rows written once, 29 bytes of valid-row columns (16 of invalid-row columns) written
and read, the offsets written, the hashes read, sorted (keys and indices, written once)
and compared.  The baseline is the restatement of the reference's loop with its dict
(tests/export_vcf_common.ref_export) over the first ``--host-sample`` lines; its files
must equal K14's.

    python tools/export_vcf_probe.py [--rows 1e7] [--host-sample 1e6] [--out profiles/export_vcf_probe.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
sys.path.insert(0, "tests")
import torch

import cadd_update_probe as K13
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.cadd import CaddTable
from annotatedvdb_amd.engine import Engine

HBM_TBPS = 8.0
stats = K13.stats


def mark_invalid(text: torch.Tensor, rows: int) -> int:
    """The alt of every 64th line becomes N, in the key and in the metaseq id alike; returns how many."""
    lines = text.view(rows // 8, K13.GROUP)
    for col in (14, 42):  # (the first line of a group is an SNV line)
        lines[::8, col] = ord("N")
    return (rows // 8 + 7) // 8


def passes(eng, text, n_lines, reps):
    """The library entries alone and the candidate sort, by device events: (size, write VCF, write invalid, sort) ms lists."""
    nb = text.numel()
    row_start, pk_hash, inv_start = (eng.empty(n_lines, torch.int64) for _ in range(3))
    pk_len, ms_len, out_len, inv_pk_len, inv_out_len = (eng.empty(n_lines, torch.int32) for _ in range(5))
    flags = eng.empty(n_lines, torch.uint8)
    counts = eng.empty(N.EXPVCF_N_COUNTS, torch.int64)
    ws = eng.scratch("export_vcf", N.size("avdb_export_vcf_workspace_size", nb, n_lines))
    bufs = None
    out = {"size": [], "write_vcf": [], "write_invalid": [], "sort": []}
    for r in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        e[0].record()
        eng._launch("avdb_export_vcf_size", text, nb, n_lines, N.EXIST_ALL_CONTIGS, row_start, pk_len, ms_len, out_len,
                    flags, pk_hash, inv_start, inv_pk_len, inv_out_len, counts, ws, ws.numel())
        e[1].record()
        if bufs is None:
            cnt = dict(zip(N.EXPVCF_COUNTS, counts.cpu().tolist()))
            bufs = (eng.empty(cnt["vcf_bytes"], torch.uint8), eng.empty(cnt["valid"] + 1, torch.int64),
                    eng.empty(max(1, cnt["invalid_bytes"]), torch.uint8), eng.empty(cnt["invalid"] + 1, torch.int64),
                    eng.empty(2, torch.int64), eng.empty(2, torch.int64))
        e[2].record()
        eng._launch("avdb_export_vcf_write", text, nb, n_lines, N.EXPVCF_STREAM_VCF, cnt["valid"], row_start, pk_len,
                    ms_len, out_len, flags, bufs[0], cnt["vcf_bytes"], bufs[1], bufs[4], ws, ws.numel())
        e[3].record()
        e[4].record()
        eng._launch("avdb_export_vcf_write", text, nb, n_lines, N.EXPVCF_STREAM_INVALID, cnt["invalid"], inv_start,
                    inv_pk_len, None, inv_out_len, None, bufs[2], cnt["invalid_bytes"], bufs[3], bufs[5], ws, ws.numel())
        e[5].record()
        e[6].record()
        skey, _ = torch.sort(pk_hash[:cnt["valid"]])
        same = (skey[1:] == skey[:-1]).sum()
        e[7].record()
        torch.cuda.synchronize()
        if r:
            for name, k in (("size", 0), ("write_vcf", 2), ("write_invalid", 4), ("sort", 6)):
                out[name].append(e[k].elapsed_time(e[k + 1]))
    assert bufs[4].cpu().tolist() == [cnt["vcf_bytes"], 0] and bufs[5].cpu().tolist() == [cnt["invalid_bytes"], 0]
    assert int(same) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--positions", type=float, default=4e6)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/export_vcf_probe.json")
    a = ap.parse_args()
    rows, positions, reps = int(a.rows) // 8 * 8, int(a.positions), max(5, a.reps)
    eng = Engine(0)
    tabs = [CaddTable(eng.cadd_table_build(f(positions, eng.device)), eng) for f in (K13.snv_table, K13.indel_table)]
    text = K13.export_text(rows, positions, eng.device)
    n_invalid = mark_invalid(text, rows)
    torch.cuda.synchronize()
    got = {}

    def run_k14():
        got.pop("k14", None)  # (the output of the run before is freed first)
        got["k14"] = eng.export_vcf(text)

    def run_k13():
        got.pop("k13", None)
        got["k13"] = eng.cadd_update_rows(text, tabs[0], tabs[1], chromosome="chr22")

    run_k14()
    run_k13()
    t14, t13 = [], []
    for _ in range(reps):  # alternating, so that both see the same machine
        for run, ts in ((run_k14, t14), (run_k13, t13)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
    r = got["k14"]
    c = r.counts
    assert c["valid"] + c["invalid"] == rows and c["invalid"] == n_invalid and c["dropped"] == 0
    assert r.n_files == c["valid"] // 10_000_000 + 1
    assert got["k13"].n == rows
    got.pop("k13")
    p = passes(eng, text, rows, reps)
    nv, ni = c["valid"], c["invalid"]
    alg = 2 * text.numel() + c["vcf_bytes"] + c["invalid_bytes"] + 2 * 29 * nv + 2 * 16 * ni + 8 * (nv + 1) + \
        8 * (ni + 1) + 8 * nv + 2 * 16 * nv
    # the baseline: the restatement of the reference's loop over the first lines of the same export
    import export_vcf_common as X
    n_s = min(int(a.host_sample), rows) // 8 * 8
    sample = text[:n_s // 8 * K13.GROUP].cpu().numpy().tobytes()
    t0 = time.perf_counter()
    files, invalid, ctr = X.ref_export(sample)
    host_s = time.perf_counter() - t0
    vcf = r.vcf_text[:int(r.vcf_row_off[ctr["valid"]])].cpu().numpy().tobytes()
    assert files == [vcf] and invalid == r.invalid_text[:int(r.invalid_row_off[ctr["invalid"]])].cpu().numpy().tobytes()
    b14, b13 = stats(t14), stats(t13)
    med = {k: stats(v)["median"] for k, v in p.items()}
    entries = med["size"] + med["write_vcf"] + med["write_invalid"]
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "text_bytes": text.numel(),
        "counts": {k: c[k] for k in ("valid", "invalid", "dropped", "vcf_bytes", "invalid_bytes")}, "n_files": r.n_files,
        "reps": reps,
        "call_ms": b14, "call_ms_all": [round(t, 3) for t in t14],
        "call_rows_per_s": {k: round(rows / v * 1e3) for k, v in b14.items()},
        "size_pass_ms": stats(p["size"]), "write_vcf_ms": stats(p["write_vcf"]),
        "write_invalid_ms": stats(p["write_invalid"]), "candidate_sort_ms": stats(p["sort"]),
        "algorithmic_bytes": alg,
        "algorithmic_GBps_call_median": round(alg / b14["median"] / 1e6, 2),
        "algorithmic_GBps_entries_median": round(alg / entries / 1e6, 2),
        "share_of_8TBps_entries_median": round(alg / entries / 1e6 / (HBM_TBPS * 1e3), 4),
        "k13_call_ms": b13, "k13_call_ms_all": [round(t, 3) for t in t13],
        "call_ns_per_input_byte": {"k14": round(b14["median"] * 1e6 / text.numel(), 5),
                                   "k13": round(b13["median"] * 1e6 / text.numel(), 5)},
        "ratio_k14_over_k13_call_median": round(b14["median"] / b13["median"], 3),
        "ratio_k14_entries_over_k13_call_median": round(entries / b13["median"], 3),
        "host_loop_sample_rows": n_s, "host_loop_s": round(host_s, 4), "host_loop_rows_per_s": round(n_s / host_s),
        "ratio_call_median_over_host_loop": round((rows / b14["median"] * 1e3) / (n_s / host_s), 1),
    }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""K15 probe: a whole-genome VCF split by chromosome on the GPU (lines/s, GB/s), beside a
plain device copy of the same bytes and the reference loop's restatement over a sample
of the text, in the same run.

Workload, synthesised on the device (it is input, not part of the timing): ``--rows``
dbSNP-like lines of 105 bytes,
``NC_0000CC.VV<TAB>PPPPPPPPP<TAB>rsNNNNNNNNN<TAB>A<TAB>C<TAB>.<TAB>.<TAB>RS=NNNNNNNNN;dbSNPBuildID=155;SSR=0;VC=SNV;GNO;FREQ=1000G:0.9``
with the RefSeq accessions of chr1..22, X and Y as CHROM and the chromosome map of those 24
accessions: (a) sorted, each contig one run of lines, as dbSNP ships its file; (b) the
contigs interleaved line by line, the worst case for the write pass (every wave holds 24
streams).

Timed: the whole Engine.split_vcf call through its final sync (line count, size pass,
allocation of the blob, write pass) by the host clock, and by device events the size
entry and the write entry alone; a ``torch.clone`` of the text, the ceiling the write pass
is read against; (a), (b) and the clone alternate.  One warm-up, then ``--reps`` repeats:
median, minimum and maximum.  Algorithmic bytes: the text read by the size pass and again
by the write pass and written once, 3 x the text bytes (the 13 bytes of per-line arrays
written and read again are left out).  The baseline is a restatement of the reference's
loop (decode, rstrip, split, dict lookup, print to 25 open files) over the first
``--host-sample`` lines of the sorted text, without the gzip read the reference also pays;
its files must equal the heads of K15's streams.

    python tools/split_vcf_probe.py [--rows 1e7] [--host-sample 1e6] [--out profiles/split_vcf_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, ".")
import torch

from annotatedvdb_amd import _native as N
from annotatedvdb_amd.chromosomes import CHROM_NAMES
from annotatedvdb_amd.engine import ChromMap, Engine

ACCESSIONS = ["NC_0000%02d.%02d" % (c, v) for c, v in zip(range(1, 25), (11, 12, 12, 12, 10, 12, 14, 11, 12, 11, 10, 12,
                                                                        11, 9, 10, 10, 11, 10, 10, 11, 9, 11, 11, 10))]
TEMPLATE = b"NC_000000.00\t000000000\trs000000000\tA\tC\t.\t.\tRS=000000000;dbSNPBuildID=155;SSR=0;VC=SNV;GNO;FREQ=1000G:0.9\n"
WIDTH = len(TEMPLATE)
DIGITS = 9
NUMBER_AT = (13, 25, 46)  # POS, the rs number, RS=


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def vcf_text(rows: int, interleaved: bool, device) -> torch.Tensor:
    """``rows`` lines of TEMPLATE with the accession of the line's contig and the line's number in the three number fields."""
    acc = torch.tensor([list(a.encode()) for a in ACCESSIONS], dtype=torch.uint8, device=device)
    text = torch.tensor(list(TEMPLATE), dtype=torch.uint8, device=device).repeat(rows, 1)
    row = torch.arange(rows, device=device)
    contig = row % 24 if interleaved else torch.div(row * 24, rows, rounding_mode="floor")
    text[:, :12] = acc[contig]
    for k in range(DIGITS):
        d = (torch.div(row, 10 ** (DIGITS - 1 - k), rounding_mode="floor") % 10 + 48).to(torch.uint8)
        for at in NUMBER_AT:
            text[:, at + k] = d
    return text.view(-1)


def passes(eng, cm, text, n_lines, reps):
    """The two library entries alone, by device events: (size, write) ms lists."""
    nb = text.numel()
    code = eng.empty(n_lines, torch.uint8)
    line_start = eng.empty(n_lines, torch.int64)
    out_len = eng.empty(n_lines, torch.int32)
    counts = eng.empty(N.SPLIT_N_COUNTS, torch.int64)
    ws = eng.scratch("split_vcf", N.size("avdb_vcf_split_workspace_size", nb, n_lines))
    blob = eng.empty(nb, torch.uint8)
    stream_off = eng.empty(27, torch.int64)
    totals = eng.empty(2, torch.int64)
    out = {"size": [], "write": []}
    for r in range(reps + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        eng._launch("avdb_vcf_split_size", text, nb, n_lines, cm.handle, code, line_start, out_len, counts, ws, ws.numel())
        e[1].record()
        eng._launch("avdb_vcf_split_write", text, nb, n_lines, code, line_start, out_len, blob, nb, stream_off, None,
                    totals, ws, ws.numel())
        e[2].record()
        torch.cuda.synchronize()
        if r:
            out["size"].append(e[0].elapsed_time(e[1]))
            out["write"].append(e[1].elapsed_time(e[2]))
    assert totals.cpu().tolist() == [nb, 0]
    return out


def host_loop(sample: bytes, mapping, directory):
    """split_vcf_by_chr.py's run() restated (no gzip, no warnings): seconds, and the files' bytes without their header."""
    fh = {c: open(os.path.join(directory, "chr%s.vcf" % c), "w") for c in CHROM_NAMES}
    lines = sample.split(b"\n")[:-1]
    t0 = time.perf_counter()
    for line in lines:
        line = line.decode("utf-8").rstrip()
        if line.startswith("#"):
            continue
        values = line.split("\t")
        print(line, file=fh[mapping[values[0]]])
    for f in fh.values():
        f.close()
    secs = time.perf_counter() - t0
    files = {}
    for c in CHROM_NAMES:
        with open(os.path.join(directory, "chr%s.vcf" % c), "rb") as f:
            files[c] = f.read()
    return secs, files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e7)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="profiles/split_vcf_probe.json")
    a = ap.parse_args()
    rows, reps = int(a.rows), max(5, a.reps)
    eng = Engine(0)
    mapping = {acc: CHROM_NAMES[i] for i, acc in enumerate(ACCESSIONS)}
    cm = ChromMap.for_split(eng, mapping)
    texts = {"sorted": vcf_text(rows, False, eng.device), "interleaved": vcf_text(rows, True, eng.device)}
    nb = texts["sorted"].numel()
    torch.cuda.synchronize()
    got = {}

    def run_split(name):
        got.pop(name, None)  # (the output of the run before is freed first)
        got[name] = eng.split_vcf(texts[name], cm)

    def run_clone(name="clone"):
        got.pop(name, None)
        got[name] = texts["sorted"].clone()
        torch.cuda.synchronize()

    runs = (("sorted", lambda: run_split("sorted")), ("interleaved", lambda: run_split("interleaved")), ("clone", run_clone))
    for _, run in runs:
        run()
    ms = {name: [] for name, _ in runs}
    for _ in range(reps):  # alternating, so that all see the same machine
        for name, run in runs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    got.pop("clone")
    for name in ("sorted", "interleaved"):
        r = got[name]
        assert r.text.numel() == nb and r.first_other is None and r.counts["host_lines"] == 0
        assert sum(r.counts["lines"][:24]) == rows and min(r.counts["lines"][:24]) >= rows // 24
    # (lines are of one width: a stream's bytes are its lines; line 0 of either text opens stream 0)
    assert got["sorted"].stream_off[1] - got["sorted"].stream_off[0] == got["sorted"].counts["lines"][0] * WIDTH
    assert torch.equal(got["interleaved"].stream(0)[:WIDTH], texts["interleaved"][:WIDTH])
    p = {name: passes(eng, cm, texts[name], rows, reps) for name in ("sorted", "interleaved")}
    # the baseline: the reference's loop restated, over the first lines of the sorted text
    n_s = min(int(a.host_sample), rows)
    sample = texts["sorted"][:n_s * WIDTH].cpu().numpy().tobytes()
    with tempfile.TemporaryDirectory() as d:
        host_s, files = host_loop(sample, mapping, d)
    for c, label in enumerate(CHROM_NAMES):
        assert files[label] == got["sorted"].stream(c)[:len(files[label])].cpu().numpy().tobytes(), label
    b = {name: stats(v) for name, v in ms.items()}
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "line_bytes": WIDTH, "text_bytes": nb, "reps": reps,
        "algorithmic_bytes": 3 * nb,
        "clone_ms": b["clone"], "clone_GBps_read_plus_write_median": round(2 * nb / b["clone"]["median"] / 1e6, 1),
        "host_loop_sample_rows": n_s, "host_loop_s": round(host_s, 4), "host_loop_rows_per_s": round(n_s / host_s),
        "host_loop_caveat": "the restated loop reads its lines from memory: the reference also pays a gzip read per line",
    }
    for name in ("sorted", "interleaved"):
        size, write = stats(p[name]["size"]), stats(p[name]["write"])
        res[name] = {
            "call_ms": b[name], "call_ms_all": [round(t, 3) for t in ms[name]],
            "call_rows_per_s_median": round(rows / b[name]["median"] * 1e3),
            "size_pass_ms": size, "write_pass_ms": write,
            "algorithmic_GBps_call_median": round(3 * nb / b[name]["median"] / 1e6, 1),
            "algorithmic_GBps_entries_median": round(3 * nb / (size["median"] + write["median"]) / 1e6, 1),
            "write_pass_over_clone_median": round(write["median"] / b["clone"]["median"], 2),
            "ratio_call_median_over_host_loop": round((rows / b[name]["median"] * 1e3) / (n_s / host_s), 1),
        }
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

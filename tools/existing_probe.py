"""K12 probe: the --skipExisting key set built from an export of AnnotatedVDB.Variant
(rows/s, GB/s of text) and K6's table build over its keys, beside the host parse of
ExistingVariants.from_tsv on a sample of the same rows.

Workload: an export synthesised on the device (it is input, not part of the timing):
dbSNP-like rows ``CC:PPPPPPPPP:R:A<TAB>CC:PPPPPPPPP:R:A:rsNNNNNNNNN<TAB><13-level bin
path>``, 155 bytes a line, under a header line.  About 350 bytes of device memory per
row hold the text, the blobs, the offsets and the workspace.

The build time is the whole Engine.existing_table_build call through its final sync
(line count, size pass, allocation of the blobs, write pass), by the host clock; the
key-set time is Engine.keyset_build over the built keys, by device events.  One
warm-up, then ``--reps`` repeats: median, minimum and maximum.  Algorithmic bytes: the
text read once, plus the three blobs and their offsets written.

    python tools/existing_probe.py [--rows 2e7] [--host-sample 1e6] [--out profiles/existing_probe.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from annotatedvdb_amd.engine import Engine

HEADER = b"metaseq_id\trecord_primary_key\tbin_index\n"
B_DIGITS = (1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4)  # digits of the bin number at levels 1..13
HBM_TBPS = 8.0


def template():
    """(one line as bytes with '0' where digits go, {field: [columns]})"""
    key = b"00:000000000:A:C"
    line = key + b"\t" + key + b":rs000000000\tchr00"
    cols = {"chrom": [0, 17, len(line) - 2], "pos": [3, 20], "ref": [13, 30], "alt": [15, 32], "rs": [36], "bins": []}
    for lv, d in enumerate(B_DIGITS, 1):
        line += b".L%d.B" % lv
        cols["bins"].append((len(line), d))
        line += b"0" * d
    return line + b"\n", cols


def export_text(rows: int, device) -> torch.Tensor:
    line, cols = template()
    L = len(line)
    out = torch.empty(len(HEADER) + rows * L, dtype=torch.uint8, device=device)
    out[:len(HEADER)] = torch.tensor(list(HEADER), dtype=torch.uint8, device=device)
    body = out[len(HEADER):].view(rows, L)
    body[:] = torch.tensor(list(line), dtype=torch.uint8, device=device)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)

    def digits(dst, col, v, n):
        for k in range(n):
            dst[:, col + k] = ((v // 10 ** (n - 1 - k)) % 10 + 48).to(torch.uint8)

    chunk = 1 << 22
    for a in range(0, rows, chunk):
        i = torch.arange(a, min(rows, a + chunk), dtype=torch.int64, device=device)
        dst = body[a:a + i.numel()]
        chrom = 10 + i * 13 // rows  # sorted by contig, then position, as an export by primary key is
        pos = 100_000_000 + (i * 37) % 140_000_000
        h = (i * 6364136223846793005 >> 17) & 0x7FFFFFFF
        for c in cols["chrom"]:
            digits(dst, c, chrom, 2)
        for c in cols["pos"]:
            digits(dst, c, pos, 9)
        for c in cols["ref"]:
            dst[:, c] = acgt[h & 3]
        for c in cols["alt"]:
            dst[:, c] = acgt[(h + 1 + (h >> 2) % 3) & 3]
        digits(dst, cols["rs"][0], h % 1_000_000_000, 9)
        for lv, (c, d) in enumerate(cols["bins"], 1):
            lo = 10 ** (d - 1) if d > 1 else 1
            digits(dst, c, lo + (pos >> (14 - lv)) % (9 * lo if d > 1 else 9), d)
    return out


def stats(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


def host_parse(path: str):
    """ExistingVariants.from_tsv's loop, without the constructor."""
    t0 = time.perf_counter()
    entries, pks = [], []
    with open(path) as fh:
        for line in fh:
            f = line.rstrip("\n").split("\t")
            if len(f) < 3 or f[0] == "metaseq_id":
                continue
            entries.append((f[0], [{"primary_key": f[1], "bin_index": f[2]}]))
            pks.append(f[1])
    return time.perf_counter() - t0, len(entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=2e7)
    ap.add_argument("--host-sample", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/existing_probe.json")
    a = ap.parse_args()
    rows, reps = int(a.rows), max(5, a.reps)
    eng = Engine(0)
    text = export_text(rows, eng.device)
    torch.cuda.synchronize()
    built = {}

    def build():
        built.clear()  # (the blobs of the run before are freed first)
        built["cols"] = eng.existing_table_build(text)

    build()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        build()
        ts.append((time.perf_counter() - t0) * 1e3)
    c = built["cols"]
    assert c.n_rows == rows and c.counts["frag_host"] == 0 and c.counts["noncanon"] == 0 and c.counts["skipped"] == 1
    line, _ = template()
    k0 = int(c.key_off[1])
    assert c.keys[:k0].cpu().numpy().tobytes() == text[len(HEADER):len(HEADER) + k0].cpu().numpy().tobytes()
    tk = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        table = eng.keyset_build(c.keys, c.key_off)
        e1.record()
        torch.cuda.synchronize()
        del table
        if r:
            tk.append(e0.elapsed_time(e1))
    alg = text.numel() + c.counts["key_bytes"] + c.counts["pk_bytes"] + c.counts["frag_bytes"] + 3 * 8 * (rows + 1)
    n_s = min(int(a.host_sample), rows, 1_000_000)
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "sample.tsv")
        with open(p, "wb") as fh:
            fh.write(text[:len(HEADER) + n_s * len(line)].cpu().numpy().tobytes())
        host_s, host_rows = host_parse(p)
    assert host_rows == n_s
    b = stats(ts)
    res = {
        "device": torch.cuda.get_device_name(0), "rows": rows, "line_bytes": len(line), "text_bytes": text.numel(),
        "reps": reps, "build_ms": {k: round(v, 3) for k, v in b.items()}, "build_ms_all": [round(t, 3) for t in ts],
        "build_rows_per_s": {k: round(rows / v * 1e3) for k, v in b.items()},
        "build_text_GBps": {k: round(text.numel() / v / 1e6, 2) for k, v in b.items()},
        "algorithmic_bytes": alg,
        "algorithmic_GBps_median": round(alg / b["median"] / 1e6, 2),
        "share_of_8TBps_median": round(alg / b["median"] / 1e6 / (HBM_TBPS * 1e3), 4),
        "keyset_build_ms": {k: round(v, 3) for k, v in stats(tk).items()},
        "keyset_build_keys_per_s_median": round(rows / float(np.median(tk)) * 1e3),
        "host_parse_sample_rows": n_s, "host_parse_s": round(host_s, 4), "host_parse_rows_per_s": round(n_s / host_s),
    }
    out = json.dumps(res)
    print(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

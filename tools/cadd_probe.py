"""K10 probe: CADD table build (ms, GB/s of slab text) and allele join (ms, variants/s)
on chr22-sized synthetic inputs, with HIP events.

Workload: the C1 records (synth.np_c1: 1.1 M position-sorted chr22 variants, 88 %
SNVs) against an SNV table of 3 rows per position over the same span, as CADD's
whole-genome SNV file has (every position, its reference base against the three
others; 32-byte lines, so the full span is 3.3 GB of text).  The indel records of
C1 find an empty indel table.  The table text is generated on the device (it is
input, not part of the timing).

The build time is the whole Engine.cadd_table_build call: line count, the kernels,
and the two host syncs around them.  The last figure is the reference-structured
host loop (cadd_updater.py:187-221 without the database: a dict of position ->
rows, the same membership test, float() of the two scores) over a sample of the
same variants, its dict holding only the positions that sample asks for.  pysam
is not installed here, so the reference's real cost — one tabix seek and
decompress per variant — is NOT in that figure; it is a floor for the host side.

    python tools/cadd_probe.py [--positions N] [--variants N] [--host-sample N]
"""
import argparse
import json
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from annotatedvdb_amd import _native as N
from annotatedvdb_amd import synth
from annotatedvdb_amd.cadd import CaddTable
from annotatedvdb_amd.engine import Engine, RecordBatch

LINE = 32  # "22\tPPPPPPPP\tR\tA\td.dddddd\tdd.ddd\n"


def table_text(lo: int, positions: int, device) -> torch.Tensor:
    """3 rows for each of ``positions`` positions from ``lo`` (8-digit positions)."""
    assert 10_000_000 <= lo and lo + positions <= 100_000_000
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)
    out = torch.empty((positions, 3, LINE), dtype=torch.uint8, device=device)
    out[:, :, 0:3] = torch.tensor(list(b"22\t"), dtype=torch.uint8, device=device)
    for k in (11, 13, 15, 24):
        out[:, :, k] = 9    # tab
    out[:, :, 17], out[:, :, 27], out[:, :, 31] = 46, 46, 10  # '.', '.', newline
    chunk = 1 << 22
    for a in range(0, positions, chunk):
        p = torch.arange(lo + a, lo + min(positions, a + chunk), dtype=torch.int64, device=device)
        for k in range(8):
            out[a:a + p.numel(), :, 3 + k] = ((p // 10 ** (7 - k)) % 10 + 48).to(torch.uint8)[:, None]
        ref = (p * 2654435761 >> 9) & 3
        out[a:a + p.numel(), :, 12] = acgt[ref][:, None]
        for j in range(3):
            out[a:a + p.numel(), j, 14] = acgt[(ref + 1 + j) & 3]
            h = ((p * 3 + j) * 6364136223846793005 >> 20) & 0xFFFFFFFF
            for k, col in enumerate((16, 18, 19, 20, 21, 22, 23, 25, 26, 28, 29, 30)):
                out[a:a + p.numel(), j, col] = ((h >> (2 * k)) % 10 + 48).to(torch.uint8)
    return out.reshape(-1)


def timed(fn, warmup: int, reps: int):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return ts


def host_loop(text: bytes, lo: int, sample):
    """buffer_variant without the database over ``sample`` (pos, ref, alt) tuples."""
    rows, d = {}, {}
    for pos in {s[0] for s in sample}:
        k = (pos - lo) * 3 * LINE
        if 0 <= k < len(text):
            rows[pos] = [tuple(text[k + j * LINE:k + (j + 1) * LINE - 1].decode().split("\t")) for j in range(3)]
    t0 = time.perf_counter()
    hits = 0
    for pos, ref, alt in sample:
        if len(ref) > 1 or len(alt) > 1:
            continue  # the empty indel table
        for match in rows.get(pos, ()):
            alleles = [match[2], match[3]]
            if ref in alleles and alt in alleles:
                d[pos] = {"CADD_raw_score": float(match[4]), "CADD_phred": float(match[5])}
                hits += 1
                break
    return time.perf_counter() - t0, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=synth.C1_HI - synth.C1_LO + 1)
    ap.add_argument("--variants", type=int, default=synth.C1_N)
    ap.add_argument("--host-sample", type=int, default=200_000)
    a = ap.parse_args()
    eng = Engine(0)
    dev = eng.device
    text = table_text(synth.C1_LO, a.positions, dev)
    torch.cuda.synchronize()
    built = {}

    def build():
        built["cols"] = eng.cadd_table_build(text)

    ts = timed(build, 1, 5)
    table = CaddTable(built["cols"], eng)
    assert table.counts["rows"] == 3 * a.positions and table.counts["score_host"] == 0 and table.counts["bad"] == 0
    build_ms = min(ts)
    c1 = synth.np_c1(a.variants)
    keep = c1["pos"] < synth.C1_LO + a.positions if a.positions < synth.C1_HI - synth.C1_LO + 1 else slice(None)
    b = RecordBatch(**{k: torch.from_numpy(v if k == "heap" else v[keep]).to(dev) for k, v in c1.items()})
    ctr = eng.new_cadd_counters()
    out = tuple(eng.empty(b.n, dt) for dt in (torch.int32, torch.uint8, torch.float64, torch.float64))
    tm = timed(lambda: eng.cadd_match(table.cols, None, b, ctr, out=out), 3, 20)
    match_ms = min(tm)
    kind = out[1].cpu().numpy()
    # the host loop over a sample of the same variants
    n_s = min(a.host_sample, b.n)
    pos, off, rl, al = (c1[k][keep][:n_s] for k in ("pos", "allele_off", "ref_len", "alt_len"))
    heap = c1["heap"].tobytes()
    sample = [(int(p), heap[o:o + r].decode(), heap[o + r:o + r + l].decode())
              for p, o, r, l in zip(pos.tolist(), off.tolist(), rl.tolist(), al.tolist())]
    need = (int(pos.max()) - synth.C1_LO + 1) * 3 * LINE if n_s else 0  # the text those positions lie in
    host_s, host_hits = host_loop(text[:need].cpu().numpy().tobytes(), synth.C1_LO, sample)
    assert host_hits == int((kind[:n_s] == N.CADD_SNV).sum()), (host_hits, int((kind[:n_s] == N.CADD_SNV).sum()))
    print(json.dumps({
        "device": torch.cuda.get_device_name(0), "table_rows": table.counts["rows"], "text_bytes": text.numel(),
        "build_ms": round(build_ms, 3), "build_ms_all": [round(t, 3) for t in ts],
        "build_GBps": round(text.numel() / build_ms / 1e6, 2),
        "variants": b.n, "matched": int((kind != N.CADD_NONE).sum()),
        "match_ms": round(match_ms, 4), "match_ms_median": round(float(np.median(tm)), 4),
        "match_variants_per_s": round(b.n / match_ms * 1e3),
        "host_loop_sample": n_s, "host_loop_s": round(host_s, 4),
        "host_loop_variants_per_s": round(n_s / host_s) if host_s else None}))


if __name__ == "__main__":
    main()

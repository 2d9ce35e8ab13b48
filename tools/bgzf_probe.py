"""K11 probe: what reading a bgzip VCF costs with the inflate on the GPU and with
Python's gzip on one host thread, on one box, arms alternating.

    python tools/bgzf_probe.py [--mb 320] [--reps 5] [--out DIR]
    python tools/bgzf_probe.py --kernel-only --grids 2048,4096   # (a) alone, AVDB_OPT_K11_GRID values alternating
    AVDB_LIB=other/libavdb_hip.so python tools/bgzf_probe.py --kernel-only --tag arm   # one arm of a library A/B

The input is synth.py dbSNP-like VCF text (8 seeds, made and compressed by a process
pool; never timed), framed as bgzip writes it: members of 65,280 input bytes at level 6
and the EOF member.  Per repetition, in this order:
  (a) k_bgzf_inflate alone: compressed bytes and the member index already on the
      device, HIP events around avdb_bgzf_inflate; ms and GB/s of output
  (b) bgzf.BgzfFile(path).read(): file read, index, H2D of the compressed bytes,
      kernel; wall time to a device synchronise
  (c) gzip.open(path).read() and the H2D copy of the text (what the load path did
      before K11); wall time to a device synchronise
The outputs of (a), (b) and (c) are compared byte for byte once.  One JSON line per
measurement and a summary line (medians) on stdout.
"""

from __future__ import annotations

import argparse
import gzip
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
BLOCK = 65280


def _member(data: bytes) -> bytes:
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
    raw = c.compress(data) + c.flush()
    total = 18 + len(raw) + 8
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", total - 1) + raw + \
        struct.pack("<II", zlib.crc32(data), len(data))


def _segment(job):
    """(seed, lines) -> (text, its members): one pool task."""
    from annotatedvdb_amd import synth
    seed, n_lines = job
    text = synth.vcf_text(n_lines, seed=seed)
    return text, b"".join(_member(text[i:i + BLOCK]) for i in range(0, len(text), BLOCK))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mb", type=int, default=320, help="text size (about)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workers", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--kernel-only", action="store_true", help="measure (a) alone")
    ap.add_argument("--grids", default="", help="comma separated K11 grids (workgroups) to alternate in (a); "
                    "default: the library's own")
    ap.add_argument("--tag", default="", help="a label copied into every line (an A/B arm)")
    ap.add_argument("--out", default=None, help="directory for the log (bgzf_probe.jsonl)")
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from annotatedvdb_amd import _native as N
    from annotatedvdb_amd import bgzf
    from annotatedvdb_amd.engine import Engine

    log = []

    def emit(**kw):
        if args.tag:
            kw["tag"] = args.tag
        log.append(kw)
        print(json.dumps(kw), flush=True)

    n_seg = 8
    n_lines = max(1000, args.mb * 1000000 // n_seg // 107)  # (a synth line is about 107 bytes)
    t0 = time.perf_counter()
    with ProcessPoolExecutor(args.workers) as pool:
        parts = list(pool.map(_segment, [(100 + k, n_lines) for k in range(n_seg)]))
    text = b"".join(p[0] for p in parts)
    comp = b"".join(p[1] for p in parts) + EOF_MEMBER
    del parts
    tmp = tempfile.mkdtemp(prefix="bgzf_probe_")
    path = os.path.join(tmp, "probe.vcf.gz")
    with open(path, "wb") as fh:
        fh.write(comp)
    emit(what="input", text_bytes=len(text), compressed_bytes=len(comp), ratio=round(len(text) / len(comp), 3),
         members=-(-len(text) // BLOCK) + 1, made_in_s=round(time.perf_counter() - t0, 1))

    eng = Engine(0)
    dev = eng.device
    ix = eng.bgzf_index(comp)
    d_comp = torch.from_numpy(np.frombuffer(comp, dtype=np.uint8).copy()).to(dev)
    d_in = torch.from_numpy(ix.in_off.view(np.int64)).to(dev)
    d_out = torch.from_numpy(ix.out_off.view(np.int64)).to(dev)
    out = torch.empty(ix.out_bytes, dtype=torch.uint8, device=dev)
    status = torch.empty(ix.n_blocks, dtype=torch.uint8, device=dev)
    counts = torch.empty(N.BGZF_N_COUNTS, dtype=torch.int64, device=dev)

    def kernel_ms() -> float:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        N.check("avdb_bgzf_inflate", eng.lib.avdb_bgzf_inflate(
            eng.ctx, N.ptr(d_comp), d_comp.numel(), N.ptr(d_in), N.ptr(d_out), ix.n_blocks, N.ptr(out), out.numel(),
            N.ptr(status), N.ptr(counts), N.stream_handle(dev)))
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def read_k11() -> tuple:
        t = time.perf_counter()
        x = bgzf.BgzfFile(path, eng).read()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t, x

    def read_gzip() -> tuple:
        t = time.perf_counter()
        with gzip.open(path, "rb") as fh:
            raw = fh.read()
        x = torch.from_numpy(np.frombuffer(raw, dtype=np.uint8)).to(dev)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t, x

    # warm-up of every arm, and the one comparison of their outputs
    import warnings
    warnings.simplefilter("ignore")
    kernel_ms()
    assert counts.tolist()[:2] == [ix.n_blocks, 0], counts.tolist()
    ref = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(dev)
    assert torch.equal(out, ref), "(a) differs from the text"
    if not args.kernel_only:
        assert torch.equal(read_k11()[1], ref), "(b) differs from the text"
        assert torch.equal(read_gzip()[1], ref), "(c) differs from the text"
    del ref
    emit(what="outputs", equal=True)

    res = {"a": [], "b": [], "c": []}
    grids = [int(g) for g in args.grids.split(",") if g]
    by_grid = {g: [] for g in grids}
    for rep in range(args.reps):
        for g in grids:  # (the arms alternate inside each repetition)
            eng.set_option(N.OPT_K11_GRID, g)
            kernel_ms()
            ms = kernel_ms()
            by_grid[g].append(ms)
            emit(what="a_kernel_grid", grid=g, rep=rep, ms=round(ms, 3), out_gb_s=round(len(text) / ms / 1e6, 2))
        eng.set_option(N.OPT_K11_GRID, 0)
        ms = kernel_ms()
        res["a"].append(ms)
        emit(what="a_kernel", rep=rep, ms=round(ms, 3), out_gb_s=round(len(text) / ms / 1e6, 2))
        if args.kernel_only:
            continue
        s, _ = read_k11()
        res["b"].append(s)
        emit(what="b_bgzf_file_read", rep=rep, wall_s=round(s, 4), out_gb_s=round(len(text) / s / 1e9, 3))
        s, _ = read_gzip()
        res["c"].append(s)
        emit(what="c_gzip_then_h2d", rep=rep, wall_s=round(s, 4), out_gb_s=round(len(text) / s / 1e9, 3))
    med = {k: float(np.median(v)) for k, v in res.items() if v}
    summary = dict(what="summary", text_bytes=len(text), compressed_bytes=len(comp), reps=args.reps,
                   a_kernel_ms=round(med["a"], 3), a_out_gb_s=round(len(text) / med["a"] / 1e6, 2))
    for g in grids:
        summary["grid_%d_ms" % g] = round(float(np.median(by_grid[g])), 3)
    if not args.kernel_only:
        summary.update(b_wall_s=round(med["b"], 4), c_wall_s=round(med["c"], 4), c_over_b=round(med["c"] / med["b"], 2))
    emit(device=torch.cuda.get_device_name(0), **summary)
    os.remove(path)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "bgzf_probe%s.jsonl" % ("_" + args.tag if args.tag else "")), "a") as fh:
            for row in log:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()

"""K18a probe: the consequences of VEP JSON lines ranked and sorted (Engine.vep_consequences) and its
two library entries, beside K17's qc_table_build passes on K17's probe input, a torch.clone of the
text and ``vep_line`` (the reference's pass over a line, in Python) over a sample, all in one run.

Workload (it is input, not part of the timing): ``--templates`` synthetic lines of the tests'
generator (tests/vep_common.py) over the shipped ranking, every line with all its consequences in
one array of 1 to ``--max-csq`` elements (uniform), the other keys of VEP's output beside them; the
block of templates is tiled on the device to ``--lines`` lines.  The line shape (mean bytes and
mean consequences per line) is recorded in the result.

Timed: the whole Engine call through its final sync by the host clock, and the library entries
alone by device events.  One warm-up, then ``--reps`` repeats: median, minimum and maximum.

    python tools/vep_consequence_probe.py [--lines 2e5] [--out profiles/vep_consequence_probe.json]
"""
import argparse
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
import qc_update_probe as K17
import vep_common as V
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.vep_consequences import ConsequenceRanking, vep_line


def template_lines(n: int, max_csq: int):
    rows = V.read_ranking_rows()
    gen = V.LineGenerator(V.combos_of(rows), 18)
    return [V.dumps(gen.obj(n_csq=1 + gen.rng.randrange(max_csq))) for _ in range(n)]


def index_passes(eng, text, n_lines, tab, reps):
    """The two library entries alone, by device events: (size ms, write ms) lists, and the counts."""
    nb = text.numel()
    i32, i64, u8 = torch.int32, torch.int64, torch.uint8
    line = [eng.empty(n_lines, dt) for dt in (i32, u8, u8, i64, i32, i64, i32)]
    counts = eng.empty(N.VEP_N_COUNTS, i64)
    ws = eng.scratch("vep_index", N.size("avdb_vep_index_workspace_size", nb, n_lines))
    size = lambda: eng._launch("avdb_vep_index_size", text, nb, n_lines, tab.ref, *line, counts, ws, ws.numel())  # noqa: E731
    size()
    c = dict(zip(N.VEP_COUNTS, counts.cpu().tolist()))
    total = c["consequences"]
    per_line = line[0].long()
    csq_off = torch.cumsum(per_line, 0) - per_line
    cols = [eng.empty(total, dt) for dt in (u8, i32, i64, i32, i64, i32, i64, i32, u8, i32, u8)]
    totals = eng.empty(2, i64)
    write = lambda: eng._launch("avdb_vep_index_write", text, nb, n_lines, tab.ref, line[0], line[1], csq_off, total,  # noqa: E731
                                *cols, totals, ws, ws.numel())
    t = K16.events([size, write], reps)
    assert totals.cpu().tolist() == [total, 0]
    return t, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=float, default=2e5)
    ap.add_argument("--templates", type=int, default=251)  # (a prime: no wave meets the same template every trip)
    ap.add_argument("--max-csq", type=int, default=60)
    ap.add_argument("--qc-rows", type=float, default=4e6)
    ap.add_argument("--host-sample", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/vep_consequence_probe.json")
    a = ap.parse_args()
    reps = max(5, a.reps)
    eng = Engine(0)
    ranking = ConsequenceRanking(V.RANKING_FILE)
    templates = template_lines(a.templates, a.max_csq)
    block = eng._as_text(V.slab(templates))
    tiles = max(1, int(a.lines) // a.templates)
    text = block.repeat(tiles)
    n_lines = tiles * a.templates
    torch.cuda.synchronize()
    stats, timed, events = K13.stats, K16.timed, K16.events
    got = {}

    def call():
        got.pop("res", None)
        got["res"] = eng.vep_consequences(text, ranking)

    t_call = timed(call, reps)
    res = got["res"]
    c = res.counts
    assert c["lines"] == n_lines and c["host_lines"] == 0, c
    # the first block of templates against the host path, object for object
    t0 = time.perf_counter()
    want = [vep_line(line, ranking) for line in templates]
    host_s = time.perf_counter() - t0
    n_s = min(a.host_sample, a.templates)
    for i in range(n_s):
        assert res.ranked(i) == want[i], i
    del got["res"], res
    (t_size, t_write), c2 = index_passes(eng, text, n_lines, ranking.table(eng), reps)
    assert c2 == c
    (t_clone,) = events([lambda: text.clone()], reps)
    text_bytes = text.numel()
    del text
    torch.cuda.empty_cache()
    # K17's table passes on K17's probe input, in the same run
    qc_rows = int(a.qc_rows) // 400 * 400
    vcf = K17.vcf_text(qc_rows, 4_000_000, eng.device)
    torch.cuda.synchronize()
    t_qs, t_qw = K17.table_passes(eng, vcf, qc_rows, K17.VERSION.lower().encode(), reps)
    bc = stats(t_call)
    out = {
        "device": torch.cuda.get_device_name(0), "lines": n_lines, "text_bytes": text_bytes,
        "templates": a.templates, "mean_line_bytes": round(text_bytes / n_lines, 1),
        "mean_consequences_per_line": round(c["consequences"] / n_lines, 2), "consequences": c["consequences"],
        "max_consequences_per_line": a.max_csq, "reps": reps,
        "vep_consequences_call_ms": bc, "vep_index_size_pass_ms": stats(t_size), "vep_index_write_pass_ms": stats(t_write),
        "clone_text_ms": stats(t_clone),
        "text_GBps_size_pass_median": round(text_bytes / stats(t_size)["median"] / 1e6, 1),
        "text_GBps_write_pass_median": round(text_bytes / stats(t_write)["median"] / 1e6, 1),
        "qc_rows": qc_rows, "qc_vcf_bytes": vcf.numel(), "qc_table_size_pass_ms": stats(t_qs),
        "qc_table_write_pass_ms": stats(t_qw),
        "qc_vcf_GBps_size_pass_median": round(vcf.numel() / stats(t_qs)["median"] / 1e6, 1),
        "vep_line_sample_lines": len(templates), "vep_line_s": round(host_s, 3),
        "vep_line_lines_per_s": round(len(templates) / host_s),
        "device_lines_per_s_call_median": round(n_lines / bc["median"] * 1e3),
    }
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()

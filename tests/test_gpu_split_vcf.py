"""K15 on the GPU: a whole-genome VCF split by chromosome (Engine.split_vcf) against the
reference's golden and against the library's host entries, array for array and blob for
blob, with sentinel-filled buffers."""

import random

import pytest

import bgzf_common as Z
import split_vcf_common as S
import test_split_vcf_host as H
from annotatedvdb_amd import _native as N

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 256    # lines of a workgroup trip (kBlock)
WAVE = 64
STAGE = 36 * 1024  # the LDS stage of a trip's text
GRID = 4096   # workgroups at most: tile 4096 is workgroup 0's second trip
KEYS = S.LABELS + [b"chrUn"]  # a key of every stream, 25 the unplaced one


@pytest.fixture(scope="module")
def host():
    from annotatedvdb_amd.engine import Engine
    return Engine("host")


def both(engine, host, text, what=""):
    engine.poison = 0xA5
    try:
        return S.same_on_both(engine, host, text, what=what)
    finally:
        engine.poison = None


# ---- 1: the partition at its edges ------------------------------------------------------
@pytest.mark.parametrize("n_lines", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_g1_line_counts(engine, host, n_lines):
    # streams cycling through all 26 codes line by line: every wave is mixed
    cyc = [KEYS[i % 26] for i in range(n_lines)]
    code, _, cnt, blob, _ = both(engine, host, S.slab_of(cyc), "cycling")
    assert code.tolist() == [i % 26 for i in range(n_lines)]
    # one stream throughout: every wave and tile is uniform; with and without the last newline
    for key, end in ((b"7", True), (b"X", False), (b"chrUn", True)):
        code, _, _, blob, _ = both(engine, host, S.slab_of([key] * n_lines, newline_at_end=end), "uniform")
        assert len(set(code.tolist())) == min(1, n_lines) and blob.count(b"\n") == n_lines
    # comments scattered: lanes without output inside uniform waves, and whole waves of them
    rng = random.Random(n_lines)
    comments = {i for i in range(n_lines) if rng.random() < 0.2 or 64 <= i < 128}
    _, _, cnt, _, _ = both(engine, host, S.slab_of([b"2"] * n_lines, comments=comments), "comments")
    assert cnt[N.SPLIT_COUNT_COMMENTS] == len(comments) and cnt[N.SPLIT_COUNT_LINES + 1] == n_lines - len(comments)


def test_g1_stream_changes_at_wave_and_tile_edges(engine, host):
    n = 3 * TILE
    for at in (WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE):
        chroms = [b"1"] * at + [b"2"] * (n - at)  # the change exactly at line `at`
        code, _, cnt, _, _ = both(engine, host, S.slab_of(chroms), "change at %d" % at)
        assert cnt[N.SPLIT_COUNT_LINES] == at and cnt[N.SPLIT_COUNT_LINES + 1] == n - at
    # a tile uniform except for its last line, its first line, one lane of each wave
    for odd in ([TILE - 1], [0], [2 * TILE - 1, 2 * TILE], list(range(5, n, WAVE))):
        chroms = [b"M" if i in odd else b"22" for i in range(n)]
        both(engine, host, S.slab_of(chroms), "odd lines %r" % odd[:3])
    # sorted contigs, a few lines each: many streams in one tile, each a run
    chroms = [k for k in KEYS for _ in range(23)]
    both(engine, host, S.slab_of(chroms), "sorted runs")


def test_g1_line_lengths_and_the_stage(engine, host):
    rng = random.Random(15)
    # lengths 0 .. 200 mixed with one 40,000-byte line, past the LDS stage: its tile is read from global memory
    n = 700
    lengths = [rng.randint(0, 200) for _ in range(n)]
    lengths[300] = 40_000
    chroms = [rng.choice(KEYS) for _ in range(n)]
    code, out_len, _, blob, _ = both(engine, host, S.slab_of(chroms, lengths), "long line")
    assert max(out_len.tolist()) > STAGE and len(blob) > 40_000
    # a tile whose lines together exceed the stage, between tiles that fit
    lengths = [20] * TILE + [200] * TILE + [20] * TILE
    assert sum(lengths[TILE:2 * TILE]) > STAGE
    both(engine, host, S.slab_of([rng.choice(KEYS[:3]) for _ in lengths], lengths), "tile past the stage")
    both(engine, host, S.slab_of([b"5"] * len(lengths), lengths), "uniform tile past the stage")
    # empty lines, whitespace tails and '\r\n' ends among the lines
    lines = []
    for i in range(600):
        lines.append(S.vcf_line(rng.choice(KEYS), i, rng.randint(0, 60)) + rng.choice([b"", b"\r", b" \t", b"\t\t\r"]))
        if i % 7 == 0:
            lines.append(rng.choice([b"", b"  ", b"#c", b"\r"]))
    both(engine, host, b"\n".join(lines), "tails")


def test_g1_scan_levels_and_grid_trips(engine, host):
    rng = random.Random(16)
    # 12,000 short lines: 47 tiles, a matrix of 47 * 26 + 1 = 1,223 entries, two tiles of the scan
    n = 12_000
    assert ((n + TILE - 1) // TILE) * 26 > 1024
    chroms = [KEYS[(i // 37) % 26] if i % 5 else rng.choice(KEYS) for i in range(n)]
    _, _, cnt, _, _ = both(engine, host, S.slab_of(chroms, [rng.randint(0, 12) for _ in range(n)]), "12,000 lines")
    assert min(cnt[:26]) > 0
    # more tiles than workgroups: workgroup 0 and its neighbours take a second trip with the same LDS
    n = GRID * TILE + 3 * TILE + 17
    text = b"1\n" * (GRID * TILE) + S.slab_of([KEYS[i % 26] for i in range(n - GRID * TILE)])
    _, _, cnt, blob, _ = both(engine, host, text, "second trip")
    assert sum(cnt[:26]) == n and blob.startswith(b"1\n1\n")


# ---- 2: the rule and the golden on the device ---------------------------------------------
def test_g2_edge_slabs_on_the_device(engine, host):
    planted = 0
    for name, text in S.edge_slabs():
        code, out_len, cnt, _, _ = both(engine, host, text, name)
        S.check_against_ref(engine, text, what=name)
        planted += 5 if name.startswith("tail_") else name == "lone_ff_tail"
        # the lines flagged for the host are the planted ones: a device that flags all cannot pass
        assert cnt[N.SPLIT_COUNT_HOST_LINES] == (5 if name.startswith("tail_") else name == "lone_ff_tail"), name
    assert planted == 5 * len(S.HOST_TAILS) + 1


def test_g2_map_on_the_device(engine, host):
    from annotatedvdb_amd.engine import ChromMap
    mapping = S.chrmap()
    dev_map, host_map = ChromMap.for_split(engine, mapping), ChromMap.for_split(host, mapping)
    text = S.map_slab(mapping, n=900, seed=6)
    engine.poison = 0xA5
    try:
        code, _, cnt, _, _ = S.same_on_both(engine, host, text, dev_map, host_map, "map")
        S.check_against_ref(engine, text, mapping, dev_map, "map")
    finally:
        engine.poison = None
    assert len(set(code.tolist())) == 26


def test_g2_golden_on_the_device(engine, host, tmp_path):
    engine.poison = 0xA5
    try:
        H.check_golden(engine, tmp_path, suffixes=(".vcf.gz",))
        H.check_cases(engine)
    finally:
        engine.poison = None
    for name, (text, with_map, _) in S.golden()[0].items():
        cm = (engine.split_chrom_map(S.chrmap()), host.split_chrom_map(S.chrmap())) if with_map else (None, None)
        S.same_on_both(engine, host, text, *cm, what=name)
    assert engine.split_vcf(S.golden()[0]["run1"][0]).text.is_cuda


# ---- 3: the engine and the driver on the device ---------------------------------------------
def test_g3_engine_host_lines_and_capacity(engine):
    engine.poison = 0xA5
    try:
        H.check_host_lines(engine)  # (asserts the LINE_HOST count equals the lines planted)
        H.check_engine(engine)
        H.check_capacity(engine)
        H.check_patched_lines(engine)
    finally:
        engine.poison = None


def test_g3_bgzip_input_through_the_driver(engine, tmp_path):
    from annotatedvdb_amd import split_vcf_by_chr as D
    text, with_map, want = S.golden()[0]["run2"]
    src = tmp_path / "run2.vcf.gz"
    src.write_bytes(Z.bgzip(text, block=30000))
    out = tmp_path / "out"
    lines = D.main(["-f", str(src), "-o", str(out), "-c", S.CHRMAP, "--batchBytes", "65536"], engine=engine)
    H.check_files(out, want, lines)

"""K17 on the GPU: the ADSP QC table (Engine.qc_table_build) and the update rows
(Engine.qc_update_rows, QCUpdater.buffer_export) against the reference's golden and against the
library's host entries, array for array, with poisoned buffers."""

import json
import random

import numpy as np
import pytest

import bgzf_common as Z
import hash_common as H
import qc_common as Q
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.adsp_qc import QCUpdater

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRIP = 256           # lines of a workgroup trip (kBlock)
SIZE_GRID = 4096     # workgroups at most in a size pass: line 4096 * 256 is workgroup 0's second trip
WRITE_GRID = 2048    # and in a write pass
JSON_STAGE = 64 * 1024
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513]
REL = "17k"


@pytest.fixture(scope="module")
def host():
    from annotatedvdb_amd.engine import Engine
    return Engine("host")


def poisoned(engine, f):
    engine.poison = 0xA5
    try:
        return f()
    finally:
        engine.poison = None


def both_tables(engine, host, vcf, slab=None, version="R1"):
    """The table on the device (poisoned buffers) and from the host entries: equal in every array."""
    dev = poisoned(engine, lambda: engine.qc_table_build(vcf if slab is None else slab, version))
    ref = host.qc_table_build(vcf, version)
    Q.assert_same(Q.table_arrays(dev), Q.table_arrays(ref), "table: device against host entries")
    assert dev.keys.is_cuda or dev.n_rows == 0
    return dev, ref


def both_rows(engine, host, tables, export, slab=None, **kw):
    dev_t, ref_t = tables
    dev_t.hit.zero_()
    ref_t.hit.zero_()
    dev = poisoned(engine, lambda: Q.rows_arrays(engine.qc_update_rows(export if slab is None else slab, dev_t, **kw)))
    ref = Q.rows_arrays(host.qc_update_rows(export, ref_t, **kw))
    Q.assert_same(dev, ref, "rows: device against host entries")
    assert np.array_equal(dev_t.hit.cpu().numpy(), ref_t.hit.numpy())
    return dev


@pytest.fixture(scope="module")
def fuzz_tables(engine, host):
    """A table of 513 lines that average more than one alt, on both engines, and its ids."""
    vcf, ids = Q.fuzz_vcf(random.Random(1717), 513, multi_alt=0.7, host=0.05)
    return both_tables(engine, host, vcf), ids, vcf


# ---- 1: the golden on the device ------------------------------------------------------------
def test_g1_golden_on_the_device(engine):
    g = Q.golden()

    def run(mode):
        t = engine.qc_table_build(g["vcf"], g["version"])
        assert t.counts["host_lines"] == g["host_lines"] and t.keys.is_cuda
        first = (t.flags & N.QC_ROW_FIRST) != 0
        host_lines = int((first & ((t.flags & N.QC_LINE_HOST) != 0)).sum())
        device_lines = int(first.sum()) - host_lines
        assert device_lines >= 9 * host_lines > 0  # (rendered on the device, not all sent to the host)
        u = QCUpdater(t)
        u.buffer_export(g["export"], update_existing=bool(mode))
        return t, u
    for mode in (0, 1):
        t, u = poisoned(engine, lambda: run(mode))
        want, ctr, missing = Q.ref_update(g["vcf"], g["export"], REL, update_existing=bool(mode))
        assert u.update_text() == Q.rows_text(want)
        key = lambda x: (x[0], x[1], x[2] is True, x[3])  # noqa: E731
        assert sorted(set(u.update_buffer()), key=key) == sorted(set(g["tuples"][mode]), key=key)
        assert u.unmatched() == missing and sorted(missing) == sorted(g["missing"])
        assert (u.get_count("skipped"), u.get_count("not_in_vcf")) == (ctr["skipped"], ctr["not_in_vcf"])
    assert Q.table_tuples(t) == [(i, js, f) for i, js, f, _ in Q.ref_table(g["vcf"], REL)[0]]


def test_g1_golden_cases_on_the_device(engine, host):
    """Every one-line case of the golden the reference accepts, in one slab: the to_numeric edge values
    rendered on the device as the host entries render them, and as the reference did."""
    cases = [c for c in Q.golden()["cases"] if c[1] is None]
    vcf = b"".join(c[2] for c in cases)
    dev, ref = both_tables(engine, host, vcf, version="17K")
    want = [(i, c[5], c[4]) for c in cases for i in c[3]]
    assert Q.table_tuples(dev) == want
    assert 0 < dev.counts["host_lines"] < len(cases) // 2


# ---- 2: fuzzed slabs of both passes, device against host entries ------------------------------
@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_vcf_slabs(engine, host, n_lines):
    for seed, kw in ((1, {}), (2, {"multi_alt": 0.8, "samples": 0.5})):
        vcf, ids = Q.fuzz_vcf(random.Random(1000 * n_lines + seed), n_lines, **kw)
        dev, ref = both_tables(engine, host, vcf)
        c = dev.counts
        assert c["lines"] == n_lines
        want, ctr = Q.ref_table(vcf, "r1")
        assert {k: c[k] for k in ctr} == ctr
        assert Q.table_tuples(dev) == [(i, js, f) for i, js, f, _ in want]
        if seed == 2 and n_lines >= 255:
            assert dev.n_rows > n_lines  # more rows than lines within a 256-line trip
        if n_lines >= 255:
            assert 0 < c["host_lines"] < n_lines // 4 and 0 < c["pass"] < c["entries"]
        export = Q.fuzz_export(random.Random(seed), ids, 40)
        both_rows(engine, host, (dev, ref), export)


@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_export_slabs(engine, host, fuzz_tables, n_lines):
    tables, ids, vcf = fuzz_tables
    for seed, kw in ((1, {}), (2, {"update_existing": True}), (3, {"contigs": ["1", "X", "GL000219.1"]})):
        export = Q.fuzz_export(random.Random(1000 * n_lines + seed), ids, n_lines)
        dev = both_rows(engine, host, tables, export, **kw)
        c = dev["counts"]
        # (a host row found to have QC values keeps its place among the rows, without bytes, and counts skipped)
        assert dev["n"] + c["skipped"] + c["skipped_lines"] + c["not_in_vcf"] == n_lines
        assert c["rows"] - dev["n"] == int((np.diff(dev["row_off"]) == 0).sum()) <= c["host_rows"]
        want, ctr, _ = Q.ref_update(vcf, export, "r1", **kw)
        assert dev["text"].tobytes() == Q.rows_text(want)
        assert dev["n"] == ctr["rows"] and {k: c[k] for k in ("skipped", "skipped_lines", "not_in_vcf")} == \
            {k: ctr[k] for k in ("skipped", "skipped_lines", "not_in_vcf")}
        if n_lines >= 255 and not kw:
            assert min(dev["n"], c["skipped"], c["skipped_lines"], c["not_in_vcf"], c["host_rows"]) > 0, c


@pytest.mark.parametrize("n_keys", [0, 1, 512, 513, 1025])
def test_g2_table_sizes_around_the_slot_doubling(engine, host, n_keys):
    """512 keys fill 1,024 slots to a half, 513 double them, 1,025 double them again."""
    rng = random.Random(n_keys)
    lines = [b"%d\t%d\t.\tA\tC\t%d\t%s\tAC=%d;AF=0.%d;DB\tGT" % (1 + k % 22, 1000 + k, k, (b"PASS", b".")[k % 2], k, 1 + k % 9)
             for k in range(n_keys)]
    vcf = b"\n".join(lines) + (b"\n" if lines else b"")
    tables = both_tables(engine, host, vcf)
    assert tables[0].n_rows == n_keys and tables[0].keyset.numel() == 12 * H.slots(n_keys)
    assert H.slots(n_keys) == {0: 1024, 1: 1024, 512: 1024, 513: 2048, 1025: 4096}[n_keys]
    ids = [b"%d:%d:A:C" % (1 + k % 22, 1000 + k) for k in range(n_keys)] + [b"1:5:A:C", b"2:1000:A:C"]
    rng.shuffle(ids)
    export = b"".join(i + b":rs1\t" + i + b"\t\\N\n" for i in ids)
    dev = both_rows(engine, host, tables, export)
    assert dev["n"] == n_keys == int(tables[0].hit.sum()) and dev["counts"]["not_in_vcf"] == 2
    assert dev["text"].tobytes().count(b"\ttrue\t") == (n_keys + 1) // 2


def test_g2_rows_across_scan_tiles_and_write_trips(engine, host, fuzz_tables):
    """3,200 export lines: the output lengths' scan runs over three 1,024-row tiles and the write
    pass over many trips, whose spans start at every byte of an 8-byte word."""
    tables, ids, _ = fuzz_tables
    rng = random.Random(26)
    export = b"".join(b"%s:rs%d\t%s\t\\N\n" % (i.encode(), rng.randint(1, 10 ** rng.randint(1, 9)), i.encode())
                      for i in (rng.choice(ids) for _ in range(3200)))
    dev = both_rows(engine, host, tables, export)
    off = dev["row_off"]
    assert dev["n"] == 3200 and len({int(off[k]) % 8 for k in range(0, dev["n"], TRIP)}) >= 4
    assert {int(off[k]) % 8 for k in range(dev["n"])} == set(range(8))


def test_g2_depth_one_key_on_the_device(engine, host):
    """The release nested at depth 2 only, as a string value at depth 1, as a prefix of a longer key;
    a backslash sends the row to the host."""
    line = b"1\t100\t.\tA\tG\t50\tPASS\tAC=1\tGT\n"
    tables = both_tables(engine, host, line)
    cols = {b'{"r1": {}}': 0, b'{"r0": {"a": [1, {"b": "}"}]}, "r1": 5}': 0, b'{"r1" : 1}': 0, b'{"x": "{", "r1": 1}': 0,
            b'{"r0": "a\\\\"b", "r1": 1}': 0, b"\\N": 1, b"": 1, b"{}": 1, b'{"r0": {"r1": 1}}': 1,
            b'{"r0": "r1", "k": "r1"}': 1, b'{"r1x": 1, "xr1": 2}': 1, b'{"k": ["r1", {"r1": 1}]}': 1,
            b'{"r0": "say \\\\"r1\\\\": 1"}': 1}
    export = b"".join(b"pk%d\t1:100:A:G\t%s\n" % (k, c) for k, c in enumerate(cols))
    dev = both_rows(engine, host, tables, export)
    kept = [int(r.split(b"\t")[0][2:]) for r in dev["text"].tobytes().split(b"\n")[:-1]]
    assert kept == [k for k, v in enumerate(cols.values()) if v]
    assert dev["counts"]["host_rows"] == 2 and dev["counts"]["skipped"] == len(cols) - len(kept)
    assert both_rows(engine, host, tables, export, update_existing=True)["n"] == len(cols)


# ---- 3: trips longer than the stages -----------------------------------------------------------
def test_g3_trips_longer_than_the_stages(engine, host):
    """A 40,000-byte allele in both texts (the size passes read those trips from global memory, the
    key and row writers store them from the lanes), an INFO of one item, one of 2,000 items (the
    repeated-key walk gives it up: the host's) and one of 700, and a JSON longer than the write stage
    rendered on the device."""
    rng = random.Random(40)
    big = "".join(rng.choice("ACGT") for _ in range(40000))
    vcf, ids = Q.fuzz_vcf(rng, 300)
    word = "".join(rng.choice("GHJKLMPQ") for _ in range(18000))
    extra = ["3\t77\t.\t%s\tA,C\t50\tPASS\tAC=1;AF=0.5\tGT" % big,
             "4\t88\t.\tA\tG\t.\t.\t" + ";".join("K%d=%d.%d" % (k, k, k % 7) for k in range(2000)) + "\tGT",
             "4\t89\t.\tA\t%s\t.\tPASS\tDB\tGT" % big,
             "4\t90\t.\tA\tG\t.\t.\tONE=1\tGT",
             "4\t91\t.\tA\tG\t.\tPASS\t" + ";".join("W%d=%s%d" % (k, word, k) for k in range(5)) + "\tGT:AD",
             "4\t92\t.\tA\tG\t.\t.\t" + ";".join("K%d=-%d" % (k, k) for k in range(700)) + "\tGT"]
    lines = vcf.rstrip(b"\n").split(b"\n")
    lines[100:100] = [x.encode() for x in extra]
    vcf = b"\n".join(lines) + b"\n"
    tables = both_tables(engine, host, vcf)
    rows = {i: (js, f) for i, js, f in Q.table_tuples(tables[0])}
    for k, i in ((1, "4:88:A:G"), (3, "4:90:A:G"), (4, "4:91:A:G"), (5, "4:92:A:G")):
        assert rows[i] == Q.ref_line(extra[k].encode(), "r1")[1:], i
    assert "3:77:%s:C" % big in rows and len(rows["4:91:A:G"][0]) > JSON_STAGE
    flags = {int(s): int(f) for s, f in zip(tables[0].line_start.cpu(), tables[0].flags.cpu())}
    at = {k: vcf.index(extra[k].encode()) for k in range(6)}
    assert flags[at[1]] & N.QC_LINE_HOST and not any(flags[at[k]] & N.QC_LINE_HOST for k in (0, 2, 3, 4, 5))
    ids = ids + ["3:77:%s:A" % big, "3:77:%s:C" % big, "4:88:A:G", "4:91:A:G"]
    export = Q.fuzz_export(rng, ids, 400, long_allele=40000)
    export = b"".join(b"%s\t%s\n" % (i.encode(), i.encode()) for i in ids[-4:]) + export
    dev = both_rows(engine, host, tables, export)
    want, _, _ = Q.ref_update(vcf, export, "r1")
    assert dev["text"].tobytes() == Q.rows_text(want)
    assert int(np.diff(dev["row_off"]).max()) > JSON_STAGE and sum(len(ln) > 40000 for ln in export.split(b"\n")) >= 3


# ---- 4: a second grid-stride trip of each size pass -----------------------------------------------
def test_g4_second_grid_stride_trip_of_the_export_pass(engine, host, fuzz_tables):
    """More export lines than SIZE_GRID workgroups take in one trip (and more rows than WRITE_GRID
    workgroups): workgroup 0 comes back for lines 4096 * 256 ..; the lines there differ from the
    16-line block repeated before them."""
    tables, ids, vcf = fuzz_tables
    short = sorted({i for i in ids if len(i) < 16})[:64]
    assert len(short) == 64
    block = b"".join(b"%s\t%s\n" % (m.encode(), m.encode()) for m in short[:16])
    tail = b"".join(b"%s:rs1\t%s\t\\N\n" % (m.encode(), m.encode()) for m in short[16:64]) * 7
    text = block * (SIZE_GRID * TRIP // 16) + tail[:-1]
    assert len(text) < 48 << 20
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(engine.device)
    dev = both_rows(engine, host, tables, text, slab=slab)
    assert dev["n"] == SIZE_GRID * TRIP + 48 * 7 > WRITE_GRID * TRIP
    want, _, _ = Q.ref_update(vcf, tail, "r1")
    assert dev["text"][int(dev["row_off"][SIZE_GRID * TRIP]):].tobytes() == Q.rows_text(want)


def test_g4_second_grid_stride_trip_of_the_table_pass(engine, host):
    """More VCF lines than SIZE_GRID workgroups take in one trip: the two passes called directly on
    both engines (no key set over a million equal keys), the tail's lines differing from the block."""
    block = b"".join(b"%d\t%d\t.\tA\tC\t.\t.\tDB\tG\n" % (1 + k, 7 + k) for k in range(16))
    tail_lines = [b"X\t%d\t.\tAC\tG,T\t%d.50\tPASS\tAC=-%d;AF=0.00%d;DB\tGT:DP\n" % (100 + k, k, k, k) for k in range(300)]
    text = block * (SIZE_GRID * TRIP // 16) + b"".join(tail_lines)
    assert len(text) < 48 << 20
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(engine.device)
    rc, cnt, out, totals = Q.raw_table_passes(engine, slab)
    rc_h, cnt_h, out_h, totals_h = Q.raw_table_passes(host, text)
    assert rc == rc_h == 0 and cnt == cnt_h and totals == totals_h
    assert cnt["entries"] == SIZE_GRID * TRIP + 300 and cnt["rows"] == SIZE_GRID * TRIP + 600 and cnt["host_lines"] == 0
    Q.assert_same(out, out_h, "second trip of the table pass: device against host entries")
    js = out["json"][:cnt["json_bytes"]].tobytes()
    want = "".join(Q.ref_line(ln, "r1")[1] for ln in tail_lines)
    assert js.endswith(want.encode()) and cnt["pass"] == 300


# ---- 5: capacity, errors -----------------------------------------------------------------------------
def test_g5_capacity_and_sentinels_on_the_device(engine, fuzz_tables):
    tables, ids, vcf = fuzz_tables
    rc, cnt, out, totals = Q.raw_table_passes(engine, vcf)
    n, kb, jb = cnt["rows"], cnt["key_bytes"], cnt["json_bytes"]
    assert rc == 0 and totals == [kb, jb, n, 0] and n > 300
    assert (out["keys"][kb:] == 0xA5).all() and (out["json"][jb:] == 0xA5).all()
    for name, size in (("flags", 1), ("json_len", 4), ("json_off", 8), ("line_start", 8)):
        assert (out[name].view(np.uint8)[size * n:] == 0xA5).all(), name
    assert (out["key_off"].view(np.uint8)[8 * (n + 1):] == 0xA5).all()
    ne = cnt["entries"]
    for i, size in enumerate((8, 4, 4, 4, 1)):
        assert (out["ent_%d" % i].view(np.uint8)[size * ne:] == 0xA5).all(), i
    for short in ("key", "json"):
        rc, _, out2, totals2 = Q.raw_table_passes(engine, vcf, **{short + "_cap": (kb if short == "key" else jb) - 1})
        assert rc == 0 and totals2 == [kb, jb, n, 1]
        for name in ("keys", "json", "key_off", "json_off", "json_len", "line_start", "flags"):
            assert (out2[name].view(np.uint8) == 0xA5).all(), (short, name)
    export = Q.fuzz_export(random.Random(5), ids, 700)
    rc, ucnt, buf, utot, cap = Q.raw_update_passes(engine, export, tables[0])
    assert rc == 0 and utot == [cap, 0] and cap > 1000 and (buf[cap:] == 0xA5).all()
    rc, _, buf, utot, _ = Q.raw_update_passes(engine, export, tables[0], cap=cap - 1)
    assert rc == 0 and utot == [cap, 1] and (buf == 0xA5).all()


def test_g5_errors_raise_on_the_device(engine):
    line = b"1\t100\t.\tA\tG\t50\tPASS\tAC=1\tGT\n"
    t = engine.qc_table_build(line, "r1")
    with pytest.raises(ValueError, match="line 2 of the export"):
        engine.qc_update_rows(b"a\t1:100:A:G\n1:5:A\t1:5:A\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        engine.qc_update_rows(b"a\t1:100\r:A:G\t\\N\n", t)
    with pytest.raises(ValueError, match="line 2 of the export"):
        engine.qc_update_rows(b"a\t1:100:A:G\t\\N\nb\t1:100:A:G\tnot json\n", t)
    with pytest.raises(ValueError, match="Infinity") as ei:
        engine.qc_table_build(b"#c\n" + line + b"1\t100\t.\tA\tG\t.\t.\tAF=inf\tGT\n", "r1")
    assert ei.value.line == 3
    assert json.loads(Q.table_tuples(t)[0][1]) == {"r1": {"info": {"AC": 1}, "filter": "PASS", "qual": 50, "format": "GT"}}


def test_g5_write_entry_on_an_empty_slab(engine, host):
    """avdb_qc_table_write on a zero-byte slab (no lines, so no scans and no kernels), totals and
    key_off poisoned: without rows zero totals and key_off[0] = 0; a row that nothing bears out sets
    totals[3] and leaves key_off alone, the device entry returning OK and the host entry ERANGE."""
    poison = int(np.frombuffer(b"\xA5" * 8, dtype=np.int64)[0])
    for eng, over_rc in ((engine, 0), (host, N.AVDB_ERANGE)):
        suffix, tail = Q._runner(eng, "qc_table", "avdb_qc_table_workspace_size", 0, 0)
        full = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), 0xA5,  # noqa: E731
                                        dtype=torch.uint8, device=eng.device).view(dt)
        for n_rows, want_rc, want, want_off in ((0, 0, [0, 0, 0, 0], 0), (1, over_rc, [0, 0, 0, 1], poison)):
            ents = [full(1, torch.int64)] + [full(1, torch.int32) for _ in range(3)] + [full(1, torch.uint8)]
            key_off, totals = full(n_rows + 1, torch.int64), full(4, torch.int64)
            rc = Q._call(eng, "avdb_qc_table_write" + suffix, None, 0, 0, 0, n_rows, b"r1", 2, *ents,
                         full(8, torch.uint8), 0, key_off, full(8, torch.uint8), 0, full(1, torch.int64),
                         full(1, torch.int32), full(1, torch.int64), full(1, torch.uint8), totals, *tail)
            assert (rc, totals.cpu().tolist(), int(key_off[0])) == (want_rc, want, want_off), (eng.host_only, n_rows)
            assert key_off.cpu().tolist()[1:] == [poison] * n_rows


# ---- 6: bgzip input ------------------------------------------------------------------------------------
def test_g6_bgzip_pair_through_read_whole(engine, host, tmp_path):
    from annotatedvdb_amd import bgzf
    g = Q.golden()
    vcf_path, exp_path = tmp_path / "qc.vcf.gz", tmp_path / "export.tsv.gz"
    vcf_path.write_bytes(Z.bgzip(g["vcf"], block=20000))
    exp_path.write_bytes(Z.bgzip(g["export"], block=20000))
    slab = bgzf.read_whole(str(vcf_path), engine)
    assert isinstance(slab, torch.Tensor) and slab.is_cuda and slab.numel() == len(g["vcf"])
    tables = both_tables(engine, host, g["vcf"], slab=slab, version=g["version"])
    u = poisoned(engine, lambda: QCUpdater(str(vcf_path), g["version"], engine))
    n = poisoned(engine, lambda: u.buffer_export(str(exp_path)))
    want, _, missing = Q.ref_update(g["vcf"], g["export"], REL)
    assert n == len(want) and u.update_text() == Q.rows_text(want) and u.unmatched() == missing
    both_rows(engine, host, tables, g["export"], slab=bgzf.read_whole(str(exp_path), engine))

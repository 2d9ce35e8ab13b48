"""K16 on the GPU: the SnpEff LOF/NMD table (Engine.lof_table_build) and the update rows
(Engine.lof_update_rows, LOFUpdater.buffer_export) against the reference's golden and against the
library's host entries, array for array, with poisoned buffers."""

import random

import numpy as np
import pytest

import bgzf_common as Z
import hash_common as H
import lof_common as L
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.snpeff_lof import LOFUpdater

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRIP = 256           # lines of a workgroup trip (kBlock)
SIZE_GRID = 4096     # workgroups at most in the size pass: line 4096 * 256 is workgroup 0's second trip
WRITE_GRID = 2048    # and in the write pass
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 513]


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


def both_tables(engine, host, vcf, slab=None):
    """The table on the device (poisoned buffers) and from the host entries: equal in every array."""
    dev = poisoned(engine, lambda: engine.lof_table_build(vcf if slab is None else slab))
    ref = host.lof_table_build(vcf)
    L.assert_same(L.table_arrays(dev), L.table_arrays(ref), "table: device against host entries")
    assert dev.keys.is_cuda or dev.n_rows == 0
    return dev, ref


def both_rows(engine, host, tables, export, slab=None, **kw):
    dev_t, ref_t = tables
    dev_t.hit.zero_()
    ref_t.hit.zero_()
    dev = poisoned(engine, lambda: L.rows_arrays(engine.lof_update_rows(export if slab is None else slab, dev_t, **kw)))
    ref = L.rows_arrays(host.lof_update_rows(export, ref_t, **kw))
    L.assert_same(dev, ref, "rows: device against host entries")
    assert np.array_equal(dev_t.hit.cpu().numpy(), ref_t.hit.numpy())
    return dev


@pytest.fixture(scope="module")
def fuzz_tables(engine, host):
    """A table of 513 lines that average more than one alt, on both engines, and its ids."""
    vcf, ids = L.fuzz_vcf(random.Random(1616), 513, annotated=0.9, multi_alt=0.7, host=0.05)
    return both_tables(engine, host, vcf), ids, vcf


# ---- 1: the golden on the device ------------------------------------------------------------
def test_g1_golden_on_the_device(engine):
    g = L.golden()

    def run(mode):
        t = engine.lof_table_build(g["vcf"])
        assert t.counts["host_lines"] == g["host_lines"] and t.keys.is_cuda
        device_rows = int(((t.flags & N.LOF_LINE_HOST) == 0).sum())
        assert device_rows > 9 * (t.n_rows - device_rows) > 0  # (rendered on the device, not all sent to the host)
        u = LOFUpdater(t)
        u.buffer_export(g["export"], update_existing=bool(mode))
        return t, u
    for mode in (0, 1):
        t, u = poisoned(engine, lambda: run(mode))
        want, ctr, missing = L.ref_update(g["vcf"], g["export"], update_existing=bool(mode))
        assert u.update_text() == L.rows_text(want)
        assert sorted(set(u.update_buffer())) == sorted(set(g["tuples"][mode]))
        assert u.unmatched() == missing and sorted(missing) == sorted(g["missing"])
        assert (u.get_count("skipped"), u.get_count("not_annotated")) == (ctr["skipped"], ctr["not_annotated"])
    assert L.table_rows(t) == [(i, js) for i, js, _ in L.ref_table(g["vcf"])[0]]


# ---- 2: fuzzed slabs of both passes, device against host entries ------------------------------
@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_vcf_slabs(engine, host, n_lines):
    for seed, kw in ((1, {}), (2, {"multi_alt": 0.8, "annotated": 0.9})):
        vcf, ids = L.fuzz_vcf(random.Random(1000 * n_lines + seed), n_lines, **kw)
        dev, ref = both_tables(engine, host, vcf)
        c = dev.counts
        assert c["lines"] == n_lines
        want, ctr = L.ref_table(vcf)
        assert {k: c[k] for k in ctr} == ctr
        assert L.table_rows(dev) == [(i, js) for i, js, _ in want]
        if seed == 2 and n_lines >= 255:
            assert dev.n_rows > n_lines  # more rows than lines within a 256-line trip
        export = L.fuzz_export(random.Random(seed), ids, 40)
        both_rows(engine, host, (dev, ref), export)


@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_export_slabs(engine, host, fuzz_tables, n_lines):
    tables, ids, vcf = fuzz_tables
    for seed, kw in ((1, {}), (2, {"update_existing": True}), (3, {"contigs": ["1", "X", "GL000219.1"]})):
        export = L.fuzz_export(random.Random(1000 * n_lines + seed), ids, n_lines)
        dev = both_rows(engine, host, tables, export, **kw)
        c = dev["counts"]
        assert c["rows"] + c["skipped"] + c["skipped_lines"] + c["not_annotated"] == n_lines
        want, ctr, _ = L.ref_update(vcf, export, **kw)
        assert dev["text"].tobytes() == L.rows_text(want) and {k: c[k] for k in ctr} == ctr
        if n_lines >= 255 and not kw:
            assert min(c["rows"], c["skipped"], c["skipped_lines"], c["not_annotated"]) > 0, c


@pytest.mark.parametrize("n_keys", [0, 1, 512, 513, 1025])
def test_g2_table_sizes_around_the_slot_doubling(engine, host, n_keys):
    """512 keys fill 1,024 slots to a half, 513 double them, 1,025 double them again."""
    rng = random.Random(n_keys)
    lines = [b"%d\t%d\t.\tA\tC\t.\t.\tAC=1;LOF=(G%d|E|%d|0.%d)" % (1 + k % 22, 1000 + k, k, k % 50, 1 + k % 9)
             for k in range(n_keys)]
    vcf = b"\n".join(lines) + (b"\n" if lines else b"")
    tables = both_tables(engine, host, vcf)
    assert tables[0].n_rows == n_keys and tables[0].keyset.numel() == 12 * H.slots(n_keys)
    assert H.slots(n_keys) == {0: 1024, 1: 1024, 512: 1024, 513: 2048, 1025: 4096}[n_keys]
    ids = [b"%d:%d:A:C" % (1 + k % 22, 1000 + k) for k in range(n_keys)] + [b"1:5:A:C", b"2:1000:A:C"]
    rng.shuffle(ids)
    export = b"".join(i + b":rs1\t" + i + b"\t\\N\n" for i in ids)
    dev = both_rows(engine, host, tables, export)
    assert dev["n"] == n_keys == int(tables[0].hit.sum()) and dev["counts"]["not_annotated"] == 2


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


# ---- 3: trips longer than the stages -----------------------------------------------------------
def test_g3_trips_longer_than_the_stages(engine, host):
    """A 40,000-byte allele in both texts (the size passes read those trips from global memory, the
    key and row writers store them from the lanes) and a LOF value of 600 groups, whose one JSON
    exceeds the write stage."""
    rng = random.Random(40)
    big = "".join(rng.choice("ACGT") for _ in range(40000))
    vcf, ids = L.fuzz_vcf(rng, 300, annotated=0.8)
    groups = ",".join("(G%d|ENSG%d|%d|0.%d)" % (k, k, k % 40, 1 + k % 99) for k in range(600))
    extra = ["3\t77\t.\t%s\tA,C\t.\t.\tAC=1;NMD=(BIG|E|1|0.5)" % big, "4\t88\t.\tA\tG\t.\t.\tAC=2;LOF=" + groups,
             "4\t89\t.\tA\t%s\t.\t.\tAC=2" % big]
    lines = vcf.rstrip(b"\n").split(b"\n")
    lines[100:100] = [x.encode() for x in extra]
    vcf = b"\n".join(lines) + b"\n"
    tables = both_tables(engine, host, vcf)
    rows = dict(L.table_rows(tables[0]))
    assert "3:77:%s:C" % big in rows and len(rows["4:88:A:G"]) > 32 * 1024
    assert rows["4:88:A:G"] == L.ref_line(extra[1].encode())[1]
    ids = ids + ["3:77:%s:A" % big, "3:77:%s:C" % big, "4:88:A:G"]
    export = L.fuzz_export(rng, ids, 400, long_allele=40000)
    export = b"".join(b"%s\t%s\n" % (i.encode(), i.encode()) for i in ids[-3:]) + export
    dev = both_rows(engine, host, tables, export)
    want, _, _ = L.ref_update(vcf, export)
    assert dev["text"].tobytes() == L.rows_text(want)
    assert int(np.diff(dev["row_off"]).max()) > 40000 and sum(len(ln) > 40000 for ln in export.split(b"\n")) >= 3


# ---- 4: a second grid-stride trip of the export pass ---------------------------------------------
def test_g4_second_grid_stride_trip(engine, host, fuzz_tables):
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
    want, _, _ = L.ref_update(vcf, tail)
    assert dev["text"][int(dev["row_off"][SIZE_GRID * TRIP]):].tobytes() == L.rows_text(want)


# ---- 5: capacity, errors -----------------------------------------------------------------------------
def test_g5_capacity_and_sentinels_on_the_device(engine, fuzz_tables):
    tables, ids, vcf = fuzz_tables
    rc, cnt, out, totals = L.raw_table_passes(engine, vcf)
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
        rc, _, out2, totals2 = L.raw_table_passes(engine, vcf, **{short + "_cap": (kb if short == "key" else jb) - 1})
        assert rc == 0 and totals2 == [kb, jb, n, 1]
        for name in ("keys", "json", "key_off", "json_off", "json_len", "line_start", "flags"):
            assert (out2[name].view(np.uint8) == 0xA5).all(), (short, name)
    export = L.fuzz_export(random.Random(5), ids, 700)
    rc, ucnt, buf, utot, cap = L.raw_update_passes(engine, export, tables[0])
    assert rc == 0 and utot == [cap, 0] and cap > 1000 and (buf[cap:] == 0xA5).all()
    rc, _, buf, utot, _ = L.raw_update_passes(engine, export, tables[0], cap=cap - 1)
    assert rc == 0 and utot == [cap, 1] and (buf == 0xA5).all()


def test_g5_errors_raise_on_the_device(engine):
    line = b"1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)\n"
    t = engine.lof_table_build(line)
    with pytest.raises(ValueError, match="line 2 of the export"):
        engine.lof_update_rows(b"a\t1:100:A:G\n1:5:A\t1:5:A\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        engine.lof_update_rows(b"a\t1:100\r:A:G\t\\N\n", t)
    with pytest.raises(AttributeError) as ei:
        engine.lof_table_build(b"#c\n" + line + b"1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=5\n")
    assert ei.value.line == 3


def test_g5_write_entry_on_an_empty_slab(engine, host):
    """avdb_lof_table_write on a zero-byte slab (no lines, so no scans and no kernels), totals and
    key_off poisoned: without rows zero totals and key_off[0] = 0; a row that nothing bears out sets
    totals[3] and leaves key_off alone, the device entry returning OK and the host entry ERANGE."""
    poison = int(np.frombuffer(b"\xA5" * 8, dtype=np.int64)[0])
    for eng, over_rc in ((engine, 0), (host, N.AVDB_ERANGE)):
        suffix, tail = L._runner(eng, "lof_table", "avdb_lof_table_workspace_size", 0, 0)
        full = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), 0xA5,  # noqa: E731
                                        dtype=torch.uint8, device=eng.device).view(dt)
        for n_rows, want_rc, want, want_off in ((0, 0, [0, 0, 0, 0], 0), (1, over_rc, [0, 0, 0, 1], poison)):
            ents = [full(1, torch.int64)] + [full(1, torch.int32) for _ in range(3)] + [full(1, torch.uint8)]
            key_off, totals = full(n_rows + 1, torch.int64), full(4, torch.int64)
            rc = L._call(eng, "avdb_lof_table_write" + suffix, None, 0, 0, 0, n_rows, *ents, full(8, torch.uint8), 0,
                         key_off, full(8, torch.uint8), 0, full(1, torch.int64), full(1, torch.int32),
                         full(1, torch.int64), full(1, torch.uint8), totals, *tail)
            assert (rc, totals.cpu().tolist(), int(key_off[0])) == (want_rc, want, want_off), (eng.host_only, n_rows)
            assert key_off.cpu().tolist()[1:] == [poison] * n_rows


# ---- 6: bgzip input ------------------------------------------------------------------------------------
def test_g6_bgzip_pair_through_read_whole(engine, host, tmp_path):
    from annotatedvdb_amd import bgzf
    g = L.golden()
    vcf_path, exp_path = tmp_path / "x.vcf.gz", tmp_path / "export.tsv.gz"
    vcf_path.write_bytes(Z.bgzip(g["vcf"], block=20000))
    exp_path.write_bytes(Z.bgzip(g["export"], block=20000))
    slab = bgzf.read_whole(str(vcf_path), engine)
    assert isinstance(slab, torch.Tensor) and slab.is_cuda and slab.numel() == len(g["vcf"])
    tables = both_tables(engine, host, g["vcf"], slab=slab)
    u = poisoned(engine, lambda: LOFUpdater(str(vcf_path), engine))
    n = poisoned(engine, lambda: u.buffer_export(str(exp_path)))
    want, _, missing = L.ref_update(g["vcf"], g["export"])
    assert n == len(want) and u.update_text() == L.rows_text(want) and u.unmatched() == missing
    both_rows(engine, host, tables, g["export"], slab=bgzf.read_whole(str(exp_path), engine))

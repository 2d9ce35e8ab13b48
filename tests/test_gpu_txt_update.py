"""K19 on the GPU: the table of a tab-delimited annotation file (Engine.txt_table_build), the update
rows from an export (Engine.txt_update_rows) and from a file of primary keys (Engine.txt_direct_rows)
against the reference's golden and against the library's host entries, array for array, with
poisoned buffers."""

import random

import numpy as np
import pytest

import hash_common as H
import txt_common as T
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.text_update import TextUpdater

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TRIP = 256           # lines of a workgroup trip (kBlock)
SIZE_GRID = 4096     # workgroups at most in a size pass: line 4096 * 256 is workgroup 0's second trip
WRITE_GRID = 2048    # and in a write pass
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


def both_tables(engine, host, text, id_type="METASEQ"):
    """The table on the device (poisoned buffers) and from the host entries: equal in every array."""
    dev = poisoned(engine, lambda: engine.txt_table_build(text, id_type))
    ref = host.txt_table_build(text, id_type)
    T.same_arrays(T.table_arrays(dev), T.table_arrays(ref), "table: device against host entries")
    assert dev.keys.is_cuda or dev.n_rows == 0
    return dev, ref


def both_rows(engine, host, tables, export, id_type="METASEQ", slab=None, **kw):
    dev_t, ref_t = tables
    dev_t.hit.zero_()
    ref_t.hit.zero_()
    dev = poisoned(engine, lambda: T.rows_arrays(engine.txt_update_rows(export if slab is None else slab, dev_t, id_type,
                                                                        **kw), N.TXTUPD_COUNTS))
    ref = T.rows_arrays(host.txt_update_rows(export, ref_t, id_type, **kw), N.TXTUPD_COUNTS)
    T.same_arrays(dev, ref, "rows: device against host entries")
    assert np.array_equal(dev_t.hit.cpu().numpy(), ref_t.hit.numpy())
    return dev


def both_direct(engine, host, text, slab=None, **kw):
    dev = poisoned(engine, lambda: T.rows_arrays(engine.txt_direct_rows(text if slab is None else slab, **kw),
                                                 N.TXTDIR_COUNTS))
    ref = T.rows_arrays(host.txt_direct_rows(text, **kw), N.TXTDIR_COUNTS)
    T.same_arrays(dev, ref, "direct rows: device against host entries")
    return dev


def counts_of(arrays, names):
    return dict(zip(names, (int(x) for x in arrays["counts"])))


@pytest.fixture(scope="module")
def fuzz_tables(engine, host):
    """Tables of 513 data lines for both looked-up columns, on both engines, with their ids and texts."""
    out = {}
    for id_type in ("METASEQ", "REFSNP"):
        text, ids = T.fuzz_file(random.Random(1919), 513, id_type, 7, 3, host=0.05)
        out[id_type] = (both_tables(engine, host, text, id_type), ids, text)
    return out


# ---- 1: the golden on the device ------------------------------------------------------------
@pytest.mark.parametrize("id_type", T.ID_TYPES)
def test_g1_golden_on_the_device(engine, id_type):
    g = T.golden()
    text = g["files"][id_type]
    host_lines, data = g["host"][id_type]
    for datasource in ("dbSNP", "ADSP"):
        adsp = datasource == "ADSP"

        def run():
            u = TextUpdater(text, id_type, datasource, engine)
            n = u.buffer_file() if id_type == "PRIMARY_KEY" else u.buffer_export(g["export"])
            return u, n
        u, n = poisoned(engine, run)
        if id_type == "PRIMARY_KEY":
            want, missing = T.ref_direct(text, adsp), []
            rows = engine.txt_direct_rows(text, adsp=adsp)
            assert rows.text.is_cuda and rows.counts["host_rows"] == host_lines
            assert rows.n - host_lines > 9 * host_lines > 0  # (rendered on the device, not all sent to the host)
        else:
            want, ctr, missing = T.ref_update(text, g["export"], id_type, adsp)
            t = u.table()
            assert t.keys.is_cuda and t.counts["host_lines"] == host_lines
            device_rows = int(((t.flags & N.TXT_LINE_HOST) == 0).sum())
            assert device_rows > 9 * (t.n_rows - device_rows) > 0
            rows = engine.txt_update_rows(g["export"], t, id_type, adsp=adsp)
            assert rows.n - rows.counts["host_rows"] > 9 * rows.counts["host_rows"] > 0
            assert T.table_rows(t) == T.ref_table(text, id_type)[0]
            assert u.get_count("not_in_file") == ctr["not_in_file"]
        assert n == len(want) and u.update_text() == T.rows_text(want)
        assert sorted(u.update_buffer(), key=repr) == sorted(T.golden_expected(id_type, datasource), key=repr)
        assert u.unmatched() == missing == g["missing"][id_type]


# ---- 2: fuzzed slabs of the three passes, device against host entries --------------------------
@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_file_slabs(engine, host, n_lines):
    for seed, id_type in ((1, "METASEQ"), (2, "REFSNP")):
        text, ids = T.fuzz_file(random.Random(1000 * n_lines + seed), n_lines, id_type)
        dev, ref = both_tables(engine, host, text, id_type)
        want, ctr = T.ref_table(text, id_type)
        assert {k: dev.counts[k] for k in ctr} == ctr and dev.n_rows == n_lines
        assert T.table_rows(dev) == want
        export = T.fuzz_export(random.Random(seed), ids, 40)
        both_rows(engine, host, (dev, ref), export, id_type, adsp=bool(seed - 1))


@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_export_slabs(engine, host, fuzz_tables, n_lines):
    for seed, id_type, kw in ((1, "METASEQ", {}), (2, "REFSNP", {"adsp": True}), (3, "METASEQ", {"contigs": ["1", "X", "GL1"]}),
                              (4, "REFSNP", {})):
        tables, ids, text = fuzz_tables[id_type]
        export = T.fuzz_export(random.Random(1000 * n_lines + seed), ids, n_lines)
        dev = both_rows(engine, host, tables, export, id_type, **kw)
        c = counts_of(dev, N.TXTUPD_COUNTS)
        assert c["rows"] + c["skipped_lines"] + c["not_in_file"] == len(T.text_lines(export))
        want, ctr, _ = T.ref_update(text, export, id_type, **kw)
        assert dev["text"].tobytes() == T.rows_text(want) and {k: c[k] for k in ctr} == ctr
        if n_lines >= 255 and not kw:
            assert min(c["rows"], c["skipped_lines"], c["not_in_file"]) > 0, c


@pytest.mark.parametrize("n_lines", SIZES)
def test_g2_fuzzed_direct_slabs(engine, host, n_lines):
    for seed, adsp in ((1, False), (2, True)):
        text, _ = T.fuzz_file(random.Random(1000 * n_lines + seed), n_lines, "PRIMARY_KEY", host=0.05)
        dev = both_direct(engine, host, text, adsp=adsp)
        assert dev["text"].tobytes() == T.rows_text(T.ref_direct(text, adsp))
        c = counts_of(dev, N.TXTDIR_COUNTS)
        assert c["rows"] == n_lines and c["rows"] + c["skipped_lines"] == c["lines"] == len(T.text_lines(text))


@pytest.mark.parametrize("n_lines", [1, 257, 1100])
def test_g2_unmatched_and_repeated_ids_are_picked_on_the_device(engine, host, n_lines):
    """TextUpdater.unmatched() and repeated_ids() probe every key in the table's own key set on the
    device and bring only the picked ids to the host: the same lists as the host engine's and the
    restatement's, in file order, for ids repeated twice and more."""
    for seed, id_type in ((1, "METASEQ"), (2, "REFSNP")):
        rng = random.Random(77 * n_lines + seed)
        text, ids = T.fuzz_file(rng, n_lines, id_type, 5, 2)
        export = T.fuzz_export(rng, ids, n_lines, hit=0.5)
        dev, ref = (TextUpdater(text, id_type, engine=e) for e in (engine, host))
        assert dev.unmatched() == ref.unmatched() == [i.decode() for i, _ in dict(T.ref_table(text, id_type)[0]).items()]
        for u in (dev, ref):
            u.buffer_export(export)
        missing = T.ref_update(text, export, id_type)[2]
        assert dev.unmatched() == ref.unmatched() == missing
        assert dev.repeated_ids() == ref.repeated_ids() == T.ref_repeated(text, id_type)
        if n_lines > 1000:
            assert len(missing) > 50 and len(dev.repeated_ids()) > 20


@pytest.mark.parametrize("n_keys", [0, 1, 512, 513, 1025])
def test_g2_table_sizes_around_the_slot_doubling(engine, host, n_keys):
    """512 keys fill 1,024 slots to a half, 513 double them, 1,025 double them again."""
    rng = random.Random(n_keys)
    text = b"variant\tgwas_flags\n" + b"".join(b"%d:%d:A:C\tv%d\n" % (1 + k % 22, 1000 + k, k) for k in range(n_keys))
    tables = both_tables(engine, host, text)
    assert tables[0].n_rows == n_keys and tables[0].keyset.numel() == 12 * H.slots(n_keys)
    assert H.slots(n_keys) == {0: 1024, 1: 1024, 512: 1024, 513: 2048, 1025: 4096}[n_keys]
    ids = [b"%d:%d:A:C" % (1 + k % 22, 1000 + k) for k in range(n_keys)] + [b"1:5:A:C", b"2:1000:A:C"]
    rng.shuffle(ids)
    export = b"".join(i + b":rs1\t" + i + b"\t\\N\n" for i in ids)
    dev = both_rows(engine, host, tables, export)
    c = counts_of(dev, N.TXTUPD_COUNTS)
    assert c["rows"] == n_keys == int(tables[0].hit.sum()) and c["not_in_file"] == 2


def test_g2_fields_and_ids_across_word_and_line_boundaries(engine, host):
    """Ids of 7 .. 70 bytes and values of 0 .. 130: fields begin and end at every byte of an 8-byte
    word and of a 64-byte line of the text, rows at every byte of a word of the output; 3,200 rows
    run the lengths' scan over several tiles and the write pass over many trips."""
    rng = random.Random(64)
    lines, ids = [b"other_annotation\tvariant\tgwas_flags"], []
    for k in range(3200):
        i = b"%d:%s:A:C" % (1 + k % 22, b"7" * (k % 63) + b"%d" % k)
        ids.append(i)
        lines.append(b"o" * rng.randint(1, 130) + b"\t" + i + b"\t" + b"g" * ((k * 7) % 67))
    text = b"\n".join(lines) + b"\n"
    starts = np.cumsum([0] + [len(x) + 1 for x in lines])
    assert {int(s) % 64 for s in starts} == set(range(64))
    tables = both_tables(engine, host, text)
    assert T.table_rows(tables[0]) == T.ref_table(text, "METASEQ")[0]
    for name in ("key_off", "json_off"):
        off = T.table_arrays(tables[0])[name]
        assert {int(x) % 8 for x in off} == set(range(8)) and len({int(x) % 64 for x in off}) == 64
    export = b"".join(b"%s:rs%d\t%s\n" % (i, rng.randint(1, 10 ** rng.randint(1, 9)), i) for i in ids)
    dev = both_rows(engine, host, tables, export, adsp=True)
    off = dev["row_off"]
    assert len(off) == 3201 and {int(x) % 8 for x in off} == set(range(8))
    assert len({int(off[k]) % 8 for k in range(0, 3200, TRIP)}) >= 4
    pk = text.replace(b"other_annotation\tvariant", b"variant\tother_annotation", 1)
    d = both_direct(engine, host, pk)  # (the first column read as primary keys: rows of every length again)
    assert {int(x) % 8 for x in d["row_off"]} == set(range(8))


# ---- 3: trips longer than the stages -----------------------------------------------------------
def test_g3_trips_longer_than_the_stages(engine, host):
    """One value of 70,000 bytes: its line is longer than a size pass's window (that trip is read
    from global memory) and its tail longer than a write trip's 64 KB at most of LDS (those trips
    are written bytewise), in the table, the update rows and the direct rows."""
    rng = random.Random(40)
    big = "".join(rng.choice("abcdefg {}\":,") for _ in range(70000)).lstrip('"')
    text, ids = T.fuzz_file(rng, 300, "METASEQ", 4, 1)
    lines = text.rstrip(b"\n").split(b"\n")
    n_cols = lines[0].count(b"\t") + 1
    lines[100:100] = [b"\t".join([b"a", b"3:77:A:C"] + [big.encode()] * (n_cols - 2))]
    text = b"\n".join(lines) + b"\n"
    tables = both_tables(engine, host, text)
    rows = dict(T.table_rows(tables[0]))
    assert len(rows[b"3:77:A:C"]) > 64 * 1024 and T.table_rows(tables[0]) == T.ref_table(text, "METASEQ")[0]
    export = b"3:77:A:C:rs1\t3:77:A:C\n" + T.fuzz_export(rng, ids, 400) + b"3:77:A:C\t3:77:A:C\trs5\n"
    dev = both_rows(engine, host, tables, export)
    want, _, _ = T.ref_update(text, export, "METASEQ")
    assert dev["text"].tobytes() == T.rows_text(want) and int(np.diff(dev["row_off"]).max()) > 70000
    d = both_direct(engine, host, text.replace(b"a\t3:77:A:C", b"a:b:c\t3:77:A:C"))
    assert int(np.diff(d["row_off"]).max()) > 70000


def test_g3_a_trip_that_all_matches_one_id_and_one_where_none_does(engine, host, fuzz_tables):
    tables, ids, text = fuzz_tables["REFSNP"]
    _, metaseq, rs = ids[7]
    hit = b"".join(b"%s:pk%d\t%s\t%s\n" % (metaseq.encode(), k, metaseq.encode(), rs.encode()) for k in range(TRIP))
    miss = b"".join(b"%s:pk%d\t%s\trs0%d\n" % (metaseq.encode(), k, metaseq.encode(), k) for k in range(TRIP))
    dev = both_rows(engine, host, tables, hit + miss + hit, "REFSNP")
    c = counts_of(dev, N.TXTUPD_COUNTS)
    assert c["rows"] == 2 * TRIP and c["not_in_file"] == TRIP and len(set(dev["match"].tolist())) == 1
    assert int(tables[0].hit.sum()) == 1
    want, _, missing = T.ref_update(text, hit + miss + hit, "REFSNP")
    assert dev["text"].tobytes() == T.rows_text(want) and len(missing) == len(set(i[0] for i in ids)) - 1


# ---- 4: a second grid-stride trip ------------------------------------------------------------------
def test_g4_second_grid_stride_trip_of_the_file_passes(engine, host):
    """One line past SIZE_GRID * 256 minimal lines: workgroup 0 comes back for the last one (and the
    write passes, WRITE_GRID workgroups, for half of them); the line there differs from the others.
    The table's entries are compared raw (no key set is built over a million equal ids)."""
    n = SIZE_GRID * TRIP
    text = b"variant\tg\n" + b"1\tx\n" * (n - 1) + b"2:7\ty"
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(engine.device)
    d = both_direct(engine, host, text, slab=slab)
    assert len(d["row_off"]) == n + 1 and d["text"][-16:].tobytes() == b"\tx\n1\tchr1\tx\n2:7\tchr2\ty\n"[-16:]
    shape = T.shape_of(text[:100])
    rc, cnt, dev, tot = T.raw_table_passes(engine, slab, shape)
    rc2, cnt2, ref, tot2 = T.raw_table_passes(host, text, shape)
    assert rc == rc2 == 0 and cnt == cnt2 and tot == tot2 == [n + 2, 2 * n + 1, n, 0]
    T.same_arrays(dev, ref, "table entries: device against host entries")
    assert dev["keys"][:n + 2].tobytes()[-4:] == b"12:7" and dev["body"][:2 * n + 1].tobytes()[-5:] == b"\tx2\ty"


def test_g4_second_grid_stride_trip_of_the_export_pass(engine, host, fuzz_tables):
    tables, ids, text = fuzz_tables["METASEQ"]
    short = sorted({i[1] for i in ids if len(i[1]) < 16})[:64]
    assert len(short) == 64
    block = b"".join(b"%s\t%s\n" % (m.encode(), m.encode()) for m in short[:16])
    tail = b"".join(b"%s:rs1\t%s\t\\N\n" % (m.encode(), m.encode()) for m in short[16:64]) * 7
    export = block * (SIZE_GRID * TRIP // 16) + tail[:-1]
    assert len(export) < 48 << 20
    slab = torch.from_numpy(np.frombuffer(export, dtype=np.uint8).copy()).to(engine.device)
    dev = both_rows(engine, host, tables, export, slab=slab)
    assert len(dev["row_off"]) - 1 == SIZE_GRID * TRIP + 48 * 7 > WRITE_GRID * TRIP
    want, _, _ = T.ref_update(text, tail, "METASEQ")
    assert dev["text"][int(dev["row_off"][SIZE_GRID * TRIP]):].tobytes() == T.rows_text(want)


# ---- 5: capacity, errors, empty inputs -----------------------------------------------------------------
def test_g5_capacity_and_sentinels_on_the_device(engine, fuzz_tables):
    tables, ids, text = fuzz_tables["METASEQ"]
    shape = T.shape_of(text)
    rc, cnt, out, totals = T.raw_table_passes(engine, text, shape)
    n, kb, bb, ne = cnt["rows"], cnt["key_bytes"], cnt["json_bytes"], cnt["entries"]
    assert rc == 0 and totals == [kb, bb, n, 0] and 300 < n < ne == 513  # (the host lines have no row yet)
    assert (out["keys"][kb:] == 0xA5).all() and (out["body"][bb:] == 0xA5).all()
    for name, size in (("flags", 1), ("body_len", 4), ("body_off", 8), ("line_start", 8)):
        assert (out[name].view(np.uint8)[size * n:] == 0xA5).all(), name
    assert (out["key_off"].view(np.uint8)[8 * (n + 1):] == 0xA5).all()
    for short in ("key", "body"):
        rc, _, out2, totals2 = T.raw_table_passes(engine, text, shape, **{short + "_cap": (kb if short == "key" else bb) - 1})
        assert rc == 0 and totals2 == [kb, bb, n, 1]
        for name in ("keys", "body", "key_off", "body_off", "body_len", "line_start", "flags"):
            assert (out2[name].view(np.uint8) == 0xA5).all(), (short, name)
    export = T.fuzz_export(random.Random(5), ids, 700)
    rc, ucnt, buf, utot = T.raw_update_passes(engine, export, tables[0])
    cap = ucnt["out_bytes"]
    assert rc == 0 and utot == [cap, 0] and cap > 1000 and (buf["text"][cap:] == 0xA5).all()
    assert (buf["row_off"].view(np.uint8)[8 * (ucnt["rows"] + 1):] == 0xA5).all()
    rc, _, buf, utot = T.raw_update_passes(engine, export, tables[0], cap=cap - 1)
    assert rc == 0 and utot == [cap, 1] and (buf["text"] == 0xA5).all()
    rc, dcnt, buf, dtot = T.raw_direct_passes(engine, text, shape, adsp=True)
    cap = dcnt["out_bytes"]
    assert rc == 0 and dtot == [cap, 0] and cap > 1000 and (buf["text"][cap:] == 0xA5).all()
    rc, _, buf, dtot = T.raw_direct_passes(engine, text, shape, adsp=True, cap=cap - 1)
    assert rc == 0 and dtot == [cap, 1] and (buf["text"] == 0xA5).all()


def test_g5_errors_raise_on_the_device(engine):
    t = engine.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\tx\n")
    with pytest.raises(ValueError, match="line 2 of the export"):
        engine.txt_update_rows(b"a\t1:5:A:C\n1:5:A\t1:5:A\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        engine.txt_update_rows(b"a\t1:5\r:A:C\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        engine.txt_direct_rows(b"variant\tgwas_flags\n1:5:A:C\tx\ry\n")
    with pytest.raises(ValueError, match="cannot carry") as ei:
        engine.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\tx\n\n1:6:A:C\t\\N\n")
    assert ei.value.line == 4
    with pytest.raises(TypeError) as ei:
        engine.txt_direct_rows(b"gwas_flags\tvariant\nx\t1:5:A:C\nx\n")
    assert ei.value.line == 3


def test_g5_empty_inputs(engine, host):
    for text in (b"variant\tgwas_flags", b"variant\tgwas_flags\n", b"variant\tgwas_flags\n\n\r\n"):
        tables = both_tables(engine, host, text)
        assert tables[0].n_rows == 0
        dev = both_rows(engine, host, tables, b"a\t1:100:A:G\t\\N\n")
        assert counts_of(dev, N.TXTUPD_COUNTS)["not_in_file"] == 1
        assert len(both_direct(engine, host, text)["row_off"]) == 1
    tables = both_tables(engine, host, b"variant\tgwas_flags\n1:5:A:C\tx")
    for export in (b"", b"record_primary_key\tmetaseq_id\n\nshort\n\r\n"):
        dev = both_rows(engine, host, tables, export)
        c = counts_of(dev, N.TXTUPD_COUNTS)
        assert c["rows"] == 0 and c["skipped_lines"] == len(T.text_lines(export)) and dev["text"].size == 0
    # the entries themselves on no lines at all (the Python surface refuses a file without a header)
    for eng in (engine, host):
        rc, cnt, out, totals = T.raw_table_passes(eng, b"", (0, 2, 0, 0))
        assert rc == 0 and totals == [0, 0, 0, 0] and cnt["lines"] == 0 and out["key_off"][0] == 0
        rc, cnt, out, totals = T.raw_direct_passes(eng, b"", (0, 2, 0, 0))
        assert rc == 0 and totals == [0, 0] and out["row_off"][0] == 0


def test_g5_write_entry_on_an_empty_slab(engine, host):
    """avdb_txt_table_write on a zero-byte slab (no lines, so no scans and no kernels), totals and
    key_off poisoned: without rows zero totals and key_off[0] = 0; a row is refused up front (an entry
    is one row, and there is none), on the device and on the host, and nothing is written."""
    from annotatedvdb_amd.slab_passes import SlabPass
    poison = int(np.frombuffer(b"\xA5" * 8, dtype=np.int64)[0])
    for eng in (engine, host):
        sp = SlabPass(eng, b"", "txt_table", "avdb_txt_table_workspace_size")
        for n_rows, want_rc, want, want_off in ((0, 0, [0, 0, 0, 0], 0), (1, N.AVDB_EINVAL, [poison] * 4, poison)):
            ents = [T.poisoned(eng, 1, dt) for dt in (torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)]
            key_off, totals = T.poisoned(eng, n_rows + 1, torch.int64), T.poisoned(eng, 4, torch.int64)
            try:
                rc = sp.call("avdb_txt_table_write", sp.tp, sp.nb, sp.n_lines, 0, n_rows, 0, 2, 0, 0, *ents,
                             T.poisoned(eng, 8, torch.uint8), 0, key_off, T.poisoned(eng, 8, torch.uint8), 0,
                             T.poisoned(eng, 1, torch.int64), T.poisoned(eng, 1, torch.int32),
                             T.poisoned(eng, 1, torch.int64), T.poisoned(eng, 1, torch.uint8), totals)
            except N.NativeError as e:
                rc = e.rc
                assert "more rows than entries" in str(e)
            assert (rc or 0, totals.cpu().tolist(), int(key_off[0])) == (want_rc, want, want_off), (eng.host_only, n_rows)


# ---- 6: bgzip input ------------------------------------------------------------------------------------
def test_g6_bgzip_pair_through_the_driver(engine, tmp_path):
    import bgzf_common as Z
    from annotatedvdb_amd import update_variant_annotation
    g = T.golden()
    path, exp_path = tmp_path / "flags.txt.gz", tmp_path / "export.tsv.gz"
    path.write_bytes(Z.bgzip(g["files"]["REFSNP"], block=20000))
    exp_path.write_bytes(Z.bgzip(g["export"], block=20000))
    got = poisoned(engine, lambda: update_variant_annotation.main(
        ["--fileName", str(path), "--variantIdType", "REFSNP", "--export", str(exp_path), "--allowMissing"], engine))
    want, ctr, missing = T.ref_update(g["files"]["REFSNP"], g["export"], "REFSNP")
    assert (tmp_path / "flags.txt.gz.updates").read_bytes() == T.rows_text(want)
    assert got["update"] == len(want) and got["missing"] == len(missing) and got["not_in_file"] == ctr["not_in_file"]

"""K19 on the host-only engine (the library's _host entries run the kernels' per-line code): the
generic annotation update against the golden the reference's own code produced
(tests/golden/make_golden_txt.py) and against the restatement of txt_common.py."""

import gzip
import os
import random

import numpy as np
import pytest

import bgzf_common as B
import txt_common as T
from annotatedvdb_amd import _native as N
from annotatedvdb_amd import update_variant_annotation
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.text_update import TextUpdater, host_line, read_file_header, read_header, update_sql


@pytest.fixture(scope="module")
def eng():
    return Engine("host")


def test_restatement_pinned_to_golden():
    g = T.golden()
    for id_type in T.ID_TYPES:
        for datasource in ("dbSNP", "ADSP"):
            adsp = datasource == "ADSP"
            want = T.golden_expected(id_type, datasource)
            if id_type == "PRIMARY_KEY":
                assert T.ref_direct(g["files"][id_type], adsp) == want
            else:
                rows, ctr, missing = T.ref_update(g["files"][id_type], g["export"], id_type, adsp)
                assert sorted(rows, key=repr) == want and len(want) > 1000
                assert missing == g["missing"][id_type]
    for case, id_type, exc, text, tuples in g["cases"]:
        if exc is None:
            got = [T.row_tuple("PK:" + look if id_type != "PRIMARY_KEY" else look, label, values, False)
                   for _, look, label, values in T.ref_records(text, id_type)]
            assert got == tuples, case


@pytest.mark.parametrize("datasource", ["dbSNP", "ADSP"])
@pytest.mark.parametrize("id_type", T.ID_TYPES)
def test_golden_end_to_end(eng, id_type, datasource):
    g = T.golden()
    adsp = datasource == "ADSP"
    u = TextUpdater(g["files"][id_type], id_type, datasource, eng)
    host, data = g["host"][id_type]
    if id_type == "PRIMARY_KEY":
        assert u.buffer_file() == data
        want = T.ref_direct(g["files"][id_type], adsp)
        assert u.unmatched() == [] and u.get_count("line") == data
    else:
        t = u.table()
        assert t.counts["host_lines"] == host and t.counts["entries"] == data and t.counts["bad"] == 0
        assert host * 10 < data
        assert T.table_rows(t) == T.ref_table(g["files"][id_type], id_type)[0]
        want, ctr, missing = T.ref_update(g["files"][id_type], g["export"], id_type, adsp)
        assert u.buffer_export(g["export"]) == len(want)
        assert u.unmatched() == missing == g["missing"][id_type]
        assert u.get_count("not_in_file") == ctr["not_in_file"] and u.get_count("line") == data
        assert len(u.repeated_ids()) > 5
    sql = {legacy: w for h, d, legacy, w in g["sql"] if h == u.header().fields and d == datasource}
    assert len(sql) == 2 and all(u.build_update_sql(useLegacyPk=legacy) == w for legacy, w in sql.items())
    assert u.update_text() == T.rows_text(want)
    assert u.update_buffer(sizeOnly=True) == len(want) == u.get_count("update")
    assert u.update_buffer() == want
    assert sorted(u.update_buffer(), key=repr) == sorted(T.golden_expected(id_type, datasource), key=repr)
    u.reset_update_buffer()
    assert u.update_buffer() == [] and u.update_text() == b""


def test_update_sql_text_is_the_references(eng):
    """Every statement the reference's own build_update_sql produced for the golden (the three
    files' headers, one with bin_index and plain columns, dbSNP / ADSP, useLegacyPk off / on)."""
    g = T.golden()
    assert len(g["sql"]) == 20 and {tuple(h) for h, _, _, _ in g["sql"]} >= {
        tuple(read_header(g["files"][t][:4096], t).fields) for t in T.ID_TYPES}
    for header, datasource, legacy, want in g["sql"]:
        id_type = "REFSNP" if "ref_snp_id" in header else "METASEQ"
        u = TextUpdater(("\t".join(header) + "\n").encode(), id_type, datasource, eng)
        assert u.build_update_sql(useLegacyPk=legacy) == want, (header, datasource, legacy)
        assert update_sql([h for h in header if h != "variant"], datasource == "ADSP", legacy) == want
    kinds = "".join(w for _, _, _, w in g["sql"])
    assert "::ltree" in kinds and "jsonb_merge" in kinds and "Public.Variant" in kinds and "position = d.position" in kinds


@pytest.mark.parametrize("case,id_type,exc,text,tuples", T.golden()["cases"], ids=[c[0] for c in T.golden()["cases"]])
def test_cases(eng, case, id_type, exc, text, tuples):
    if exc == "KeyError":  # a REFSNP file without the ref_snp_id column: refused at the header
        with pytest.raises(ValueError, match="ref_snp_id"):
            TextUpdater(text, id_type, engine=eng)
        return
    if exc is not None:
        with pytest.raises(Exception) as ei:
            TextUpdater(text, id_type, engine=eng)
        assert type(ei.value).__name__ == exc and ei.value.line == 2
        return
    u = TextUpdater(text, id_type, engine=eng)
    if id_type == "PRIMARY_KEY":
        u.buffer_file()
    else:
        look = tuples[0][0][3:]
        if id_type == "METASEQ" and look.count(":") != 3:  # no metaseq id an export could hold: the table row
            assert T.table_rows(u.table()) == [(look.encode(), b"\t" + T.rows_text([tuples[0][2:]])[:-1])]
            return
        u.buffer_export(("PK:%s\t1:1:A:C\t%s\n" % (look, look) if id_type == "REFSNP" else
                         "PK:%s\t%s\t\\N\n" % (look, look)).encode("utf-8"))
    assert u.update_buffer() == tuples


HOST_CASES = {"quoted", "quoted_null", "doubled_quote", "non_ascii", "variant_missing"}


def test_device_subset(eng):
    """Which one-line cases the per-line code renders itself, and which it leaves to Python."""
    for case, id_type, exc, text, tuples in T.golden()["cases"]:
        if exc == "KeyError":
            continue
        rc, cnt, out, totals = T.raw_table_passes(eng, text, T.shape_of(text, "METASEQ" if id_type == "PRIMARY_KEY" else id_type))
        assert rc == 0 and cnt["entries"] == 1 and cnt["skipped_lines"] == 1
        assert (cnt["host_lines"] == 1) == (case in HOST_CASES), case
        assert cnt["bad"] == (case == "variant_missing") and cnt["rows"] == (case not in HOST_CASES)


@pytest.mark.parametrize("seed,id_type,n,n_exp,n_cols,id_pos", [
    (1, "METASEQ", 0, 5, 2, 0), (2, "METASEQ", 1, 1, 2, 1), (3, "REFSNP", 65, 64, 3, 1), (4, "METASEQ", 300, 257, 32, 31),
    (5, "REFSNP", 513, 700, 32, 0), (6, "METASEQ", 257, 300, 17, 8), (7, "REFSNP", 100, 100, None, None),
    (8, "METASEQ", 100, 100, None, None)])
def test_fuzz_table_and_update_against_restatement(eng, seed, id_type, n, n_exp, n_cols, id_pos):
    rng = random.Random(seed)
    text, ids = T.fuzz_file(rng, n, id_type, n_cols, id_pos)
    export = T.fuzz_export(rng, ids, n_exp)
    want_t, ctr_t = T.ref_table(text, id_type)
    t = eng.txt_table_build(text, id_type)
    assert T.table_rows(t) == want_t
    assert {k: t.counts[k] for k in ctr_t} == ctr_t
    assert t.counts["key_bytes"] == t.keys.numel() and t.counts["json_bytes"] == t.json.numel()
    for adsp, contigs in ((False, None), (True, None), (False, ["1", "X"])):
        want, ctr, missing = T.ref_update(text, export, id_type, adsp, contigs)
        t.hit.zero_()
        rows = eng.txt_update_rows(export, t, id_type, adsp=adsp, contigs=contigs)
        assert rows.text.numpy().tobytes() == T.rows_text(want)
        assert {k: rows.counts[k] for k in ctr} == ctr
        u = TextUpdater(text, id_type, "ADSP" if adsp else "dbSNP", eng)
        u.buffer_export(export, contigs=contigs)
        assert u.update_buffer() == want and u.unmatched() == missing
        assert u.repeated_ids() == T.ref_repeated(text, id_type)


@pytest.mark.parametrize("seed,n,n_cols,id_pos", [(1, 0, 2, 0), (2, 1, 2, 1), (3, 65, 5, 2), (4, 300, 32, 31),
                                                  (5, 513, 32, 0), (6, 200, None, None)])
def test_fuzz_direct_against_restatement(eng, seed, n, n_cols, id_pos):
    rng = random.Random(100 + seed)
    text, ids = T.fuzz_file(rng, n, "PRIMARY_KEY", n_cols, id_pos, host=0.05)
    for adsp in (False, True):
        want = T.ref_direct(text, adsp)
        rows = eng.txt_direct_rows(text, adsp=adsp)
        assert rows.text.numpy().tobytes() == T.rows_text(want) and rows.n == len(want) == n
        assert rows.counts["skipped_lines"] == len(T.text_lines(text)) - n


def test_last_line_of_an_id_wins_and_every_primary_key(eng):
    text = b"variant\tgwas_flags\nrs7\tFIRST\n2:7:C:T\tx\nrs7\tLAST\n"
    export = b"1:100:A:G:rs7\t1:100:A:G\trs7\n1:101:A:G:rs7\t1:101:A:G\trs7\r\n3:1:A:C\t3:1:A:C\t\\N\n"
    with pytest.raises(ValueError, match="ref_snp_id"):
        eng.txt_table_build(text, "REFSNP")
    text = text.replace(b"variant\t", b"ref_snp_id\tvariant\t").replace(b"rs7\t", b"rs7\trs7\t").replace(b"2:7", b"rs8\t2:7")
    t = eng.txt_table_build(text, "REFSNP")
    rows = eng.txt_update_rows(export, t, "REFSNP")
    assert rows.text.numpy().tobytes() == b"1:100:A:G:rs7\tchr1\trs7\tLAST\n1:101:A:G:rs7\tchr1\trs7\tLAST\n"
    assert rows.match.tolist() == [2, 2] and t.hit.tolist() == [0, 0, 1] and rows.counts["not_in_file"] == 1
    u = TextUpdater(text, "REFSNP", engine=eng)
    u.buffer_export(export)
    assert u.unmatched() == ["rs8"] and u.repeated_ids() == ["rs7"]


def test_value_errors(eng):
    for head, id_type, what in ((b"gwas_flags\tposition\n", "METASEQ", "no column 'variant'"),
                                (b"variant\n", "METASEQ", "no column to update"),
                                (b"\nvariant\tgwas_flags\n", "METASEQ", "no column 'variant'"),
                                (b"", "METASEQ", "empty file"),
                                (b"variant\t" + b"\t".join(b"c%d" % i for i in range(32)) + b"\n", "METASEQ", "33 columns"),
                                (b"variant\tx\tx\n", "METASEQ", "twice"),
                                (b"variant\tgwas_flags\n", "REFSNP", "ref_snp_id"),
                                (b"variant\tgwas_flags\n", "RSID", "variant id type")):
        with pytest.raises(ValueError, match=what):
            TextUpdater(head, id_type, engine=eng)
    assert len(read_header(b"variant\t" + b"\t".join(b"c%d" % i for i in range(31)) + b"\n").fields) == 32
    with pytest.raises(ValueError, match="cannot carry") as ei:
        eng.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\tx\n1:6:A:C\t\\N\n")
    assert ei.value.line == 3
    with pytest.raises(ValueError, match="cannot carry") as ei:
        eng.txt_direct_rows(b"variant\tgwas_flags\n\n1:6:A:C\t\\N\n")
    assert ei.value.line == 3
    with pytest.raises(ValueError, match="to look the row up by"):
        eng.txt_table_build(b"variant\tgwas_flags\n\tx\n")
    with pytest.raises(ValueError, match="carriage return"):
        eng.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\tx\ry\n")
    with pytest.raises(ValueError, match="carriage return"):
        eng.txt_direct_rows(b"variant\tgwas_flags\n1:5:A:C\tx\r")
    with pytest.raises(UnicodeDecodeError):
        eng.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\t\xff\n")
    t = eng.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\tx\n")
    with pytest.raises(ValueError, match="line 2 of the export"):
        eng.txt_update_rows(b"a\t1:5:A:C\n1:5:A\t1:5:A\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        eng.txt_update_rows(b"a\t1:5\r:A:C\n", t)
    with pytest.raises(ValueError, match="id_type"):
        eng.txt_update_rows(b"", t, "PRIMARY_KEY")
    u = TextUpdater(b"variant\tgwas_flags\n1:5:A:C\tx\n", "PRIMARY_KEY", engine=eng)
    with pytest.raises(ValueError, match="buffer_file"):
        u.buffer_export(b"")
    with pytest.raises(ValueError, match="buffer_export"):
        TextUpdater(b"variant\tgwas_flags\n1:5:A:C\tx\n", "METASEQ", engine=eng).buffer_file()
    assert host_line(b"1:5:A:C\t\"NULL\"\r", read_header(b"variant\tx\n")) == (b"1:5:A:C", b"1", b"\\N")


def test_empty_inputs(eng):
    for text in (b"variant\tgwas_flags", b"variant\tgwas_flags\n", b"variant\tgwas_flags\n\n\r\n"):
        t = eng.txt_table_build(text)
        assert t.n_rows == 0 and t.key_off.tolist() == [0]
        rows = eng.txt_update_rows(b"a\t1:100:A:G\t\\N\n", t)
        assert rows.n == 0 and rows.counts["not_in_file"] == 1
        assert eng.txt_direct_rows(text).n == 0
    t = eng.txt_table_build(b"variant\tgwas_flags\n1:5:A:C\tx")
    assert eng.txt_update_rows(b"", t).n == 0
    rows = eng.txt_update_rows(b"record_primary_key\tmetaseq_id\n\nshort\n", t)
    assert rows.n == 0 and rows.counts["skipped_lines"] == 3 and rows.text.numel() == 0


def test_argument_checks(eng):
    text = np.frombuffer(b"variant\tg\n1:5:A:C\tx\n", dtype=np.uint8).copy()
    nb, nl = len(text), 2
    i64, i32, u8 = (lambda: np.zeros(4, np.int64)), (lambda: np.zeros(4, np.int32)), (lambda: np.zeros(64, np.uint8))
    ents = [i64(), i32(), i32(), i32(), u8()]
    counts = np.zeros(16, np.int64)

    def bad(entry, *args, match):
        with pytest.raises(N.NativeError, match=match) as ei:
            eng._call(entry, *args)
        assert ei.value.rc == N.AVDB_EINVAL

    shape_ok = (1, 2, 0, 0)
    for shape, what in (((1, 1, 0, 0), "n_fields"), ((1, 33, 0, 0), "n_fields"), ((1, 2, 2, 0), "id_col"),
                        ((1, 2, 0, 2), "key_col")):
        bad("avdb_txt_table_size_host", text, nb, nl, *shape, *ents, counts, match=what)
        bad("avdb_txt_table_write_host", text, nb, nl, 1, 1, *shape, *ents, u8(), 8, i64(), u8(), 8, i64(), i32(), i64(),
            u8(), i64(), match=what)
        if what != "key_col":
            bad("avdb_txt_direct_size_host", text, nb, nl, *shape[:3], 0, i64(), i32(), u8(), counts, match=what)
            bad("avdb_txt_direct_write_host", text, nb, nl, 1, *shape[:3], 0, i64(), i32(), u8(), u8(), 8, i64(), i64(),
                match=what)
    bad("avdb_txt_table_size_host", None, nb, nl, *shape_ok, *ents, counts, match="null text")
    bad("avdb_txt_table_size_host", text, nb, nl, *shape_ok, *ents, None, match="null argument")
    bad("avdb_txt_table_size_host", text, nb, nl, *shape_ok, None, *ents[1:], counts, match="null output array")
    bad("avdb_txt_table_size_host", text, nb, nb + 1, *shape_ok, *ents, counts, match="more lines")
    wr = [u8(), 8, i64(), u8(), 8, i64(), i32(), i64(), u8(), i64()]
    bad("avdb_txt_table_write_host", text, nb, nl, 1, 1, *shape_ok, *ents, *wr[:-1], None, match="null argument")
    bad("avdb_txt_table_write_host", text, nb, nl, 1, 1, *shape_ok, *ents[:4], None, *wr, match="null entry array")
    bad("avdb_txt_table_write_host", text, nb, nl, 1, 1, *shape_ok, *ents, *wr[:5], None, *wr[6:], match="null row array")
    bad("avdb_txt_table_write_host", text, nb, nl, 3, 1, *shape_ok, *ents, *wr, match="out of range")
    bad("avdb_txt_table_write_host", text, nb, nl, 1, 2, *shape_ok, *ents, *wr, match="more rows than entries")
    odd = u8()[1:]
    bad("avdb_txt_table_write_host", text, nb, nl, 1, 1, *shape_ok, *ents, odd, *wr[1:], match="8-byte aligned")
    bad("avdb_txt_table_write_host", text, nb, nl, 1, 1, *shape_ok, *ents, None, *wr[1:], match="null output")
    bad("avdb_txt_direct_size_host", text, nb, nl, 1, 2, 0, 0, None, i32(), u8(), counts, match="null output array")
    bad("avdb_txt_direct_write_host", text, nb, nl, 1, 1, 2, 0, 0, i64(), i32(), u8(), odd, 8, i64(), i64(),
        match="8-byte aligned")
    bad("avdb_txt_direct_write_host", text, nb, nl, 1, 1, 2, 0, 0, i64(), i32(), u8(), u8(), 8, None, i64(),
        match="null argument")
    t = eng.txt_table_build(text.tobytes())
    import ctypes
    view = t.view()
    vp = ctypes.byref(view)
    cols = [i64(), i32(), i32(), i32(), u8()]
    bad("avdb_txt_update_size_host", text, nb, nl, None, 0xFFFFFFFF, 1, 0, *cols, counts, match="null table")
    bad("avdb_txt_update_size_host", text, nb, nl, vp, 0xFFFFFFFF, 0, 0, *cols, counts, match="key_col")
    bad("avdb_txt_update_size_host", text, nb, nl, vp, 0xFFFFFFFF, 3, 0, *cols, counts, match="key_col")
    bad("avdb_txt_update_size_host", text, nb, nl, vp, 0xFFFFFFFF, 1, 0, *cols[:4], None, counts, match="null output array")
    bad("avdb_txt_update_write_host", text, nb, nl, 1, vp, 0, *cols, odd, 8, i64(), i64(), match="8-byte aligned")
    bad("avdb_txt_update_write_host", text, nb, nl, 3, vp, 0, *cols, u8(), 8, i64(), i64(), match="out of range")
    small = N.TxtTableView(1, *([1] * 3), 0, 1, 1, 1, 1, 1, 1)
    bad("avdb_txt_update_size_host", text, nb, nl, ctypes.byref(small), 0xFFFFFFFF, 1, 0, *cols, counts,
        match="key set smaller")
    small.struct_size = 8
    bad("avdb_txt_update_size_host", text, nb, nl, ctypes.byref(small), 0xFFFFFFFF, 1, 0, *cols, counts,
        match="another size")
    for name in ("table", "update", "direct"):
        assert N.size(f"avdb_txt_{name}_workspace_size", 100, 3) >= 256
        assert N.symbol(f"avdb_txt_{name}_workspace_size")(100, 3, None) == N.AVDB_EINVAL


def test_short_workspace_is_refused_before_anything_runs(eng):
    """The device entries check their workspace first: absent, one byte short and misaligned ones
    are AVDB_ERANGE (no device is touched)."""
    import ctypes
    text = np.frombuffer(b"variant\tg\n1:5:A:C\tx\n", dtype=np.uint8).copy()
    nb, nl = len(text), 2
    i64, i32, u8 = (lambda: np.zeros(4, np.int64)), (lambda: np.zeros(4, np.int32)), (lambda: np.zeros(64, np.uint8))
    ents, counts = [i64(), i32(), i32(), i32(), u8()], np.zeros(16, np.int64)
    t = eng.txt_table_build(text.tobytes())
    view = t.view()
    vp = ctypes.byref(view)
    calls = {
        "table": [("avdb_txt_table_size", (text, nb, nl, 1, 2, 0, 0, *ents, counts)),
                  ("avdb_txt_table_write", (text, nb, nl, 1, 1, 1, 2, 0, 0, *ents, u8(), 8, i64(), u8(), 8, i64(), i32(),
                                            i64(), u8(), i64()))],
        "update": [("avdb_txt_update_size", (text, nb, nl, vp, 0xFFFFFFFF, 1, 0, *ents, counts)),
                   ("avdb_txt_update_write", (text, nb, nl, 1, vp, 0, *ents, u8(), 8, i64(), i64()))],
        "direct": [("avdb_txt_direct_size", (text, nb, nl, 1, 2, 0, 0, i64(), i32(), u8(), counts)),
                   ("avdb_txt_direct_write", (text, nb, nl, 1, 1, 2, 0, 0, i64(), i32(), u8(), u8(), 8, i64(), i64()))],
    }
    for name, entries in calls.items():
        need = N.size(f"avdb_txt_{name}_workspace_size", nb, nl)
        raw = np.zeros(need + 512, np.uint8)
        at = (-raw.ctypes.data) % 256
        for entry, args in entries:
            for ws, size in ((None, 0), (raw[at:], need - 1), (raw[at + 8:], need)):
                with pytest.raises(N.NativeError, match="256-byte aligned workspace") as ei:
                    N.call(entry, eng.ctx, *args, ws, size, None)
                assert ei.value.rc == N.AVDB_ERANGE, entry


def test_capacity_one_byte_short(eng):
    rng = random.Random(7)
    text, ids = T.fuzz_file(rng, 200, "METASEQ", 6, 2, host=0.0)
    export = T.fuzz_export(rng, ids, 300)
    shape = T.shape_of(text)
    rc, cnt, out, totals = T.raw_table_passes(eng, text, shape)
    n, kb, bb = cnt["rows"], cnt["key_bytes"], cnt["json_bytes"]
    assert rc == 0 and totals == [kb, bb, n, 0] and n == 200
    assert (out["keys"][kb:] == 0xA5).all() and (out["body"][bb:] == 0xA5).all() and (out["flags"][n:] == 0xA5).all()
    assert (out["key_off"].view(np.uint8)[8 * (n + 1):] == 0xA5).all() and out["key_off"][n] == kb
    for short in ("key", "body"):
        rc, _, out2, totals2 = T.raw_table_passes(eng, text, shape, **{short + "_cap": (kb if short == "key" else bb) - 1})
        assert rc == N.AVDB_ERANGE and totals2 == [kb, bb, n, 1]
        for name in ("keys", "body", "key_off", "body_off", "body_len", "line_start", "flags"):
            assert (out2[name].view(np.uint8) == 0xA5).all(), (short, name)
    t = eng.txt_table_build(text)
    rc, ucnt, buf, utot = T.raw_update_passes(eng, export, t)
    cap = ucnt["out_bytes"]
    assert rc == 0 and utot == [cap, 0] and cap > 0 and (buf["text"][cap:] == 0xA5).all()
    rc, _, buf, utot = T.raw_update_passes(eng, export, t, cap=cap - 1)
    assert rc == N.AVDB_ERANGE and utot == [cap, 1] and (buf["text"] == 0xA5).all()
    rc, dcnt, buf, dtot = T.raw_direct_passes(eng, text, shape)
    cap = dcnt["out_bytes"]
    assert rc == 0 and dtot == [cap, 0] and (buf["text"][cap:] == 0xA5).all()
    rc, _, buf, dtot = T.raw_direct_passes(eng, text, shape, cap=cap - 1)
    assert rc == N.AVDB_ERANGE and dtot == [cap, 1] and (buf["text"] == 0xA5).all()


def test_driver(eng, tmp_path):
    g = T.golden()
    exp_path = str(tmp_path / "export.tsv.gz")
    with open(exp_path, "wb") as fh:
        fh.write(B.bgzip(g["export"], block=3000))
    for id_type, pack in (("METASEQ", lambda b: B.bgzip(b, block=4000)), ("REFSNP", gzip.compress)):
        path = str(tmp_path / (id_type + ".txt.gz"))
        with open(path, "wb") as fh:
            fh.write(pack(g["files"][id_type]))
        argv = ["--fileName", path, "--variantIdType", id_type, "--export", exp_path, "--datasource", "ADSP"]
        assert update_variant_annotation.cli(argv, eng) == 1
        want, ctr, missing = T.ref_update(g["files"][id_type], g["export"], id_type, True)
        assert open(path + ".unmatched").read().split("\n")[:-1] == missing and not os.path.exists(path + ".updates")
        out = str(tmp_path / ("out_" + id_type))
        assert update_variant_annotation.cli(argv + ["--allowMissing", "--outDir", out], eng) == 0
        base = os.path.join(out, os.path.basename(path))
        assert open(base + ".updates", "rb").read() == T.rows_text(want)
        assert open(base + ".update.sql").read() == TextUpdater(g["files"][id_type], id_type, "ADSP", eng).build_update_sql() + "\n"
        want1, _, _ = T.ref_update(g["files"][id_type], g["export"], id_type, False, ["1", "M"])
        got = update_variant_annotation.main(["--fileName", path, "--variantIdType", id_type, "--export", exp_path,
                                              "--allowMissing", "--outDir", out, "--existingContigs", "chr1,M"], eng)
        assert open(base + ".updates", "rb").read() == T.rows_text(want1) and got["update"] == len(want1)
    plain = str(tmp_path / "pk.txt")
    with open(plain, "wb") as fh:
        fh.write(g["files"]["PRIMARY_KEY"])
    assert update_variant_annotation.cli(["--fileName", plain, "--variantIdType", "PRIMARY_KEY"], eng) == 0
    assert open(plain + ".updates", "rb").read() == T.rows_text(T.ref_direct(g["files"]["PRIMARY_KEY"]))
    assert not os.path.exists(plain + ".unmatched")
    with open(plain, "wb") as fh:
        fh.write(b"variant\tgwas_flags\tnot_a_column\tnor_this\n1:5:A:C\tx\ty\tz\n")
    with pytest.raises(ValueError, match="not_a_column, nor_this"):
        update_variant_annotation.main(["--fileName", plain, "--variantIdType", "PRIMARY_KEY"], eng)
    # the header is checked from the file's first bytes, before the file is read whole: what
    # follows them may be anything (here a gzip stream cut short)
    cut = str(tmp_path / "cut.txt.gz")
    with open(cut, "wb") as fh:
        fh.write(gzip.compress(b"variant\tnot_a_column\n" + os.urandom(200000))[:-5000])
    with pytest.raises(ValueError, match="not_a_column"):
        update_variant_annotation.main(["--fileName", cut, "--variantIdType", "PRIMARY_KEY"], eng)
    for pack in (bytes, gzip.compress, lambda b: B.bgzip(b, block=3000)):
        with open(cut, "wb") as fh:
            fh.write(pack(g["files"]["REFSNP"]))
        assert read_file_header(cut, "REFSNP") == read_header(g["files"]["REFSNP"][:4096], "REFSNP")
    with pytest.raises(SystemExit):
        update_variant_annotation.main(["--fileName", plain, "--variantIdType", "METASEQ"], eng)

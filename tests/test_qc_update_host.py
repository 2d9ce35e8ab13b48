"""K17 on the host-only engine (the library's _host entries run the kernels' per-line code): the
ADSP QC table and the update rows against the golden the reference's own code produced
(tests/golden/make_golden_qc.py) and against the restatement of qc_common.py."""

import json
import random

import numpy as np
import pytest

import bgzf_common as B
import qc_common as Q
from annotatedvdb_amd import _native as N
from annotatedvdb_amd import update_from_qc_pvcf_file
from annotatedvdb_amd.adsp_qc import QCUpdater, qc_line
from annotatedvdb_amd.engine import Engine

REL = "17k"
BASE = b"1\t100\t.\tA\tG\t50\tPASS\t%s\tGT:DP"


@pytest.fixture(scope="module")
def eng():
    return Engine("host")


@pytest.fixture(scope="module")
def golden_table(eng):
    g = Q.golden()
    return eng.qc_table_build(g["vcf"], g["version"])


def dedup(tuples):
    """The reference appends a hit's tuple once per ALT allele of the line: the set is what an
    UPDATE ... FROM (VALUES ...) means."""
    return sorted(set(tuples), key=lambda t: (t[0], t[1], t[2] is True, t[3]))


def test_restatement_pinned_to_golden():
    g = Q.golden()
    assert g["version"].lower() == REL
    for mode in (0, 1):
        rows, ctr, missing = Q.ref_update(g["vcf"], g["export"], REL, update_existing=bool(mode))
        assert dedup(rows) == dedup(g["tuples"][mode]) and len(rows) == len(set(rows))
        assert sorted(missing) == sorted(g["missing"])
    assert len(g["tuples"][1]) > len(g["tuples"][0]) > 500 and g["skipped"][0] > 0 == g["skipped"][1]
    for case, exc, line, ids, flag, js in g["cases"]:
        if exc is None:
            assert Q.ref_line(line, REL) == (ids, js, flag), case
        else:
            with pytest.raises(Exception) as ei:
                Q.ref_line(line, REL)
            assert type(ei.value).__name__ == exc, case
    raised = {c[1] for c in g["cases"]}
    assert {"IndexError", "ImportError", "ValueError", "AttributeError", "TypeError"} <= raised


def test_golden_table(eng, golden_table):
    g = Q.golden()
    want, ctr = Q.ref_table(g["vcf"], REL)
    t = golden_table
    assert Q.table_tuples(t) == [(i, js, flag) for i, js, flag, _ in want]
    for name in ("lines", "comment_lines", "rows"):
        assert t.counts[name] == ctr[name], name
    assert t.counts["entries"] == g["data_lines"] and t.counts["bad"] == 0
    # the share of the lines the per-line code renders is what the generator set: not everything goes to the host
    assert t.counts["host_lines"] == g["host_lines"] and 0 < 10 * g["host_lines"] <= g["data_lines"]
    first = t.flags.numpy() & N.QC_ROW_FIRST != 0
    assert first.sum() == g["data_lines"]
    assert ((t.flags.numpy()[first] & N.QC_LINE_HOST) != 0).sum() == g["host_lines"]
    starts = t.line_start.numpy()
    lines = Q.text_lines(g["vcf"])
    offs = np.cumsum([0] + [len(x) + 1 for x in lines])
    assert [int(s) for s in starts] == [int(offs[no]) for _, _, _, no in want]
    assert t.counts["key_bytes"] == t.keys.numel() and t.counts["json_bytes"] == t.json.numel()
    assert t.counts["pass"] == sum(1 for x in lines if not x.startswith(b"#") and x.split(b"\t")[6] == b"PASS")


@pytest.mark.parametrize("mode", [0, 1])
def test_golden_update_rows(eng, golden_table, mode):
    g = Q.golden()
    rows, ctr, missing = Q.ref_update(g["vcf"], g["export"], REL, update_existing=bool(mode))
    u = QCUpdater(golden_table)
    golden_table.hit.zero_()
    assert u.buffer_export(g["export"], update_existing=bool(mode)) == len(rows)
    assert u.update_text() == Q.rows_text(rows)
    assert u.update_buffer() == rows and dedup(u.update_buffer()) == dedup(g["tuples"][mode])
    assert u.update_buffer(sizeOnly=True) == len(rows)
    for name in ("skipped", "not_in_vcf"):
        assert u.get_count(name) == ctr[name], name
    assert u.get_count("update") == ctr["rows"] and u.get_count("line") == g["data_lines"]
    assert u.unmatched() == missing and sorted(missing) == sorted(g["missing"])
    novel = u.novel_lines()
    assert novel and len(novel) == len(set(novel))
    held = [i for ln in novel for i in Q.ref_line(ln, REL)[0]]
    assert set(missing) <= set(held)
    u.reset_update_buffer()
    assert u.update_buffer() == [] and u.update_text() == b""


CASES = Q.golden()["cases"]


@pytest.mark.parametrize("case,exc,line,ids,flag,js", CASES, ids=[c[0] for c in CASES])
def test_cases(eng, case, exc, line, ids, flag, js):
    """Every one-line case, the to_numeric edge values among them (value_NN, qual_value_NN): through
    qc_line and through the host entries, rendered as the reference renders it or raised as it raises."""
    text = b"#h\n1\t5\t.\tA\tC\t.\t.\tAC=1\tGT\n" + line
    if exc is None:
        t = eng.qc_table_build(text, "17K")
        assert Q.table_tuples(t)[1:] == [(i, js, flag) for i in ids]
        assert qc_line(line, REL) == ([i.encode() for i in ids], js.encode(), flag is True)
    else:
        with pytest.raises(Exception) as ei:
            eng.qc_table_build(text, "17K")
        assert type(ei.value).__name__ == exc and ei.value.line == 3
        with pytest.raises(Exception) as ei:
            qc_line(line, REL)
        assert type(ei.value).__name__ == exc


# the cases the per-line code renders itself; every other one is flagged HOST (value_NN: by the number rules)
DEVICE_CASES = {"plain", "multi_alt", "sample_columns", "nine_fields_exactly", "chr_prefix", "mt", "pos_leading_zero",
                "rs_id", "alt_star", "info_dot", "filter_lower_pass", "filter_hash", "qual_float", "qual_negative",
                "format_number", "flag_only", "trailing_semicolon", "double_semicolon", "equals_in_value", "empty_key",
                "hash", "trailing_blanks"}
DEVICE_VALUES = {"5", "-5", "007", "-007", "0", "-0", "-00", "0.0", "-0.0", "0.00", "-.0", ".5", "5.", "-5.", ".",
                 "0.00001", "0.0001", "-0.00001", "0.000012345", "123456789012345", "1234567890123456",
                 "0.123456789012345", "123456789012345.0", "1000000000000000.0", "10000000000000000.0",
                 "100000000000000000000.0", "0.000000000000000000001", "123456789012345678901234567890",
                 "-123456789012345678901234567890", "00000000000000000001.5", "1.50000000000000000000", "PASS", "1,2",
                 "0x1F", "A#B"}


def test_device_subset(eng):
    """Which one-line cases the per-line code renders itself, and which it leaves to Python: a case it
    renders is rendered as the reference renders it (test_cases), every other one is flagged HOST."""
    seen = set()
    for case, exc, line, ids, flag, js in CASES:
        rc, cnt, out, totals = Q.raw_table_passes(eng, line, release=REL.encode())
        assert rc == 0 and cnt["entries"] == 1, case
        inside = cnt["host_lines"] == 0 and cnt["rows"] == len(ids)
        if case.startswith(("value_", "qual_value_")):
            f = line.split(b"\t")
            v = (f[7][2:] if case.startswith("value_") else f[5]).decode()
            assert inside == (v in DEVICE_VALUES), (case, v, cnt)
            seen.add(v)
        else:
            assert inside == (case in DEVICE_CASES), (case, cnt)
        assert exc is None or not inside, case
        assert cnt["bad"] == (1 if case in ("eight_fields", "empty_line") else 0)
        if inside:
            n = cnt["json_bytes"]
            assert out["json"][:n].tobytes().decode() == js and (out["json"][n:] == 0xA5).all(), case
            assert cnt["pass"] == (1 if flag else 0)
    assert DEVICE_VALUES <= seen


def test_signed_numbers(eng):
    """The signed front of number_plain, value by value against json.dumps(to_numeric(v))."""
    rng = random.Random(3)
    values = ["-" * rng.randint(0, 1) + "0" * rng.choice((0, 0, 1, 3)) + str(rng.randint(0, 10 ** rng.randint(1, 15))) +
              rng.choice(("", ".", ".0", ".%0*d" % (rng.randint(1, 8), rng.randint(0, 999)))) for _ in range(300)]
    values += ["-" * (k % 2) + "0." + "0" * k + "125" for k in range(0, 24)] + ["1" + "0" * k + ".0" for k in range(0, 30)]
    values += ["." + "0" * k + "5" for k in range(0, 12)] + ["9" * k for k in range(1, 41)]
    text = b"\n".join(BASE % ("V=" + v).encode() for v in values) + b"\n"
    t = eng.qc_table_build(text, "r1")
    assert t.counts["host_lines"] < len(values) // 3  # (the texts of more than 15 significant digits)
    for v, (_, js, _) in zip(values, Q.table_tuples(t)):
        assert js == json.dumps({"r1": {"info": {"V": Q.to_numeric(v)}, "filter": "PASS", "qual": 50,
                                        "format": "GT:DP"}}), v
    rc, cnt, out, totals = Q.raw_table_passes(eng, text)
    dev = [i for i, f in enumerate(out["ent_4"][:len(values)]) if not f & N.QC_LINE_HOST]
    assert len(dev) == len(values) - t.counts["host_lines"]
    for i in dev:  # what the device keeps is what the rules name: at most 15 significant digits, or an integer
        digits = values[i].lstrip("-").replace(".", "").strip("0")
        assert len(digits) <= 15 or "." not in values[i], values[i]


def test_last_record_of_an_id_wins_and_both_primary_keys(eng):
    vcf = BASE % b"AC=1" + b"\n2\t7\t.\tC\tT\t.\t.\tAC=9\tGT\n" + (BASE % b"AC=2").replace(b"PASS", b"LowQual") + b"\n"
    export = b"1:100:A:G:rs1\t1:100:A:G\t\\N\n1:100:A:G:rs2\t1:100:A:G\n3:1:A:C\t3:1:A:C\t\\N\n"
    t = eng.qc_table_build(vcf, "R1")
    rows = eng.qc_update_rows(export, t)
    text = rows.text.numpy().tobytes().decode()
    assert text.count('"AC": 2') == 2 and '"AC": 1' not in text and text.count("\t\\N\t") == 2
    assert [r.split("\t")[0] for r in text.splitlines()] == ["1:100:A:G:rs1", "1:100:A:G:rs2"]
    assert rows.match.tolist() == [2, 2] and t.hit.tolist() == [0, 0, 1]
    assert rows.counts["not_in_vcf"] == 1 and rows.counts["rows"] == 2
    u = QCUpdater(t)
    assert u.unmatched() == ["2:7:C:T"] and u.novel_lines() == [b"2\t7\t.\tC\tT\t.\t.\tAC=9\tGT"]
    assert u.get_datasource() == "r1"


def test_depth_one_key(eng):
    """The release nested at depth 2 only, as a string value at depth 1, as a prefix of a longer key:
    no QC of this release.  A backslash sends the row to the host, which settles it."""
    t = eng.qc_table_build(BASE % b"AC=1" + b"\n", "R1")
    skip = [b'{"r1": {}}', b'{"r0": {"a": [1, {"b": "}"}]}, "r1": 5}', b'{"r1" : 1}', b'{"x": "{", "r1": 1}',
            b'{"r0": "a\\\\"b", "r1": 1}', b'{"r1": "a\\\\\\\\"}']
    keep = [b"\\N", b"", b"null", b"{}", b'{"r0": {"r1": 1}}', b'{"r0": "r1", "k": "r1"}', b'{"r1x": 1, "xr1": 2}',
            b'{"R1": 1}', b'{"k": ["r1", {"r1": 1}]}', b'{"r0": "say \\\\"r1\\\\": 1"}', b'{"r0": "r1\\\\"", "k": 1}']
    for col, want in [(c, 0) for c in skip] + [(c, 1) for c in keep]:
        export = b"pk\t1:100:A:G\t" + col + b"\n"
        rows = eng.qc_update_rows(export, t)
        assert (rows.n, rows.counts["skipped"]) == (want, 1 - want), col
        assert rows.counts["host_rows"] == (1 if b"\\\\" in col or col == b"null" else 0), col
        assert Q.ref_update(BASE % b"AC=1" + b"\n", export, "r1")[1]["skipped"] == 1 - want, col
        assert eng.qc_update_rows(export, t, update_existing=True).n == 1
    with pytest.raises(ValueError, match="line 2 of the export") as ei:
        eng.qc_update_rows(b"a\t1:100:A:G\t\\N\nb\t1:100:A:G\tnot json\n", t)
    assert ei.value.line == 2


def test_update_existing_and_contigs(eng):
    vcf = BASE % b"AC=1" + b"\n" + b"chr2\t7\t.\tC\tT,G\t.\t.\tDB\tGT\t0/1\r\n"
    export = (b"record_primary_key\tmetaseq_id\tadsp_qc\r\n"
              b"1:100:A:G\t1:100:A:G\t{\"r1\": {}}\r\n2:7:C:G\t2:7:C:G\t\\N\textra\n\nshort\n2:7:C:T\t2:7:C:T\t\n"
              b"GL1:5:A:C\tGL1:5:A:C\t{}\n")
    t = eng.qc_table_build(vcf, "r1")
    for upd, contigs in ((False, None), (True, None), (False, ["2"]), (True, ["1", "GL1"])):
        want, ctr, _ = Q.ref_update(vcf, export, "r1", update_existing=upd, contigs=contigs)
        rows = eng.qc_update_rows(export, t, update_existing=upd, contigs=contigs)
        assert rows.text.numpy().tobytes() == Q.rows_text(want), (upd, contigs)
        assert {k: rows.counts[k] for k in ctr} == ctr, (upd, contigs)
    assert eng.qc_update_rows(export, t).counts["skipped"] == 1


def test_header_fields_and_release(eng):
    line = b"1\t100\t.\tA\tG\t50\tPASS\tAC=1\n"
    t = eng.qc_table_build(line, "R1", header_fields="#CHROM,POS,ID,REF,ALT,QUAL,FILTER,INFO".split(","))
    assert t.counts["host_lines"] == 1
    assert Q.table_tuples(t) == [("1:100:A:G", json.dumps({"r1": {"info": {"AC": 1}, "filter": "PASS", "qual": 50,
                                                                  "format": None}}), True)]
    with pytest.raises(IndexError):
        eng.qc_table_build(line, "R1")
    same = eng.qc_table_build(BASE % b"AC=1", "R1", header_fields="#chrom,pos,id,ref,alt,qual,filter,info,format".split(","))
    assert same.counts["host_lines"] == 0
    for bad in ("", 'r"1', "r\\1", "r\t1", "é", "x" * 65):
        with pytest.raises(ValueError, match="version"):
            eng.qc_table_build(line, bad)
    assert N.call("avdb_qc_table_size_host", eng.ctx, None, 0, 0, b'r"', 2, None, None, None, None, None,
                  np.zeros(N.QC_N_COUNTS, dtype=np.int64), check=False) == N.AVDB_EINVAL


def test_errors_raise(eng):
    t = eng.qc_table_build(BASE % b"AC=1" + b"\n", "r1")
    with pytest.raises(ValueError, match="line 2 of the export"):
        eng.qc_update_rows(b"a\t1:100:A:G\n1:5:A\t1:5:A\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        eng.qc_update_rows(b"a\t1:100\r:A:G\t\\N\n", t)
    with pytest.raises(ValueError, match="carriage return"):
        eng.qc_table_build(BASE % b"AC=1;X=a\rb" + b"\n", "r1")
    with pytest.raises(ValueError, match="Infinity") as ei:
        eng.qc_table_build(b"#c\n" + BASE % b"AC=1" + b"\n" + BASE % b"AF=-inf" + b"\n", "r1")
    assert ei.value.line == 3
    with pytest.raises(IndexError) as ei:
        eng.qc_table_build(BASE % b"AC=1" + b"\n\n", "r1")
    assert ei.value.line == 2


def test_empty_inputs(eng):
    for vcf in (b"", b"#only\n"):
        t = eng.qc_table_build(vcf, "r1")
        assert t.n_rows == 0 and t.key_off.tolist() == [0]
        rows = eng.qc_update_rows(b"a\t1:100:A:G\t\\N\n", t)
        assert rows.n == 0 and rows.counts["not_in_vcf"] == 1
        assert QCUpdater(t).unmatched() == [] and QCUpdater(t).novel_lines() == []
    t = eng.qc_table_build(BASE % b"AC=1", "r1")
    assert eng.qc_update_rows(b"", t).n == 0


@pytest.mark.parametrize("seed,n_vcf,n_exp", [(1, 0, 5), (2, 1, 1), (3, 65, 64), (4, 300, 257), (5, 513, 700)])
def test_fuzz_against_restatement(eng, seed, n_vcf, n_exp):
    rng = random.Random(seed)
    vcf, ids = Q.fuzz_vcf(rng, n_vcf, multi_alt=0.5, host=0.1)
    export = Q.fuzz_export(rng, ids, n_exp)
    want_t, ctr_t = Q.ref_table(vcf, "r1")
    t = eng.qc_table_build(vcf, "R1")
    assert Q.table_tuples(t) == [(i, js, flag) for i, js, flag, _ in want_t]
    assert {k: t.counts[k] for k in ctr_t} == ctr_t
    for upd in (False, True):
        want, ctr, missing = Q.ref_update(vcf, export, "r1", update_existing=upd)
        t.hit.zero_()
        u = QCUpdater(t)
        u.buffer_export(export, update_existing=upd)
        assert u.update_text() == Q.rows_text(want)
        assert u.unmatched() == missing
        assert (u.get_count("skipped"), u.get_count("not_in_vcf")) == (ctr["skipped"], ctr["not_in_vcf"])


def test_capacity_one_byte_short(eng):
    rng = random.Random(7)
    vcf, ids = Q.fuzz_vcf(rng, 200, host=0.0)
    export = Q.fuzz_export(rng, ids, 300)
    rc, cnt, out, totals = Q.raw_table_passes(eng, vcf)
    assert rc == 0 and totals == [cnt["key_bytes"], cnt["json_bytes"], cnt["rows"], 0] and cnt["rows"] > 20
    n, kb, jb = cnt["rows"], cnt["key_bytes"], cnt["json_bytes"]
    assert (out["keys"][kb:] == 0xA5).all() and (out["json"][jb:] == 0xA5).all()
    assert (out["flags"][n:] == 0xA5).all() and (out["json_len"].view(np.uint8)[4 * n:] == 0xA5).all()
    assert (out["key_off"].view(np.uint8)[8 * (n + 1):] == 0xA5).all() and out["key_off"][n] == kb
    for short in ("key", "json"):
        rc, cnt2, out2, totals2 = Q.raw_table_passes(eng, vcf, **{short + "_cap": (kb if short == "key" else jb) - 1})
        assert rc == N.AVDB_ERANGE and totals2[3] == 1 and totals2[:3] == [kb, jb, n]
        for name in ("keys", "json", "key_off", "json_off", "json_len", "line_start", "flags"):
            assert (out2[name].view(np.uint8) == 0xA5).all(), (short, name)
    t = eng.qc_table_build(vcf, "r1")
    rc, ucnt, buf, utot, cap = Q.raw_update_passes(eng, export, t)
    assert rc == 0 and utot == [cap, 0] and cap > 0 and (buf[cap:] == 0xA5).all()
    rc, _, buf, utot, _ = Q.raw_update_passes(eng, export, t, cap=cap - 1)
    assert rc == N.AVDB_ERANGE and utot == [cap, 1] and (buf == 0xA5).all()


def test_cli_end_to_end(eng, tmp_path):
    g = Q.golden()
    vcf_path, exp_path, out_path, novel_path = (str(tmp_path / n) for n in ("qc.vcf.gz", "export.tsv.gz", "rows.tsv",
                                                                            "novel.vcf"))
    with open(vcf_path, "wb") as fh:
        fh.write(B.bgzip(g["vcf"], block=4000))
    with open(exp_path, "wb") as fh:
        fh.write(B.bgzip(g["export"], block=3000))
    argv = ["--fileName", vcf_path, "--export", exp_path, "--version", g["version"], "--outFile", out_path]
    for mode in (0, 1):
        want, ctr, missing = Q.ref_update(g["vcf"], g["export"], REL, update_existing=bool(mode))
        got = update_from_qc_pvcf_file.main(argv + ["--novelOut", novel_path] + (["--updateExistingValues"] if mode else []),
                                            eng)
        text = open(out_path, "rb").read()
        assert text == Q.rows_text(want)
        tuples = [QCUpdater._tuple(r) for r in text.decode().split("\n")[:-1]]
        assert dedup(tuples) == dedup(g["tuples"][mode])
        novel = open(novel_path, "rb").read().split(b"\n")
        assert novel[0].startswith(b"#CHROM\tPOS") and novel[-1] == b""
        assert got == {"line": g["data_lines"], "update": ctr["rows"], "skipped": ctr["skipped"],
                       "not_in_vcf": ctr["not_in_vcf"], "novel": len(novel) - 2}
        assert set(missing) <= {i for ln in novel[1:-1] for i in Q.ref_line(ln, REL)[0]}


def test_loaders_and_docs_point_to_this_module():
    import inspect
    import os
    from annotatedvdb_amd import slab_passes
    assert "adsp_qc" in inspect.getsource(slab_passes)
    root = os.path.dirname(Q.HERE)
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "K17" in open(os.path.join(root, name)).read(), name

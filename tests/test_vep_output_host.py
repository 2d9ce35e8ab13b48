"""K18c on the host: the host path of a line, the library's ``_host`` entries (the kernels' per-block,
per-line and per-row code compiled for the host side), the export join with the extra column, the updater
and the command, against the reference's own objects recorded in tests/golden/vep_output.tsv.gz.  No GPU."""

import json
import os
import subprocess
import sys

import pytest

import vep_common as V
import vep_output_common as O
import vep_rows_common as R
from conftest import ROOT
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.vep_consequences import ConsequenceRanking
from annotatedvdb_amd.vep_rows import VEPUpdater, update_sql, vep_output_line


@pytest.fixture(scope="module")
def golden():
    return O.read_golden()


@pytest.fixture(scope="module")
def ranking():
    return ConsequenceRanking(V.RANKING_FILE)


@pytest.fixture(scope="module")
def host_engine():
    return Engine("host")


@pytest.fixture(scope="module")
def host_tables(golden, ranking, host_engine):
    """Per form of ``input``'s dict: the golden lines a build takes, and the table of the host entries over them."""
    out = {}
    for identity_only in (False, True):
        lines = O.loadable(golden, identity_only)
        host_engine.poison = 0xA5
        out[identity_only] = (lines, host_engine.vep_rows_table_build(
            V.slab([l[0].decode("utf-8") for l in lines]), ranking, vep_output=True, identity_only=identity_only))
        host_engine.poison = None
    return out


def test_vep_output_line_against_the_reference(golden):
    seen = set()
    for kind, forms, line in golden["lines"]:
        for identity_only, (outcome, cleaned, _) in forms.items():
            seen.add(outcome)
            if outcome == "ok":
                assert vep_output_line(line, identity_only) == cleaned, (kind, line[:200])
            elif outcome in ("raise:IndexError", "raise:ImportError", "raise:JSONDecodeError") or kind == "no_input":
                with pytest.raises(Exception) as err:
                    vep_output_line(line, identity_only)
                assert type(err.value).__name__ == outcome.split(":")[1], (kind, outcome, err.value)
    assert {"ok", "rerank", "raise:KeyError", "raise:IndexError", "raise:ImportError", "raise:JSONDecodeError"} <= seen
    five = [forms for kind, forms, _ in golden["lines"] if kind == "five_fields"]
    assert five and all(f[False][0] == "raise:IndexError" and f[True][0] == "ok" for f in five)


def test_golden_covers_the_arrangements(golden):
    """Dropped members first, last, adjacent, all five and none; input first, in the middle and last; a line that
    is only input; nested kept members; a dropped key's name inside a string and under colocated_variants;
    multi-allelic lines."""
    seen = set()
    for kind, forms, line in golden["lines"]:
        if kind is not None or forms[False][0] != "ok":
            continue
        keys = list(json.loads(line))
        drop = [k in O.DROPPED for k in keys]
        seen.add("first" if drop[0] else "kept_first")
        seen.add("last" if drop[-1] else "kept_last")
        if sum(drop) == 5 and "".join("d" if d else "k" for d in drop).count("ddddd"):
            seen.add("all_five_adjacent")
        if not any(drop):
            seen.add("none" if len(keys) > 1 else "only_input")
        at = keys.index("input")
        seen.add("input_first" if at == 0 else "input_last" if at == len(keys) - 1 else "input_middle")
        if b'"panel":[1,2.5,{' in line:
            seen.add("nested")
        if b'\\"transcript_consequences\\":' in line:
            seen.add("name_in_string")
        if b'"transcript_consequences":[{"x":1}]' in line:
            seen.add("name_under_colocated")
        if len(forms[False][2]) > 2:
            seen.add("three_alts")
        assert len(json.loads(line)["input"].split("\t")) >= 8
    assert seen >= {"first", "kept_first", "last", "kept_last", "all_five_adjacent", "none", "only_input", "input_first",
                    "input_middle", "input_last", "nested", "name_in_string", "name_under_colocated", "three_alts"}


def test_cleaned_texts_of_the_host_entries_are_the_golden(host_tables):
    for identity_only, (lines, t) in host_tables.items():
        got = O.cleaned_texts(t)
        flags = t.cleaned_flags.tolist()
        assert len(got) == len(lines)
        n_device = 0
        for text, flag, (line, kind, outcome, cleaned, rows) in zip(got, flags, lines):
            assert text == vep_output_line(line, identity_only), (kind, line[:200])
            if outcome == "ok":
                assert text == cleaned, (kind, line[:200])
            if flag == 0:  # the device's own text: json.dumps of the cleaned dict, the dict the reference's
                n_device += 1
                assert json.dumps(json.loads(text)) == text and json.loads(text) == json.loads(cleaned)
        assert n_device == len(lines) - t.cleaned_counts["host_lines"]
        # the rows of a line share its text
        want = [cleaned for _, _, outcome, cleaned, rows in lines if outcome == "ok" for _ in rows]
        assert O.row_cleaned(t) == want
        assert t.cleaned.numel() == sum(t.cleaned_len.tolist()) == t.cleaned_counts["out_bytes"]
    full, ident = O.cleaned_texts(host_tables[False][1]), O.cleaned_texts(host_tables[True][1])
    assert any('"info": {"RS": ' in x and '"GENEINFO": "SHOX:6473"' in x and '"U3": true' in x for x in full)
    assert any('"info": {".": true}' in x for x in full) and any('"qual": 29.5' in x for x in full)
    assert any('"SMALL": 1.234e-05' in x and '"DP": 7' in x and '"Z": 0.0' in x for x in full)
    assert any('"BIG": 12345678901234567890' in x and '"K:1": "v"' in x for x in full)
    assert not any('"qual"' in x for x in ident) and any('"input": {"chrom": "chr2", "pos": ' in x for x in ident)
    assert any('"chrom": 1, ' in x for x in ident) and any('"chrom": "MT"' in x for x in ident)
    assert any('"chrom": "Y"' in x and '"ref": "C", "alt": "T"' in x for x in ident)  # letters value_json leaves to Python


def test_counts_by_reason_are_as_constructed(host_tables):
    """Every line the generator built for the device is the device's, every host case is counted under its
    reason, in both forms of the dict: a build cannot pass by sending lines to the host."""
    for identity_only, (lines, t) in host_tables.items():
        want = dict.fromkeys(N.VEPOUT_COUNTS, 0)
        want["lines"] = len(lines)
        for _, kind, _, _, _ in lines:
            reason = O.reason_of(kind, identity_only)
            if reason is not None:
                want["host_lines"] += 1
                want[reason] += 1
        want["out_bytes"] = t.cleaned_counts["out_bytes"]
        assert t.cleaned_counts == want
        assert 0 < want["host_lines"] and 10 * want["host_lines"] <= len(lines)
        assert [f != 0 for f in t.cleaned_flags.tolist()] == \
            [O.reason_of(kind, identity_only) is not None for _, kind, _, _, _ in lines]
        assert [N.VEPOUT_REASONS[f - 1] for f in t.cleaned_flags.tolist() if f] == \
            [O.reason_of(kind, identity_only) for _, kind, _, _, _ in lines if O.reason_of(kind, identity_only)]
    got = host_tables[False][1].cleaned_counts
    assert got["kept_text"] == 3 and got["input_value"] == 5 and got["eight_fields"] == 0  # (fewer than eight raises)
    assert host_tables[True][1].cleaned_counts["input_value"] == 1


def test_raising_lines_raise_from_the_build_with_their_line(golden, ranking, host_engine):
    ok = [l[0].decode() for l in O.loadable(golden, False)[:3]]
    for kind, cls, reason in (("five_fields", IndexError, "eight_fields"), ("numeric_info", ImportError, "input_value")):
        line = next(line for k, _, line in golden["lines"] if k == kind).decode("utf-8")
        with pytest.raises(cls) as err:
            host_engine.vep_rows_table_build(V.slab(ok + [line]), ranking, vep_output=True)
        assert err.value.line == 4 and err.value.counts[reason] == 1 and err.value.counts["host_lines"] == 1
        t = host_engine.vep_rows_table_build(V.slab(ok + [line]), ranking, vep_output=True, identity_only=True)
        assert t.cleaned_counts["host_lines"] == 0 and t.n_rows >= 4


@pytest.mark.parametrize("adsp,update_existing", [(False, False), (False, True), (True, False), (True, True)])
def test_update_rows_of_the_golden(golden, host_tables, host_engine, adsp, update_existing):
    lines, t = host_tables[adsp]  # identityOnly=self.is_adsp()
    t.hit.zero_()
    host_engine.poison = 0xA5
    rows = host_engine.vep_update_rows(golden["export"], t, O.ALG_ID, adsp=adsp, update_existing=update_existing)
    host_engine.poison = None
    want = golden["updates"][(adsp, update_existing)]
    assert rows.text.numpy().tobytes().decode("utf-8") == want
    assert rows.n == want.count("\n") > 100
    assert all(len(r.split("\t")) == (7 if adsp else 6) for r in want.splitlines())
    assert rows.row_off.tolist()[-1] == len(want.encode("utf-8")) == rows.counts["out_bytes"]
    texts = O.row_cleaned(t)
    assert [r.split("\t")[4] for r in want.splitlines()] == [texts[m] for m in rows.match.tolist()]


def test_switches_off_the_table_and_rows_are_k18b(golden, ranking, host_engine):
    lines = [l[0].decode("utf-8") for l in O.loadable(golden, True)]
    plain = host_engine.vep_rows_table_build(V.slab(lines), ranking)
    with_col = host_engine.vep_rows_table_build(V.slab(lines), ranking, vep_output=True, identity_only=True)
    R.assert_same_table(with_col, plain)
    assert plain.cleaned is None and plain.row_entry is None and with_col.cleaned is not None
    a = host_engine.vep_update_rows(golden["export"], plain, O.ALG_ID, adsp=True)
    b = host_engine.vep_update_rows(golden["export"], with_col, O.ALG_ID, adsp=True)
    rows = golden["updates"][(True, False)].splitlines()  # (K18b's rows: the golden's without their fifth column)
    assert a.text.numpy().tobytes().decode("utf-8") == "".join(
        "\t".join(r.split("\t")[:4] + r.split("\t")[5:]) + "\n" for r in rows)
    assert a.match.tolist() == b.match.tolist() and a.counts["rows"] == b.counts["rows"] == len(rows)


def test_updater_and_update_sql(golden, host_tables, ranking, host_engine):
    lines, t = host_tables[True]
    t.hit.zero_()
    u = VEPUpdater(t, alg_id=O.ALG_ID, adsp=True)
    n = u.buffer_export(golden["export"])
    want = golden["updates"][(True, False)]
    assert n == want.count("\n") and u.update_text().decode("utf-8") == want
    buf = u.update_buffer()
    assert len(buf[0]) == 7 and buf[0][-1] == "true" and json.loads(buf[0][4])["input"]["chrom"] is not None
    sql = u.update_sql()
    assert "vep_output = jsonb_merge(COALESCE(v.vep_output ,'{}'::jsonb), d.vep_output::jsonb), row_algorithm_id = " \
        "d.row_algorithm_id" in sql
    assert "adsp_ranked_consequences,vep_output,row_algorithm_id,is_adsp_variant)" in sql
    assert update_sql(True) == update_sql(True, False) and "vep_output" not in update_sql(True)
    with pytest.raises(ValueError):
        VEPUpdater(host_engine.vep_rows_table_build(V.slab(lines[0][0].decode() for _ in range(1)), ranking), vep_output=True)
    # identity_only defaults to adsp
    text = V.slab([l[0].decode("utf-8") for l in lines[:8]])
    assert VEPUpdater(text, ranking, adsp=True, vep_output=True, engine=host_engine).table().identity_only is True
    assert VEPUpdater(text, ranking, adsp=False, vep_output=True, engine=host_engine).table().identity_only is False
    assert VEPUpdater(text, ranking, adsp=True, vep_output=True, identity_only=False,
                      engine=host_engine).table().identity_only is False


def test_edges_on_the_host_entries(ranking, host_engine):
    """The member drop's edges, the sizes around a block, the nesting limit, small slabs and random lines: the
    host entries against vep_output_line, all on the device's side."""
    rows = V.read_ranking_rows()
    for lines, n_host in ((O.edge_lines(), 0), (O.small_lines(0), 0), (O.small_lines(1), 0), (O.small_lines(2), 0),
                          ([O.nested_line(O.V_MAX_DEPTH + 1)], 1), (O.random_device_lines(rows, 7, 257), 0)):
        for identity_only in (False, True):
            t = host_engine.vep_rows_table_build(V.slab(lines), ranking, vep_output=True, identity_only=identity_only)
            assert t.cleaned_counts["host_lines"] == n_host and t.cleaned_counts["lines"] == len(lines)
            assert O.cleaned_texts(t) == [vep_output_line(l, identity_only) for l in lines]
    assert len(O.sized_line(64)) == 64 and len(O.three_block_drop_line()) > 3 * 64


def test_update_write_boundaries_on_the_host_entries(ranking, host_engine):
    """Rows whose head, body, cleaned text and tail each end 63, 64 and 65 bytes past a 64-byte boundary."""
    for adsp in (False, True):
        lines, export, want = O.boundary_join_cases(ranking, O.ALG_ID, adsp, adsp)
        t = host_engine.vep_rows_table_build(V.slab(lines), ranking, vep_output=True, identity_only=adsp)
        rows = host_engine.vep_update_rows(export, t, O.ALG_ID, adsp=adsp)
        text = rows.text.numpy().tobytes().decode("utf-8")
        assert text == O.expected_update_text(lines, export, ranking, O.ALG_ID, adsp, False, adsp)
        assert rows.n == len(want) == 12
        for row, (part, past) in zip(text.splitlines(), want):
            f = row.split("\t")
            ends = [len(f[0]) + 1 + len(f[1]) + 1]
            ends.append(ends[0] + len(f[2]) + 1 + len(f[3]))
            ends.append(ends[1] + 1 + len(f[4]))
            ends.append(len(row) + 1)
            assert ends[part] % 64 == past % 64 and ends[1] - ends[0] > 64 and ends[2] - ends[1] > 64


def test_cli_end_to_end(golden, tmp_path):
    """The command with --vepOutput on the golden's lines (those the reference raises for left out) and export."""
    import gzip
    keep = O.loadable(golden, True)
    src, exp, out = tmp_path / "vep.json.gz", tmp_path / "export.tsv", tmp_path / "rows.tsv"
    with gzip.open(src, "wb") as fh:
        fh.write(b"\n".join(l[0] for l in keep) + b"\n")
    exp.write_bytes(golden["export"])
    cmd = [sys.executable, "-m", "annotatedvdb_amd.load_vep_result", "--fileName", str(src), "--rankingFile",
           V.RANKING_FILE, "--export", str(exp), "--outFile", str(out), "--algInvocationId", str(O.ALG_ID),
           "--datasource", "ADSP", "--device", "host", "--vepOutput", "--skipMissing"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    done = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 2, done.stderr[-2000:]  # (lines that need a re-rank; an exception would be 1)
    assert out.read_text() == golden["updates"][(True, False)]
    sql = open(str(out) + ".update.sql").read()
    assert "d(record_primary_key,chromosome,adsp_most_severe_consequence,adsp_ranked_consequences,vep_output," \
        "row_algorithm_id,is_adsp_variant)" in sql
    unranked = [row.split("\t") for row in open(str(out) + ".unranked").read().splitlines()]
    assert [r[0] for r in unranked] == [str(i + 1) for i, l in enumerate(keep) if l[2] == "rerank"] != []

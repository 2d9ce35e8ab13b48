"""K18a on the host: the ranking reader, the host path of a line and the library's ``_host``
entries (the kernels' per-block code compiled for the host side) against the reference's own
objects recorded in tests/golden/vep_consequences.tsv.gz.  No GPU."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vep_common as V
from conftest import ROOT
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.vep_consequences import (ConsequenceRanking, UnrankedCombination, alleles_of, most_severe_of,
                                               vep_line)


@pytest.fixture(scope="module")
def golden():
    return V.read_golden()


@pytest.fixture(scope="module")
def rankings(golden, tmp_path_factory):
    frac = tmp_path_factory.mktemp("vep") / "fractional.txt"
    frac.write_text(golden["files"]["fractional"])
    return {"shipped": ConsequenceRanking(V.RANKING_FILE), "fractional": ConsequenceRanking(str(frac))}


@pytest.fixture(scope="module")
def host_engine():
    return Engine("host")


@pytest.fixture(scope="module")
def host_results(golden, rankings, host_engine):
    """Per ranking: its golden lines and the batch result of the host entries over them."""
    out = {}
    for name, ranking in rankings.items():
        lines = [g for g in golden["lines"] if g[0] == name]
        text = b"\n".join(g[3] for g in lines) + b"\n"
        host_engine.poison = 0xA5
        out[name] = (lines, host_engine.vep_consequences(text, ranking))
        host_engine.poison = None
    return out


def test_ranking_matches_reference(golden, rankings):
    for name, ranking in rankings.items():
        got = [[k, v] for k, v in ranking.rankings().items()]
        assert got == golden["rankings"][name]
        assert [type(v) for _, v in got] == [type(v) for _, v in golden["rankings"][name]]
    shipped = rankings["shipped"]
    assert len(shipped.rankings()) == 293 and len(shipped.terms) == 31
    assert list(shipped.rankings().values()) == list(range(1, 294))


def test_ranking_without_rank_column_is_load_order(tmp_path):
    p = tmp_path / "r.txt"
    p.write_text('consequence\tadsp_ranking\nstop_gained\t9\n"b_variant,a_variant"\t2.5\nintron_variant\t1\n')
    r = ConsequenceRanking(str(p))
    assert list(r.rankings().items()) == [("stop_gained", 1), ("a_variant,b_variant", 2), ("intron_variant", 3)]


def test_rank_of(rankings):
    r = rankings["shipped"]
    assert r.rank_of(["missense_variant"]) == 129
    assert r.rank_of(["not_a_term"]) is None  # an unknown single term: None, not an error
    assert r.rank_of(["splice_region_variant", "missense_variant"]) == 128
    assert r.rank_of(["missense_variant", "splice_region_variant"]) == 128
    assert r.rank_of(["splice_region_variant,missense_variant"]) is None  # one term, looked up as it is
    for terms in (["missense_variant", "intergenic_variant"], ["missense_variant", "missense_variant"], []):
        with pytest.raises(UnrankedCombination) as err:
            r.rank_of(terms)
        assert isinstance(err.value, LookupError) and err.value.combination == ",".join(terms)
    f = rankings["fractional"]
    assert f.rank_of(["missense_variant"]) == 2.5 and f.rank_of(["TF_binding_site_variant"]) == 7.0
    assert isinstance(f.rank_of(["TF_binding_site_variant"]), float) and isinstance(f.rank_of(["stop_gained"]), int)


def test_ranking_rejects_what_the_device_cannot_hold():
    with pytest.raises(ValueError):
        ConsequenceRanking([("a_variant,a_variant", None)])
    with pytest.raises(ValueError):
        ConsequenceRanking([("t%d" % i, None) for i in range(65)])
    with pytest.raises(ValueError):
        ConsequenceRanking([("a_variant", "first")])
    assert len(ConsequenceRanking([("t%d" % i, None) for i in range(64)]).terms) == 64


def test_table_build_rejects_more_than_64_terms(host_engine):
    masks = np.array([1, 2], dtype=np.uint64)
    slot_mask, slot_entry = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.int32)
    assert host_engine._call("avdb_vep_table_build", 2, masks, 2, slot_mask, slot_entry, 4) == 0
    assert sorted(slot_entry.tolist()) == [-1, -1, 0, 1]
    with pytest.raises(N.NativeError) as err:
        host_engine._call("avdb_vep_table_build", 65, masks, 2, slot_mask, slot_entry, 4)
    assert err.value.rc == N.AVDB_EINVAL


def check_line(outcome, want_ranked, want_severe, ranked_of):
    if outcome == "ok":
        got = ranked_of()
        assert got == want_ranked
        for key in got:  # the lists' order, and the alleles' (dict equality does not see it)
            assert list(got[key] or ()) == list(want_ranked[key] or ())
        assert alleles_of(got) == list(want_severe)
        for va, c in want_severe.items():
            assert most_severe_of(got, va) == c
    elif outcome == "rerank":
        with pytest.raises(LookupError):
            ranked_of()
    else:
        cls = {"TypeError": TypeError, "KeyError": KeyError, "JSONDecodeError": json.JSONDecodeError}[outcome[6:]]
        with pytest.raises(cls):
            ranked_of()


def test_vep_line_alone(golden, rankings):
    for name, _, outcome, line, ranked, severe in golden["lines"]:
        check_line(outcome, ranked, severe, lambda: vep_line(line, rankings[name]))


def test_golden_through_host_entries(host_results):
    for name, (lines, res) in host_results.items():
        assert res.n_lines == len(lines)
        for i, (_, _, outcome, _, ranked, severe) in enumerate(lines):
            check_line(outcome, ranked, severe, lambda: res.ranked(i))
            if outcome == "ok":
                for va, c in severe.items():
                    assert res.most_severe(i, va) == c


def test_counts_by_reason_are_as_constructed(host_results):
    for name, (lines, res) in host_results.items():
        want = dict.fromkeys(N.VEP_COUNTS, 0)
        want["lines"] = len(lines)
        flags = res.flags.numpy()
        for i, (_, kind, _, line, _, _) in enumerate(lines):
            if kind is None:
                assert flags[i] == 0, (i, N.VEP_REASONS[flags[i] - 1], line[:200])
            else:
                reason = V.REASON_OF[kind]
                assert flags[i] == 1 + N.VEP_REASONS.index(reason), (i, kind, flags[i])
                want["host_lines"] += 1
                want[reason] += 1
        want["consequences"] = int(res.n_csq.sum())
        assert res.counts == want
        host = want["host_lines"]
        assert 0 < host and 9 * host <= len(lines) - host


def test_device_rows_of_the_golden(host_results):
    """What the arrays say directly: spans, order numbers, the permutation, the group heads."""
    lines, res = host_results["shipped"]
    h = res._host()
    for i in np.flatnonzero(h["flags"] == 0)[:300]:
        obj = json.loads(lines[i][3])
        assert res.line_id(i) == obj["id"]
        assert json.loads(b'"' + res._span(h["input_start"][i], h["input_len"][i]) + b'"') == obj["input"]
        off, n = int(h["csq_off"][i]), int(h["n_csq"][i])
        flat = [(t, k, e) for t, key in enumerate(V.TYPES) for k, e in enumerate(obj.get(key + "_consequences") or ())]
        assert n == len(flat)
        for r, (t, k, e) in enumerate(flat):
            assert (h["type"][off + r], h["order"][off + r]) == (t, k)
            assert json.loads(res._span(h["el_start"][off + r], h["el_len"][off + r])) == e
            assert res._span(h["al_start"][off + r], h["al_len"][off + r]).decode() == e["variant_allele"]
        assert sorted(h["sorted"][off:off + n].tolist()) == list(range(n))
    host = np.flatnonzero(h["flags"])
    for i in host:  # blank rows
        off, n = int(h["csq_off"][i]), int(h["n_csq"][i])
        assert (h["entry"][off:off + n] == -1).all() and h["sorted"][off:off + n].tolist() == list(range(n))


def test_crlf_and_missing_final_newline(rankings, host_engine):
    lines = V.golden_lines(V.read_ranking_rows(), 7, 8)
    text = "\r\n".join(l for l, _ in lines[:8]).encode()
    res = host_engine.vep_consequences(text, rankings["shipped"])
    # (the carriage returns are no whitespace of the lines: only the generator's host line is flagged)
    assert res.n_lines == 8 and [bool(f) for f in res.flags.tolist()] == [kind is not None for _, kind in lines[:8]]
    for i, (line, kind) in enumerate(lines[:8]):
        if kind is None:
            assert res.ranked(i) == vep_line(line, rankings["shipped"])


def test_cli_on_bgzip(golden, tmp_path):
    """The command on a bgzip copy of the golden's lines (those the reference raises for left out:
    the command stops at such a line, as the reference's loader does)."""
    import gzip
    import zlib
    keep = [g for g in golden["lines"] if g[0] == "shipped" and not g[2].startswith("raise")]
    text = b"\n".join(g[3] for g in keep) + b"\n"
    src = tmp_path / "vep.json.gz"
    with open(src, "wb") as fh:  # BGZF members of 60000 bytes, and the empty one that ends the file
        for at in list(range(0, len(text), 60000)) + [len(text)]:
            chunk = text[at:at + 60000]
            c = zlib.compressobj(6, zlib.DEFLATED, -15)
            body = c.compress(chunk) + c.flush()
            fh.write(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + (len(body) + 25).to_bytes(2, "little") + body +
                     zlib.crc32(chunk).to_bytes(4, "little") + len(chunk).to_bytes(4, "little"))
    assert gzip.open(src).read() == text
    out = tmp_path / "summary.tsv"
    done = subprocess.run([sys.executable, "-m", "annotatedvdb_amd.vep_consequences", "--fileName", str(src),
                           "--rankingFile", V.RANKING_FILE, "--out", str(out), "--device", "host"],
                          env=dict(os.environ, PYTHONPATH=ROOT), cwd=ROOT, capture_output=True, text=True)
    assert done.returncode == 2, done.stderr[-2000:]  # (lines that need a re-rank; an exception would be 1)
    want_rows, want_unranked = [], []
    for i, (_, _, outcome, line, ranked, severe) in enumerate(keep):
        if outcome == "rerank":
            want_unranked.append(str(i + 1))
            continue
        obj = json.loads(line)
        vid = obj.get("id") if isinstance(obj, dict) else None
        for va, c in severe.items():
            t = next(k for k in V.TYPES if va in (ranked.get(k + "_consequences") or ()))
            want_rows.append("\t".join([vid or "", va, t, "" if c["rank"] is None else str(c["rank"]),
                                        "true" if c["consequence_is_coding"] else "false",
                                        ",".join(c["consequence_terms"])]))
    assert out.read_text().splitlines() == want_rows
    got_unranked = [row.split("\t") for row in open(str(out) + ".unranked").read().splitlines()]
    assert [r[0] for r in got_unranked] == want_unranked and want_unranked and all(len(r) == 3 for r in got_unranked)
    assert any("," in r[2] for r in got_unranked)  # (the combination; empty for a line without terms)


def test_block_edges_on_host_entries(rankings, host_engine):
    """Every structural feature on every lane and on both sides of a 64-byte edge; lines of exactly 64 and 128 bytes."""
    lines = V.edge_lines()
    res = host_engine.vep_consequences(V.slab(lines), rankings["shipped"])
    assert res.counts["host_lines"] == 0 and res.counts["lines"] == len(lines)
    V.assert_ranked_as_vep_line(res, lines, rankings["shipped"], vep_line)
    obj = json.loads(lines[70])
    assert res.line_id(70) == "rs5" and res._span(res._host()["input_start"][70], res._host()["input_len"][70]) == \
        json.dumps(obj["input"])[1:-1].encode()


def test_counts_and_small_slabs_on_host_entries(rankings, host_engine):
    rows = V.read_ranking_rows()
    counts = [0, 1, 63, 64, 65, N.VEP_MAX_CSQ, N.VEP_MAX_CSQ + 1]
    lines = V.count_lines(rows, counts)
    res = host_engine.vep_consequences(V.slab(lines), rankings["shipped"])
    assert res.n_csq.tolist() == counts
    assert res.flags.tolist() == [0] * 6 + [1 + N.VEP_REASONS.index("too_many")]
    V.assert_ranked_as_vep_line(res, lines, rankings["shipped"], vep_line)
    for n in (0, 1, 2):
        small = V.small_lines(n)
        res = host_engine.vep_consequences(V.slab(small), rankings["shipped"])
        assert res.n_lines == n and res.counts["consequences"] == n and res.counts["host_lines"] == 0
        V.assert_ranked_as_vep_line(res, small, rankings["shipped"], vep_line)

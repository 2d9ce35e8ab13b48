"""K18d on the device: the kernels run on poisoned buffers and are compared array for array and byte for byte
with the library's host entries (the same per-block, per-line and per-row code compiled for the host side),
and text for text with the reference's ``allele_frequencies`` of the golden and with
``allele_frequencies_line``."""

import json

import pytest

import vep_common as V
import vep_freq_common as F
import vep_output_common as O
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.vep_consequences import ConsequenceRanking

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return F.read_golden()


@pytest.fixture(scope="module")
def ranking():
    return ConsequenceRanking(V.RANKING_FILE)


@pytest.fixture(scope="module")
def host_engine():
    return Engine("host")


def both(engine, host_engine, lines, ranking, form, vep_output=False):
    """The table of the lines with its frequency texts on the device, on poisoned buffers, and through the host
    entries; compared.  Returns both."""
    text = V.slab(lines)
    kw = dict(vep_output=vep_output, identity_only=form[0], allele_frequencies=True, match_refsnp=form[1])
    engine.poison = 0xA5
    try:
        got = engine.vep_rows_table_build(text, ranking, **kw)
    finally:
        engine.poison = None
    want = host_engine.vep_rows_table_build(text, ranking, **kw)
    F.assert_same_freq(got, want)
    if vep_output:
        O.assert_same_cleaned(got, want)
    return got, want


def update_both(engine, host_engine, export, table, host_table, **kw):
    engine.poison = 0xA5
    try:
        got = engine.vep_update_rows(export, table, F.ALG_ID, **kw)
    finally:
        engine.poison = None
    want = host_engine.vep_update_rows(export, host_table, F.ALG_ID, **kw)
    assert got.n == want.n and got.counts == want.counts
    for name in ("text", "row_off", "match"):
        assert getattr(got, name).cpu().tolist() == getattr(want, name).tolist(), name
    assert table.hit.cpu().tolist() == host_table.hit.tolist()
    return got


@pytest.fixture(scope="module")
def tables(engine, host_engine, golden, ranking):
    out = {}
    for form in F.FORMS:
        lines = F.loadable(golden, form)
        out[form] = (lines,) + both(engine, host_engine, [l[0].decode("utf-8") for l in lines], ranking, form,
                                    vep_output=form[0] != form[1])  # (the two datasources' tables carry vep_output)
    return out


@pytest.mark.parametrize("form", F.FORMS)
def test_golden(tables, form):
    lines, t, _ = tables[form]
    got = F.freq_texts(t)
    assert got == [text for _, _, outcome, rows in lines if outcome == "ok" for _, text in rows]
    want = dict.fromkeys(N.VEPFREQ_COUNTS, 0)
    want["lines"] = len(lines)
    for _, kind, _, _ in lines:
        reason = F.reason_of(kind, *form)
        if reason is not None:
            want["host_lines"] += 1
            want[reason] += 1
    want["out_bytes"], want["rows"] = t.freq_counts["out_bytes"], t.n_rows
    assert t.freq_counts == want and 0 < want["host_lines"] and 10 * want["host_lines"] <= len(lines)
    assert [N.VEPFREQ_REASONS[f - 1] if f else None for f in t.freq_flags.cpu().tolist()] == \
        [F.reason_of(kind, *form) for _, kind, _, _ in lines]
    assert t.freq.numel() == t.freq_counts["out_bytes"] == sum(map(len, got))


@pytest.mark.parametrize("form", [(False, True), (True, False)])
def test_walk_edges(engine, host_engine, ranking, form):
    """colocated_variants, the chosen frequencies object and the allele key beginning 63, 64 and 65 bytes into a
    line, the object over more than three blocks; a COSMIC_MUTATION string on every lane across a block edge;
    allele objects of 1, 63 and 64 members, one group taking all and the groups alternating member by member,
    with and without FREQ; 1, 2 and 3 elements with the winner in each place; nesting at AVDB_VEP_MAX_DEPTH;
    rows that are {}."""
    lines = F.edge_lines()
    t, _ = both(engine, host_engine, lines, ranking, form)
    assert t.freq_counts["host_lines"] == 0 and t.freq_counts["lines"] == len(lines)
    assert F.freq_texts(t) == F.expected_texts(lines, *form)
    assert F.freq_texts(t).count("{}") >= 5


def test_members_and_nesting_beyond_the_limits_are_the_hosts(engine, host_engine, ranking):
    assert F.V_MAX_DEPTH == N.VEP_MAX_DEPTH and N.VEPFREQ_MAX_MEMBERS == 64
    lines = [F.members_line(64, True), F.members_line(65, True), F.nested_line(N.VEP_MAX_DEPTH),
             F.nested_line(N.VEP_MAX_DEPTH + 1)]
    t, _ = both(engine, host_engine, lines, ranking, (False, False))
    assert t.freq_flags.cpu().tolist() == [0, 1 + N.VEPFREQ_REASONS.index("members"), 0,
                                           1 + N.VEPFREQ_REASONS.index("depth")]
    texts = F.freq_texts(t)
    assert texts == F.expected_texts(lines, False, False)
    assert list(json.loads(texts[0])) == ["GnomAD", "1000Genomes", "ESP", "New"]


@pytest.mark.parametrize("n", [0, 1, 2, N.VEP_GRID_WAVES + 1])
def test_slab_sizes(engine, host_engine, ranking, n):
    lines = F.small_lines(n)
    t, _ = both(engine, host_engine, lines, ranking, (False, True))
    assert t.n_rows == n and t.freq_counts["host_lines"] == 0 and t.freq_counts["lines"] == n
    assert t.freq_off.numel() == n == t.freq_len.numel()
    texts = F.freq_texts(t)
    for i in sorted({0, n - 1} & set(range(n))):
        assert [texts[i]] == F.expected_texts([lines[i]], False, True) and '"gmaf"' in texts[i]


def test_random_lines(engine, host_engine, ranking):
    lines = F.random_device_lines(V.read_ranking_rows(), 257257, 257)
    for form in F.FORMS:
        t, _ = both(engine, host_engine, lines, ranking, form)
        assert t.freq_counts["host_lines"] == 0
        assert F.freq_texts(t) == F.expected_texts(lines, *form)


@pytest.mark.parametrize("adsp,update_existing", [(False, False), (True, False), (True, True)])
def test_update_rows_of_the_golden(engine, host_engine, golden, tables, adsp, update_existing):
    """Skipped records, update-existing, ids the table lacks and table rows no record matches (hit); with
    vep_output."""
    lines, t, host_t = tables[(True, False) if adsp else (False, True)]
    t.hit.zero_()
    host_t.hit.zero_()
    rows = update_both(engine, host_engine, golden["export"], t, host_t, adsp=adsp, update_existing=update_existing)
    assert rows.text.cpu().numpy().tobytes().decode("utf-8") == golden["updates"][(adsp, update_existing, True)]
    assert rows.counts["not_annotated"] > 0 and 0 < int(t.hit.sum()) < t.n_rows
    assert (rows.counts["skipped"] > 0) == (not update_existing)


def test_update_rows_of_the_golden_without_vep_output(engine, host_engine, golden, tables):
    lines, t, host_t = tables[(False, False)]
    rows = update_both(engine, host_engine, golden["export"], t, host_t)
    text = rows.text.cpu().numpy().tobytes().decode("utf-8")
    assert rows.n > 100 and all(len(r.split("\t")) == 6 for r in text.splitlines())
    texts = F.freq_texts(t)
    assert [r.split("\t")[2] for r in text.splitlines()] == [texts[m] for m in rows.match.cpu().tolist()]
    assert "{}" in [r.split("\t")[2] for r in text.splitlines()]


@pytest.mark.parametrize("adsp", [False, True])
@pytest.mark.parametrize("vep_output", [False, True])
def test_update_write_boundaries(engine, host_engine, ranking, adsp, vep_output):
    """Rows whose head, frequency text, body, cleaned text and tail each end 63, 64 and 65 bytes past a 64-byte
    boundary, with and without vep_output."""
    lines, export, want = F.boundary_join_cases(ranking, F.ALG_ID, adsp, vep_output)
    t, host_t = both(engine, host_engine, lines, ranking, (adsp, False), vep_output=vep_output)
    rows = update_both(engine, host_engine, export, t, host_t, adsp=adsp)
    assert rows.n == len(want)
    assert rows.text.cpu().numpy().tobytes().decode("utf-8") == \
        F.expected_update_text(lines, export, ranking, F.ALG_ID, adsp, False, adsp, False, vep_output)
    for text in (b"", export[:export.index(b"\n") + 1]):  # exports of 0 and 1 records
        update_both(engine, host_engine, text, t, host_t, adsp=adsp)

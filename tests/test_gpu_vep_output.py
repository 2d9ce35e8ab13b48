"""K18c on the device: the kernels run on poisoned buffers and are compared array for array and byte for
byte with the library's host entries (the same per-block, per-line and per-row code compiled for the host
side), and text for text with the reference's cleaned results of the golden and with ``vep_output_line``."""

import pytest

import vep_common as V
import vep_output_common as O
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.vep_consequences import ConsequenceRanking
from annotatedvdb_amd.vep_rows import vep_output_line

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return O.read_golden()


@pytest.fixture(scope="module")
def ranking():
    return ConsequenceRanking(V.RANKING_FILE)


@pytest.fixture(scope="module")
def host_engine():
    return Engine("host")


def both(engine, host_engine, lines, ranking, identity_only):
    """The table of the lines with its cleaned texts on the device, on poisoned buffers, and through the host
    entries; compared.  Returns both."""
    text = V.slab(lines)
    engine.poison = 0xA5
    try:
        got = engine.vep_rows_table_build(text, ranking, vep_output=True, identity_only=identity_only)
    finally:
        engine.poison = None
    want = host_engine.vep_rows_table_build(text, ranking, vep_output=True, identity_only=identity_only)
    O.assert_same_cleaned(got, want)
    return got, want


def update_both(engine, host_engine, export, table, host_table, **kw):
    engine.poison = 0xA5
    try:
        got = engine.vep_update_rows(export, table, O.ALG_ID, **kw)
    finally:
        engine.poison = None
    want = host_engine.vep_update_rows(export, host_table, O.ALG_ID, **kw)
    assert got.n == want.n and got.counts == want.counts
    for name in ("text", "row_off", "match"):
        assert getattr(got, name).cpu().tolist() == getattr(want, name).tolist(), name
    assert table.hit.cpu().tolist() == host_table.hit.tolist()
    return got


@pytest.fixture(scope="module")
def tables(engine, host_engine, golden, ranking):
    out = {}
    for identity_only in (False, True):
        lines = O.loadable(golden, identity_only)
        out[identity_only] = (lines,) + both(engine, host_engine, [l[0].decode("utf-8") for l in lines], ranking,
                                             identity_only)
    return out


@pytest.mark.parametrize("identity_only", [False, True])
def test_golden(tables, identity_only):
    lines, t, _ = tables[identity_only]
    got, flags = O.cleaned_texts(t), t.cleaned_flags.cpu().tolist()
    for text, (line, kind, outcome, cleaned, rows) in zip(got, lines):
        if outcome == "ok":
            assert text == cleaned, (kind, line[:200])
    want = dict.fromkeys(N.VEPOUT_COUNTS, 0)
    want["lines"] = len(lines)
    for _, kind, _, _, _ in lines:
        reason = O.reason_of(kind, identity_only)
        if reason is not None:
            want["host_lines"] += 1
            want[reason] += 1
    want["out_bytes"] = t.cleaned_counts["out_bytes"]
    assert t.cleaned_counts == want and 0 < want["host_lines"] and 10 * want["host_lines"] <= len(lines)
    assert [f != 0 for f in flags] == [O.reason_of(kind, identity_only) is not None for _, kind, _, _, _ in lines]
    # the rows of a multi-allelic line share one text
    entries = t.row_entry.cpu().tolist()
    assert O.row_cleaned(t) == [cleaned for _, _, outcome, cleaned, rows in lines if outcome == "ok" for _ in rows]
    assert any(entries[i] == entries[i + 1] == entries[i + 2] for i in range(len(entries) - 2))


@pytest.mark.parametrize("identity_only", [False, True])
def test_member_and_block_edges(engine, host_engine, ranking, identity_only):
    """One line padded by 0..130 bytes in front of a dropped member and in front of input: every key quote, colon,
    member edge and the carry of "a kept member came before" on every lane and both sides of a block edge;
    members of 63, 64, 65 and 128 bytes, kept and dropped; lines of exactly 64 and 128 bytes; a dropped member
    over three blocks; nesting up to AVDB_VEP_MAX_DEPTH; everything but input dropped; only input."""
    lines = O.edge_lines()
    t, _ = both(engine, host_engine, lines, ranking, identity_only)
    assert t.cleaned_counts["host_lines"] == 0 and t.cleaned_counts["lines"] == len(lines)
    assert O.cleaned_texts(t) == [vep_output_line(l, identity_only) for l in lines]


def test_nesting_beyond_the_limit_is_the_hosts(engine, host_engine, ranking):
    assert O.V_MAX_DEPTH == N.VEP_MAX_DEPTH
    lines = [O.nested_line(N.VEP_MAX_DEPTH), O.nested_line(N.VEP_MAX_DEPTH + 1)]
    t, _ = both(engine, host_engine, lines, ranking, False)
    assert t.cleaned_flags.cpu().tolist() == [0, 1 + N.VEPOUT_REASONS.index("depth")]
    assert O.cleaned_texts(t) == [vep_output_line(l, False) for l in lines]


@pytest.mark.parametrize("n", [0, 1, 2, N.VEP_GRID_WAVES + 1])
def test_slab_sizes(engine, host_engine, ranking, n):
    lines = O.small_lines(n)
    t, _ = both(engine, host_engine, lines, ranking, False)
    assert t.n_rows == n and t.cleaned_counts["host_lines"] == 0 and t.cleaned_counts["lines"] == n
    assert t.cleaned_off.numel() == n and t.row_entry.cpu().tolist()[:n] == list(range(n))
    texts = O.cleaned_texts(t)
    for i in sorted({0, n - 1} & set(range(n))):
        assert texts[i] == vep_output_line(lines[i], False)


def test_random_lines(engine, host_engine, ranking):
    lines = O.random_device_lines(V.read_ranking_rows(), 257257, 257)
    for identity_only in (False, True):
        t, _ = both(engine, host_engine, lines, ranking, identity_only)
        assert t.cleaned_counts["host_lines"] == 0
        assert O.cleaned_texts(t) == [vep_output_line(l, identity_only) for l in lines]


@pytest.mark.parametrize("adsp,update_existing", [(False, False), (True, False), (True, True)])
def test_update_rows_of_the_golden(engine, host_engine, golden, tables, adsp, update_existing):
    """Skipped records, update-existing, ids the table lacks and table rows no record matches (hit)."""
    lines, t, host_t = tables[adsp]
    t.hit.zero_()
    host_t.hit.zero_()
    rows = update_both(engine, host_engine, golden["export"], t, host_t, adsp=adsp, update_existing=update_existing)
    assert rows.text.cpu().numpy().tobytes().decode("utf-8") == golden["updates"][(adsp, update_existing)]
    assert rows.counts["not_annotated"] > 0 and 0 < int(t.hit.sum()) < t.n_rows
    assert (rows.counts["skipped"] > 0) == (not update_existing)


@pytest.mark.parametrize("adsp", [False, True])
def test_update_write_boundaries(engine, host_engine, ranking, adsp):
    """Rows whose head, body, cleaned text and tail each end 63, 64 and 65 bytes past a 64-byte boundary."""
    lines, export, want = O.boundary_join_cases(ranking, O.ALG_ID, adsp, adsp)
    t, host_t = both(engine, host_engine, lines, ranking, adsp)
    rows = update_both(engine, host_engine, export, t, host_t, adsp=adsp)
    assert rows.n == len(want)
    assert rows.text.cpu().numpy().tobytes().decode("utf-8") == \
        O.expected_update_text(lines, export, ranking, O.ALG_ID, adsp, False, adsp)
    for text in (b"", export[:export.index(b"\n") + 1]):  # exports of 0 and 1 records
        update_both(engine, host_engine, text, t, host_t, adsp=adsp)

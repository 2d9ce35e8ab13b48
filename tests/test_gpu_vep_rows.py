"""K18b on the device: the kernels run on poisoned buffers and are compared array for array and byte for
byte with the library's host entries (the same per-block, per-line and per-row code compiled for the host
side), and row for row with the reference's rows of the golden and with ``vep_rows_line``."""

import pytest

import vep_common as V
import vep_rows_common as R
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine
from annotatedvdb_amd.vep_consequences import ConsequenceRanking
from annotatedvdb_amd.vep_rows import vep_rows_line

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return R.read_golden()


@pytest.fixture(scope="module")
def rankings(golden, tmp_path_factory):
    frac = tmp_path_factory.mktemp("vep_rows") / "fractional.txt"
    frac.write_text(golden["files"]["fractional"])
    return {"shipped": ConsequenceRanking(V.RANKING_FILE), "fractional": ConsequenceRanking(str(frac))}


@pytest.fixture(scope="module")
def host_engine():
    return Engine("host")


def both(engine, host_engine, lines, ranking):
    """The table of the lines on the device, on poisoned buffers, and through the host entries; compared."""
    text = V.slab(lines)
    engine.poison = 0xA5
    try:
        got = engine.vep_rows_table_build(text, ranking)
    finally:
        engine.poison = None
    R.assert_same_table(got, host_engine.vep_rows_table_build(text, ranking))
    return got


def update_both(engine, host_engine, export, table, host_table, **kw):
    engine.poison = 0xA5
    try:
        got = engine.vep_update_rows(export, table, R.ALG_ID, **kw)
    finally:
        engine.poison = None
    want = host_engine.vep_update_rows(export, host_table, R.ALG_ID, **kw)
    assert got.n == want.n and got.counts == want.counts
    for name in ("text", "row_off", "match"):
        assert getattr(got, name).cpu().tolist() == getattr(want, name).tolist(), name
    assert table.hit.cpu().tolist() == host_table.hit.tolist()
    return got


@pytest.fixture(scope="module")
def shipped(engine, host_engine, golden, rankings):
    lines = R.loadable(golden, "shipped")
    return lines, both(engine, host_engine, [l.decode("utf-8") for l, _, _, _ in lines], rankings["shipped"])


def check_golden(lines, t):
    assert R.table_rows(t) == [tuple(r) for _, _, outcome, rows in lines if outcome == "ok" for r in rows]
    host = sum(kind is not None for _, kind, _, _ in lines)
    assert t.counts["host_lines"] == host and len(lines) - host >= 9 * host > 0
    for _, kind, _, _ in lines:
        if kind is not None:
            assert t.counts[R.REASON_OF[kind]] > 0


def test_golden(shipped):
    check_golden(*shipped)


def test_fractional_and_tied_ranks(engine, host_engine, golden, rankings):
    lines = R.loadable(golden, "fractional")
    t = both(engine, host_engine, [l.decode("utf-8") for l, _, _, _ in lines], rankings["fractional"])
    check_golden(lines, t)
    texts = {ms.split('"rank": ')[1].split(",")[0] for _, ms, _ in R.table_rows(t) if ms != "{}"}
    assert len({len(x) for x in texts}) >= 3, texts  # rank texts of differing lengths (1, 10, 2.5, 2.75, ...)


def test_block_edges_and_element_sizes(engine, host_engine, rankings):
    """One element whose string value is padded by 0..130 bytes: every structural ',' and ':', every escaped
    quote, every backslash run and the closing '}' on every lane and both sides of a block edge; elements of
    exactly 63, 64, 65 and 128 input bytes."""
    lines = R.edge_lines()
    t = both(engine, host_engine, lines, rankings["shipped"])
    assert t.counts["host_lines"] == 0 and t.n_rows == len(lines)
    assert R.table_rows(t) == R.expected_rows(lines, rankings["shipped"])


def test_order_number_digits_and_the_cap(engine, host_engine, rankings):
    lines = R.order_lines()
    t = both(engine, host_engine, lines, rankings["shipped"])
    assert t.counts["host_lines"] == t.counts["too_many"] == 1  # 513 consequences
    assert R.table_rows(t) == R.expected_rows(lines, rankings["shipped"])
    ranked = R.table_rows(t)[4][2]
    for k in (9, 10, 99, 100, 511):
        assert '"vep_consequence_order_num": %d,' % k in ranked


def test_rows_without_consequences(engine, host_engine, rankings):
    lines = R.empty_row_lines()
    t = both(engine, host_engine, lines, rankings["shipped"])
    assert t.counts["host_lines"] == 0
    rows = R.table_rows(t)
    assert rows == R.expected_rows(lines, rankings["shipped"])
    assert [ms == "{}" for _, ms, _ in rows] == [False, True, True, True, True, False, False, True]


@pytest.mark.parametrize("n", [0, 1, 2, N.VEP_GRID_WAVES + 1])
def test_slab_sizes(engine, host_engine, rankings, n):
    lines = R.small_lines(n)
    t = both(engine, host_engine, lines, rankings["shipped"])
    assert t.n_rows == n and t.counts["host_lines"] == 0 and t.counts["lines"] == n
    rows = R.table_rows(t)
    for i in sorted({0, n - 1} & set(range(n))):
        assert [rows[i]] == [tuple(r) for r in vep_rows_line(lines[i], rankings["shipped"])]


def test_random_lines(engine, host_engine, rankings):
    lines = R.random_device_lines(V.read_ranking_rows(), 257257, 257)
    t = both(engine, host_engine, lines, rankings["shipped"])
    assert t.counts["host_lines"] == 0
    assert R.table_rows(t) == R.expected_rows(lines, rankings["shipped"])


@pytest.mark.parametrize("adsp,update_existing", [(False, False), (True, True)])
def test_update_rows_of_the_golden(engine, host_engine, golden, rankings, shipped, adsp, update_existing):
    lines, t = shipped
    host_t = host_engine.vep_rows_table_build(V.slab([l.decode("utf-8") for l, _, _, _ in lines]), rankings["shipped"])
    t.hit.zero_()
    rows = update_both(engine, host_engine, golden["export"], t, host_t, adsp=adsp, update_existing=update_existing)
    assert rows.text.cpu().numpy().tobytes().decode("utf-8") == golden["updates"][(adsp, update_existing)]


def test_small_join(engine, host_engine, rankings):
    """Exports of 0 and 1 records; hit, miss and skipped records; two keys of one id; the repeated id."""
    lines, export = R.join_cases()
    t = both(engine, host_engine, lines, rankings["shipped"])
    host_t = host_engine.vep_rows_table_build(V.slab(lines), rankings["shipped"])
    rows = update_both(engine, host_engine, export, t, host_t)
    got = [r.split("\t") for r in rows.text.cpu().numpy().tobytes().decode().splitlines()]
    assert [r[0] for r in got] == ["pk_a", "pk_b", "pk_e"] and '"stop_gained"' in got[0][2]
    assert rows.counts["skipped"] == 1 and rows.counts["not_annotated"] == 1 and t.hit.cpu().tolist() == [0, 1, 1, 0]
    for text, kw in ((b"", {}), (b"pk_a\t1:300:A:G\t\\N\n", {"adsp": True}), (export, {"update_existing": True})):
        update_both(engine, host_engine, text, t, host_t, **kw)

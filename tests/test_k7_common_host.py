"""k7_common's reference is pinned without a GPU (the C oracle on every KEY_OK record, the
reference project's own keys in tests/golden/c1_prefix.tsv.gz), and its builders reach
the edges test_gpu_k7_edges.py relies on them to reach: asserted here, so a builder that
loses an edge fails this test instead of hollowing out the GPU one."""

import gzip
import os

import numpy as np
import pytest

import k7_common as K
from conftest import GOLDEN
from oracle import avdb_oracle as O

MAX_LENS = (50, 120)


def _all_batches(max_len):
    """(name, Batch) of every builder at ``max_len``."""
    out = [("window", K.batch(K.window_cases(max_len)[0])), ("bad_byte", K.batch(K.bad_byte_cases(max_len)[0])),
           ("prefix_suffix", K.batch(K.prefix_suffix_cases()[0])), ("threshold", K.batch(K.threshold_tiles()[0])),
           ("flush", K.batch(K.flush_tiles()[0]))]
    out += [("heap_edge%d" % i, K.batch(recs, heap_shift=s)) for i, (recs, s) in enumerate(K.heap_edge_cases())]
    return out


def _oracle_keys(b, idx, digests, max_len):
    """The C oracle's keys of records ``idx`` of the batch."""
    import oracle
    idx = np.asarray(idx, dtype=np.int64)
    m = len(idx)
    cols = [np.ascontiguousarray(x[idx]) for x in (b.chrom, b.pos, b.allele_off, b.ref_len, b.alt_len, b.ext_id)]
    dg = np.ascontiguousarray(digests[idx])
    out = np.zeros(int((b.ref_len[idx].astype(np.int64) + b.alt_len[idx]).sum()) + 80 * m + 8, dtype=np.uint8)
    off = np.zeros(m + 1, dtype=np.uint64)
    c, p, o, r, a, e = cols
    oracle.c_oracle().avdb_oracle_primary_keys(c.ctypes.data, p.ctypes.data, o.ctypes.data, r.ctypes.data,
                                               a.ctypes.data, b.heap.ctypes.data, e.ctypes.data, dg.ctypes.data, m,
                                               max_len, out.ctypes.data, off.ctypes.data)
    raw = out.tobytes()
    return [raw[int(off[k]):int(off[k + 1])] for k in range(m)]


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", MAX_LENS)
def test_reference_equals_c_oracle_on_ok_records(max_len):
    for name, b in _all_batches(max_len):
        dg = K.digest_rows(b.n, seed=3)
        st, keys, _ = K.expected(b.recs, max_len, digests=dg, over=b.over)
        ok = [i for i, s in enumerate(st) if s == K.KEY_OK]
        assert len(ok) >= (100 if name == "flush" else b.n // 2), name  # (flush tiles are mostly empty spans)
        got = _oracle_keys(b, ok, dg, max_len)
        bad = [i for i, g in zip(ok, got) if g != keys[i]]
        assert not bad, (name, [(b.recs[i], keys[i]) for i in bad[:3]])


def test_reference_conventions():
    dg = K.digest_rows(8)
    long_ = K.Rec(9, 1234567890, b"A" * 30, b"C" * 21, 12, K.make_code(1, 9))
    recs = [K.Rec(0, 100, b"A", b"G"), K.Rec(1, 5, b"A:C", b"A"), K.Rec(2, 9, b"C", b"T", K.INTERNED | 4, 0),
            long_, K.Rec(30, 12, b"A", b"C", 0, 0), K.Rec(22, 0, b"", b"A", 1 << 32), K.Rec(3, 7, b"\x80", b"T"),
            K.Rec(4, 8, b"AC", b"GT", over=1)]
    st, keys, paths = K.expected(recs, 50)
    assert st == [K.KEY_OK, K.KEY_HOST, K.KEY_HOST, K.KEY_NEED_DIGEST, K.KEY_HOST, K.KEY_OK, K.KEY_HOST, K.KEY_HOST]
    assert keys == [b"1:100:A:G", b"2:5:A:C:A", b"", b"", b"", b"X:0::A:rs4294967296", b"4:7:\x80:T", b"5:8:AC:GT"]
    assert paths == [b"", b"", b"chr3", b"chr10.L1.B10", b"", b"", b"", b""]
    assert K.exemptions(recs, st, keys) == [None, (0, 9), None, None, None, None, (0, 7), (0, 9)]
    st, keys, _ = K.expected(recs[3:4], 50, defer=True)
    assert st == [K.KEY_DIGEST_PENDING] and keys == [b"10:1234567890:" + bytes(32) + b":rs12"]
    assert K.exemptions(recs[3:4], st, keys) == [(14, 46)] and K.body_at(long_) == 14
    st, keys, _ = K.expected(recs, 50, digests=dg)
    assert st[3] == K.KEY_OK and keys[3] == b"10:1234567890:" + dg[3].tobytes() + b":rs12"
    assert K.expected(recs[3:4], 51)[0] == [K.KEY_OK]  # r + a == max_len: short
    # the fabricated codes' paths, restated here from generate_bin_index_references.py:54,60-61,74
    assert K.path_text(9, K.make_code(13, 11, 0xFFF)) == ("chr10.L1.B12" + "".join(
        ".L%d.B2" % lv for lv in range(2, 14))).encode()
    assert len(K.path_text(9, K.make_code(13, 8))) == 87 and len(K.path_text(21, K.make_code(13, 9))) == 88
    assert K.path_text(0, K.BIN_NONE) == b"" and K.path_text(24, 0) == b"chrM"


def test_reference_reproduces_the_reference_projects_keys():
    """tests/golden/c1_prefix.tsv.gz: VariantPKGenerator's keys and BinIndex's paths."""
    from annotatedvdb_amd import synth
    from annotatedvdb_amd.chromosomes import length_table
    with gzip.open(os.path.join(GOLDEN, "c1_prefix.tsv.gz"), "rt") as fh:
        fh.readline()
        rows = [ln.rstrip("\n").split("\t") for ln in fh][:4000]
    d = synth.np_c1(synth.C1_N, seed=1)
    heap = d["heap"].tobytes()
    lengths = length_table()
    recs = []
    for i, row in enumerate(rows):
        o, r, a = int(d["allele_off"][i]), int(d["ref_len"][i]), int(d["alt_len"][i])
        code, _ = O.bin_code(lengths[int(d["chrom"][i])], int(d["pos"][i]), int(row[1]))
        recs.append(K.Rec(int(d["chrom"][i]), int(d["pos"][i]), heap[o:o + r], heap[o + r:o + r + a],
                          int(d["ext_id"][i]), code))
    st, keys, paths = K.expected(recs, 50)
    assert st == [K.KEY_OK] * len(rows)
    assert [k.decode() for k in keys] == [row[0] for row in rows]
    assert [p.decode() for p in paths] == [row[2] for row in rows]


# ---------------------------------------------------------------------------
# the batch builder
# ---------------------------------------------------------------------------
def test_batch_sets_offsets_and_phases():
    recs = [K.Rec(0, 1, b"ACG", b"T", phase=5), K.Rec(1, 2, b"", b"GG", phase=5), K.Rec(2, 3, b"A", b"C"),
            K.Rec(3, 4, b"TTTT", b"", phase=0)]
    for shift in range(8):
        b = K.batch(recs, heap_shift=shift)
        m1, m2 = b.phases()
        assert [int(m1[i]) for i in (0, 1, 3)] == [5, 5, 0] and int(m2[0]) == 0
        assert int(b.allele_off[2]) == int(b.allele_off[1]) + 2  # (no phase: packed)
        h = b.heap.tobytes()
        for i, r in enumerate(recs):
            o = int(b.allele_off[i])
            assert h[o:o + len(r.ref) + len(r.alt)] == r.ref + r.alt
        assert b.heap_bytes == int(b.allele_off[3]) + 4 and not b.over.any()
        data = sum(len(r.ref) + len(r.alt) for r in recs)
        assert h.count(b":") == b.heap_bytes - data  # (the gaps are ':')
    b = K.batch([K.Rec(0, 1, b"", b"")])
    assert b.heap_bytes == 1
    b = K.batch([K.Rec(0, 1, b"AC", b"G"), K.Rec(0, 1, b"AC", b"GT", over=1)], heap_shift=3)
    assert b.heap_bytes == 6 and b.over.tolist() == [False, True] and int(b.allele_off[1]) + 4 == b.heap_bytes + 1
    b = K.batch([K.Rec(24, (1 << 32) - 1, b"A", b"C", (1 << 64) - 1, K.BIN_NONE)], pad=3)
    assert b.pos.view(np.uint32)[0] == (1 << 32) - 1 and b.ext_id.view(np.uint64)[0] == (1 << 64) - 1
    assert b.code.view(np.uint32)[0] == K.BIN_NONE and b.heap_bytes == 5


def test_span_cells_and_staging():
    assert K.span_cell(32, 32) == ("empty", 0) and K.span_cell(19, 19) == ("empty", 3)
    assert K.span_cell(16, 48) == ("aligned", 0) and K.span_cell(16, 21) == ("tail", 5)
    assert K.span_cell(16, 53) == ("tail", 5) and K.span_cell(19, 32) == ("head", 3) and K.span_cell(19, 64) == ("head", 3)
    assert K.span_cell(19, 24) == ("inside", 3) and K.span_cell(19, 33) == ("cross", 3)
    assert K.span_cell(19, 47) == ("cross", 3) and K.span_cell(19, 49) == ("general", 3)
    # kst: gk1 - (gk0 & ~15) + 16 <= kKeyWave
    assert K.staged(0, 2544, K.KEY_WAVE) and not K.staged(0, 2545, K.KEY_WAVE)
    assert K.staged(31, 31 + 2529, K.KEY_WAVE) and not K.staged(31, 31 + 2530, K.KEY_WAVE)
    assert K.staged(5, 5 + 5611, K.PATH_WAVE) and not K.staged(5, 5 + 5612, K.PATH_WAVE)
    assert K.tile_spans([1] * 64 + [2] * 64 + [0] * 64 + [3]) == [(0, 64), (64, 192), (192, 192), (192, 195)]
    assert (K.TILE, K.CHUNK, K.WIN_BYTES, K.KEY_WAVE, K.PATH_WAVE, K.SMALL_GROUP_N) == (64, 16, 56, 2560, 5632, 4 << 20)


# ---------------------------------------------------------------------------
# coverage: what the GPU tests rely on
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", MAX_LENS)
def test_window_cases_cover_every_phase_and_length(max_len):
    recs, info = K.window_cases(max_len)
    lens = K.window_lens(max_len)
    assert set(K.WIN_LENS) <= set(lens) and (max_len == 50 or set(K.WIDE_LENS) <= set(lens))
    cells = {(ph, n) for ph in range(8) for n in lens}
    assert info["ref_cells"] >= cells and info["alt_cells"] >= cells
    assert info["pairs_at_7"] >= set(K.PHASE7_PAIRS) and info["pairs_alt_at_7"] >= set(K.PHASE7_PAIRS)
    assert info["long_phases"] == set(range(8))
    assert any(len(r.ref) + len(r.alt) == max_len + 1 for r in recs)
    assert any(len(r.ref) + len(r.alt) == max_len for r in recs)
    assert info["max_word"] == 7  # all seven window words: 49 bytes at phase 7
    assert info["wide"] > 0 and info["mixed_tiles"] >= 1  # `wide` true and false within one tile
    if max_len == 50:  # only a 50-byte allele at phase 7 leaves the window
        assert info["wide_cells"] == {(7, 50)}
    else:
        assert info["wide_cells"] >= {(ph, n) for ph in range(8) for n in K.WIDE_LENS} | {(7, 50)}
    assert len(recs) % K.TILE != 0 and len(recs) > 4 * K.TILE


@pytest.mark.parametrize("max_len", MAX_LENS)
def test_bad_byte_cases_cover_every_position(max_len):
    recs, info = K.bad_byte_cases(max_len)
    wl = 100 if max_len == 120 else 50
    want = {(kind, which, at, v) for kind, n, pos in (("win", 20, range(8, 16)), ("wide", wl, range(wl - 10, wl - 2)))
            for which in ("ref", "alt") for at in (0, n - 1) + tuple(pos) for v in K.BAD_BYTES}
    assert info["bad_at"] == want and info["bad"] == len(want) == 160
    assert info["host"] == 160 and info["wide_host"] == 80 and info["win_host"] == 80
    assert info["near_miss"] == 64
    st, _, _ = K.expected(recs, max_len, digests=K.digest_rows(len(recs)))
    # at least 7 clean records between two bad ones; the near-miss records are KEY_OK
    host = [i for i, s in enumerate(st) if s == K.KEY_HOST]
    assert min(b - a for a, b in zip(host, host[1:])) >= 8
    near = recs[len(recs) - 64:]
    assert all(s == K.KEY_OK for s in st[len(recs) - 64:])
    assert {x for r in near for x in r.ref + r.alt} & set(K.NEAR_MISS) == set(K.NEAR_MISS)
    assert not any(0x3A in r.ref + r.alt for r in near)
    b = K.batch(recs)
    m1, m2 = b.phases()
    lanes = set()  # the byte lane (address & 7) of every bad byte: all eight, for both kinds
    for i in host:
        r = recs[i]
        for data, m in ((r.ref, m1[i]), (r.alt, m2[i])):
            lanes |= {(len(data) > 20, (int(m) + k) & 7) for k, x in enumerate(data) if x == 0x3A or x >= 0x80}
    assert lanes == {(w, k) for w in (False, True) for k in range(8)}


def test_prefix_suffix_cases_cover_every_width():
    recs, info = K.prefix_suffix_cases()
    assert set(K.PS_CONTIGS) == {0, 8, 9, 21, 22, 23, 24, 25, 30}
    assert {0, 1, 9, 10, 99, 100, 10 ** 9 - 1, 10 ** 9, 1 << 31, (1 << 32) - 1} <= set(K.PS_POS) and len(K.PS_POS) == 22
    assert set(K.PS_EXT) == {0, 1, 9, 10, 10 ** 9 - 1, 10 ** 9, (1 << 32) - 1, 1 << 32, 10 ** 10, 10 ** 18,
                             (1 << 63) - 1, (1 << 63) | 5}
    assert info["short"] == {(c, p, e) for c in K.PS_CONTIGS for p in K.PS_POS for e in K.PS_EXT}
    assert info["long_pos"] == {(w, p) for w in (0, 1, 2) for p in K.PS_POS}  # (label bytes, POS)
    assert info["long_ext"] == {(w, e) for w in (0, 1, 2) for e in K.PS_EXT}
    assert info["long_contigs"] == set(K.PS_CONTIGS)
    assert info["pos_digits"] == set(range(1, 11)) and info["ext_digits"] == {1, 2, 9, 10, 11, 19}
    assert 13 in info["colon_at"] and min(info["colon_at"]) == 3
    assert all(K.is_long(r, 120) == (len(r.ref) > 1) for r in recs)


def _threshold_sides(staged, lo, hi):
    return {(p, s) for p, t, s in staged if lo <= t <= hi}


def test_threshold_tiles_cover_both_sides_at_every_phase():
    recs, info = K.threshold_tiles()
    assert len(recs) % K.TILE == 0
    k, p = info["keys"]["staged"], info["paths"]["staged"]
    both = {(ph, s) for ph in range(K.CHUNK) for s in (False, True)}
    assert _threshold_sides(k, 2520, 2570) == both and _threshold_sides(p, 5590, 5632) == both
    assert {t for _, t, _ in k} >= set(K.KEY_SWEEP) and {t for _, t, _ in p} >= set(K.PATH_SWEEP)
    # the last staged and the first direct total at every phase
    kk, pp = {(ph, t): s for ph, t, s in k}, {(ph, t): s for ph, t, s in p}
    for ph in range(K.CHUNK):
        assert kk[(ph, 2544 - ph)] and not kk[(ph, 2545 - ph)]
        assert pp[(ph, 5616 - ph)] and not pp[(ph, 5617 - ph)]
    # interleaved with small staged tiles: direct tiles have staged neighbours (one image: staged -> direct -> staged)
    for st in (k, p):
        direct = [i for i, x in enumerate(st) if not x[2]]
        assert direct and all(st[i - 1][2] and st[i + 1][2] for i in direct if 0 < i < len(st) - 1)
    # short bodies (a direct tile of short keys), paths of 87 and 88 bytes on two-character contigs, level 13
    assert all(len(r.ref) + len(r.alt) <= 50 for r in recs)
    big = [r for r in recs if r.code != K.BIN_NONE and r.code >> 28 == 13 and r.c < K.N_CONTIGS]
    assert {len(K.path_text(r.c, r.code)) for r in big} == {87, 88} and all(9 <= r.c < 22 for r in big)
    assert {(r.code & 0x0FFFFFFF) >> 12 for r in big} == set(range(12))
    assert max(len(K.path_text(r.c, r.code)) for r in recs) <= 98  # avdb_primary_keys_bound's path bytes


def test_flush_tiles_cover_every_category_and_phase():
    recs, info = K.flush_tiles()
    assert len(recs) % K.TILE == 0
    ph = set(range(1, K.CHUNK))
    for name, inside_max in (("keys", 10), ("paths", 11)):
        by = {c: {p for cc, p in info[name]["cells"] if cc == c} for c in K.CATEGORIES}
        assert by["empty"] == ph | {0} and by["aligned"] == {0} and by["tail"] == ph, name
        assert by["head"] == ph and by["cross"] == ph and by["general"] == ph, name
        assert by["inside"] == set(range(1, inside_max + 1)), name
        assert all(s for _, _, s in info[name]["staged"])  # sparse tiles are always staged
        spans = info[name]["spans"]
        assert spans[0][0] == spans[0][1] == 0 and spans[-1][0] == spans[-1][1]  # empty first and last
        live = [i for i, s in enumerate(spans) if s[1] > s[0]]
        assert any(spans[i][0] == spans[i][1] and spans[i][0] % K.CHUNK for i in range(live[0], live[-1]))
    assert {t for _, t, _ in info["keys"]["staged"]} == set(K.FLUSH_KEY_TOTALS)  # 0 and 5..40
    assert set(range(8, 41)) | {0, 4, 5} <= set(K.flush_path_totals())
    assert info["levels"] == set(range(14))
    # each tile: at most 3 live keys and 3 paths
    _, keys, paths = K.expected(recs, 50)
    for t in range(0, len(recs), K.TILE):
        assert sum(1 for x in keys[t:t + K.TILE] if x) <= 3 and sum(1 for x in paths[t:t + K.TILE] if x) <= 3


def test_heap_edge_cases():
    cases = K.heap_edge_cases()
    shifts = lambda f: sorted(s for recs, s in cases if f(K.batch(recs, heap_shift=s)))  # noqa: E731
    assert shifts(lambda b: b.n == 70 and not b.over.any()) == list(range(8))
    assert shifts(lambda b: b.heap_bytes < K.WIN_BYTES) == list(range(8))
    assert shifts(lambda b: b.over.any()) == [0, 5]
    mods = set()
    for recs, s in cases:
        b = K.batch(recs, heap_shift=s)
        assert int(b.allele_off[0]) == 0 and b.heap.tobytes().count(b":") == 0  # packed from byte 0, no pad
        last = int(b.allele_off[-1]) + int(b.ref_len[-1]) + int(b.alt_len[-1])
        if b.over.any():
            assert b.over.tolist() == [False] * (b.n - 1) + [True] and last == b.heap_bytes + 1
            st, _, _ = K.expected(recs, 50, over=b.over)
            assert st[-1] == K.KEY_HOST
        else:
            assert last == b.heap_bytes
            mods.add(b.heap_bytes % 8)
    assert mods >= set(range(1, 8))


@pytest.mark.parametrize("max_len", MAX_LENS)
def test_exempt_spans_stay_under_an_eighth(max_len):
    """Bytes are not compared only in the span of a KEY_HOST record that has one and in the
    32 digest bytes of a pending key: at most 1/8 of the records and of the key bytes of
    every batch, with digests and deferred."""
    for name, b in _all_batches(max_len) + [("pattern", K.batch(K.pattern_records()))]:
        for defer in (False, True):
            dg = None if defer else K.digest_rows(b.n)
            st, keys, _ = K.expected(b.recs, max_len, digests=dg, defer=defer, over=b.over)
            recs_share, bytes_share = K.exempt_share(b.recs, st, keys)
            assert recs_share <= 0.125 and bytes_share <= 0.125, (name, defer, recs_share, bytes_share)


def test_pattern_rotates():
    b = K.batch(K.pattern_records())
    assert b.n % 256 != 0 and b.heap_bytes % 2 == 1 and not b.over.any()
    assert 10_000 < b.n < 60_000

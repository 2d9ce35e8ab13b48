"""K4 (`csrc/avdb_digest.hip`: `k_vrs_digest`, the `k_long_*` compaction kernels and
`k_sha512t24u`) where `synth.alleles` cannot reach: every ALT-length residue and block
count up to 514, the clamp bucket's mixed block counts, every (contig, digit count) row
of the SequenceLocation table, blocks that reach past the heap end, heaps of fewer than
eight bytes, and the entry paths no engine call selects (tests/k4_common.py).

Every expected digest is `hashlib` through the oracle's serialiser (`K.expected`); K4 is
never its own reference.  Every comparison is exact bytes over every record of every
batch: a row of the digest output is the oracle's 32 characters for a long record,
`'?' * 32` for a long record on an unlabelled contig, and the 0xA5 the engine's poison
left there for a short one.
"""

import functools

import numpy as np
import pytest

import k4_common as K
from annotatedvdb_amd.chromosomes import CHROM_NAMES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = 0xA5
GUARD = 0x5C  # around buffers of the tests' own


def _N():
    from annotatedvdb_amd import _native
    return _native


def _new_engine():
    from annotatedvdb_amd.engine import Engine
    e = Engine(0, sequence_digests=K.SEQ_DIGESTS)
    e.poison = POISON
    return e


@pytest.fixture(scope="module")
def eng(engine):
    """An engine of this module's own (the session's is given other digests by other
    tests), every output and workspace filled with 0xA5 before the kernels run."""
    e = _new_engine()
    yield e
    e.close()


def _pack(recs, device):
    from annotatedvdb_amd.engine import pack_records
    return pack_records([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs],
                        [r[3] for r in recs]).to(device)


def _want(recs, max_len=K.MAX_LEN):
    """(is_long uint8[n], digest rows uint8[n, 32]) as K4 must leave them."""
    exp = K.expected(K.SEQ_DIGESTS, recs, max_len)
    rows = np.full((len(recs), 32), POISON, dtype=np.uint8)
    for i, e in enumerate(exp):
        if e is not None:
            rows[i] = np.frombuffer(e, dtype=np.uint8)
    return np.array([e is not None for e in exp], dtype=np.uint8), rows


@functools.lru_cache(maxsize=None)
def _want_mix():
    return _want(K.mix_records())


def _check(recs, dig, is_long, want, label=""):
    want_long, want_rows = want
    n = len(recs)
    if is_long is not None:
        got_long = is_long.cpu().numpy()[:n]
        bad = np.nonzero(got_long != want_long)[0]
        assert bad.size == 0, (label, "is_long", bad[:8].tolist(), got_long[bad[:8]].tolist())
    got = dig.cpu().numpy().reshape(-1, 32)[:n]
    bad = np.nonzero((got != want_rows).any(axis=1))[0]
    assert bad.size == 0, (label, "digest", bad.size,
                           [(int(i), recs[i][0], recs[i][1], len(recs[i][2]), len(recs[i][3]),
                             K.blocks(len(recs[i][3])), got[i].tobytes(), want_rows[i].tobytes()) for i in bad[:4]])


# ---------------------------------------------------------------------------
# 1. the mix against the oracle: default grid, and one workgroup
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [0, 1], ids=["default-grid", "one-workgroup"])
def test_k4_mix_vs_oracle(engine, grid):
    """All ALT-length and position cases, short records between them and contig codes
    25 / 200 / 255, shuffled.  With AVDB_OPT_K4_GRID = 1 the one workgroup walks the whole
    bucket-major list: every wave straddles buckets, the lanes of the clamp bucket (31..45,
    80 and 514 blocks) share waves with each other and with shorter messages, and the
    grid-stride loop takes several trips."""
    N = _N()
    recs = K.mix_records()
    e = _new_engine()
    try:
        if grid:
            e.set_option(N.OPT_K4_GRID, grid)
        b = _pack(recs, e.device)
        dig, is_long = e.vrs_digest(b, K.MAX_LEN)
        want = _want_mix()
        assert int(want[0].sum()) > 4 * 256  # (more long records than one workgroup has lanes)
        _check(recs, dig, is_long, want)
        q = [i for i, r in enumerate(recs) if r[0] >= K.N_CONTIGS and K.is_long(r)]
        assert len(q) >= 6 and all(dig[i].cpu().numpy().tobytes() == b"?" * 32 for i in q)
        short = np.nonzero(want[0] == 0)[0]
        assert short.size > 500 and (dig.cpu().numpy()[short] == POISON).all()
    finally:
        e.close()


# ---------------------------------------------------------------------------
# 2. the keyed K2's codes (long_code) instead of K4's own length pass
# ---------------------------------------------------------------------------
def test_k4_codes_ready_mix_vs_oracle(eng, monkeypatch):
    """`avdb_record_prep_keyed` classifies the mix (the bucket clamp is `long_code`'s
    too), K4 takes the codes: `k_long_hist_codes` / `k_long_scatter_codes`."""
    N = _N()
    recs = K.mix_records()
    b = _pack(recs, eng.device)
    kt = eng.new_key_text(b.n, b.heap.numel())
    ws = eng.empty(N.size("avdb_vrs_digest_workspace_size", b.n), torch.uint8)
    eng.record_prep(b, want_lcp=False, keys=kt, key_digest=True, digest_workspace=ws)
    assert "codes" in eng._pending
    flags = []
    launch = eng._launch
    monkeypatch.setattr(eng, "_launch", lambda name, *a: (flags.append((name, a[-1])), launch(name, *a))[1])
    dig, is_long = eng.vrs_digest(b, K.MAX_LEN, workspace=ws)
    assert "codes" not in eng._pending and flags == [("avdb_vrs_digest_ex", N.DIGEST_CODES_READY)]
    _check(recs, dig, is_long, _want_mix())


# ---------------------------------------------------------------------------
# 3. the heap ends at the last ALT byte
# ---------------------------------------------------------------------------
HEAP_END_ALTS = tuple(range(264)) + (300, 1000, 4000)
LEAD = ((4, 1234567, b"G", b"GTACGTAC"), K.position_records()[40])  # a short and a long record


@functools.lru_cache(maxsize=None)
def _heap_end_cases():
    rng = np.random.default_rng(44)
    by_len = {len(r[3]): r for r in K.alt_length_records()[:521]}
    last = [by_len[a] if a in by_len else (a % K.N_CONTIGS, 31 * a, K.bases(rng, K.REF_LEN), K.bases(rng, a))
            for a in HEAP_END_ALTS]
    return tuple(LEAD + (r,) for r in last)


def _run_heap_end(eng, cases, shift, max_len=K.MAX_LEN):
    """Each case (a tuple of records) as a batch of its own whose heap is exactly its
    allele bytes, a view `shift` bytes past an 8-aligned address of one buffer of 0xFF
    bytes.  The SoA arrays of case i are 4-entry-strided views (16-byte aligned, the
    vector form).  Returns the stacked digests and flags; the buffer is unchanged."""
    from annotatedvdb_amd.engine import RecordBatch
    m = len(cases[0])
    assert all(len(c) == m for c in cases)
    stride = (m + 3) & ~3
    heaps = [b"".join(r[2] + r[3] for r in c) for c in cases]
    at, total = [], 64
    for h in heaps:
        at.append(total + shift)
        total = (total + shift + len(h) + 64 + 7) & ~7
    buf = np.full(total, 0xFF, dtype=np.uint8)
    cols = {k: np.zeros(len(cases) * stride, dtype=t) for k, t in
            (("chrom", np.uint8), ("pos", np.int64), ("allele_off", np.int64), ("ref_len", np.int32),
             ("alt_len", np.int32))}
    for i, (c, h) in enumerate(zip(cases, heaps)):
        buf[at[i]:at[i] + len(h)] = np.frombuffer(h, dtype=np.uint8)
        o = 0
        for k, r in enumerate(c):
            j = i * stride + k
            cols["chrom"][j], cols["pos"][j], cols["allele_off"][j] = r[0], r[1], o
            cols["ref_len"][j], cols["alt_len"][j] = len(r[2]), len(r[3])
            o += len(r[2]) + len(r[3])
        assert o == len(h)
    cols["pos"] = cols["pos"].astype(np.int32)
    dev = {k: torch.from_numpy(v).to(eng.device) for k, v in cols.items()}
    dbuf = torch.from_numpy(buf).to(eng.device)
    assert dbuf.data_ptr() % 8 == 0
    digs, flags = [], []
    for i, c in enumerate(cases):
        s = slice(i * stride, i * stride + len(c))
        heap = dbuf[at[i]:at[i] + len(heaps[i])]
        assert heap.data_ptr() % 8 == shift and heap.numel() == len(heaps[i])
        b = RecordBatch(heap=heap, **{k: v[s] for k, v in dev.items()})
        assert b.ref_len.data_ptr() % 16 == 0 and b.alt_len.data_ptr() % 16 == 0
        d, f = eng.vrs_digest(b, max_len)
        digs.append(d)
        flags.append(f)
    assert bool((dbuf == torch.from_numpy(buf).to(eng.device)).all())
    return torch.stack(digs).cpu().numpy(), torch.stack(flags).cpu().numpy()


def _check_cases(cases, got, max_len=K.MAX_LEN):
    digs, flags = got
    assert digs.shape == (len(cases), len(cases[0]), 32) and flags.shape == digs.shape[:2]
    for i, c in enumerate(cases):
        want_long, want_rows = _want(c, max_len)
        label = (i, [(r[0], r[1], len(r[2]), len(r[3])) for r in c])
        assert flags[i].tolist() == want_long.tolist(), label
        assert digs[i].tobytes() == want_rows.tobytes(), label + (digs[i].tobytes(),)


@pytest.mark.parametrize("shift", [0, 3], ids=["aligned", "base+3"])
def test_k4_heap_end(eng, shift):
    """The batch's last record ends the heap, `heap_bytes` exact and 0xFF bytes behind
    it, for every ALT length 0..263 (every residue at 2, 3 and 4 blocks: the `CLAMP`
    forms of `alt_word` on the prefix, ALT, suffix and padding words) and for 300, 1,000
    and 4,000 bytes (`inside` blocks up to the heap end, then clamped ones; the clamp
    bucket at the heap end).  A load that ran past the end or a mask that let one of its
    bytes through would hash a 0xFF byte.  (An `inside` block ends at or before its ALT's
    last byte, so with offsets inside the heap its own clamped form is never taken: read
    off `allele_block`, 128 ab + 128 <= 68 + a gives b0 + 128 <= altoff + a.)"""
    cases = _heap_end_cases()
    assert [len(c[-1][3]) for c in cases] == list(HEAP_END_ALTS) and all(len(c) == 3 for c in cases)
    assert {K.blocks(a) for a in HEAP_END_ALTS} == {2, 3, 4, 9, 33}
    _check_cases(cases, _run_heap_end(eng, cases, shift))


# ---------------------------------------------------------------------------
# 4. heaps of fewer than 8 bytes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_cases():
    rng = np.random.default_rng(45)
    out = []
    for h in range(1, 10):  # (8 and 9: the first heaps that hold an 8-byte load)
        for a in range(h):
            out.append(((a + h) % K.N_CONTIGS, 10 ** a + h, K.bases(rng, h - a), K.bases(rng, a)))
    return tuple((r,) for r in out)


@pytest.mark.parametrize("shift", [0, 3], ids=["aligned", "base+3"])
def test_k4_tiny_heaps(eng, shift):
    """Single-record batches whose whole heap is 1..7 bytes (every split of it into REF
    and ALT, the empty ALT included) at max_seq_len 0, and a 7-byte record at
    max_seq_len 6: the digests equal the oracle's.  Below 8 bytes no 8-byte load fits the
    heap, and `alt_word`'s clamp (`heap_bytes - 8`) has nothing to clamp to; these
    batches take `k_vrs_digest<true>`, which reads the heap bytewise.  This test sees
    the digests only: that no read leaves the heap was established by reading the code,
    not by this test."""
    cases = _tiny_cases()
    sizes = [len(c[0][2]) + len(c[0][3]) for c in cases]
    assert set(sizes) == set(range(1, 10)) and sum(1 for c in cases if not c[0][3]) == 9
    _check_cases(cases, _run_heap_end(eng, cases, shift, max_len=0), max_len=0)
    seven = tuple(c for c in cases if len(c[0][2]) + len(c[0][3]) == 7)
    assert len(seven) == 7
    _check_cases(seven, _run_heap_end(eng, seven, shift, max_len=6), max_len=6)


# ---------------------------------------------------------------------------
# 5. the entry paths no engine call selects
# ---------------------------------------------------------------------------
def _one_in(t):
    """`t`'s values as a view starting one element into a buffer of their own."""
    buf = torch.cat([t[:1], t])
    return buf[1:]


@pytest.mark.parametrize("form", ["aligned", "lengths+4", "is_long%4==1", "no-is_long", "lengths+4,no-is_long"])
def test_k4_unselected_entry_paths(eng, form):
    """`avdb_vrs_digest_ex` on the mix with length arrays that start one element into a
    buffer (`k_long_hist<false>`, `k_long_scatter<false>`), with `is_long` at an address
    that is 1 mod 4 (the same kernels), and with no `is_long` (`k_long_scatter<true>`):
    the oracle's digests and flags, as from the aligned call.  The bytes around
    `is_long[0:n]` keep their value: n % 4 == 3, and no four-flag store may spill."""
    N = _N()
    recs = K.mix_records()
    n = len(recs)
    assert n % 4 == 3
    b = _pack(recs, eng.device)
    rl, al = b.ref_len, b.alt_len
    if "lengths+4" in form:
        rl, al = _one_in(rl), _one_in(al)
        assert rl.data_ptr() % 16 == 4 and al.data_ptr() % 16 == 4
    else:
        assert rl.data_ptr() % 16 == 0 and al.data_ptr() % 16 == 0
    guard = torch.full((n + 16,), GUARD, dtype=torch.uint8, device=eng.device)
    lo = 5 if form == "is_long%4==1" else 4
    is_long = None if "no-is_long" in form else guard[lo:lo + n]
    assert guard.data_ptr() % 4 == 0 and (is_long is None or is_long.data_ptr() % 4 == lo - 4)
    need = N.size("avdb_vrs_digest_workspace_size", n)
    ws = eng.empty(need, torch.uint8)
    dig = eng.empty(n * 32, torch.uint8)
    eng._launch("avdb_vrs_digest_ex", b.chrom, b.pos, b.allele_off, rl, al, b.heap, b.heap.numel(), n, K.MAX_LEN,
                ws, need, dig, is_long, 0)
    _check(recs, dig, is_long, _want_mix(), form)
    g = guard.cpu().numpy()
    if is_long is None:
        assert (g == GUARD).all()
    else:
        assert (g[:lo] == GUARD).all() and (g[lo + n:] == GUARD).all(), (g[:lo].tolist(), g[lo + n:].tolist())


# ---------------------------------------------------------------------------
# 6. K4 writing the digests into pending keys, at the edge positions
# ---------------------------------------------------------------------------
def test_k4_key_fill_edge_positions(eng):
    """`vrs_digest(keys=...)` after a deferred K7 on the position cases: every key is
    `label:pos:<oracle digest>`, with 1- and 2-character labels and 1- to 10-digit
    positions (`key_body_at`), and every state is KEY_OK."""
    N = _N()
    recs = K.position_records()
    n = len(recs)
    assert all(r[0] < K.N_CONTIGS and K.is_long(r) for r in recs)
    b = _pack(recs, eng.device)
    out = eng.primary_keys(b, defer_digest=True)
    assert (out.state[:n] == N.KEY_DIGEST_PENDING).all()
    dig, is_long = eng.vrs_digest(b, K.MAX_LEN, keys=out)
    _check(recs, dig, is_long, _want(recs))
    assert (out.state[:n] == N.KEY_OK).all()
    keys, _ = out.host(n)
    exp = K.expected(K.SEQ_DIGESTS, recs)
    want = ["%s:%d:%s" % (CHROM_NAMES[r[0]], r[1], e.decode()) for r, e in zip(recs, exp)]
    assert {len(CHROM_NAMES[r[0]]) for r in recs} == {1, 2} and {len(str(r[1])) for r in recs} == set(range(1, 11))
    bad = [i for i in range(n) if keys[i] != want[i]]
    assert not bad, [(keys[i], want[i]) for i in bad[:4]]


# ---------------------------------------------------------------------------
# 7. k_sha512t24u at every length 0..400
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [0, 1], ids=["even-base", "odd-base"])
def test_k4_sha512t24u_every_length(eng, odd):
    """Blobs of 0..400 bytes packed back to back, the last one ending the buffer, at an
    even and at an odd base address: every residue of the bytewise tail, the 0x80 byte
    and the length word across the block edges at 111/112 and 239/240, one to four blocks."""
    from oracle import avdb_oracle as O
    rng = np.random.default_rng(46 + odd)
    blobs = [rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in range(401)]
    lens = np.array([len(x) for x in blobs], dtype=np.int64)
    off = np.zeros(len(blobs), dtype=np.int64)
    np.cumsum(lens[:-1], out=off[1:])
    raw = np.frombuffer(b"\xff" * odd + b"".join(blobs), dtype=np.uint8).copy()
    buf = torch.from_numpy(raw).to(eng.device)
    data = buf[odd:]
    assert data.data_ptr() % 2 == odd and int(off[-1] + lens[-1]) == data.numel() == 80_200
    out = eng.empty(len(blobs) * 32, torch.uint8)
    eng._launch("avdb_sha512t24u", data, torch.from_numpy(off).to(eng.device),
                torch.from_numpy(lens.astype(np.int32)).to(eng.device), len(blobs), out)
    got = out.cpu().numpy().tobytes()
    bad = [k for k, x in enumerate(blobs) if got[32 * k:32 * k + 32].decode("latin-1") != O.sha512t24u(x)]
    assert not bad, bad[:16]

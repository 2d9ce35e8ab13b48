"""K7's write pass (`k_record_keys_v2` / `key_tile`, annotatedvdb_amd/csrc/avdb_keys.hip; `k_keyed_onepass`
shares `key_tile`) where the synthetic batches cannot reach: all seven window words and
the `wide` per-piece branch at max_seq_len 50 and 120, bad bytes at every byte lane, every
POS and id width, tiles on both sides of both staging thresholds at every phase, every
head / tail case of `flush_span32`, heaps that end at the last allele byte, and the
256-record groups (tests/k7_common.py; that the records reach these edges is asserted on
the CPU in test_k7_common_host.py).

Every expectation is `k7_common.expected`, plain Python; K7 is never its own reference.
Every comparison is exact: the offsets (wide, and narrow words and bases), the states,
every byte of every span but the ones `k7_common.exemptions` names (the span of a KEY_HOST
record that has one; a pending key's 32 digest bytes before the fill), and the sentinel
in every byte of the text buffers behind the totals.
"""

import numpy as np
import pytest

import k4_common as K4
import k7_common as K

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = 0xA5
FORMS = ("onepass", "twocall", "off32", "defer", "serial", "keyed-onepass")
KEYED = {"serial": "serial", "keyed-onepass": "onepass"}  # KeyedStep layouts


def _N():
    from annotatedvdb_amd import _native
    return _native


@pytest.fixture(scope="module")
def eng(engine):
    """An engine of this module's own (sequence digests for K4 in the keyed forms), every
    buffer it allocates filled with the sentinel before the kernels run."""
    from annotatedvdb_amd.engine import Engine
    e = Engine(0, sequence_digests=K4.SEQ_DIGESTS)
    e.poison = SENT
    e.k7_cases = {}  # the builders' batches on the device (_case), freed with the engine
    yield e
    e.k7_cases.clear()
    e.close()


class Case:
    """A batch on the device: the heap a view `heap_shift` bytes past an 8-aligned address
    of a buffer of 0xFF bytes, ending exactly at `heap_bytes`."""

    def __init__(self, eng, recs, heap_shift=0, label=""):
        from annotatedvdb_amd.engine import RecordBatch
        self.b = b = recs if isinstance(recs, K.Batch) else K.batch(recs, heap_shift=heap_shift)
        self.label = label
        buf = np.full(b.heap_bytes + 24, 0xFF, dtype=np.uint8)
        lo = 8 + b.heap_shift
        buf[lo:lo + b.heap_bytes] = b.heap
        self.buf = torch.from_numpy(buf).to(eng.device)
        heap = self.buf[lo:lo + b.heap_bytes]
        assert heap.data_ptr() % 8 == b.heap_shift and heap.numel() == b.heap_bytes
        dev = {k: torch.from_numpy(getattr(b, k)).to(eng.device)
               for k in ("chrom", "pos", "allele_off", "ref_len", "alt_len", "ext_id")}
        self.db = RecordBatch(heap=heap, **dev)
        self.code = torch.from_numpy(b.code).to(eng.device)
        self.digest = K.digest_rows(b.n, seed=11)
        self._want = {}

    def want(self, max_len, digests=None, defer=False, codes=None, key=None):
        """(state, keys, paths) of the reference, computed once per mode."""
        if key is None or key not in self._want:
            w = K.expected(self.b.recs, max_len, digests=digests, defer=defer, over=self.b.over, codes=codes)
            if key is None:
                return w
            self._want[key] = w
        return self._want[key]


def _case(eng, name, max_len=50):
    """The builders' batches, moved to the device once per engine."""
    key = (name, max_len if name in ("window", "bad_byte") else 0)
    cases = eng.k7_cases
    if key not in cases:
        recs = {"window": lambda: K.window_cases(max_len)[0], "bad_byte": lambda: K.bad_byte_cases(max_len)[0],
                "prefix_suffix": lambda: K.prefix_suffix_cases()[0], "threshold": lambda: K.threshold_tiles()[0],
                "flush": lambda: K.flush_tiles()[0]}[name]()
        cases[key] = Case(eng, recs, label=name)
    return cases[key]


def _fill(kt):
    for t in (kt.key_off, kt.path_off, kt.state, kt.keys, kt.paths):
        t.view(torch.uint8).fill_(SENT)


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    return off


def _narrow_raw(t, want, n):
    """The narrow layout itself: n + 1 low words, sentinel padding to the next 8 bytes, one
    u64 base per 4,096 records."""
    raw = t.cpu().numpy()
    lb = (4 * (n + 1) + 7) & ~7
    assert np.array_equal(raw[: 4 * (n + 1)].view(np.uint32), (want & 0xFFFFFFFF).astype(np.uint32))
    assert (raw[4 * (n + 1):lb] == SENT).all()
    nb = (n >> 12) + 1
    assert np.array_equal(raw[lb:lb + 8 * nb].view(np.int64), want[::K.OFF32_SPAN][:nb])
    assert (raw[lb + 8 * nb:] == SENT).all()


def _compare_stream(label, text, got_off, sizes, want_text, exempt):
    n = len(sizes)
    off = _offsets(sizes)
    bad = np.nonzero(got_off != off)[0]
    assert bad.size == 0, (label, "offsets", bad[:4].tolist(), got_off[bad[:4]].tolist(), off[bad[:4]].tolist())
    tot = int(off[n])
    want = np.frombuffer(b"".join(want_text), dtype=np.uint8)
    mask = np.ones(tot, dtype=bool)
    for i, ex in enumerate(exempt):
        if ex:
            mask[off[i] + ex[0]:off[i] + ex[1]] = False
    text = text.cpu().numpy()
    diff = np.nonzero((text[:tot] != want) & mask)[0]
    if diff.size:
        i = int(np.searchsorted(off, diff[0], side="right")) - 1
        raise AssertionError((label, "text", int(diff.size), i, i // K.TILE, i % K.TILE,
                              text[off[i]:off[i + 1]].tobytes(), want_text[i]))
    tail = np.nonzero(text[tot:] != SENT)[0]
    assert tail.size == 0, (label, "bytes behind the total", tot, (tail[:8] + tot).tolist())


def _compare(case, kt, want, label):
    b = case.b
    n = b.n
    state, keys, paths = want
    got = kt.state.cpu().numpy()
    bad = np.nonzero(got[:n] != np.array(state, dtype=np.uint8))[0]
    assert bad.size == 0, (label, "state", [(int(i), int(got[i]), state[i], b.recs[i]) for i in bad[:4]])
    assert (got[n:] == SENT).all(), (label, "states behind n")
    ksz, psz = [len(k) for k in keys], [len(p) for p in paths]
    _compare_stream((label, "keys"), kt.keys, kt.key_offsets(n).cpu().numpy(), ksz, keys,
                    K.exemptions(b.recs, state, keys))
    _compare_stream((label, "paths"), kt.paths, kt.path_offsets(n).cpu().numpy(), psz, paths, [None] * n)
    if kt.off32:
        _narrow_raw(kt.key_off, _offsets(ksz), n)
        _narrow_raw(kt.path_off, _offsets(psz), n)
    else:
        assert kt.key_off.numel() == n + 1 == kt.path_off.numel()


def check(eng, case, *, max_len, code, digest, form, grid=0):
    """K7 on the batch in one of its forms, into buffers that held the sentinel; offsets,
    states, text and the untouched bytes against the reference (`_compare`).
    `code`: the bin codes K7 gets (the keyed forms take the keyed K2's own); `digest`:
    uint8[n, 32] rows or None (long records NEED_DIGEST); `grid`: AVDB_OPT_K7_GRID."""
    N = _N()
    b, db = case.b, case.db
    n = b.n
    label = (case.label, form, max_len, grid)
    dig_t = None if digest is None else torch.from_numpy(digest.reshape(-1)).to(eng.device)
    eng.set_option(N.OPT_K7_GRID, grid)
    try:
        if form in KEYED:
            from annotatedvdb_amd.pipeline import KeyedStep
            ks = KeyedStep(eng, db, digests=True, layout=KEYED[form], max_seq_len=max_len, k7_grid=grid)
            _fill(ks.kt)
            out = ks.run()
            assert ks.kt.off32 == (form == "serial")  # the benched form writes narrow offsets
            codes = out["code"].cpu().numpy().view(np.uint32)
            dg = out["digest"].cpu().numpy().reshape(n, K.DIGEST_CHARS)
            _compare(case, ks.kt, case.want(max_len, digests=dg, codes=codes), label)
            return
        if form == "twocall":
            kt = eng.primary_keys(db, code=code, digest=dig_t, max_seq_len=max_len, onepass=False)
        else:
            kt = eng.new_key_text(n, b.heap_bytes, paths=True, off32=form == "off32")
            _fill(kt)
            eng.primary_keys(db, code=code, digest=dig_t if form != "defer" else None, max_seq_len=max_len, out=kt,
                             defer_digest=form == "defer")
        if form == "defer":  # the pending layout first: prefix, suffix, states; then the filled keys
            _compare(case, kt, case.want(max_len, defer=True, key=("defer", max_len)), label + ("pending",))
            eng.fill_digests(db, dig_t, kt)
        key = ("digest" if digest is not None else "none", max_len)
        _compare(case, kt, case.want(max_len, digests=digest, key=key), label)
    finally:
        eng.set_option(N.OPT_K7_GRID, 0)


def _run(eng, case, form, max_len=50, grid=0, digest=True):
    check(eng, case, max_len=max_len, code=case.code, digest=case.digest if digest else None, form=form, grid=grid)


# ---------------------------------------------------------------------------
# one test per builder
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_len", [50, 120])
@pytest.mark.parametrize("form", FORMS + ("no-digest",))
def test_k7_window_cases(eng, form, max_len):
    """Every allele length x phase of the register window (`load_win` / `append_win`, all
    seven words), ref + alt up to max_seq_len, and the `wide` branch (`o.bytes` from the
    heap) beside windowed lanes in one tile."""
    case = _case(eng, "window", max_len)
    _run(eng, case, "onepass" if form == "no-digest" else form, max_len, digest=form != "no-digest")


@pytest.mark.parametrize("max_len", [50, 120])
@pytest.mark.parametrize("form", FORMS)
def test_k7_bad_byte_cases(eng, form, max_len):
    """':' and non-ASCII bytes at every byte lane, in the masked last word, in the word
    assembled across two window words and in a `wide` allele turn exactly their record
    KEY_HOST (`key_bad`, `key_allele_ok`); 0x39 / 0x3B / 0x7F / 0x01 do not."""
    _run(eng, _case(eng, "bad_byte", max_len), form, max_len)


@pytest.mark.parametrize("form", FORMS + ("no-digest",))
def test_k7_prefix_suffix_cases(eng, form):
    """One- and two-character labels, unlabelled contigs, POS of 1..10 digits (0 and
    2^32 - 1 included), ids of 1..19 digits on both sides of 2^32 and interned ones, with
    short and digest bodies.  The keyed forms also pin that the keyed K2's sizes
    (`key_path_sizes`) and `key_tile` agree on every width: a difference shifts every
    later offset."""
    _run(eng, _case(eng, "prefix_suffix"), "onepass" if form == "no-digest" else form, digest=form != "no-digest")


@pytest.mark.parametrize("form", FORMS)
def test_k7_threshold_tiles(eng, form):
    """Tiles on both sides of K + phase <= 2544 (keys) and P + phase <= 5616 (paths) at
    every phase: the staged and the lane-by-lane streams, short-bodied direct tiles."""
    _run(eng, _case(eng, "threshold"), form)


@pytest.mark.parametrize("form", FORMS)
def test_k7_flush_tiles(eng, form):
    """Every head / tail case of `flush_span32` at every phase, in both streams, empty
    tiles first, last and between live ones."""
    _run(eng, _case(eng, "flush"), form)


@pytest.mark.parametrize("form", FORMS)
def test_k7_heap_edges(eng, form):
    """Heaps at every address phase that end exactly at the last allele byte (0xFF bytes
    behind it), heaps shorter than one window, and a last record one byte past the heap
    end (KEY_HOST, its span reserved)."""
    for i, (recs, shift) in enumerate(K.heap_edge_cases()):
        _run(eng, Case(eng, recs, shift, "heap_edge%d" % i), form)


# ---------------------------------------------------------------------------
# one wave renders every tile in order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["threshold", "flush"])
@pytest.mark.parametrize("form", ["onepass", "off32", "defer", "serial"])
def test_k7_one_wave_renders_all_tiles(eng, form, name):
    """AVDB_OPT_K7_GRID = 1: one wave takes the tiles one after another, so its LDS images
    go staged -> direct -> staged and every flush must leave them zero; the chunks two
    tiles share are stored by the same wave in order.  (The default grid above is the
    concurrent case.)"""
    _run(eng, _case(eng, name), form, grid=1)


# ---------------------------------------------------------------------------
# 256-record groups
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["onepass", "off32"])
def test_k7_256_record_groups_repeated_pattern(eng, form):
    """From 4 Mi records on a group is four tiles that one wave renders in turn.  The edge
    pattern (all builders, max_seq_len 50) repeated to just over (4 << 20) + 4099 records;
    its record count is no multiple of 256 and its heap length is odd, so tile positions
    and allele phases rotate from period to period.  Expected: the pattern's text
    repeated, its offsets plus k times the period's totals."""
    from annotatedvdb_amd.engine import RecordBatch
    pat = K.batch(K.pattern_records())
    P, H = pat.n, pat.heap_bytes
    n = (4 << 20) + 4101
    assert n >= K.SMALL_GROUP_N and P % 256 and H % 2
    reps = -(-n // P)
    per = np.repeat(np.arange(reps, dtype=np.int64), P)[:n]
    tile = lambda a: np.tile(a, reps)[:n]  # noqa: E731
    dgp = K.digest_rows(P, seed=13)
    state, keys, paths = K.expected(pat.recs, 50, digests=dgp)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)  # noqa: E731
    heap = dev(np.tile(pat.heap, reps))
    db = RecordBatch(chrom=dev(tile(pat.chrom)), pos=dev(tile(pat.pos)), allele_off=dev(tile(pat.allele_off) + per * H),
                     ref_len=dev(tile(pat.ref_len)), alt_len=dev(tile(pat.alt_len)), heap=heap,
                     ext_id=dev(tile(pat.ext_id)))
    code, dig = dev(tile(pat.code)), dev(np.tile(dgp, (reps, 1))[:n].reshape(-1))
    kt = eng.new_key_text(n, heap.numel(), paths=True, off32=form == "off32")
    _fill(kt)
    eng.primary_keys(db, code=code, digest=dig, out=kt)
    assert torch.equal(kt.state[:n], dev(tile(np.array(state, dtype=np.uint8))))
    ex = K.exemptions(pat.recs, state, keys)
    for name, text, got_off, want_text, exempt in (("keys", kt.keys, kt.key_offsets(n), keys, ex),
                                                   ("paths", kt.paths, kt.path_offsets(n), paths, [None] * P)):
        off = _offsets([len(x) for x in want_text])
        want_off = np.concatenate([np.tile(off[:-1], reps) + np.repeat(np.arange(reps, dtype=np.int64) * off[-1], P),
                                   [reps * off[-1]]])[: n + 1]
        assert torch.equal(got_off, dev(want_off)), name
        tot = int(want_off[n])
        mask = np.ones(int(off[-1]), dtype=bool)
        for i, e in enumerate(exempt):
            if e:
                mask[off[i] + e[0]:off[i] + e[1]] = False
        want = dev(np.tile(np.frombuffer(b"".join(want_text), dtype=np.uint8), reps)[:tot])
        diff = torch.nonzero((text[:tot] != want) & dev(np.tile(mask, reps)[:tot]))
        if diff.numel():
            at = int(diff[0])
            i = int(np.searchsorted(want_off, at, side="right")) - 1
            raise AssertionError((name, int(diff.numel()), i, i % P, pat.recs[i % P],
                                  text[int(want_off[i]):int(want_off[i + 1])].cpu().numpy().tobytes(), want_text[i % P]))
        assert bool((text[tot:] == SENT).all()), (name, "bytes behind the total")

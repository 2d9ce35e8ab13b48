"""K3 (in-batch dedup) and K6 (key-set join) where synth data cannot reach: long
records that differ in one byte, `X, Y, X` runs, every grouped kernel form, and the
hash tables' collision fallbacks, wrap and size steps on inputs built to collide
(tests/hash_common.py).

Expected `keep` is keep-first per (chrom, pos, ref bytes, alt bytes, ext) from a Python
set; expected K6 matches are a first-index dict plus ``O.existing_match``.  The
collision counts come from hash_common's restatement of the hashes: if it drifted
from the device, the asserts on AVDB_CTR_HASH_COLLISIONS fail.

The second grid-stride trip of the K3 / K6 kernels is not run here:
``stream_grid(..., 4096)`` never strides below 1 M records, and the existing large
tests (C1, C4k, the 500,000-record parity check) cover it.
"""

import ctypes
import functools

import numpy as np
import pytest

import hash_common as H
from annotatedvdb_amd.chromosomes import CHROM_NAMES
from oracle import avdb_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("chrom", "pos", "allele_off", "ref_len", "alt_len", "heap", "ext_id")
COOP = 64                      # kCoopBytes: longer compares are wave-cooperative
DUMMY = (0, 1, b"N", b"N", 0)  # leading record that the unaligned views leave out
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@pytest.fixture(autouse=True)
def _poison(engine):
    old = engine.poison
    engine.poison = 0xA5
    yield
    engine.poison = old


def _N():
    from annotatedvdb_amd import _native
    return _native


def _pack(recs):
    from annotatedvdb_amd.engine import pack_records
    return pack_records([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs],
                        [r[4] for r in recs])


def _bases(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def _other(rng, c):
    return int(rng.choice([x for x in b"ACGT" if x != c]))


def _flip(rng, body, d):
    return body[:d] + bytes([_other(rng, body[d])]) + body[d + 1:]


def _snv(pos, k=0):
    return (21, pos, b"ACGT"[k & 3:(k & 3) + 1], b"CGTA"[k & 3:(k & 3) + 1], 0)


# ---------------------------------------------------------------------------
# K3 grouped: the three kernel forms
# ---------------------------------------------------------------------------
def _grouped_forms(engine, recs):
    """keep and AVDB_CTR_DUPLICATES of `recs` from the list form, the no-workspace
    form (k_dedup_grouped4) and the one-record-per-lane form (k_dedup_grouped, through
    views that start one record in).  All three read one heap."""
    from annotatedvdb_amd.engine import RecordBatch
    N = _N()
    n = len(recs)
    full = _pack([DUMMY] + list(recs)).to(engine.device)
    assert int(full.allele_off[-1]) + int(full.ref_len[-1]) + int(full.alt_len[-1]) == full.heap.numel()
    view = RecordBatch(**{f: (getattr(full, f)[1:] if f != "heap" else full.heap) for f in FIELDS})
    flat = RecordBatch(**{f: (getattr(full, f)[1:].clone() if f != "heap" else full.heap) for f in FIELDS})
    assert flat.chrom.data_ptr() % 4 == 0 and flat.pos.data_ptr() % 16 == 0
    assert view.chrom.data_ptr() % 4 != 0 and view.pos.data_ptr() % 16 != 0
    out = {}
    ctr = engine.new_counters()
    out["list"] = (engine.pk_dedup(flat, grouped=True, counters=ctr), ctr)
    # exactly Engine.pk_dedup's call, but workspace = NULL, 0
    ctr = engine.new_counters()
    keep = engine.empty(n, torch.uint8)
    assert keep.data_ptr() % 4 == 0
    N.check("avdb_pk_dedup", engine.lib.avdb_pk_dedup(
        engine.ctx, N.ptr(flat.chrom), N.ptr(flat.pos), N.ptr(flat.allele_off), N.ptr(flat.ref_len),
        N.ptr(flat.alt_len), N.ptr(flat.heap), flat.heap.numel(), N.ptr(flat.ext_id), n, 1, None, 0,
        N.ptr(keep), N.ptr(ctr), engine._stream()))
    out["no-workspace"] = (keep, ctr)
    ctr = engine.new_counters()
    out["per-lane"] = (engine.pk_dedup(view, grouped=True, counters=ctr), ctr)
    return {k: (v[0].cpu().numpy()[:n], int(v[1][N.CTR_DUPLICATES])) for k, v in out.items()}


def _check_grouped(engine, recs):
    want = np.array(H.keep_first(recs), dtype=np.uint8)
    got = _grouped_forms(engine, recs)
    for name, (keep, dups) in got.items():
        bad = np.nonzero(keep != want)[0]
        assert bad.size == 0, (name, bad[:8].tolist(), keep[bad[:8]].tolist())
        assert dups == int((want == 0).sum()), name
    assert np.array_equal(got["list"][0], got["no-workspace"][0])
    assert np.array_equal(got["list"][0], got["per-lane"][0])
    return want


ONE_BYTE_L = (65, 72, 511, 512, 513, 520, 1027, 2000)


def _one_byte_positions(L):
    return sorted(set([0, 63, 64, L - 1] + ([511, 512] if L > 512 else [])))


@functools.lru_cache(maxsize=None)
def _one_byte_batch():
    """Per (L, differing byte d, d in REF / in ALT) one position holding X, X' (X with
    byte d changed) and a copy of X'; SNVs between; two identical long records with
    ext 7 and 9 (and a third with 7); last, flush with the heap end, the L = 1027 case
    whose byte L - 1 differs."""
    rng = np.random.default_rng(2024)
    cases = []
    for L in ONE_BYTE_L:
        for d in _one_byte_positions(L):
            splits = []
            if d < L - 1:
                splits.append(d + 1 + (L - 2 - d) // 2)  # d in REF
            if d >= 1:
                splits.append(max(1, d // 2))            # d in ALT
            for r in splits:
                cases.append((L, d, r))
    last = [c for c in cases if c[0] == 1027 and c[1] == 1026]
    cases = [c for c in cases if c not in last] + last
    recs, pos = [], 5000
    for k, (L, d, r) in enumerate(cases):
        for _ in range(0 if (L, d, r) in last else k % 3):
            pos += 1
            recs.append(_snv(pos, k))
        pos += 1
        x = _bases(rng, L)
        y = _flip(rng, x, d)
        e = (0, 7)[k & 1]
        recs += [(21, pos, x[:r], x[r:], e), (21, pos, y[:r], y[r:], e), (21, pos, y[:r], y[r:], e)]
        if k == 5:  # same bytes and lengths, another refSNP id
            pos += 1
            z = _bases(rng, 300)
            recs += [(21, pos, z[:120], z[120:], 7), (21, pos, z[:120], z[120:], 9), (21, pos, z[:120], z[120:], 7)]
    return tuple(recs)


def _one_byte_cover(recs):
    """{(L, d, 'ref' | 'alt')} of adjacent long records at one position with equal
    lengths and ext that differ in exactly one byte — read off the records."""
    found = set()
    for a, b in zip(recs, recs[1:]):
        if a[:2] != b[:2] or a[4] != b[4] or len(a[2]) != len(b[2]) or len(a[3]) != len(b[3]):
            continue
        x = np.frombuffer(a[2] + a[3], dtype=np.uint8)
        y = np.frombuffer(b[2] + b[3], dtype=np.uint8)
        diff = np.nonzero(x != y)[0]
        if x.size > COOP and diff.size == 1:
            found.add((x.size, int(diff[0]), "ref" if diff[0] < len(a[2]) else "alt"))
    return found


def test_k3_grouped_one_differing_byte(engine):
    """Two long records at one position that differ in one byte are both kept, a copy of
    the second is dropped: at every step / tail shape of the cooperative compare, the
    byte in REF and in ALT, the last compare served by the heap end's zero fill; equal
    bytes under another ext are kept.  All three grouped forms."""
    recs = list(_one_byte_batch())
    cover = _one_byte_cover(recs)
    for L in ONE_BYTE_L:
        for d in _one_byte_positions(L):
            assert {k for (l, p, k) in cover if (l, p) == (L, d)}, (L, d)
        assert {k for (l, p, k) in cover if l == L} == {"ref", "alt"}, L
    ext_runs = [i for i in range(len(recs) - 1)
                if recs[i][:4] == recs[i + 1][:4] and (recs[i][4], recs[i + 1][4]) == (7, 9)
                and len(recs[i][2]) + len(recs[i][3]) > COOP]
    assert len(ext_runs) >= 1
    lastL = len(recs[-1][2]) + len(recs[-1][3])
    assert lastL > COOP and lastL % 8 and recs[-1] == recs[-2]  # (flush with the heap end: _grouped_forms)
    want = _check_grouped(engine, recs)
    for i in ext_runs:
        assert want[i] == 1 and want[i + 1] == 1
    assert want[-1] == 0 and want[-2] == 1 and want[-3] == 1


# `X` and other capitals: long records of one (ref_len, alt_len), each letter other bytes;
# `s`: a short record of another length.
XYX_PATTERNS = ("XYX", "XYZX", "XYZWX", "XsX", "XYYX", "XYsX", "XYXZYX", "XXYX", "XYZ", "XYsZX")


def _list_chunk_records(n):
    """Records per workgroup of the list form (k_dedup_mark4's chunk_of, restated)."""
    ngroups = (n + 3) // 4
    grid = min(4096, max(1, -(-ngroups // 512)))
    return 4 * -(-ngroups // grid)


def _xyx_bounds(n):
    return sorted(set(range(256, n, 256)) | set(range(_list_chunk_records(n), n, _list_chunk_records(n))))


@functools.lru_cache(maxsize=None)
def _xyx_batch(n=5000):
    """Runs of XYX_PATTERNS at consecutive positions between 0-2 SNVs; a run is placed
    across every wave (256), workgroup (1,024) and list-chunk boundary.  Returns the
    records and each run's [start, end)."""
    rng = np.random.default_rng(77)
    bounds = _xyx_bounds(n)
    recs, runs, pos = [], [], 100000
    while len(recs) < n - 12:
        i = len(recs)
        nb = next((b for b in bounds if b > i), None)
        if nb is not None and nb - i <= 10:
            fill = max(0, nb - 2 + (len(runs) & 1) - i)
        else:
            fill = int(rng.integers(0, 3))
        for _ in range(fill):
            pos += 1
            recs.append(_snv(pos, len(recs)))
        pat = XYX_PATTERNS[len(runs) % len(XYX_PATTERNS)]
        L = int(rng.integers(65, 600)) if len(runs) % 7 else int(rng.integers(513, 1100))
        r = int(rng.integers(1, L))
        x = _bases(rng, L)
        at = rng.choice(L, size=3, replace=False)
        body = {"X": x, "Y": _flip(rng, x, int(at[0])), "Z": _flip(rng, x, int(at[1])), "W": _flip(rng, x, int(at[2]))}
        pos += 1
        start = len(recs)
        for ch in pat:
            recs.append((21, pos, b"AC", b"G", 7) if ch == "s" else (21, pos, body[ch][:r], body[ch][r:], 7))
        runs.append((start, len(recs)))
    while len(recs) < n:
        pos += 1
        recs.append(_snv(pos, len(recs)))
    return tuple(recs), tuple(runs)


def _xyx_cover(recs, keep):
    """For every dropped long record: how many records of its lengths and ext but other
    bytes, and whether a short record, stand between it and its first occurrence."""
    first, between, short_between = {}, set(), 0
    for i, r in enumerate(recs):
        f = first.setdefault(r, i)
        if keep[i] or len(r[2]) + len(r[3]) <= COOP:
            continue
        mid = recs[f + 1:i]
        assert all(m[:2] == r[:2] for m in mid)
        between.add(sum(1 for m in mid if m != r and m[4] == r[4] and (len(m[2]), len(m[3])) == (len(r[2]), len(r[3]))))
        short_between += any(len(m[2]) + len(m[3]) <= COOP and len(m[2]) != len(r[2]) for m in mid)
    return between, short_between


def test_k3_grouped_xyx_runs(engine):
    """A true duplicate behind one, two and three long records of its own lengths that
    differ from it (dedup_record's mismatch branch: scan on past the candidate), also with
    a short record between; hundreds of runs, so several lanes of a wave are pending with
    different outcomes, across lane-of-4, wave, workgroup and list-chunk boundaries."""
    n = 5000
    recs, runs = _xyx_batch(n)
    recs = list(recs)
    assert len(recs) == n and len(runs) >= 200
    want = np.array(H.keep_first(recs), dtype=np.uint8)
    between, short_between = _xyx_cover(recs, want)
    assert {1, 2, 3} <= between and short_between >= 10
    assert 3 <= min(e - s for s, e in runs) and max(e - s for s, e in runs) == 6
    assert any(s // 4 != (e - 1) // 4 for s, e in runs)
    bounds = [b for b in _xyx_bounds(n) if b < n - 12]
    assert {256, 1024, 2048, _list_chunk_records(n)} <= set(bounds)
    for b in bounds:
        assert any(s < b <= e - 1 for s, e in runs), b
    # several long suspects in one wave of the list form's resolve (64 suspects per wave)
    assert int((want == 0).sum()) >= 400
    assert np.array_equal(_check_grouped(engine, recs), want)


# ---------------------------------------------------------------------------
# K3 mark: the wave-aggregated append of suspects (wave_append, avdb_wave.hpp), in
# k_dedup_mark4 and in the keyed K2
# ---------------------------------------------------------------------------
def _distinct(n):
    return [(21, 1000 + i, b"A", b"C", 0) for i in range(n)]


def _share(recs, first, last, alts):
    """Records first .. last at record first's position, their ALT from `alts`."""
    for k, i in enumerate(range(first, last + 1)):
        recs[i] = (21, recs[first][1], b"A", alts[k:k + 1], 0)
    return recs


@functools.lru_cache(maxsize=None)
def _append_cases():
    """name -> (records, suspects): the records that share their predecessor's
    position, all of them listed by both mark forms (each repeats lengths and id)."""
    return {
        # four suspects in every lane of four waves and a three-record scalar tail
        "every-lane": (tuple([(21, 500, b"A", b"C", 0)] * 1027), 1026),
        # lane 63 of the first wave alone (it also issues the wave's atomic)
        "lane-63": (tuple(_share(_distinct(1027), 251, 255, b"CCGGC")), 4),
        "lane-0": (tuple(_share(_distinct(1027), 0, 1, b"CC")), 1),
        # the second wave's lane 0, its predecessor the first wave's last record
        "next-wave-lane-0": (tuple(_share(_distinct(1027), 255, 256, b"CC")), 1),
        "none": (tuple(_distinct(4096)), 0),
    }


def _oracle_keep(b):
    import oracle
    h = {f: getattr(b, f).cpu().numpy() for f in FIELDS}
    keep = np.empty(b.n, dtype=np.uint8)
    d = oracle.c_oracle().avdb_oracle_dedup_grouped(
        h["chrom"].ctypes.data, h["pos"].ctypes.data, h["allele_off"].ctypes.data, h["ref_len"].ctypes.data,
        h["alt_len"].ctypes.data, h["heap"].ctypes.data, h["ext_id"].ctypes.data, b.n, keep.ctypes.data)
    return keep, int(d)


def _list_counts(ws):
    """The per-workgroup suspect counts at the head of a K3 list workspace that was
    filled with 0xA5 bytes before the mark ran: the entries the mark wrote."""
    head = ws[:16384].view(torch.int32).cpu().numpy().view(np.uint32)
    return head[head != 0xA5A5A5A5]


@pytest.mark.parametrize("keyed", [False, True], ids=["mark4", "keyed-k2"])
@pytest.mark.parametrize("case", ["every-lane", "lane-63", "lane-0", "next-wave-lane-0", "none"])
def test_k3_mark_wave_append(engine, case, keyed):
    """Suspects in every lane, in the wave's last lane only, in its first lane only, in
    the next wave's first lane only, and in no lane (no atomic: every workgroup's list
    count stays 0): keep and AVDB_CTR_DUPLICATES equal the C oracle's, from pk_dedup's
    own mark and from the keyed record prep's marks."""
    N = _N()
    recs, suspects = _append_cases()[case]
    n = len(recs)
    assert sum(1 for x, y in zip(recs, recs[1:]) if x[:2] == y[:2]) == suspects
    b = _pack(list(recs)).to(engine.device)
    want, ndup = _oracle_keep(b)
    assert ndup == int((want == 0).sum())
    assert ndup == {"every-lane": 1026, "lane-63": 3, "lane-0": 1, "next-wave-lane-0": 1, "none": 0}[case]
    ws = torch.full((16384 + 4 * (((n + 3) & ~3) + (1 << 22)),), 0xA5, dtype=torch.uint8, device=engine.device)
    if keyed:
        kt = engine.primary_keys(b, code=engine.record_prep(b, want_lcp=False)[1])
        engine.record_prep(b, want_lcp=False, keys=kt, dedup_workspace=ws)
        assert "marks" in engine._pending
    ctr = engine.new_counters()
    keep = engine.pk_dedup(b, grouped=True, counters=ctr, workspace=ws)
    assert "marks" not in engine._pending
    counts = _list_counts(ws)
    assert counts.size >= 1 and int(counts.sum()) == suspects, counts[:8].tolist()
    bad = np.nonzero(keep.cpu().numpy()[:n] != want)[0]
    assert bad.size == 0, bad[:8].tolist()
    assert int(ctr[N.CTR_DUPLICATES]) == ndup


# ---------------------------------------------------------------------------
# K3 hash path
# ---------------------------------------------------------------------------
def _hash_dedup(engine, recs):
    N = _N()
    ctr = engine.new_counters()
    keep = engine.pk_dedup(_pack(recs).to(engine.device), grouped=False, counters=ctr)
    return keep.cpu().numpy()[:len(recs)], int(ctr[N.CTR_DUPLICATES]), int(ctr[N.CTR_HASH_COLLISIONS])


def _check_hash(engine, recs, collisions):
    want = np.array(H.keep_first(recs), dtype=np.uint8)
    keep, dups, coll = _hash_dedup(engine, recs)
    print("K3 hash path: n = %d, AVDB_CTR_HASH_COLLISIONS predicted %d, observed %d"
          % (len(recs), collisions, coll))
    bad = np.nonzero(keep != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), keep[bad[:8]].tolist())
    assert dups == int((want == 0).sum())
    assert coll == collisions
    return want


def test_k3_hash_unsorted_xyx(engine):
    recs, _ = _xyx_batch(5000)
    perm = np.random.default_rng(5).permutation(len(recs))
    recs = [recs[i] for i in perm]
    want = _check_hash(engine, recs, 0)
    assert int((want == 0).sum()) >= 400


def test_k3_hash_unsorted_synth(engine):
    from annotatedvdb_amd import synth
    from annotatedvdb_amd.engine import RecordBatch
    N = _N()
    n = 50_000
    b = synth.alleles(n, seed=91, long_frac=0.3, dup_frac=0.3)
    perm = torch.from_numpy(np.random.default_rng(6).permutation(n)).to(b.device)
    p = RecordBatch(**{f: (getattr(b, f)[perm].contiguous() if f != "heap" else b.heap) for f in FIELDS})
    h = {f: getattr(p, f).cpu().numpy() for f in FIELDS}
    heap = h["heap"].tobytes()
    seen, want = set(), np.ones(n, dtype=np.uint8)
    for i in range(n):
        o, L = int(h["allele_off"][i]), int(h["ref_len"][i]) + int(h["alt_len"][i])
        k = (int(h["chrom"][i]), int(h["pos"][i]), int(h["ref_len"][i]), heap[o:o + L], int(h["ext_id"][i]))
        if k in seen:
            want[i] = 0
        seen.add(k)
    assert int((want == 0).sum()) > n // 5
    ctr = engine.new_counters()
    keep = engine.pk_dedup(p, grouped=False, counters=ctr).cpu().numpy()
    assert np.array_equal(keep, want)
    assert int(ctr[N.CTR_DUPLICATES]) == int((want == 0).sum()) and int(ctr[N.CTR_HASH_COLLISIONS]) == 0


def _spread(rng, base, groups):
    """`base` with each group's members inserted at random places, in the group's order."""
    keyed = [(float(i), 0, r) for i, r in enumerate(base)]
    for g, members in enumerate(groups):
        at = np.sort(rng.uniform(0, len(base), len(members)))
        keyed += [(float(a), 1 + g, m) for a, m in zip(at, members)]
    keyed.sort(key=lambda t: (t[0], t[1]))
    return [t[2] for t in keyed]


@functools.lru_cache(maxsize=None)
def _k3_collision_batch():
    rng = np.random.default_rng(11)
    groups = []
    for k in range(8):  # equal fingerprints by alleles (one of them long: a cooperative-size compare)
        rl, al = ((12, 8), (9, 7), (70, 30), (1, 15))[k % 4]
        a = (int(rng.integers(0, 25)), int(rng.integers(1, 10 ** 8)), _bases(rng, rl), _bases(rng, al), (0, 7)[k & 1])
        groups.append((a, H.colliding_record_by_alleles(a)))
    for k in range(8):  # equal fingerprints by position and ext
        a = (int(rng.integers(0, 25)), int(rng.integers(1, 10 ** 8)), _bases(rng, 1 + k % 3), _bases(rng, 1),
             (0, 7, -5, 1 << 40)[k % 4])
        groups.append((a, H.colliding_record_by_position(a, a[1] + 1 + 1000 * k)))
    # [A, B] / [A, B, B] / [B, A, A] / [A, B, A, B]: in the last three a true duplicate of
    # the slot's loser stands later, so the fallback scan has to find it
    shapes = ((0, 1), (0, 1, 1), (1, 0, 0), (0, 1, 0, 1))
    members = [[g[j] for j in shapes[k % 4]] for k, g in enumerate(groups)]
    n_base = 3000 - sum(len(m) for m in members)
    base = [(int(rng.integers(0, 25)), 1000 + 3 * i, _bases(rng, 1 + i % 4), _bases(rng, 1), (0, 7, 9)[i % 3])
            for i in range(n_base)]
    return tuple(_spread(rng, base, members)), tuple(groups)


def test_k3_hash_constructed_collisions(engine):
    """Record pairs with equal fingerprints (by alleles, and by position + ext with
    identical alleles: the winner check's (chrom, pos) guard): keep-first stays exact
    through k_dedup_resolve's fallback scan, and the collision counter equals the number
    of records whose slot winner is another key."""
    recs, groups = _k3_collision_batch()
    recs = list(recs)
    assert len(recs) == 3000 and len(groups) == 16
    for a, b in groups:
        assert a != b and H.k3_fingerprint(a) == H.k3_fingerprint(b)
    assert sum(1 for a, b in groups if a[1] == b[1]) >= 8 and sum(1 for a, b in groups if a[1] != b[1]) >= 8
    collided = {r for g in groups for r in g}
    assert sum(1 for r in recs if r in collided) <= 64
    predicted = H.k3_predict_collisions(recs)
    assert predicted >= 16
    want = _check_hash(engine, recs, predicted)
    # a dropped record whose slot winner is another key: only the scan finds its duplicate
    first = {}
    for i, r in enumerate(recs):
        first.setdefault(H.k3_fingerprint(r), i)
    assert sum(1 for i, r in enumerate(recs) if not want[i] and recs[first[H.k3_fingerprint(r)]] != r) >= 8


def test_k3_hash_wrap_at_last_slot(engine):
    """Distinct records whose home slot is the last of 1,024: the probe wraps to slot 0."""
    at_last = H.k3_records_at_slot(1023, 1024, 5)
    assert len(at_last) >= 3 and len(set(at_last)) == len(at_last)
    rng = np.random.default_rng(12)
    base = [(1, 100 + i, _bases(rng, 1), _bases(rng, 2), 0) for i in range(300)]
    recs = _spread(rng, base, [at_last + [at_last[-1]]])
    assert len(recs) <= 512 and H.slots(len(recs)) == 1024
    want = _check_hash(engine, recs, 0)
    assert int((want == 0).sum()) == 1


@pytest.mark.parametrize("n", [1, 2, 512, 513, 1024, 1025])
def test_k3_hash_table_size_steps(engine, n):
    rng = np.random.default_rng(n)
    distinct = n if n == 1 else n - max(1, n // 4)
    recs = [(2, 10 + i // 2, _bases(rng, 1 + i % 3), b"ACGT"[i % 2:i % 2 + 1], 0) for i in range(distinct)]
    recs += [recs[int(k)] for k in rng.integers(0, distinct, n - distinct)]
    if n > 2:
        recs = [recs[i] for i in rng.permutation(n)]
    sz = ctypes.c_size_t()
    engine.lib.avdb_pk_dedup_workspace_size(n, ctypes.byref(sz))
    assert sz.value == 8 * n + 12 * H.slots(n) + 256  # fp[n] u64 | keys[slots] u64 | idx[slots] u32
    want = _check_hash(engine, recs, H.k3_predict_collisions(recs))
    assert int((want == 0).sum()) == n - distinct


# ---------------------------------------------------------------------------
# K6
# ---------------------------------------------------------------------------
LONG_LAST_KEY = b"1:77:" + b"A" * 40 + b":G"  # (the key blob ends in a key longer than any probe)


def _keyset(engine, keys):
    off = np.zeros(len(keys) + 1, dtype=np.int64)
    if keys:
        np.cumsum([len(k) for k in keys], out=off[1:])
    kt = torch.from_numpy(np.frombuffer(b"".join(keys), dtype=np.uint8).copy()).to(engine.device)
    ot = torch.from_numpy(off).to(engine.device)
    return engine.keyset_build(kt, ot), kt, ot


def _record_of(ms):
    c, p, r, a = H.split_metaseq(ms)
    return (CHROM_NAMES.index(c.decode()), int(p), r, a)


def _metaseq(rec):
    return b"%s:%d:%s:%s" % (CHROM_NAMES[rec[0]].encode(), rec[1], rec[2], rec[3])


def _first_index(keys):
    first = {}
    for i, k in enumerate(keys):
        first.setdefault(k.decode("latin-1"), i)
    return first


def _expect_records(keys, recs, check_alt):
    """match, kind and the strings K6 looks up (exact; switched after an exact miss)."""
    N = _N()
    first = _first_index(keys)
    match, kind, lookups = [], [], []
    for rec in recs:
        if rec[0] >= 25:
            match.append(-1)
            kind.append(N.MATCH_HOST)
            continue
        ms = _metaseq(rec)
        m = O.existing_match(first, ms.decode("latin-1"), check_alt)
        exact = first.get(ms.decode("latin-1"), -1) >= 0
        match.append(m)
        kind.append(N.MATCH_EXACT if exact else (N.MATCH_SWITCHED if m >= 0 else N.MATCH_NONE))
        lookups.append(ms)
        if not exact and check_alt:
            lookups.append(_metaseq((rec[0], rec[1], rec[3], rec[2])))
    return np.array(match, dtype=np.int32), np.array(kind, dtype=np.uint8), lookups


def _check_records(engine, ks, keys, recs, check_alt, label=""):
    N = _N()
    match, kind, lookups = _expect_records(keys, recs, check_alt)
    predicted = H.k6_predict_collisions(keys, lookups)
    b = _pack([r + (0,) for r in recs]).to(engine.device)
    ctr = engine.new_counters()
    m, k = engine.keyset_probe(*ks, b, check_alt, ctr)
    m, k = m.cpu().numpy(), k.cpu().numpy()
    coll = int(ctr[N.CTR_HASH_COLLISIONS])
    print("K6 records %s check_alt=%d: AVDB_CTR_HASH_COLLISIONS predicted %d, observed %d"
          % (label, check_alt, predicted, coll))
    bad = np.nonzero((m != match) | (k != kind))[0]
    assert bad.size == 0, (bad[:8].tolist(), m[bad[:8]].tolist(), match[bad[:8]].tolist(), k[bad[:8]].tolist())
    assert int(ctr[N.CTR_EXISTING]) == int((match >= 0).sum())
    assert coll == predicted
    return match, kind, predicted


def _check_text(engine, ks, keys, strings, skip=None, label=""):
    N = _N()
    first = _first_index(keys)
    live = [s for i, s in enumerate(strings) if skip is None or not skip[i]]
    match = np.array([-1 if skip is not None and skip[i] else first.get(s.decode("latin-1"), -1)
                      for i, s in enumerate(strings)], dtype=np.int32)
    predicted = H.k6_predict_collisions(keys, live)
    off = np.zeros(len(strings) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    q = torch.from_numpy(np.frombuffer(b"".join(strings), dtype=np.uint8).copy()).to(engine.device)
    sk = None if skip is None else torch.from_numpy(np.asarray(skip, dtype=np.uint8)).to(engine.device)
    ctr = engine.new_counters()
    m = engine.keyset_probe_text(*ks, q, torch.from_numpy(off).to(engine.device), len(strings), sk, ctr).cpu().numpy()
    coll = int(ctr[N.CTR_HASH_COLLISIONS])
    print("K6 text %s: AVDB_CTR_HASH_COLLISIONS predicted %d, observed %d" % (label, predicted, coll))
    bad = np.nonzero(m != match)[0]
    assert bad.size == 0, (bad[:8].tolist(), m[bad[:8]].tolist(), match[bad[:8]].tolist())
    assert int(ctr[N.CTR_EXISTING]) == int((match >= 0).sum())
    assert coll == predicted
    return match, predicted


def _ordinary_keys(rng, n, chroms=(2, 23)):
    alle = (b"A", b"C", b"G", b"T", b"AC", b"GTT", b"ACGTACGTA")
    pos = rng.choice(10 ** 8, size=n, replace=False) + 1
    return [b"%d:%d:%s:%s" % (int(rng.integers(*chroms)), int(p), alle[int(rng.integers(0, 7))],
                               alle[int(rng.integers(0, 4))]) for p in pos]


@functools.lru_cache(maxsize=None)
def _k6_collision_keys():
    """2,000 ordinary keys and 12 colliding pairs (A, B), three of each of: only A is a
    key, only B, both with A first, both with B first — spread through the key array.
    A + "T" and B + "T" are keys too and stand before them all: keys that a compare
    without the length test would take for A and B."""
    rng = np.random.default_rng(21)
    pairs = H.colliding_metaseq_pairs(12)
    members = [((a,), (b,), (a, b), (b, a))[k % 4] for k, (a, b) in enumerate(pairs)]
    keys = [s + b"T" for p in pairs for s in p] + _spread(rng, _ordinary_keys(rng, 2000), members) + [LONG_LAST_KEY]
    return tuple(keys), tuple(pairs)


@pytest.mark.parametrize("check_alt", [True, False])
def test_k6_constructed_collisions(engine, check_alt):
    """Keys with equal 64-bit hashes: the slot's owner is the first of them, a probe for
    the other is counted as a collision and resolved by the exact scan — found when it
    is a key (also as the switched form of a record), missed when it is not."""
    keys, pairs = _k6_collision_keys()
    keys = list(keys)
    first = _first_index(keys)
    for k, (a, b) in enumerate(pairs):
        assert a != b and H.k6_hash(a) == H.k6_hash(b)
        assert ((a.decode("latin-1") in first), (b.decode("latin-1") in first)) == \
            ((True, False), (False, True), (True, True), (True, True))[k % 4]
    ks = _keyset(engine, keys)
    rng = np.random.default_rng(22)
    recs = []
    for a, b in pairs:
        ra, rb = _record_of(a), _record_of(b)
        # A, B, and records whose switched form is B / A
        recs += [ra, rb, (rb[0], rb[1], rb[3], rb[2]), (ra[0], ra[1], ra[3], ra[2])]
    recs += [_record_of(keys[int(i)]) for i in rng.integers(24, len(keys) - 1, 300)]
    recs += [_record_of(k) for k in _ordinary_keys(rng, 100)]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    match, kind, predicted = _check_records(engine, ks, keys, recs, check_alt, "collisions")
    assert predicted >= 12
    N = _N()
    by_rec = {r: (int(m), int(k)) for r, m, k in zip(recs, match, kind)}
    for k, (a, b) in enumerate(pairs):
        ra, rb = _record_of(a), _record_of(b)
        sw_b = (rb[0], rb[1], rb[3], rb[2])
        if k % 4 == 0:    # only A is a key: B misses (its collision is in `predicted`)
            assert by_rec[rb] == (-1, N.MATCH_NONE) and by_rec[ra][1] == N.MATCH_EXACT
            assert by_rec[sw_b] == (-1, N.MATCH_NONE)
        elif k % 4 == 2:  # A owns the slot, B is found by the scan, also as a switched form
            assert by_rec[rb] == (first[b.decode("latin-1")], N.MATCH_EXACT)
            assert by_rec[sw_b] == ((first[b.decode("latin-1")], N.MATCH_SWITCHED) if check_alt
                                    else (-1, N.MATCH_NONE))
    if check_alt:  # (the string entry once)
        strings = [s for p in pairs for s in p] + [keys[int(i)] for i in rng.integers(0, len(keys), 300)] + \
            _ordinary_keys(rng, 100) + [pairs[0][1] + b"T", pairs[0][1] + b"TT"]
        strings = [strings[i] for i in rng.permutation(len(strings))]
        _, predicted = _check_text(engine, ks, keys, strings, label="collisions")
        assert predicted >= 12


def test_k6_first_hit_under_duplicate_keys(engine):
    rng = np.random.default_rng(23)
    keys = _ordinary_keys(rng, 1500)
    dups = [b"7:%d:AC:G" % (500 + d) for d in range(5)]
    want = {}
    for d, s in enumerate(dups):
        at = sorted(int(x) for x in rng.choice(len(keys), size=3, replace=False))
        for j in at:
            keys[j] = s
    first = _first_index(keys)
    for s in dups:
        idx = [i for i, k in enumerate(keys) if k == s]
        assert len(idx) == 3 and idx[2] - idx[0] > 1
        want[s] = idx[0]
    ks = _keyset(engine, keys)
    match, kind, _ = _check_records(engine, ks, keys, [_record_of(s) for s in dups], True, "duplicate keys")
    assert match.tolist() == [want[s] for s in dups] == [first[s.decode()] for s in dups]
    tmatch, _ = _check_text(engine, ks, keys, dups, label="duplicate keys")
    assert tmatch.tolist() == match.tolist()


def test_k6_labels_positions_and_host_contigs(engine):
    """Contig labels 1 / 9 / 10 / 22 / X / Y / M and 1- to 10-digit positions as
    metaseq_prefix renders them; contig codes >= 25 go to the host uncounted."""
    N = _N()
    rng = np.random.default_rng(24)
    recs = [(c, p, b"AC", b"G") for c in (0, 8, 9, 21, 22, 23, 24) for p in (1, 9, 10, 999999999, 4294967295)]
    strings = [b"%s:%d:AC:G" % (CHROM_NAMES[c].encode(), p) for c, p, _, _ in recs]
    assert b"X:4294967295:AC:G" in strings and b"10:1:AC:G" in strings and b"M:9:AC:G" in strings
    keys = _spread(rng, _ordinary_keys(rng, 200), [[s] for s in strings])
    ks = _keyset(engine, keys)
    host = [(25, 1, b"AC", b"G"), (255, 9, b"AC", b"G"), (25, 4294967295, b"AC", b"G")]
    match, kind, _ = _check_records(engine, ks, keys, recs + host, True, "labels")
    assert match[:len(recs)].tolist() == [keys.index(s) for s in strings]
    assert kind[:len(recs)].tolist() == [N.MATCH_EXACT] * len(recs)
    assert match[len(recs):].tolist() == [-1] * 3 and kind[len(recs):].tolist() == [N.MATCH_HOST] * 3
    tmatch, _ = _check_text(engine, ks, keys, strings, label="labels")
    assert tmatch.tolist() == match[:len(recs)].tolist()


def test_k6_near_misses(engine):
    N = _N()
    near = [b"1:5:A:GG", b"1:5:AG:G", b"1:50:A:G", b"11:5:A:G"]
    one = [b"1:5:A:G", b"1:7:C:C", b"3:9:T:T"]
    ks = _keyset(engine, one)
    probes = [_record_of(s) for s in near] + [(0, 5, b"G", b"A"), (0, 5, b"A", b"G"), (0, 7, b"C", b"C"), (0, 8, b"C", b"C")]
    m, k, _ = _check_records(engine, ks, one, probes, True, "near misses")
    assert m.tolist() == [-1, -1, -1, -1, 0, 0, 1, -1]
    assert k.tolist() == [0, 0, 0, 0, N.MATCH_SWITCHED, N.MATCH_EXACT, N.MATCH_EXACT, 0]  # REF == ALT: never SWITCHED
    m, k, _ = _check_records(engine, ks, one, probes, False, "near misses")
    assert m.tolist() == [-1, -1, -1, -1, -1, 0, 1, -1] and k.tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    tm, _ = _check_text(engine, ks, one, near + [b"1:5:G:A", b"1:5:A:G", b"1:5:A:", b"1:5:A:G\0"], label="near misses")
    assert tm.tolist() == [-1, -1, -1, -1, -1, 0, -1, -1]
    # the other way round
    ks = _keyset(engine, near)
    for check_alt in (True, False):
        m, k, _ = _check_records(engine, ks, near, [(0, 5, b"A", b"G"), (0, 5, b"G", b"A")] + [_record_of(s) for s in near],
                                 check_alt, "near keys")
        assert m.tolist() == [-1, -1, 0, 1, 2, 3]
    tm, _ = _check_text(engine, ks, near, [b"1:5:A:G"] + near, label="near keys")
    assert tm.tolist() == [-1, 0, 1, 2, 3]


@pytest.mark.parametrize("n_keys", [0, 1, 512, 513, 1024, 1025])
def test_k6_key_count_steps(engine, n_keys):
    """1,024 slots up to 512 keys, 2,048 from 513, 4,096 from 1,025; no key at all."""
    keys = [b"2:%d:C:T" % (i + 1) for i in range(n_keys)]
    ks = _keyset(engine, keys)
    assert ks[0].numel() == 12 * H.slots(n_keys)
    assert (n_keys == 0) == (ks[1].numel() == 0)  # (then the engine passes keys = NULL)
    present = [keys[i] for i in sorted({0, n_keys // 2, n_keys - 1} & set(range(n_keys)))]
    strings = present + [b"2:%d:C:T" % (n_keys + 1), b"2:1:C:TT", b"22:1:C:T"]
    match, kind, _ = _check_records(engine, ks, keys, [_record_of(s) for s in strings], True, "n_keys=%d" % n_keys)
    assert int((match >= 0).sum()) == len(present)
    tmatch, _ = _check_text(engine, ks, keys, strings, label="n_keys=%d" % n_keys)
    assert tmatch.tolist() == match.tolist()
    if n_keys > 1:  # every key, in one probe
        m, _ = _check_text(engine, ks, keys, keys, label="n_keys=%d all" % n_keys)
        assert m.tolist() == list(range(n_keys))


def test_k6_wrap_at_last_slot(engine):
    at_last = H.k6_keys_at_slot(1023, 1024, 6)
    assert len(at_last) >= 4 and len(set(at_last)) == len(at_last)
    rng = np.random.default_rng(25)
    inside, absent = at_last[:-1], at_last[-1]
    keys = _spread(rng, _ordinary_keys(rng, 300, chroms=(2, 23)), [[s] for s in inside])
    assert len(keys) <= 512 and H.slots(len(keys)) == 1024
    assert sum(1 for k in keys if H.k6_home(H.k6_hash(k), 1024) == 1023) >= 3
    ks = _keyset(engine, keys)
    strings = inside + [absent]
    match, kind, _ = _check_records(engine, ks, keys, [_record_of(s) for s in strings], True, "wrap")
    assert match.tolist() == [keys.index(s) for s in inside] + [-1]
    tmatch, _ = _check_text(engine, ks, keys, strings, label="wrap")
    assert tmatch.tolist() == match.tolist()


def test_k6_probe_text_skip(engine):
    rng = np.random.default_rng(26)
    keys = _ordinary_keys(rng, 600)
    ks = _keyset(engine, keys)
    strings = [keys[int(i)] for i in rng.integers(0, len(keys), 200)] + _ordinary_keys(rng, 50)
    skip = [int(i % 3 == 1) * (1 + i % 250) for i in range(len(strings))]  # (any non-zero byte skips)
    match, _ = _check_text(engine, ks, keys, strings, skip=skip, label="skip")
    assert all(m == -1 for m, s in zip(match, skip) if s)
    unskipped, _ = _check_text(engine, ks, keys, strings, label="no skip")
    assert int((unskipped >= 0).sum()) > int((match >= 0).sum()) > 0

"""k4_common's builders cover what test_gpu_k4_edges.py relies on them to cover (no
kernel: the GPU tests tie the restated block arithmetic to the device)."""

import k4_common as K
from oracle import avdb_oracle as O


def test_block_and_bucket_arithmetic():
    assert K.AL_FIXED_BYTES == 68 + 54 == len(O.vrs_allele_blob("x" * 32, b""))
    assert K.blocks(0) == 2 and K.blocks(117) == 2 and K.blocks(118) == 3
    assert K.bucket(3701) == 30 and K.bucket(3702) == 31 and K.bucket(65_537) == 31
    assert K.blocks(10_000) == 80 and K.blocks(65_537) == 514
    for k in range(3, 45):  # 128 k - 139: the last length of k blocks
        assert K.blocks(128 * k - 139) == k and K.blocks(128 * k - 138) == k + 1
    # the padded message of an a-byte ALT: hashlib's own block count
    for a in (0, 117, 118, 3701, 3702):
        assert K.blocks(a) == (len(O.vrs_allele_blob("x" * 32, b"A" * a)) + K.SHA_PAD_BYTES + 127) // 128
    assert [K.ndigits(x) for x in (0, 9, 10, 999999999, 1000000000, K.U32_MAX)] == [1, 1, 2, 9, 10, 10]


def test_sequence_digests_span_the_alphabet():
    d = K.SEQ_DIGESTS
    assert len(d) == K.N_CONTIGS == len(set(d))
    for s in d:
        assert len(s) == 32 and "-" in s and "_" in s and set(s.encode()) <= set(K.B64URL)
    assert len(set("".join(d))) >= 60  # (of the alphabet's 64)


def _no_repeat(b):
    return all(x != y for x, y in zip(b, b[1:])) and set(b) <= set(b"ACGT")


def test_alt_length_cases():
    lens = K.alt_lengths()
    recs = K.alt_length_records()
    assert len(lens) == 649 and [len(r[3]) for r in recs] == lens
    assert sum(lens) == 572_491
    assert set(range(521)) <= set(lens)
    assert {a % 128 for a in lens if a <= 520} == set(range(128))
    assert {K.blocks(a) for a in lens} == set(range(2, 46)) | {80, 514}
    for k in range(3, 45):
        assert {128 * k - 140, 128 * k - 139, 128 * k - 138} <= set(lens)
    clamp = [a for a in lens if K.bucket(a) == K.CLAMP_BUCKET]
    assert len(clamp) >= 40 and len({K.blocks(a) for a in clamp}) >= 15
    assert {K.bucket(a) for a in lens} == set(range(2, 32))
    for c, pos, ref, alt in recs:
        assert len(ref) == K.REF_LEN and c < K.N_CONTIGS and pos >= 1
        assert _no_repeat(ref) and _no_repeat(alt)
    assert len({r[3] for r in recs if len(r[3]) >= 16}) == sum(1 for a in lens if a >= 16)


def test_position_cases():
    recs = K.position_records()
    forms = K.position_forms()
    assert sorted(forms) == list(K.DIGIT_SUMS)
    assert len(recs) == K.N_CONTIGS * (len(K.DIGIT_SUMS) + 1)
    pairs = {(r[0], K.digit_sum(r)) for r in recs}
    assert pairs == {(c, s) for c in range(K.N_CONTIGS) for s in K.DIGIT_SUMS}
    used = {(r[1] - 1, len(r[2])) for r in recs}
    assert used == {f for fs in forms.values() for f in fs}  # every form, on some contig
    assert {(0, 1), (1, 1), (9, 1), (10, 60), (70, 60), (999999999, 1), (1000000000, 60),
            (K.TOP_START, 60)} <= used
    assert {K.ndigits(r[1]) for r in recs} == set(range(1, 11))  # (the key text's position)
    for r in recs:
        assert 1 <= r[1] and r[1] - 1 + len(r[2]) <= K.U32_MAX and K.is_long(r)
        assert _no_repeat(r[2]) and _no_repeat(r[3])
    assert {r[0] for r in recs if r[1] - 1 == K.TOP_START} == set(range(K.N_CONTIGS))
    assert any(len(r[3]) == 0 for r in recs)
    # ALTs of the 1-base REFs: 2 and 3 blocks, the suffix on both sides of the block edge
    assert {K.blocks(len(r[3])) for r in recs if len(r[2]) == 1} == {2, 3}


def test_mix():
    mix = K.mix_records()
    n = len(mix)
    assert n % 4 == 3
    long_ = [r for r in mix if K.is_long(r)]
    short = [r for r in mix if not K.is_long(r)]
    every = set(K.alt_length_records()) | set(K.position_records())
    assert every <= set(long_)
    assert len(short) >= len(every) // 2 - 1
    assert any(len(r[2]) == 1 and len(r[3]) == 1 for r in short) and any(len(r[2]) != len(r[3]) for r in short)
    assert {r[0] for r in long_ if r[0] >= K.N_CONTIGS} == {25, 200, 255}
    assert {r[0] for r in short if r[0] >= K.N_CONTIGS} == {25, 200}
    # shuffled: long and short alternate irregularly, buckets are spread over the batch
    flags = [K.is_long(r) for r in mix]
    assert 0.2 * n < sum(1 for x, y in zip(flags, flags[1:]) if x != y) < 0.7 * n
    first = [K.bucket(len(r[3])) for r in mix[: n // 4] if K.is_long(r)]
    assert len(set(first)) >= 20 and K.CLAMP_BUCKET in first
    assert K.mix_records() is mix  # (built once)


def test_expected_is_the_oracle_serialisation():
    # vrs-python's published VRS 1.1 example (tests/test_oracle_golden.py): APOE rs7412
    digs = list(K.SEQ_DIGESTS)
    digs[18] = "IIB53T8CNeJJdUqzn9V_JnRtQadwWCbl"
    rec = (18, 44908822, b"C", b"T")
    assert K.expected(digs, [rec], 1, schema="1.1") == [b"EgHPXXhULTwoP4-ACfs-YCXaeUQJBjH_"]
    assert K.expected(digs, [rec], 2, schema="1.1") == [None]
    assert K.expected(digs, [(25,) + rec[1:], (200,) + rec[1:]], 1) == [b"?" * 32] * 2
    # the default schema: location digest inside the Allele blob, both through sha512t24u
    recs = [K.alt_length_records()[0], K.alt_length_records()[300], K.position_records()[0],
            K.position_records()[19], (3, 5, b"A", b"G")]
    want = []
    for c, pos, ref, alt in recs[:4]:
        loc = O.sha512t24u(O.vrs_location_blob(K.SEQ_DIGESTS[c], pos - 1, pos - 1 + len(ref)))
        assert loc != O.sha512t24u(O.vrs_location_blob(K.SEQ_DIGESTS[(c + 1) % 25], pos - 1, pos - 1 + len(ref)))
        want.append(O.sha512t24u(O.vrs_allele_blob(loc, alt)).encode())
    got = K.expected(K.SEQ_DIGESTS, recs)
    assert got == want + [None] and all(len(g) == 32 for g in got[:4])
    assert K.expected(K.SEQ_DIGESTS, recs[4:], 1)[0] is not None

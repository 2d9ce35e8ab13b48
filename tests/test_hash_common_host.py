"""hash_common's builders against hash_common's own restatement of the K3 / K6 hashes
(no kernel: the GPU tests tie the restatement to the device through the collision
counter)."""

import pytest

import hash_common as H


def test_mixer_is_a_64_bit_permutation_step():
    assert H.mix(0) == 0
    assert H.mix(1) == 0xB456BCFC34C2CB2C  # fmix64(1), MurmurHash3's published finaliser
    assert H.mix(1 << 64 | 5) == H.mix(5)
    assert len({H.mix(x) for x in range(4096)}) == 4096


def test_slot_rule():
    assert [H.slots(n) for n in (0, 1, 512, 513, 1024, 1025, 2048, 2049)] == \
        [1024, 1024, 1024, 2048, 2048, 4096, 4096, 8192]


def test_k6_hash_known_pair_and_closing():
    a, b = b"1:1000:ACGTACGTAT:G", b"1:1000:CK9\xf2\xe5L\xc5/BT:G"
    assert H.k6_hash(a) == H.k6_hash(b) == 0x82E8B167693CD42D
    assert H.colliding_strings(a, b[:8]) == b
    # the length closes the hash: zero bytes appended change it, 256 of them included
    # in the partial word only through the (len << 56) term
    assert len({H.k6_hash(b"\0" * n) for n in range(0, 24)}) == 24
    assert H.k6_hash(b"") == H.mix(H.IV) and H.k6_hash(b"\0" * 3) == H.mix(H.IV ^ (3 << 56))


def test_colliding_strings_and_metaseq_pairs():
    pairs = H.colliding_metaseq_pairs(12)
    assert len(pairs) == 12 and len({a for a, _ in pairs}) == 12
    for a, b in pairs:
        assert a != b and len(a) == len(b) and H.k6_hash(a) == H.k6_hash(b)
        ca, pa, ra, aa = H.split_metaseq(a)
        cb, pb, rb, ab = H.split_metaseq(b)
        assert (ca, pa, aa) == (cb, pb, ab) and ra != rb and len(ra) == len(rb)
        assert H.k6_predict_collisions([a], [b]) == 1 and H.k6_predict_collisions([a, b], [a, b]) == 1
        assert H.k6_predict_collisions([b], [b]) == 0
    with pytest.raises(ValueError):
        H.colliding_strings(b"short", b"12345678")
    with pytest.raises(ValueError):
        H.colliding_strings(b"0123456789abcdef", b"01234567")


def test_colliding_records_of_both_kinds():
    base = (3, 123456, b"ACGTACGTACGT", b"TTGACA", 7)
    x = H.colliding_record_by_alleles(base)
    assert x != base and x[:2] == base[:2] and x[4] == base[4]
    assert (len(x[2]), len(x[3])) == (len(base[2]), len(base[3]))
    assert H.k3_fingerprint(x) == H.k3_fingerprint(base)
    for p2, e in ((123457, 0), (5, -3), (4294967295, 1 << 62)):
        r = (3, 123456, b"A", b"G", e)
        y = H.colliding_record_by_position(r, p2)
        assert y[1] == p2 and y[2:4] == r[2:4] and -(1 << 63) <= y[4] < (1 << 63)
        assert H.k3_fingerprint(y) == H.k3_fingerprint(r)
    assert H.k3_predict_collisions([base, x, x, base]) == 2
    assert H.keep_first([base, x, x, base]) == [1, 1, 0, 0]
    # the fingerprint covers every field
    fps = {H.k3_fingerprint(r) for r in (base, (4,) + base[1:], base[:1] + (1,) + base[2:],
                                          base[:4] + (9,), (3, 123456, b"ACGTACGTACGTT", b"TGACA", 7),
                                          (3, 123456, b"ACGTACGTACGT", b"TTGACC", 7))}
    assert len(fps) == 6
    with pytest.raises(ValueError):
        H.colliding_record_by_alleles((0, 1, b"ACGT", b"ACGT", 0))


def test_slot_search_reaches_the_last_slot():
    keys = H.k6_keys_at_slot(1023, 1024, 99)
    assert len(keys) >= 3 and len(set(keys)) == len(keys)
    assert all(H.k6_home(H.k6_hash(k), 1024) == 1023 for k in keys)
    recs = H.k3_records_at_slot(1023, 1024, 99)
    assert len(recs) >= 3 and len(set(recs)) == len(recs)
    assert all(H.k3_home(H.k3_fingerprint(r), 1024) == 1023 for r in recs)

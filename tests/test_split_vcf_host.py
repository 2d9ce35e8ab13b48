"""K15 (a whole-genome VCF split by chromosome) through the library's host entries
(avdb_vcf_split_size_host / avdb_vcf_split_write_host on an avdb_ctx_create(-1, ...)
context): the same per-line code the kernels run, checked against the reference's own
files (tests/golden/split_vcf.tsv.gz) and a restatement of the rule.  No GPU."""

import ctypes
import gzip
import os

import numpy as np
import pytest

import split_vcf_common as S
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import ChromMap, Engine

EXCEPTIONS = {"KeyError": KeyError, "UnicodeDecodeError": UnicodeDecodeError}


@pytest.fixture(scope="module")
def host():
    return Engine("host")


def run_driver(eng, tmp_path, name, text, with_map, extra=(), suffix=""):
    from annotatedvdb_amd import split_vcf_by_chr as D
    src = tmp_path / (name + suffix)
    src.write_bytes(gzip.compress(text) if suffix.endswith(".gz") else text)
    out = tmp_path / ("out_" + name + suffix.replace(".", "_") + "_".join(extra[:2]).replace("-", ""))
    argv = ["-f", str(src), "-o", str(out)] + (["-c", S.CHRMAP] if with_map else []) + list(extra)
    return out, D.main(argv, engine=eng)


def check_files(out, want, lines):
    assert sorted(os.listdir(out)) == sorted(want)
    for name, data in want.items():
        assert (out / name).read_bytes() == data, name
        assert lines[name[3:-4]] == data.count(b"\n") - 1, name  # (the header line is not a data line)


# ---- 1: the golden ------------------------------------------------------------------
def check_golden(eng, tmp_path, suffixes=(".vcf", ".vcf.gz")):
    runs, _ = S.golden()
    assert set(runs) == {"run1", "run2"}
    for name, (text, with_map, want) in runs.items():
        assert len(want) == 25 and text.count(b"\n") > 2800
        for suffix in suffixes:
            out, lines = run_driver(eng, tmp_path, name, text, with_map, suffix=suffix)
            check_files(out, want, lines)


def test_s1_golden_files(host, tmp_path):
    check_golden(host, tmp_path)


def test_s1_golden_holds_what_it_should():
    runs, cases = S.golden()
    text1, _, files1 = runs["run1"]
    assert not text1.endswith(b"\n") and b"\r\n" in text1 and b" \t \r\n" in text1 and b"\n#\n" in text1
    assert all(len(v) > len(S.HEADER) and v.startswith(S.HEADER) for v in files1.values())
    assert b"\r" not in b"".join(files1.values())
    n_fields = {len(line.split(b"\t")) for line in files1["chr1.vcf"].split(b"\n")[1:-1]}
    assert 8 in n_fields and max(n_fields) > 8
    text2, with_map, files2 = runs["run2"]
    assert with_map and b"NC_000001.11\t" in text2 and b"\n7\t" in text2
    keys = [line.split(b"\t")[0] for line in text2.split(b"\n")[2:60]]
    assert len(set(keys)) >= 20 and sum(a != b for a, b in zip(keys, keys[1:])) > 50  # contigs interleaved line by line
    raised = {c: e for c, e, _, _ in cases}
    assert raised["chr_prefix"] == raised["mt"] == raised["empty_line"] == raised["unmapped_accession"] == "KeyError"
    assert raised["lone_ff_at_end"] == "UnicodeDecodeError" and raised["label_ok"] is None


def check_cases(eng):
    _, cases = S.golden()
    for case, raised, with_map, line in cases:
        cm = eng.split_chrom_map(S.chrmap()) if with_map else None
        if raised is None:
            res = eng.split_vcf(line, cm)
            assert sum(res.counts["lines"][:25]) + res.counts["comments"] == 1 and res.first_other is None, case
        else:
            with pytest.raises(EXCEPTIONS[raised]) as info:
                eng.split_vcf(line, cm)
            if raised == "KeyError":
                assert info.value.line == 1, case
    # what the KeyError carries: the key the reference's dict lookup raises with
    for line, with_map, key in ((b"1\t5\nchr1\t7\n", False, "chr1"), (b"#c\n\n", False, ""),
                                (b"NW_1.1\t5\n", True, "NW_1.1"), (b"NT_187361.1\t5\n", True, "Un_KI270302v1"),
                                (b"J01415.2\t5\n", True, "MT")):
        with pytest.raises(KeyError) as info:
            eng.split_vcf(line, eng.split_chrom_map(S.chrmap()) if with_map else None)
        assert info.value.args == (key,) and info.value.line == 2 - with_map, line
    with pytest.raises(ValueError):
        eng.split_vcf(b"1\t5\n", unknown="drop")


def test_s1_recorded_exceptions(host):
    check_cases(host)


# ---- 2: the rule, array for array ---------------------------------------------------------
@pytest.mark.parametrize("name,text", S.edge_slabs(), ids=[n for n, _ in S.edge_slabs()])
def test_s2_edge_slabs(host, name, text):
    code, start, out_len, cnt, off, blob, dst = S.check_against_ref(host, text, what=name)
    flagged = int(sum(bool(int(x) & S.HOST) for x in out_len))
    if name.startswith("tail_"):
        assert flagged == 5 and cnt[N.SPLIT_COUNT_HOST_LINES] == 5
    elif name == "lone_ff_tail":
        assert flagged == 1
    else:
        assert flagged == 0, name  # the same bytes mid-line are not flagged
    if name == "labels":
        assert code.tolist() == list(range(25))
    if name in ("near_labels", "whitespace_only"):
        assert set(code.tolist()) == {S.OTHER}
    if name == "bare_keys":  # (a bare `1 ` is the label 1 after the strip; before a tab it is no label)
        assert code.tolist()[:25] == list(range(25)) and code.tolist()[25:].count(S.OTHER) == len(S.NEAR_LABELS) - 1
    if name == "hash_after_blank":
        assert code.tolist() == [S.OTHER, S.OTHER, S.NONE, S.NONE]
    if name == "label_and_tabs":
        assert code.tolist() == [22, 0, 23, S.OTHER] and out_len.tolist() == [2, 2, 2, 3]


def test_s2_map_rule(host):
    mapping = S.chrmap()
    cm = ChromMap.for_split(host, mapping)
    text = S.map_slab(mapping)
    code, _, _, cnt, _, _, _ = S.check_against_ref(host, text, mapping, cm, "map")
    assert cnt[N.SPLIT_COUNT_LINES + S.OTHER] > 20 and len(set(code.tolist())) == 26
    # this script's rule, not K0's: no MT -> M step, the plain key 7 is looked up as text
    by_key = {k: c for k, c in zip((l.split(b"\t")[0] for _, l in S.split_lines(text)), code.tolist())}
    assert by_key[b"J01415.2"] == S.OTHER and by_key[b"7"] == 6 and by_key[b"CM000685.2"] == 22
    assert by_key[b"NT_187361.1"] == S.OTHER and by_key[b"1"] == S.OTHER
    k0 = ChromMap(host, mapping)  # the existing constructor is as it was
    assert k0.n_keys == cm.n_keys == len(mapping)


# ---- 3: capacity and sentinels --------------------------------------------------------
def check_capacity(eng):
    text = S.golden()[0]["run1"][0]
    code, start, out_len, cnt, off, blob, dst = S.ref_split(text)
    _, _, _, g_cnt, st = S.raw_size(eng, text)
    cap = len(blob)
    assert g_cnt == cnt and cap > 100_000
    for short in (cap - 1, cap // 2, 0):
        rc, front, out, totals, _, _ = S.raw_write(eng, st, short)
        # (the device entry does not wait for its own scan: it reports through totals)
        assert rc == (N.AVDB_ERANGE if eng.host_only else 0) and totals == [cap, 1]
        assert (front == 0xA5).all() and (out == 0xA5).all()  # nothing is written at all
    for room in (cap, cap + 8):
        rc, front, out, totals, g_off, _ = S.raw_write(eng, st, room, want_dst=False)
        assert rc == 0 and totals == [cap, 0] and np.array_equal(g_off, off)
        assert (front == 0xA5).all() and (out[cap:] == 0xA5).all() and out[:cap].tobytes() == blob


def test_s3_capacity_and_sentinels(host):
    check_capacity(host)


def check_patched_lines(eng):
    """What the write pass makes of the arrays a caller changed: a shorter out_len is a prefix,
    a code outside 0..25 and an out_len of 0 give no output, bit 31 is ignored."""
    import torch
    text = b"1\t5\tAAAA\n2\t6\n1\t7\n3\t8\n"
    _, _, _, _, st = S.raw_size(eng, text)
    st["out_len"][0] = 4 | (1 << 31) - (1 << 32)  # "1\t5" + LF, LINE_HOST still set
    st["code"][1] = N.SPLIT_NONE
    st["out_len"][3] = 0
    st["code"][2] = 24
    rc, _, out, totals, off, dst = S.raw_write(eng, st, 8)
    assert rc == 0 and totals == [8, 0] and out[:8].tobytes() == b"1\t5\n1\t7\n"
    assert off.tolist() == [0] + [4] * 24 + [8, 8] and dst.tolist() == [0, 2 ** 64 - 1, 4, 2 ** 64 - 1]
    assert isinstance(st["out_len"], torch.Tensor)


def test_s3_patched_lines(host):
    check_patched_lines(host)


def test_s3_argument_checks(host):
    sz = ctypes.c_size_t()
    assert host.lib.avdb_vcf_split_workspace_size(100, 3, None) == N.AVDB_EINVAL
    assert host.lib.avdb_vcf_split_workspace_size(100, 3, ctypes.byref(sz)) == 0 and sz.value % 256 == 0
    z = np.zeros(N.SPLIT_N_COUNTS, np.uint64)
    t = np.frombuffer(b"1\t5\n", np.uint8)
    a8, a64, a32 = np.zeros(1, np.uint8), np.zeros(1, np.uint64), np.zeros(1, np.uint32)
    call = lambda name, *args: N.call(name, *args, check=False)  # noqa: E731
    # the device entries refuse bad arguments before any GPU work (this context has no GPU)
    assert call("avdb_vcf_split_size", host.ctx, None, 5, 1, None, a8, a64, a32, z, None, 0, None) == N.AVDB_EINVAL
    assert call("avdb_vcf_split_size", host.ctx, t, 4, 1, None, a8, a64, a32, z, None, 0, None) == N.AVDB_ERANGE
    assert call("avdb_vcf_split_write", host.ctx, t, 4, 1, a8, a64, a32, a8, 1, None, None, a64, None, 0,
                None) == N.AVDB_EINVAL
    assert call("avdb_vcf_split_size_host", None, t, 4, 1, None, a8, a64, a32, z) == N.AVDB_EINVAL  # no context
    assert call("avdb_vcf_split_size_host", host.ctx, None, 4, 1, None, a8, a64, a32, z) == N.AVDB_EINVAL  # null text
    assert call("avdb_vcf_split_size_host", host.ctx, t, 4, 5, None, a8, a64, a32, z) == N.AVDB_EINVAL  # lines > bytes
    assert call("avdb_vcf_split_size_host", host.ctx, t, 4, 1, None, None, a64, a32, z) == N.AVDB_EINVAL
    assert call("avdb_vcf_split_size_host", host.ctx, t, 4, 1, None, a8, a64, a32, None) == N.AVDB_EINVAL
    off, tot = np.zeros(27, np.uint64), np.zeros(2, np.uint64)
    assert call("avdb_vcf_split_write_host", host.ctx, t, 4, 1, a8, a64, a32, None, 4, off, None, tot) == N.AVDB_EINVAL
    assert call("avdb_vcf_split_write_host", host.ctx, t, 4, 1, a8, a64, a32, a8, 0, None, None, tot) == N.AVDB_EINVAL
    assert call("avdb_vcf_split_write_host", host.ctx, t, 4, 1, a8, None, a32, a8, 0, off, None, tot) == N.AVDB_EINVAL
    # no lines: NULL arrays are fine, the offsets and the totals are written
    off[:] = 7
    assert call("avdb_vcf_split_write_host", host.ctx, None, 0, 0, None, None, None, None, 0, off, None, tot) == 0
    assert off.tolist() == [0] * 27 and tot.tolist() == [0, 0]


# ---- 4: the engine ----------------------------------------------------------------------
def check_engine(eng):
    planted = [b"NW_1.1\t5\tA\tC", b"chrUn\t6", b"", b"MT\t7"]
    lines = [S.vcf_line(S.LABELS[i % 25], i) for i in range(120)]
    for k, p in zip((3, 40, 41, 119), planted):
        lines.insert(k, p)
    text = b"\n".join(lines) + b"\n"
    res = eng.split_vcf(text, unknown="keep")
    assert res.other_text.cpu().numpy().tobytes() == b"".join(p + b"\n" for p in planted)
    assert res.first_other == 3 and res.counts["lines"][S.OTHER] == 4 and res.counts["host_lines"] == 0
    assert res.stream_off[26] == res.text.numel() == sum(res.counts["bytes"])
    assert res.stream(0).cpu().numpy().tobytes() == b"".join(l + b"\n" for l in lines if l.startswith(b"1\t"))
    with pytest.raises(IndexError):
        res.stream(26)
    with pytest.raises(KeyError) as info:
        eng.split_vcf(text)
    assert info.value.args == ("NW_1.1",) and info.value.line == 4
    empty = eng.split_vcf(b"")
    assert empty.text.numel() == 0 and empty.stream_off == [0] * 27 and empty.first_other is None


def check_host_lines(eng):
    """Lines the host decides: a planted 0x1F tail that turns an unknown key into `1`, tails
    Python strips, a comment, and the order of the two errors."""
    text = b"2\t5\n1\x1f\n1\t7\xc2\xa0 \n#c\x1e\n3\t8\xc2\x85\n1\t9\x1c\x1d\t\n4\t1\xe2\x80\x83\n5\t2\xc3\xa9\n"
    res = eng.split_vcf(text)
    assert res.counts["host_lines"] == 7 and res.first_other is None and res.counts["comments"] == 1
    assert res.stream(0).cpu().numpy().tobytes() == b"1\n1\t7\n1\t9\n"
    assert res.stream(2).cpu().numpy().tobytes() == b"3\t8\n" and res.stream(3).cpu().numpy().tobytes() == b"4\t1\n"
    assert res.stream(4).cpu().numpy().tobytes() == b"5\t2\xc3\xa9\n"  # a character rstrip() keeps
    assert res.counts["lines"][:5] == [3, 1, 1, 1, 1] and sum(res.counts["bytes"]) == res.text.numel()
    bad = b"1\t5\xff\n"
    with pytest.raises(UnicodeDecodeError):
        eng.split_vcf(b"1\t1\n" + bad + b"chr1\t2\n")  # the decode error comes first
    with pytest.raises(KeyError):
        eng.split_vcf(b"chr1\t2\n" + bad)              # the unplaced line comes first
    with pytest.raises(UnicodeDecodeError):
        eng.split_vcf(b"chr1\t2\n" + bad, unknown="keep")
    with pytest.raises(UnicodeDecodeError):
        eng.split_vcf(b"#note \xff\n")
    # a host line that ends unplaced is the first unplaced line
    with pytest.raises(KeyError) as info:
        eng.split_vcf(b"1\t1\n1 \tx\x1f\n")
    assert info.value.args == ("1 ",) and info.value.line == 2


def test_s4_engine_keep_and_raise(host):
    check_engine(host)


def test_s4_host_lines(host):
    check_host_lines(host)


# ---- 5: the driver ----------------------------------------------------------------------
def test_s5_driver_slabs_and_unplaced(host, tmp_path):
    runs, _ = S.golden()
    for name, (text, with_map, want) in runs.items():
        out, lines = run_driver(host, tmp_path, name, text, with_map, extra=("--batchBytes", "4096"), suffix=".vcf.gz")
        check_files(out, want, lines)  # many slabs give the files of one slab
    text, _, want = runs["run1"]
    planted = [b"chr1\t5\trs1\tA\tC\t.\t.\t.", b"GL000009.2\t7", b""]
    lines = text.split(b"\n")
    for k, p in zip((10, 1500, 2900), planted):
        lines.insert(k, p + b" \r")
    mixed = b"\n".join(lines)
    unplaced = tmp_path / "unplaced.txt"
    out, n = run_driver(host, tmp_path, "mixed", mixed, False, extra=("--batchBytes", "30000", "--unplaced", str(unplaced)))
    check_files(out, want, n)
    assert unplaced.read_bytes() == b"".join(p + b"\n" for p in planted)
    with pytest.raises(KeyError) as info:
        run_driver(host, tmp_path, "mixed2", mixed, False, extra=("--batchBytes", "30000"))
    assert info.value.args == ("chr1",) and info.value.line == 11
    # the files of a run that raised hold their header lines (the first slab was not written)
    assert all((tmp_path / "out_mixed2batchBytes_30000" / ("chr%s.vcf" % c.decode())).read_bytes() == S.HEADER
               for c in S.LABELS)
    from annotatedvdb_amd import split_vcf_by_chr as D
    with pytest.raises(SystemExit):
        D.main(["-o", str(tmp_path / "x")], engine=host)
    with pytest.raises(SystemExit):
        D.main(["-f", "a", "-o", str(tmp_path / "x"), "--batchBytes", "0"], engine=host)
    assert not (tmp_path / "x").exists()
    empty = tmp_path / "empty.vcf"
    empty.write_bytes(b"")
    assert set(D.main(["-f", str(empty), "-o", str(tmp_path / "e")], engine=host).values()) == {0}
    assert len(os.listdir(tmp_path / "e")) == 25

"""K14 (the VCF files of a variant export) through the library's host entries
(avdb_export_vcf_size_host / avdb_export_vcf_write_host on an avdb_ctx_create(-1, ...)
context): the same per-line code the kernels run, checked against the reference's own
files (tests/golden/export_vcf.tsv.gz) and a restatement of the reference's loop.  No GPU."""

import ctypes
import gzip
import os
import random
import re

import numpy as np
import pytest

import bgzf_common as Z
import export_vcf_common as X
import hash_common as HC
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import Engine


@pytest.fixture(scope="module")
def host():
    return Engine("host")


# ---- 1: the golden ------------------------------------------------------------------
def check_golden(eng, tmp_path):
    rows, files = X.golden()
    text = X.golden_export()
    assert set(files) == {"chr" + c for c in X.GOLDEN_CHROMOSOMES} and len(rows) > 4700
    for c in X.GOLDEN_CHROMOSOMES:
        want = files["chr" + c]
        res = eng.export_vcf(text, contigs=[c], variants_per_file=X.GOLDEN_PER_FILE)
        d = tmp_path / ("chr" + c)
        d.mkdir()
        res.files(str(d), "chr" + c)
        assert sorted(os.listdir(d)) == sorted(n for n in want if not n.endswith(".log")), c
        for name in os.listdir(d):
            assert (d / name).read_bytes() == want[name], (c, name)
        # the closing line of the reference's log: the valid count and the last file's number
        m = re.search(r"Fetched (\d+) valid records from chr%s\. Writing residuals to file (\d+)" % c,
                      want["chr%s.log" % c].decode())
        assert (int(m.group(1)), int(m.group(2))) == (res.counts["valid"], res.n_files), c
        X.check_against_ref(res, text, [c], X.GOLDEN_PER_FILE)
    got = {c: eng.export_vcf(text, contigs=[c], variants_per_file=X.GOLDEN_PER_FILE).counts for c in "12Y"}
    assert got["1"]["valid"] == 2600 and got["1"]["dropped"] == 4 and got["1"]["invalid"] == 60
    assert got["2"]["valid"] == 2000 and files["chr2"]["chr2_3.vcf"] == X.VCF_HEADER  # the header-only third file
    assert got["Y"]["valid"] == got["Y"]["invalid"] == 0 and files["chrY"]["chrY_1.vcf"] == X.VCF_HEADER


def test_v1_golden_files(host, tmp_path):
    check_golden(host, tmp_path)


def test_v1_golden_holds_what_it_should():
    rows, files = X.golden()
    ids = [r[1] for r in rows]
    for letter in b"IRDN":
        assert any(bytes([letter]) in m and not set(b"IRDN") - {letter} & set(m) for m in ids), chr(letter)
    assert any(b"<DEL>" in m for m in ids) and any(re.search(b"[ACGT]{100}N[ACGT]{50}", m) for m in ids)
    assert any(r[2] is None for r in rows) and any(len(r[1]) > 300 and len(r[0]) < 50 for r in rows)
    inv = files["chr1"]["chr1_invalid.txt"].split(b"\n")
    assert b"None" in b"".join(inv) and len({x.split(b"\t")[0] for x in inv if x}) < len([x for x in inv if x])


# ---- 2: fuzzed slabs of every line class ------------------------------------------------
@pytest.mark.parametrize("n_lines", [0, 1, 2, 255, 256, 257, 3200])
def test_v2_fuzzed_slabs(host, n_lines):
    for seed, contigs in ((1, None), (2, ["1", "X", "GL9"])):
        rng = random.Random(100 * n_lines + seed)
        text = X.fuzz_export(rng, X.fuzz_ids(rng), n_lines, repeats=0.05)
        for vpf in (10_000_000, 100):
            res = host.export_vcf(text, contigs=contigs, variants_per_file=vpf)
            _, _, ctr = X.check_against_ref(res, text, contigs, vpf)
        c = res.counts
        assert c["valid"] + c["invalid"] + c["skipped_lines"] + c["filtered"] == n_lines
        if n_lines >= 255:
            assert min(c["valid"], c["invalid"], c["skipped_lines"], c["dropped"]) > 0, c
            assert (c["filtered"] > 0) == (contigs is not None)


def test_v2_line_classes(host):
    L = X.export_line
    for text in (L("1:100:A:C", "1:100:A:C", 5), L("1:100:A:C", "1:100:A:C", 5) + b"\n",
                 L("a", "1:100:A:C", 5) + b"\r\n" + L("b", "1:100:A:<DEL>", 7) + b"\r\n",
                 L("a", "1:100:N:C", None, None) + b"\r\n" + L("b", "1:100:A:I", None, b"") + b"\r\n" +
                 L("c", "1:5:R:A", None, b"\\N") + b"\r\n" + L("d", "1:5:A:D", b"\\N\\N") + b"\textra\r\n",
                 b"\n\n" + L("k", "1:100:A:G") + b"\n\n", X.HEADER_LINE + b"\n" + L("2:5:A:C", "2:5:A:C"),
                 b"lonely\n\nalone\r\n", b"", L("", "1:1:A:C"), L("back\\slash", "1:1:A\\:C", b"\\"),
                 L("k", "1:2:A:N:more:colons", 4), L("k", "N"), L("k", "1:10:a:n\tI")):
        res = host.export_vcf(text)
        X.check_against_ref(res, text)
    res = host.export_vcf(L("k", "1:100:ACGTN:A", None, None) + b"\n" + L("j", "7:1:A:T", 3))
    assert X.files_of(res) == ([b"7\t1\tj\tA\tT\t.\t.\t.\n"], b"k\tNone\n")
    # the contig mask over a whole-table export: the label of the metaseq id decides, not the key's
    ids = ("1:100:A:C", "2:5:A:C", "M:7:G:A", "MT:7:G:A", "GL9:5:A:C", "2:5:A:<DEL>")
    text = b"\n".join(L("9:1:A:C", m) for m in ids) + b"\n"
    for contigs, n in ((["1"], 1), (["2"], 2), (["M"], 1), (["1", "2"], 3), (["GL9"], 2), (None, 6), ([], 0)):
        res = host.export_vcf(text, contigs=contigs)
        X.check_against_ref(res, text, contigs)
        assert res.counts["valid"] + res.counts["invalid"] == n and res.counts["filtered"] == 6 - n
    with pytest.raises(ValueError):
        host.export_vcf(text, variants_per_file=0)
    assert host.export_vcf(b"").n_files == 1 and host.export_vcf(b"").file_span(1) == (0, 0)
    with pytest.raises(IndexError):
        host.export_vcf(b"").file_span(2)


# ---- 3: repeated keys -------------------------------------------------------------------
def colliding_keys():
    """Two different keys with one K6 hash (neither byte a tab or a newline)."""
    a = b"1:12345:ACGTACGTACGTACGT:rs77"
    for c in b"23456789":
        try:
            b = HC.colliding_strings(a, bytes([c]) + a[1:8], forbid=b"\t\n\r")
        except ValueError:
            continue
        assert HC.k6_hash(a) == HC.k6_hash(b) and a != b
        return a, b
    raise AssertionError("no colliding pair")


def check_repeats(eng):
    L = X.export_line
    a, b = colliding_keys()
    # two keys that share pk_hash stay two lines
    text = L(a, "1:5:A:C") + b"\n" + L("x", "1:6:A:C") + b"\n" + L(b, "1:7:A:G") + b"\n"
    res = eng.export_vcf(text)
    assert res.counts["dropped"] == 0 and res.flags.tolist() == [0, 0, 0]
    X.check_against_ref(res, text)
    arrays, _, _ = X.raw_size(eng, text)
    assert arrays["pk_hash"].astype(np.uint64)[0] == arrays["pk_hash"].astype(np.uint64)[2] == HC.k6_hash(a)
    # true repeats collapse to the first place with the last id; the colliding key between them stays
    text = L(a, "1:5:A:C") + b"\n" + L(b, "1:6:A:C") + b"\n" + L(a, "1:7:AT:G") + b"\n" + L("y", "1:8:A:C") + b"\n" + \
        L(a, "1:9:A:GGG") + b"\n"
    res = eng.export_vcf(text)
    files, _, _ = X.check_against_ref(res, text)
    assert files == [b"1\t9\t" + a + b"\tA\tGGG\t.\t.\t.\n1\t6\t" + b + b"\tA\tC\t.\t.\t.\n1\t8\ty\tA\tC\t.\t.\t.\n"]
    assert res.counts["dropped"] == 2
    assert res.flags.tolist() == [N.EXPVCF_ROW_HOST, 0, N.EXPVCF_DROPPED, 0, N.EXPVCF_DROPPED]
    # a pair across a file boundary stays two; inside one file it is one
    text = b"".join(L("k%d" % (i % 4), "1:%d:A:C" % (i + 1)) + b"\n" for i in range(8))
    for vpf, dropped in ((4, 0), (5, 1), (8, 4), (3, 0), (2, 0)):
        res = eng.export_vcf(text, variants_per_file=vpf)
        X.check_against_ref(res, text, None, vpf)
        assert res.counts["dropped"] == dropped and res.n_files == 8 // vpf + 1
    # an invalid row never enters the dict
    text = L("k", "1:5:A:<DEL>") + b"\n" + L("k", "1:6:A:C") + b"\n" + L("k", "1:7:A:N") + b"\n"
    res = eng.export_vcf(text)
    X.check_against_ref(res, text)
    assert res.counts["dropped"] == 0


def check_pk_hash(eng):
    rng = random.Random(66)
    text = X.fuzz_export(rng, X.fuzz_ids(rng), 700, long_allele=300)
    arrays, cnt, _ = X.raw_size(eng, text)
    tb = text
    n = 0
    for s, p, h in zip(arrays["row_start"], arrays["pk_len"], arrays["pk_hash"].astype(np.uint64)):
        assert int(h) == HC.k6_hash(tb[int(s):int(s) + int(p)])
        n += 1
    assert n == cnt["valid"] > 400 and len({int(p) for p in arrays["pk_len"]}) > 20  # keys of many lengths, 0 too
    assert (arrays["out_len"] == arrays["ms_len"] + arrays["pk_len"] + 8).all()


def test_v3_repeated_keys(host):
    check_repeats(host)


def test_v3_pk_hash_is_k6_hash(host):
    check_pk_hash(host)


# ---- 4: capacity and sentinels --------------------------------------------------------
def check_capacity(eng):
    text = X.golden_export()
    _, cnt, st = X.raw_size(eng, text, mask=1 << 0)  # chromosome 1
    want_files, want_invalid, _ = X.ref_export(text, ["1"], 10_000_000)
    # (no repeated key is resolved here: the raw passes render every row, each with its own id)
    want_raw = b"".join(b"\t".join(ms.split(b":")[:2] + [pk] + ms.split(b":")[2:] + [b".", b".", b"."]) + b"\n"
                        for pk, ms, _ in X.golden()[0] if ms.startswith(b"1:") and not re.search(b"I|R|D|N", ms))
    for which, n, cap, tail in ((N.EXPVCF_STREAM_VCF, cnt["valid"], cnt["vcf_bytes"], b"\t.\t.\t.\n"),
                                (N.EXPVCF_STREAM_INVALID, cnt["invalid"], cnt["invalid_bytes"], b"\n")):
        assert cap > 1000
        rc, front, out, totals, off = X.raw_write(eng, st, which, n, cap)
        assert rc == 0 and totals == [cap, 0] and off[0] == 0 and off[-1] == cap
        assert (front == 0xA5).all() and (out[cap:] == 0xA5).all() and out[:cap].tobytes().endswith(tail)
        good = out[:cap].tobytes()
        if which == N.EXPVCF_STREAM_INVALID:
            assert good == want_invalid
        else:
            assert good == want_raw and len(want_raw) > len(want_files[0])
        for short in (cap - 1, cap // 2, 0):
            rc, front, out, totals, _ = X.raw_write(eng, st, which, n, short)
            # (the device entry does not wait for its own scan: it reports through totals)
            assert rc == (N.AVDB_ERANGE if eng.host_only else 0) and totals == [cap, 1]
            assert (front == 0xA5).all() and (out == 0xA5).all()  # nothing is written at all
        rc, front, out2, totals, _ = X.raw_write(eng, st, which, n, cap + 8)
        assert rc == 0 and totals == [cap, 0] and (out2[cap:] == 0xA5).all() and (front == 0xA5).all()
        assert out2[:cap].tobytes() == good


def test_v4_capacity_and_sentinels(host):
    check_capacity(host)
    sz = ctypes.c_size_t()
    assert host.lib.avdb_export_vcf_workspace_size(100, 3, None) == N.AVDB_EINVAL
    assert host.lib.avdb_export_vcf_workspace_size(100, 3, ctypes.byref(sz)) == 0 and sz.value % 256 == 0
    # the device entries refuse bad arguments before any GPU work (this context has no GPU)
    assert N.call("avdb_export_vcf_size", host.ctx, None, 5, 1, 0, *([None] * 10), None, 0, None,
                  check=False) == N.AVDB_EINVAL
    assert N.call("avdb_export_vcf_size_host", None, None, 0, 0, 0, *([None] * 10), check=False) == N.AVDB_EINVAL
    z = np.zeros(2, np.uint64)
    assert N.call("avdb_export_vcf_write_host", host.ctx, None, 0, 0, 2, 0, *([None] * 5), None, 0, z, z,
                  check=False) == N.AVDB_EINVAL  # no such stream


def test_v4_row_host_and_dropped_flags(host):
    """What the write pass makes of the two flags the caller sets: spaces over the length stored, and nothing."""
    L = X.export_line
    text = L("a", "1:5:A:C") + b"\n" + L("b", "1:6:A:C") + b"\n" + L("c", "1:7:A:C") + b"\n"
    _, cnt, st = X.raw_size(host, text)
    fl, out_len = st["vcf"][4], st["vcf"][3]
    fl[0] |= N.EXPVCF_ROW_HOST
    out_len[0] = 5
    fl[1] |= N.EXPVCF_DROPPED
    out_len[1] = 0
    cap = 5 + 16
    rc, _, out, totals, off = X.raw_write(host, st, N.EXPVCF_STREAM_VCF, 3, cap)
    assert rc == 0 and totals == [cap, 0] and off.tolist() == [0, 5, 5, cap]
    assert out[:cap].tobytes() == b"     1\t7\tc\tA\tC\t.\t.\t.\n"


# ---- 5: what raises ---------------------------------------------------------------------
def check_raises(eng):
    L = X.export_line
    for m in ("1:100:A", "1:100:A:C:T", "rs5", ""):
        text = L("1:12:A:C", "1:12:A:C") + b"\n\n" + L("k", m) + b"\n"
        with pytest.raises(ValueError, match="line 3"):
            eng.export_vcf(text)
        with pytest.raises(ValueError):
            X.ref_export(text)
    # the invalid test comes first: such an id is no BAD row
    assert eng.export_vcf(L("k", "1:100:N") + b"\n").counts["invalid"] == 1
    with pytest.raises(ValueError, match="carriage return"):
        eng.export_vcf(b"1:12:A:C\t1:12\r:A:C\n")


def test_v5_bad_rows_and_lone_cr_raise(host):
    check_raises(host)


# ---- 6: the driver ----------------------------------------------------------------------
def test_v6_driver(host, tmp_path):
    from annotatedvdb_amd import export_variant2vcf as D
    from annotatedvdb_amd.parsers import VcfEntryParser
    rows, files = X.golden()
    text = X.golden_export()
    gz, bgz, plain = tmp_path / "export.tsv.gz", tmp_path / "export.bgz.tsv.gz", tmp_path / "export.tsv"
    gz.write_bytes(gzip.compress(text))
    bgz.write_bytes(Z.bgzip(text, block=30000))
    plain.write_bytes(text)
    for path, spec, chroms in ((gz, "all", None), (bgz, "1,chrX,Y", ["1", "X", "Y"]), (plain, "autosome", None)):
        out = tmp_path / ("out_" + spec.replace(",", "_"))
        got = D.main(["--export", str(path), "--chr", spec, "-o", str(out), "--variantsPerFile", "1000", "--maxWorkers",
                      "3"], engine=host)
        chroms = chroms or [str(i) for i in range(1, 23)] + ([] if spec == "autosome" else ["X", "Y", "M"])
        assert list(got) == chroms
        want = {}
        for c in chroms:
            w = files.get("chr" + c) or {"chr%s_1.vcf" % c: X.VCF_HEADER, "chr%s_invalid.txt" % c: b"", "chr%s.log" % c: b""}
            want.update(w)
        assert sorted(os.listdir(out)) == sorted(want)
        for name, data in want.items():
            if not name.endswith(".log"):
                assert (out / name).read_bytes() == data, name
        assert "Fetched 2600 valid records from chr1. Writing residuals to file 3" in (out / "chr1.log").read_text()
        assert got["1"] == {"valid": 2600, "invalid": 60, "dropped": 4, "files": 3}
    assert got["2"]["files"] == 3 and got["3"] == {"valid": 0, "invalid": 0, "dropped": 0, "files": 1}
    # the round trip: every VCF line through the project's parser gives back its key and the export's metaseq id
    ids_of = {}
    for pk, ms, _ in rows:
        ids_of.setdefault(pk, set()).add(ms)
    out, n = tmp_path / "out_all", 0
    for name in sorted(os.listdir(out)):
        if name.endswith(".vcf"):
            lines = (out / name).read_text().split("\n")
            assert lines[0] + "\n" == X.VCF_HEADER.decode() and lines[-1] == ""
            for line in lines[1:-1]:
                entry = VcfEntryParser(line)
                pk = entry.get("id")
                ms = ":".join(str(entry.get(k)) for k in ("chrom", "pos", "ref", "alt"))
                assert ms.encode() in ids_of[pk.encode()], line
                n += 1
    all_counts = D.main(["--export", str(gz), "-o", str(out), "--variantsPerFile", "1000"], engine=host)
    assert n == sum(v["valid"] - v["dropped"] for v in all_counts.values()) > 4600
    with pytest.raises(SystemExit):
        D.main(["--export", str(gz), "-o", str(tmp_path / "x"), "--gusConfigFile", "gus.config"], engine=host)
    with pytest.raises(SystemExit):
        D.main(["-o", str(tmp_path / "x")], engine=host)
    assert not (tmp_path / "x").exists()

"""K12 on the GPU: the --skipExisting key set built from an export
(Engine.existing_table_build, ExistingVariants.from_export) against the library's
host entries, ExistingVariants.from_tsv on the same file, and the loaders' output
with either key set."""

import gzip
import json
import os

import numpy as np
import pytest

import bgzf_common as Z
import existing_common as X
from conftest import GOLDEN
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.chromosomes import CHROM_NAMES, length_table
from oracle import avdb_oracle as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def host():
    from annotatedvdb_amd.engine import Engine
    return Engine("host")


# ---- G1: the host tests' slabs through the device entries ---------------------------
SLABS = [("h1", lambda: X.H1)] + [("h2_%d" % n, (lambda n=n: X.h2(n))) for n in (0, 1, 255, 256, 257, 1023, 1024,
                                                                                  1025, 2049)] + \
        [("h3", X.h3), ("empty", lambda: b"")]


@pytest.mark.parametrize("name,make", SLABS, ids=[s[0] for s in SLABS])
def test_g1_device_equals_host_entries(engine, host, name, make):
    text = make()
    engine.poison = 0xA5
    try:
        got = X.columns(engine, text)
    finally:
        engine.poison = None
    X.assert_same(got, X.columns(host, text))


@pytest.mark.parametrize("labels", [["22", "X"], ["other"], [], None])
def test_g1_contig_mask(engine, host, labels):
    text = X.h4()
    X.assert_same(X.columns(engine, text, labels), X.columns(host, text, labels))


def test_g1_lone_cr_raises(engine):
    with pytest.raises(ValueError, match="2 carriage return"):
        engine.existing_table_build(b"a\rb\n1:1:A:C\tpk\tbin\r")


# ---- G1b: the size pass's stage fit boundary, as tests/test_gpu_cadd_edges.py e2 / e3 ---
def check_columns(engine, host, text, slab=None):
    """The device columns of ``text`` (or of ``slab``, a device tensor holding it), under
    poison, against the host entries, and both against the restatement."""
    want, ref = X.restate(text), X.columns(host, text)
    engine.poison = 0xA5
    try:
        dev = X.columns(engine, text if slab is None else slab)
    finally:
        engine.poison = None
    X.assert_same(ref, want)
    X.assert_same(dev, want)
    X.assert_same(dev, ref)
    return dev


@pytest.mark.parametrize("first", [49136, 49152, 49153, 49168])
def test_g1_size_pass_stage_fit_boundary(engine, host, first):
    """Trip 0 of k_exist_lines stages 49,136 / 49,152 bytes (the last that fits
    kExistSizeStage) or is read from global memory at 49,153 / 49,168; the trips after it
    alternate, one of them holds a line longer than the whole stage, a skipped line is
    the first or the last of every trip, the last line has no newline."""
    plan = X.fit_plan(first)
    text = X.fit_text(plan)
    fits = X.check_fit_plan(text, plan)
    assert fits[0] == (first <= X.STAGE) and 300000 < len(text) < 450000
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).to(engine.device)
    assert slab.data_ptr() % 16 == 0
    dev = check_columns(engine, host, text, slab)
    assert dev["counts"]["rows"] == len(plan) * (X.TRIP - 1) + 100 and dev["counts"]["skipped"] == len(plan)
    assert int(np.diff(dev["key_off"]).max()) > 60000 and dev["counts"]["frag_host"] > 30


@pytest.mark.parametrize("k", [1, 7, 8, 15])
def test_g1_unaligned_slab(engine, host, k):
    """The slab ``k`` bytes off 16-byte alignment, row-shaped junk before and after it:
    the stage's first word starts before the text, and the fit boundary moves with the
    address — the text is built for this residue, so 49,152 / 49,153 are again exact."""
    plan = X.fit_plan(X.STAGE if k % 2 else X.STAGE + 1)
    text = X.fit_text(plan, residue=k)
    X.check_fit_plan(text, plan, residue=k)
    whole = (X.JUNK * 3)[-k:] + text + X.JUNK * 12
    dev_whole = torch.from_numpy(np.frombuffer(whole, dtype=np.uint8).copy()).to(engine.device)
    assert dev_whole.data_ptr() % 16 == 0 and whole[:k].endswith(b"\n") and b"~" not in text
    assert k < 7 or X.restate(whole[:k])["counts"]["rows"] >= 1  # the junk before the text is a row
    slab = dev_whole[k:k + len(text)]
    assert slab.is_contiguous() and slab.data_ptr() % 16 == k
    dev = check_columns(engine, host, text, slab)
    assert not any(b"~" in dev[name] for name in ("keys", "pks", "frag"))


# ---- G2: a seeded export -----------------------------------------------------------
def _lines(n, seed):
    from annotatedvdb_amd import synth
    return synth.vcf_text(n, seed=seed).decode().splitlines()


def _metaseqs(lines):
    out = []
    for ln in lines:
        f = ln.split("\t")
        for a in f[4].split(","):
            if a != ".":
                out.append("%s:%s:%s:%s" % (f[0], f[1], f[3], a))
    return out


def _bin(rng, c):
    path, b = "chr%s" % c, 1
    for lv in range(1, 14):
        b = 2 * b - int(rng.integers(0, 2))
        path += ".L%d.B%d" % (lv, b)
    return path


NONCANON = ["HSCHR1_RANDOM_CTG%d" % i for i in range(5)] + ["chr1", "chrUn_KI270742v1", "MT"]


@pytest.fixture(scope="module")
def g2(tmp_path_factory):
    """(path, export bytes, metaseq ids of the 20,000-line record batch)"""
    rng = np.random.default_rng(12)
    ms = _metaseqs(_lines(20000, 31))
    keys = []
    for m in ms:  # as tests/test_gpu_existing.py: exact, switched, duplicated, unrelated
        u = rng.random()
        if u < 0.33:
            keys.append(m)
        elif u < 0.5:
            c, p, r, a = m.split(":")
            keys.append(":".join((c, p, a, r)))
        if rng.random() < 0.02:
            keys.append(m)
    keys += ["%d:%d:A:G" % (rng.integers(1, 23), rng.integers(1, 10**8)) for _ in range(49000)]
    keys += ["%s:%d:A:G" % (NONCANON[i % len(NONCANON)], 100 + i // 3) for i in range(200)]
    order = rng.permutation(len(keys))
    rows = []
    for j, i in enumerate(order):
        k = keys[i]
        pk = k if rng.random() < 0.5 else "%s:rs%d" % (k, rng.integers(1, 10**9))
        rows.append([k, pk, _bin(rng, k.split(":")[0])])
    for j in rng.choice(len(rows), 300, replace=False):  # repr() escapes in these
        rows[j][1 + j % 2] += ("'", "\\", "\x01", "\x7f", "é", "'\"", "中文")[j % 7]
    out = ["metaseq_id\trecord_primary_key\tbin_index\n"]
    for j, r in enumerate(rows):
        if rng.random() < 0.01:
            out.append(("junk line %d\n" % j, "\n", "two\tfields\n")[j % 3])
        out.append("\t".join(r) + ("\tmore\tcolumns" if j % 50 == 0 else "") + ("\r\n" if rng.random() < 0.05 else "\n"))
    data = "".join(out).encode("utf-8")
    path = tmp_path_factory.mktemp("k12") / "export.tsv"
    path.write_bytes(data)
    assert 59000 < data.count(b"\n") < 64000
    return str(path), data, ms


@pytest.fixture(scope="module")
def g2_sets(engine, g2):
    from annotatedvdb_amd.existing import ExistingVariants
    return ExistingVariants.from_export(g2[0], engine=engine), ExistingVariants.from_tsv(g2[0], engine=engine)


def _same_tables(dev, ref):
    assert len(dev) == len(ref)
    n = int(ref.key_off[-1])
    assert torch.equal(dev.key_off, ref.key_off) and torch.equal(dev.keys[:n], ref.keys[:n])
    n = int(ref.frag_off[-1])
    assert torch.equal(dev.frag_off, ref.frag_off) and torch.equal(dev.frag[:n], ref.frag[:n])
    dk, do, _ = dev._pk_table()
    rk, ro, _ = ref._pk_table()
    n = int(ro[-1])
    assert torch.equal(do, ro) and torch.equal(dk[:n], rk[:n])


def test_g2_blobs_equal_from_tsv(g2, g2_sets):
    dev, ref = g2_sets
    _same_tables(dev, ref)
    c = dev._cols.counts
    assert c["frag_host"] == 300 and c["noncanon"] == 200 and c["lone_cr"] == 0
    assert c["rows"] == len(ref) and c["rows"] + c["skipped"] == g2[1].count(b"\n")


def test_g2_probes_equal(engine, g2, g2_sets):
    from annotatedvdb_amd.engine import pack_records
    dev, ref = g2_sets
    recs = [m.split(":") for m in g2[2]]
    b = pack_records([CHROM_NAMES.index(r[0]) for r in recs], [int(r[1]) for r in recs],
                     [r[2].encode() for r in recs], [r[3].encode() for r in recs])
    md, kd = dev.probe(b)
    mr, kr = ref.probe(b)
    assert torch.equal(md, mr) and torch.equal(kd, kr)
    assert int((mr >= 0).sum()) > 5000 and int((kr == N.MATCH_SWITCHED).sum()) > 1000
    # K7's rendered keys of the same batch, and the export's own keys among strings that are none
    kt = engine.primary_keys(b.to(engine.device), max_seq_len=50)
    pd = dev.probe_primary_keys(kt.keys, kt.key_off, b.n, skip=kt.state[:b.n])
    pr = ref.probe_primary_keys(kt.keys, kt.key_off, b.n, skip=kt.state[:b.n])
    assert torch.equal(pd, pr) and int((pr >= 0).sum()) > 1000
    pks = [r.split("\t")[1] for r in g2[1].decode("utf-8").split("\n")[1:4000] if r.count("\t") >= 2]
    q = [None if i % 7 == 0 else (p.rstrip("\r") if i % 2 else p + "x") for i, p in enumerate(pks)] + ["", None]
    hd, hr = dev.has_primary_keys(q), ref.has_primary_keys(q)
    assert hd == hr and sum(hr) > 1000 and not any(h for h, s in zip(hr, q) if s is None)
    assert dev.has_primary_key(q[1]) is ref.has_primary_key(q[1]) is True
    assert dev.has_primary_keys([]) == ref.has_primary_keys([]) == []


def test_g2_payload_and_resolve_host(g2, g2_sets):
    dev, ref = g2_sets
    rng = np.random.default_rng(5)
    hostrows = torch.nonzero(dev._cols.flags & N.EXIST_FRAG_HOST).flatten().tolist()
    for k in rng.choice(len(ref), 150, replace=False).tolist() + hostrows[:50]:
        assert dev.payload(k) == ref.payload(k)
    ids = ["%s:%d:A:G" % (NONCANON[i % len(NONCANON)], 100 + i // 3) for i in range(0, 200, 2)]
    ids += ["%s:%d:G:A" % (NONCANON[i % len(NONCANON)], 100 + i // 3) for i in range(1, 200, 4)]  # switched
    ids += ["HSCHR1_RANDOM_CTG0:99:A:G", "chr9:100:A:G"] * 25
    assert len(ids) == 200
    got = [dev.resolve_host(m) for m in ids]
    assert got == [ref.resolve_host(m) for m in ids] and sum(k >= 0 for k in got) >= 150
    assert len(dev._index) <= 200  # built from the NONCANON rows only


# ---- G3: the loaders ----------------------------------------------------------------
def _dbsnp_loader(ex):
    from annotatedvdb_amd.loaders import VCFVariantLoader
    ld = VCFVariantLoader("dbSNP")
    ld.initialize_pk_generator("GRCh38", None)
    ld.initialize_bin_indexer(None)
    ld.set_algorithm_invocation_id(1)
    ld.initialize_copy_sql()
    ld.set_skip_existing(True, existing=ex)
    return ld


def test_g3_loader_skip_existing_matches_oracle(engine, tmp_path):
    from annotatedvdb_amd.existing import ExistingVariants
    lines = _lines(6000, 32)
    ms = _metaseqs(lines)
    rng = np.random.default_rng(4)
    keys = [m for m in ms if rng.random() < 0.4]
    payloads = [[{"primary_key": "old:%d" % i, "bin_index": "chrX.L1.B1"}] for i in range(len(keys))]
    tsv = tmp_path / "existing.tsv"
    tsv.write_text("metaseq_id\trecord_primary_key\tbin_index\n" +
                   "".join("%s\told:%d\tchrX.L1.B1\n" % (k, i) for i, k in enumerate(keys)))
    ex = ExistingVariants.from_export(str(tsv), engine=engine)
    first = {}
    for i, k in enumerate(keys):
        first.setdefault(k, i)
    ld = _dbsnp_loader(ex)
    exp_copy, exp_map = [], []
    for ln in lines:
        err, m, c = O.load_line(ln, length_table(), existing=first, payloads=payloads)
        assert err is None
        exp_copy += c
        exp_map += m
    ld.reset_copy_buffer()
    mapping = ld.load_vcf_text(("\n".join(lines) + "\n").encode())
    assert ld.last_load_stats["host_lines"] == 0
    assert ld.copy_buffer().getvalue().splitlines() == exp_copy
    assert mapping.splitlines() == exp_map
    ld.reset_copy_buffer()
    outs = ld.parse_variants(lines[:500])
    n_map = sum(1 for _ in outs)
    assert ["%s\t%s" % kv for o in outs for kv in o.items()] == exp_map[:n_map]
    hit = keys[0]
    assert ld.is_duplicate(hit) is True
    assert ld.is_duplicate(hit, returnMatch=True) == payloads[first[hit]]
    assert ld.is_duplicate("1:1:A:C", returnMatch=True) is None


def test_g3_adsp_loader_same_as_constructor_built(engine, tmp_path):
    """tests/test_gpu_adsp.py's fixture as an export: its matches, then its primary keys
    under a metaseq id no record has."""
    from annotatedvdb_amd.existing import ExistingVariants
    from annotatedvdb_amd.loaders import VCFVariantLoader
    import test_gpu_adsp as A
    fx = json.load(open(os.path.join(GOLDEN, "adsp_existing.json")))
    tsv = tmp_path / "adsp_export.tsv"
    with open(tsv, "w") as fh:
        for m, match in fx["metaseq"].items():
            fh.write("%s\t%s\t%s\n" % (m, match[0]["primary_key"], match[0]["bin_index"]))
        for pk, c in fx["primary_key"].items():
            fh.write("\t%s\t%s.L1.B1\n" % (pk, c))
    rows = A.adsp_rows()
    text = ("\n".join(r[0] for r in rows) + "\n").encode()
    res = []
    for ex in (ExistingVariants.from_export(str(tsv), engine=engine), ExistingVariants.from_tsv(str(tsv), engine=engine)):
        ld = VCFVariantLoader("ADSP")
        ld.initialize_pk_generator("GRCh38", None)
        ld.initialize_bin_indexer(None)
        ld.set_algorithm_invocation_id(1)
        ld.initialize_copy_sql()
        ld.set_skip_existing(True, existing=ex)
        mapping = ld.load_vcf_text(text, errors="record")
        batch = (mapping, ld.copy_buffer().getvalue(), [tuple(u) for u in ld.update_buffer()],
                 [ld.get_count(k) for k in A.KEYS])
        per_line = []
        for raw, err, *_ in rows[:300]:
            ld.reset_copy_buffer()
            ld.reset_update_buffer()
            try:
                r = ld.parse_variant(raw)
                per_line.append((dict(r), ld.copy_buffer().getvalue(), [tuple(u) for u in ld.update_buffer()]))
            except Exception as e:  # noqa: BLE001
                per_line.append(type(e).__name__)
        res.append((batch, per_line))
    assert res[0] == res[1]
    assert len(res[0][0][2]) > 100 and res[0][0][0]


# ---- G4: compressed input -----------------------------------------------------------
def test_g4_bgzip_and_gzip_give_the_same_tables(engine, g2, g2_sets, tmp_path):
    from annotatedvdb_amd.existing import ExistingVariants
    bz, gz = tmp_path / "export.bgz.tsv.gz", tmp_path / "export.tsv.gz"
    bz.write_bytes(Z.bgzip(g2[1], block=4000))  # lines straddle members
    gz.write_bytes(gzip.compress(g2[1]))
    for p in (bz, gz):
        _same_tables(ExistingVariants.from_export(str(p), engine=engine), g2_sets[1])


def test_g4_driver_bgzip_with_contigs(engine, g2, tmp_path):
    from annotatedvdb_amd import load_vcf_file as D
    bz, plain = tmp_path / "export.tsv.gz", tmp_path / "export22.tsv"
    bz.write_bytes(Z.bgzip(g2[1], block=4000))
    plain.write_bytes(X.filtered(g2[1], ["22"]))
    lines = [ln for ln in _lines(20000, 31) if ln.split("\t")[0] in ("21", "22")]
    text = ("\n".join(lines) + "\n").encode()
    out = []
    for argv in (["--skipExisting", "--existing", str(bz), "--existingContigs", "22"],
                 ["--skipExisting", "--existing", str(plain)],
                 ["--skipExisting", "--existing", str(plain), "--existingHost"]):
        ld = D.make_loader(D.parse_args(argv + ["--algInvocationId", "1"]), engine.device.index)
        assert (ld._existing._cols is None) == ("--existingHost" in argv)
        mapping = ld.load_vcf_text(text)
        out.append((mapping, ld.copy_buffer().getvalue(), len(ld._existing)))
    assert out[0] == out[1] == out[2]
    assert "primary_key" in out[0][0] and 0 < out[0][2] < 10000

"""K11 on the device (k_bgzf_inflate: one wave per BGZF member) against the library's
host entry — the same per-member code — and Python's gzip: the fixture chain of
bgzf_common.py, the corrupt members, the grid-stride second trip, an odd-addressed
input ending on its buffer's last byte, and the two consumers of the text (K10a and
K0) reading it where K11 left it."""

import gzip
import os

import numpy as np
import pytest

import bgzf_common as B
import cadd_common as C
from conftest import GOLDEN
from annotatedvdb_amd import _native as N

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def host():
    from annotatedvdb_amd.engine import Engine
    eng = Engine("host")
    eng.poison = SENTINEL
    return eng


@pytest.fixture()
def poisoned(engine):
    engine.poison = SENTINEL
    yield engine
    engine.poison = None
    engine.set_option(N.OPT_K11_GRID, 0)


def test_chain_equals_host_and_gzip(poisoned, host):
    chain, text = B.chain()
    ix = host.bgzf_index(chain)
    out, status, counts = poisoned.bgzf_inflate(chain, ix, raise_on_error=False)
    assert out.device.type == "cuda" and out.numel() == ix.out_bytes == len(text)  # (out_cap is exactly out_bytes)
    hout, hstatus, hcounts = host.bgzf_inflate(chain, ix, raise_on_error=False)
    assert out.cpu().numpy().tobytes() == hout.numpy().tobytes() == text == gzip.decompress(chain)
    assert status.cpu().tolist() == hstatus.tolist() == [0] * ix.n_blocks
    assert counts.tolist() == hcounts.tolist() == [ix.n_blocks, 0, 2 ** 64 - 1]
    assert poisoned.bgzf_inflate(chain).cpu().numpy().tobytes() == text  # (indexed by the call itself)


def test_corrupt_members_fail_alone_as_on_the_host(poisoned, host):
    """All corrupt members in one chain, each between good neighbours: the host entry's
    statuses, the neighbours' text, the sentinel everywhere else."""
    from annotatedvdb_amd import bgzf
    fx = B.fixtures()
    good = [fx[1], fx[8], fx[9], fx[13]]
    parts, texts = [], []
    for k, (name, bad, want) in enumerate(B.corrupt_members()):
        g = good[k % len(good)]
        parts += [g[2], bad]
        texts += [g[1], None]
    parts.append(B.EOF_MEMBER)
    texts.append(b"")
    chain = b"".join(parts)
    ix = host.bgzf_index(chain)
    assert ix.n_blocks == len(texts)
    out, status, counts = poisoned.bgzf_inflate(chain, ix, raise_on_error=False)
    hout, hstatus, hcounts = host.bgzf_inflate(chain, ix, raise_on_error=False)
    status, out = status.cpu().numpy(), out.cpu().numpy()
    assert status.tolist() == hstatus.tolist()
    n_bad = len(B.corrupt_members())
    assert counts.tolist() == hcounts.tolist() == [len(texts) - n_bad, n_bad, 1]
    for k, (name, bad, want) in enumerate(B.corrupt_members()):
        assert status[2 * k] == 0 and status[2 * k + 1] != 0, name
        assert want is None or status[2 * k + 1] == want, (name, int(status[2 * k + 1]))
    for i, t in enumerate(texts):
        lo, hi = int(ix.out_off[i]), int(ix.out_off[i + 1])
        if t is None:
            assert (out[lo:hi] == SENTINEL).all(), i
        else:
            assert out[lo:hi].tobytes() == t, i
    assert out.tobytes() == hout.numpy().tobytes()
    with pytest.raises(bgzf.BgzfError) as e:
        poisoned.bgzf_inflate(chain)
    assert (e.value.block, e.value.offset, e.value.status) == (1, int(ix.in_off[1]), int(status[1]))


def test_grid_stride_second_trip(poisoned, host):
    """5,000 tiny members on a grid of 7 waves: each wave strides over some 700."""
    rng = np.random.default_rng(9)
    lines = [b"%d\t%s\n" % (i, bytes(rng.integers(65, 70, int(rng.integers(0, 40)), dtype=np.uint8))) for i in range(5000)]
    chain = b"".join(B.member(x, 1) for x in lines) + B.EOF_MEMBER
    poisoned.set_option(N.OPT_K11_GRID, 7)
    out, status, counts = poisoned.bgzf_inflate(chain, raise_on_error=False)
    assert out.cpu().numpy().tobytes() == b"".join(lines)
    assert counts.tolist() == [5001, 0, 2 ** 64 - 1] and not status.any()


def test_odd_address_and_last_byte(poisoned, host):
    """``comp`` starts at an odd device address and its last member (a stored block, so
    the stream's last bytes are loaded as input words) ends on the buffer's last byte."""
    fx = B.fixtures()
    chain = fx[0][2] + fx[13][2] + fx[2][2]
    text = fx[0][1] + fx[13][1] + fx[2][1]
    ix = host.bgzf_index(chain)
    for lead in (1, 3):
        buf = torch.full((lead + len(chain),), 0x5A, dtype=torch.uint8, device=poisoned.device)
        buf[lead:] = torch.from_numpy(np.frombuffer(chain, dtype=np.uint8).copy()).to(poisoned.device)
        comp = buf[lead:]
        assert comp.data_ptr() % 2 == 1 and comp.data_ptr() + comp.numel() == buf.data_ptr() + buf.numel()
        out = poisoned.bgzf_inflate(comp, ix)
        assert out.cpu().numpy().tobytes() == text


def test_cadd_from_file_on_bgzf(engine, tmp_path):
    """CaddTable.from_file on a bgzip CADD file: K11's device text straight into K10a —
    the table columns of from_text."""
    from annotatedvdb_amd.cadd import CaddTable
    snv = C.golden()[0]
    p = tmp_path / "snv.tsv.gz"
    p.write_bytes(B.bgzip(snv, block=30000))
    t = CaddTable.from_file(str(p), engine=engine)
    assert t.cols.text.device.type == "cuda"
    C.assert_same_table(C.table_columns(t.cols), C.table_columns(CaddTable.from_text(snv, engine).cols), "bgzf")
    assert t.slab() == snv


def test_tokenize_reads_inflated_text(engine):
    """K0 over K11's output tensor equals K0 over the text, on 2,000 golden VCF lines."""
    with gzip.open(os.path.join(GOLDEN, "vcf_lines.tsv.gz"), "rt") as fh:
        fh.readline()
        lines = [line.rstrip("\n").split("\t")[0].replace("\\t", "\t") for line in fh][:2000]
    text = ("\n".join(lines) + "\n").encode()
    assert len(lines) == 2000
    dev = engine.bgzf_inflate(B.bgzip(text, block=50000))
    assert dev.device.type == "cuda" and dev.cpu().numpy().tobytes() == text
    a, b = engine.vcf_tokenize(dev), engine.vcf_tokenize(text)
    assert a.n_lines == b.n_lines == 2000
    la, lb = a.lines_host(), b.lines_host()
    for name in ("start", "len", "n_fields", "pos", "ext_id", "n_alt", "n_rec", "flags", "chrom"):
        assert np.array_equal(la[name], lb[name]), name
    assert torch.equal(a.rec_off[:2001], b.rec_off[:2001])
    n = a.records.n
    assert n == b.records.n
    for x, y in ((a.records.chrom, b.records.chrom), (a.records.pos, b.records.pos),
                 (a.records.allele_off, b.records.allele_off), (a.records.ref_len, b.records.ref_len),
                 (a.records.alt_len, b.records.alt_len), (a.records.ext_id, b.records.ext_id),
                 (a.rec_line, b.rec_line), (a.rec_alt, b.rec_alt)):
        assert torch.equal(x[:n], y[:n])
    assert torch.equal(a.heap_off[:2001], b.heap_off[:2001])
    hb = int(a.heap_off[2000])
    assert hb > 0 and torch.equal(a.records.heap[:hb], b.records.heap[:hb])

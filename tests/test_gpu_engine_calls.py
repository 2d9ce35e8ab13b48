"""The library entries each engine method makes, in order, and the host syncs
beside them: Python reaches the library through ``_native.call`` alone
(DESIGN.md §1), so wrapping it shows every entry.  The expected lists were
recorded on 388d9f6 (the commit before the one call path) with a recorder around
``engine.lib``; the sync counts (``torch.cuda.synchronize``, ``.cpu()`` and
``.item()`` of a device tensor) come from the same runs."""

import pytest
import torch

from annotatedvdb_amd import _native as N
from annotatedvdb_amd import synth
from annotatedvdb_amd.pipeline import KeyedStep, PrepStep

import existing_common as E
from cadd_common import batch_of

pytestmark = pytest.mark.gpu


class Recorder:
    """``with Recorder() as r``: ``r.calls`` = (symbol, arguments as given) of every
    ``N.call``; ``r.syncs`` = [synchronize, .cpu(), .item()] counts."""

    def __enter__(self):
        self.calls, self.syncs = [], [0, 0, 0]
        self._undo = []
        inner = N.call

        def call(name, *args, **kw):
            self.calls.append((name, args))
            return inner(name, *args, **kw)
        self._patch(N, "call", call)
        self._count(torch.cuda, "synchronize", 0, lambda a: True)
        self._count(torch.Tensor, "cpu", 1, lambda a: a[0].is_cuda)
        self._count(torch.Tensor, "item", 2, lambda a: a[0].is_cuda)
        return self

    def _patch(self, obj, name, new):
        own = name in vars(obj)
        old = getattr(obj, name)
        setattr(obj, name, new)
        self._undo.append((lambda: setattr(obj, name, old)) if own else (lambda: delattr(obj, name)))

    def _count(self, obj, name, slot, when):
        old = getattr(obj, name)

        def counted(*a, **kw):
            if when(a):
                self.syncs[slot] += 1
            return old(*a, **kw)
        self._patch(obj, name, counted)

    def __exit__(self, *exc):
        for undo in reversed(self._undo):
            undo()

    @property
    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture(scope="module")
def records():
    """2,000 position-sorted records: 5 % long alleles, 2 % copied duplicates."""
    b = synth.alleles(2000, seed=11, device="cuda")
    assert int(((b.ref_len + b.alt_len) > 50).sum()) > 20
    same = (b.pos[1:] == b.pos[:-1]) & (b.chrom[1:] == b.chrom[:-1]) & (b.ref_len[1:] == b.ref_len[:-1])
    assert int(same.sum()) > 10
    return b


@pytest.fixture(scope="module")
def vcf():
    return synth.vcf_text(300, seed=6)


DIGS = ["%032d" % (7 * i) for i in range(25)]


@pytest.fixture(scope="module", autouse=True)
def _digests(engine):
    engine.set_sequence_digests(DIGS)


CADD = b"## CADD\n#Chrom\tPos\tRef\tAlt\tRawScore\tPHRED\n" + b"".join(
    b"1\t%d\tA\t%s\t0.5\t12\n" % (100 + i // 3, b"CGT"[i % 3:i % 3 + 1]) for i in range(30))
CADD_IDS = ["1:100:A:C", "1:105:A:T", "1:300:A:C", "2:100:A:C"]

KEYED_RUN = [
    "avdb_vrs_digest_workspace_size", "avdb_record_prep_keyed", "avdb_pk_dedup_ex",
    "avdb_vrs_digest_workspace_size", "avdb_vrs_digest_ex",
    "avdb_primary_keys_onepass_workspace_size", "avdb_keys_off32_bytes", "avdb_primary_keys_onepass_ex"]


def test_keyed_step_entries(engine, records):
    with Recorder() as r:
        step = KeyedStep(engine, records, digests=True, layout="serial")
    assert r.names == ["avdb_primary_keys_onepass_workspace_size", "avdb_primary_keys_bound", "avdb_keys_off32_bytes",
                       "avdb_vrs_digest_workspace_size", "avdb_ctx_set_option", "avdb_ctx_set_option"]
    for _ in range(2):  # the second step takes the same hand-offs from the keyed K2 as the first
        with Recorder() as r:
            step.run()
        assert r.names == KEYED_RUN
        assert r.syncs == [0, 0, 0]
    torch.cuda.synchronize()


def test_prep_step_entries(engine, records):
    step = PrepStep(engine, records)
    with Recorder() as r:
        step.run()
    assert r.names == ["avdb_vrs_digest_workspace_size", "avdb_record_prep_keyed", "avdb_pk_dedup_ex",
                       "avdb_vrs_digest_workspace_size", "avdb_vrs_digest_ex"]
    assert r.syncs == [0, 0, 0]
    torch.cuda.synchronize()


def test_vcf_tokenize_count_free_entries(engine, vcf):
    with Recorder() as r:
        vb = engine.vcf_tokenize(vcf, want_lines=False)
    assert engine.last_vcf_path == "local" and vb.n_lines == 300
    assert r.names == ["avdb_vcf_local_workspace_size", "avdb_vcf_parse_local", "avdb_vcf_emit_local"]
    assert r.syncs == [0, 1, 0]


def test_vcf_tokenize_counted_entries(engine, vcf):
    with Recorder() as r:
        vb = engine.vcf_tokenize(vcf, want_lines=False, count_free=False)
    assert engine.last_vcf_path == "counted" and vb.n_lines == 300 and vb.lines is None
    assert r.names == ["avdb_vcf_count_workspace_size", "avdb_vcf_count_lines", "avdb_vcf_workspace_size",
                       "avdb_vcf_parse_lines2", "avdb_vcf_emit_ws"]
    assert r.syncs == [0, 2, 0]


def test_vcf_tokenize_then_format_entries(engine, vcf):
    with Recorder() as r:
        vb = engine.vcf_tokenize(vcf)
        end, code, status, _ = engine.record_prep(vb.records, want_lcp=False)
        fr = engine.vcf_format(vb, end, code, status, alg_id="1")
    assert fr.line_state.numel() == 300
    assert r.names == ["avdb_vcf_count_workspace_size", "avdb_vcf_count_lines", "avdb_vcf_workspace_size",
                       "avdb_vcf_parse_lines2", "avdb_vcf_emit", "avdb_record_prep",
                       "avdb_format_workspace_size", "avdb_vcf_format_size", "avdb_vcf_format_write"]
    assert r.syncs == [0, 3, 0]


def test_vcf_tokenize_empty_text_is_null(engine):
    """No text: an empty tensor, and NULL at the calls."""
    with Recorder() as r:
        vb = engine.vcf_tokenize(b"")
    assert vb.n_lines == 0 and vb.text.numel() == 0 and vb.records.n == 0
    assert [c[1][1] for c in r.calls if c[0] in ("avdb_vcf_count_lines", "avdb_vcf_parse_lines2")] == [None, None]


def test_cadd_entries(engine):
    with Recorder() as r:
        cols = engine.cadd_table_build(CADD)
        row, kind, raw, phred = engine.cadd_match(cols, None, batch_of(CADD_IDS))
    assert cols.n_rows == 30 and kind.tolist() == [N.CADD_SNV, N.CADD_SNV, N.CADD_NONE, N.CADD_NONE]
    assert r.names == ["avdb_vcf_count_lines", "avdb_cadd_workspace_size", "avdb_cadd_table_build", "avdb_cadd_match"]
    assert r.syncs == [0, 1, 2]


def test_existing_table_build_entries(engine):
    with Recorder() as r:
        cols = engine.existing_table_build(E.H1)
    assert cols.counts["frag_host"] == E.H1_FRAG_HOST
    assert r.names == ["avdb_vcf_count_lines", "avdb_existing_workspace_size", "avdb_existing_size",
                       "avdb_existing_write"]
    assert r.syncs == [0, 3, 2]


def test_strided_tensor_is_refused(engine, records):
    """A strided view used to be read as if dense; now the entry is not made."""
    hist = torch.zeros(2 * engine.n_l8, dtype=torch.int32, device=engine.device)[::2]
    with Recorder() as r:
        with pytest.raises(ValueError, match="avdb_record_prep: argument 13 is a strided Tensor"):
            engine.record_prep(records, hist=hist)
    assert r.names == ["avdb_record_prep"]  # (asked for, and refused before the symbol was looked up)
    assert not hist.any()
    end, code, status, _ = engine.record_prep(records, hist=hist.contiguous())
    assert int((status == N.STATUS_OK).sum()) > 0


def _arg(r, name, given):
    """Is ``given`` (by address) an argument of the recorded call of ``name``?"""
    (args,) = [c[1] for c in r.calls if c[0] == name]
    return any(isinstance(a, torch.Tensor) and a.data_ptr() == given.data_ptr() for a in args)


@pytest.mark.parametrize("short", [0, 1])
def test_given_workspace_vrs_digest(engine, records, short):
    """A workspace of exactly the queried size is the one the entry gets; one byte less and it is replaced."""
    need = N.size("avdb_vrs_digest_workspace_size", records.n)
    ws = torch.empty(need - short, dtype=torch.uint8, device=engine.device)
    with Recorder() as r:
        dig, is_long = engine.vrs_digest(records, workspace=ws)
    assert _arg(r, "avdb_vrs_digest_ex", ws) == (not short)
    want, want_long = engine.vrs_digest(records)
    assert torch.equal(is_long, want_long) and torch.equal(dig[is_long != 0], want[want_long != 0])


@pytest.mark.parametrize("short", [0, 1])
def test_given_workspace_keyed_prep(engine, records, short):
    need = N.size("avdb_keyed_prep_workspace_size", records.n)
    ws = torch.empty(need - short, dtype=torch.uint8, device=engine.device)
    kt = engine.new_key_text(records.n, int(records.heap.numel()))
    with Recorder() as r:
        end, code, status, keep = engine.keyed_prep(records, kt, defer_digest=False, workspace=ws)
    assert _arg(r, "avdb_keyed_prep", ws) == (not short)
    assert (engine.last_keyed_ws is ws) == (not short)
    assert engine.keyed_prep_lookback_errors(engine.last_keyed_ws) == 0
    want = engine.record_prep(records, want_lcp=False)
    assert torch.equal(end, want[0]) and torch.equal(code, want[1]) and torch.equal(status, want[2])

"""The one call path from Python into the library (``_native.call`` / ``size``,
``Engine._call`` / ``_launch``) on a host-only engine: argument
conversion, error text, the layout check, what a host-only engine refuses, and the
K3 list workspace size."""

import numpy as np
import pytest
import torch

from annotatedvdb_amd import _native as N
from annotatedvdb_amd.chromosomes import length_table
from annotatedvdb_amd.engine import Engine, VcfBatch, dedup_list_bytes, pack_records
from oracle import avdb_oracle as O


@pytest.fixture(scope="module")
def host():
    return Engine("host")


@pytest.fixture(scope="module")
def codes():
    """Eight (contig code, bin code) pairs, one of them unmappable."""
    chrom = np.array([0, 1, 5, 21, 22, 23, 24, 200], dtype=np.uint8)
    start = np.array([1510801, 5, 70_000_000, 16_050_000, 1, 2_781_479, 16569, 5], dtype=np.int32)
    code, status = O.bin_codes_np(chrom, start, start.copy(), length_table())
    assert status[-1] != N.STATUS_OK and not status[:-1].any()
    return chrom, code.view(np.uint32)


def _paths_raw(host, chrom, code, out, offs):
    n = len(code)
    assert N.call("avdb_format_bin_paths", host.ctx, chrom, code, n, out, len(out), offs) == N.AVDB_OK
    return bytes(out[: int(offs[n])].tolist()), [int(x) for x in offs]


def test_call_converts_tensors_arrays_and_ints(host, codes):
    chrom, code = codes
    want = host.format_paths(chrom, code)
    assert want[0].startswith("chr1.L1.B1.") and want[-1] is None and all(want[:-1])
    # arrays in, arrays out
    raw, offs = _paths_raw(host, chrom, code, np.empty(8 * 88, dtype=np.uint8), np.empty(9, dtype=np.uint64))
    assert raw == "".join(p or "" for p in want).encode()
    assert [raw[a:b].decode() or None for a, b in zip(offs, offs[1:])] == want
    # tensors in (and one array), tensors out: the same bytes
    raw_t, offs_t = _paths_raw(host, torch.from_numpy(chrom.copy()), code, torch.empty(8 * 88, dtype=torch.uint8),
                               torch.empty(9, dtype=torch.int64))
    assert (raw_t, offs_t) == (raw, offs)


def test_call_passes_none_as_null(host, codes):
    chrom, code = codes
    out, offs = np.empty(8 * 88, dtype=np.uint8), np.empty(9, dtype=np.uint64)
    with pytest.raises(N.NativeError) as e:
        N.call("avdb_format_bin_paths", host.ctx, None, code, 8, out, len(out), offs)
    assert e.value.rc == N.AVDB_EINVAL
    assert N.call("avdb_format_bin_paths", host.ctx, None, code, 8, out, len(out), offs, check=False) == N.AVDB_EINVAL
    assert host._call("avdb_format_bin_paths", None, None, 0, out, len(out), offs) == N.AVDB_OK  # (n = 0: not read)


def test_error_names_the_symbol_called(host):
    with pytest.raises(N.NativeError) as e:
        host._call("avdb_cadd_table_build_host", None, 0, 0, *[None] * 12)
    assert e.value.rc == N.AVDB_EINVAL
    assert str(e.value).startswith("avdb_cadd_table_build_host failed (rc=-1): ")
    assert N.last_error().startswith("avdb_cadd_table_build_host: ") and N.last_error() in str(e.value)
    with pytest.raises(N.NativeError, match=r"^avdb_host_alloc failed \(rc=-1\): avdb_host_alloc: null pointer"):
        N.call("avdb_host_alloc", 0, None)


def test_size_checks_the_code():
    assert N.size("avdb_vrs_digest_workspace_size", 4) > 0
    assert N.size("avdb_vcf_workspace_size", 100, 3) > 0
    with pytest.raises(N.NativeError, match="^avdb_hist_allgather_workspace_size failed"):
        N.size("avdb_hist_allgather_workspace_size", 0, 1, 1)  # a world of no ranks


@pytest.mark.parametrize("strided", [torch.zeros(16, dtype=torch.uint8)[::2], np.zeros(16, dtype=np.uint8)[::2]],
                         ids=["tensor", "ndarray"])
def test_strided_argument_is_refused_before_the_library(host, codes, strided, monkeypatch):
    chrom, code = codes
    ctx = host.ctx
    looked_up = []
    monkeypatch.setattr(N, "symbol", lambda name: looked_up.append(name))
    out, offs = np.empty(8 * 88, dtype=np.uint8), np.empty(9, dtype=np.uint64)
    with pytest.raises(ValueError, match=r"avdb_format_bin_paths: argument 1 "):
        N.call("avdb_format_bin_paths", ctx, strided, code, 8, out, len(out), offs)
    with pytest.raises(ValueError, match=r"avdb_format_bin_paths: argument 4 "):
        N.call("avdb_format_bin_paths", ctx, chrom, code, 8, strided, 8, offs)
    assert looked_up == []


def test_host_only_engine_refuses_the_kernel_entries(host):
    b = pack_records([0, 0, 1, 24], [100, 100, 5, 9], [b"A", b"A", b"CT", b"G"], [b"C", b"C", b"C", b"GA" * 30])
    assert b.n == 4
    i32 = torch.zeros(4, dtype=torch.int32)
    vb = VcfBatch(text=torch.zeros(8, dtype=torch.uint8), n_lines=1, lines=torch.zeros(80, dtype=torch.uint8),
                  rec_off=torch.zeros(2, dtype=torch.int64), heap_off=torch.zeros(2, dtype=torch.int64),
                  records=b, rec_line=i32, rec_alt=i32)
    calls = {
        "bin_assign": lambda: host.bin_assign(b.chrom, b.pos),
        "record_prep": lambda: host.record_prep(b),
        "pk_dedup": lambda: host.pk_dedup(b),
        "vrs_digest": lambda: host.vrs_digest(b),
        "primary_keys": lambda: host.primary_keys(b),
        "vcf_tokenize": lambda: host.vcf_tokenize(b"1\t100\t.\tA\tC\t.\t.\t.\n"),
        "vcf_tokenize_count_free": lambda: host.vcf_tokenize(b"1\t100\t.\tA\tC\t.\t.\t.\n", want_lines=False),
        "vcf_format": lambda: host.vcf_format(vb, i32, i32, torch.zeros(4, dtype=torch.uint8), alg_id="1"),
        "keyset_build": lambda: host.keyset_build(torch.zeros(4, dtype=torch.uint8),
                                                  torch.tensor([0, 2, 4], dtype=torch.int64)),
        "display_attributes": lambda: host.display_attributes(b, i32),
    }
    for name, fn in calls.items():
        with pytest.raises(N.NativeUnavailable, match="host-only engine"):
            fn()
    with pytest.raises(N.NativeUnavailable):
        host._launch("avdb_bin_assign", b.chrom, b.pos, None, 4, i32, None, None, None)


def test_workspace_keeps_a_buffer_that_is_large_enough(host):
    given = torch.empty(64, dtype=torch.uint8)
    assert host.workspace(64, given) is given and host.workspace(63, given) is given
    fresh = host.workspace(65, given)
    assert fresh is not given and fresh.numel() == 65 and fresh.dtype == torch.uint8
    assert host.workspace(8).numel() == 8
    host.poison = 0xA5
    try:
        assert host.workspace(8).tolist() == [0xA5] * 8
    finally:
        host.poison = None


def test_record_soa_order():
    b = pack_records([3], [7], [b"AC"], [b"A"])
    soa = b.soa()
    assert [t is u for t, u in zip(soa, (b.chrom, b.pos, b.allele_off, b.ref_len, b.alt_len, b.heap))] == [True] * 6
    assert soa[6] == 3 and len(soa) == 7


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 4097])
def test_dedup_list_bytes(n):
    assert dedup_list_bytes(n) == 16384 + 4 * ((n + 3) & ~3)
    # with the keyed steps' slack: what KeyedStep and PrepStep allocated before the helper
    assert dedup_list_bytes(n, 1 << 22) == 16384 + 4 * (((n + 3) & ~3) + (1 << 22))


def test_as_text_forms(host):
    for text in (b"ab\n", bytearray(b"ab\n"), memoryview(b"ab\n"), np.frombuffer(b"ab\n", dtype=np.uint8),
                 torch.tensor([97, 98, 10], dtype=torch.uint8)):
        t = host._as_text(text)
        assert t.dtype == torch.uint8 and t.is_contiguous() and bytes(t.tolist()) == b"ab\n"
    for text in (b"", bytearray(), np.zeros(0, dtype=np.uint8), torch.zeros(0, dtype=torch.uint8)):
        t = host._as_text(text)
        assert t.numel() == 0 and t.data_ptr() == 0  # NULL at a call

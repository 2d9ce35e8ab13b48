"""Device engine: one ``avdb_ctx`` per GPU plus torch-owned HBM buffers.

Everything here goes through ``libavdb_hip.so``; torch supplies device memory,
the current HIP stream and host<->device copies (plumbing, not compute).

Data layout in HBM (structure of arrays, one row per alt allele; see
``include/avdb.h``):

=============  =======  =====================================================
chrom          uint8    contig code (``chromosomes.CHROM_NAMES`` order)
pos            int32    1-based VCF POS (stored as u32 by the kernels)
end            int32    1-based inclusive end (optional, K1 only)
allele_off     int64    offset of REF in ``heap``; ALT follows REF
ref_len        int32
alt_len        int32
ext_id         int64    refSNP key (0 = none), see :func:`ext_id_key`
heap           uint8    concatenated raw REF+ALT bytes
=============  =======  =====================================================
"""

from __future__ import annotations

import ctypes
import os
import re
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from . import slab_passes
from .chromosomes import CHROM_NAMES, N_CHROM, length_table


# ---------------------------------------------------------------------------
# record batch (SoA)
# ---------------------------------------------------------------------------
@dataclass
class RecordBatch:
    chrom: torch.Tensor
    pos: torch.Tensor
    allele_off: Optional[torch.Tensor] = None
    ref_len: Optional[torch.Tensor] = None
    alt_len: Optional[torch.Tensor] = None
    heap: Optional[torch.Tensor] = None
    ext_id: Optional[torch.Tensor] = None
    end: Optional[torch.Tensor] = None

    @property
    def n(self) -> int:
        return int(self.chrom.numel())

    @property
    def device(self):
        return self.chrom.device

    def to(self, device, non_blocking=False) -> "RecordBatch":
        kw = {}
        for f in ("chrom", "pos", "allele_off", "ref_len", "alt_len", "heap", "ext_id", "end"):
            t = getattr(self, f)
            kw[f] = None if t is None else t.to(device, non_blocking=non_blocking)
        return RecordBatch(**kw)

    def has_alleles(self) -> bool:
        return self.heap is not None

    def soa(self) -> tuple:
        """The seven record arguments most batch entries begin with (``include/avdb.h``)."""
        return (self.chrom, self.pos, self.allele_off, self.ref_len, self.alt_len, self.heap, self.heap.numel())


@dataclass
class CaddColumns:
    """A built CADD table (K10a, ``avdb_cadd_table``): the text slab the allele
    offsets point into, one entry per data line in each column, the contig index
    and the build's counts (``N.CADD_COUNT_*``, host)."""
    text: torch.Tensor
    n_rows: int
    chrom: torch.Tensor
    pos: torch.Tensor
    ref_off: torch.Tensor
    ref_len: torch.Tensor
    alt_off: torch.Tensor
    alt_len: torch.Tensor
    raw: torch.Tensor
    phred: torch.Tensor
    flags: torch.Tensor
    first_row: torch.Tensor
    end_row: torch.Tensor
    counts: np.ndarray

    def view(self) -> "N.CaddTableView":
        """The C struct over these tensors (valid while they are alive)."""
        return N.CaddTableView(self.n_rows, N.ptr(self.text), self.text.numel(),
                               *[N.ptr(getattr(self, f)) for f in ("chrom", "pos", "ref_off", "ref_len", "alt_off",
                                                                    "alt_len", "raw", "phred", "flags", "first_row",
                                                                    "end_row")])


@dataclass
class ExistingColumns:
    """What K12 makes of an export of ``AnnotatedVDB.Variant``
    (:meth:`Engine.existing_table_build`): the blobs of the metaseq ids, the primary
    keys and the ``.mapping`` fragments with their ``int64[n_rows + 1]`` offsets, the
    per-row ``N.EXIST_*`` flags, and the build's counts by name (``N.EXIST_COUNTS``)."""
    n_rows: int
    keys: torch.Tensor
    key_off: torch.Tensor
    pks: torch.Tensor
    pk_off: torch.Tensor
    frag: torch.Tensor
    frag_off: torch.Tensor
    flags: torch.Tensor
    counts: Dict[str, int]


@dataclass
class CaddUpdateRows:
    """What K13 makes of an export of ``AnnotatedVDB.Variant``
    (:meth:`Engine.cadd_update_rows`): ``text`` holds the ``n`` update rows
    (``pk<TAB>chrom<TAB>json<LF>``, row ``i`` at ``row_off[i] .. row_off[i + 1]``),
    ``kind`` their ``N.CADD_NONE`` / ``CADD_SNV`` / ``CADD_INDEL``, ``flags`` their
    ``N.CADDUPD_*`` flags, ``counts`` the pass's counts by name (``N.CADDUPD_COUNTS``;
    ``snv`` / ``indel`` / ``not_matched`` include the rows resolved on the host)."""
    n: int
    text: torch.Tensor
    row_off: torch.Tensor
    kind: torch.Tensor
    flags: torch.Tensor
    counts: Dict[str, int]


@dataclass
class LofTable:
    """What K16a makes of the VCF SnpEff wrote (:meth:`Engine.lof_table_build`): one row per
    ALT allele of every line that carries a LOF or NMD value.  Row ``k``'s lookup id
    ``chrom:pos:ref:alt`` is ``keys[key_off[k]:key_off[k + 1]]``; ``rkeys`` / ``rkey_off`` hold
    the same keys in reverse row order and ``keyset`` the K6 hash table over them (its first of
    equal keys is the last annotated record of an id); ``json[json_off[k]:json_off[k] +
    json_len[k]]`` is the row's line's ``json.dumps({'LOF': [...], 'NMD': [...]})`` (the alts of
    a line share one span); ``line_start`` the row's line's offset in ``text``; ``flags`` the
    rows' ``N.LOF_*`` flags; ``hit[k]`` becomes 1 when an export row matches row ``k``
    (:meth:`Engine.lof_update_rows`); ``counts`` the build's counts by name (``N.LOF_COUNTS``)."""
    engine: object
    text: torch.Tensor
    n_rows: int
    keys: torch.Tensor
    key_off: torch.Tensor
    rkeys: torch.Tensor
    rkey_off: torch.Tensor
    keyset: torch.Tensor
    json: torch.Tensor
    json_off: torch.Tensor
    json_len: torch.Tensor
    line_start: torch.Tensor
    flags: torch.Tensor
    hit: torch.Tensor
    counts: Dict[str, int]

    def view(self) -> "N.LofTableView":
        """The C struct over these tensors (valid while they are alive)."""
        if self.n_rows == 0:
            return N.LofTableView()
        return N.LofTableView(self.n_rows, N.ptr(self.rkeys), N.ptr(self.rkey_off), N.ptr(self.keyset),
                              self.keyset.numel(), N.ptr(self.json), self.json.numel(), N.ptr(self.json_off),
                              N.ptr(self.json_len), N.ptr(self.hit))


@dataclass
class LofUpdateRows:
    """What K16b makes of an export of ``AnnotatedVDB.Variant`` (:meth:`Engine.lof_update_rows`):
    ``text`` holds the ``n`` update rows (``pk<TAB>chr<label><TAB>json<LF>``, row ``i`` at
    ``row_off[i] .. row_off[i + 1]``), ``match`` the table row each was rendered from,
    ``counts`` the pass's counts by name (``N.LOFUPD_COUNTS``)."""
    n: int
    text: torch.Tensor
    row_off: torch.Tensor
    match: torch.Tensor
    counts: Dict[str, int]


@dataclass
class VepRowsTable(LofTable):
    """What K18b makes of VEP ``--json`` output (:meth:`Engine.vep_rows_table_build`): :class:`LofTable`'s
    members for one row per ALT allele of every line's ``input``; row ``k``'s
    ``json[json_off[k]:json_off[k] + json_len[k]]`` is its own body,
    ``<adsp_most_severe_consequence><TAB><adsp_ranked_consequences>`` as ``json.dumps`` prints them
    (``{}`` for ``None``); ``counts`` by ``N.VEPROWS_COUNTS``; ``ranking`` the
    :class:`~annotatedvdb_amd.vep_consequences.ConsequenceRanking`; ``unranked`` the lines that need a
    re-rank and gave no rows, ``(line number, id, combination)``.  Built with ``vep_output=True``
    (K18c) it also holds every line's cleaned result once: entry (line) ``e``'s text is
    ``cleaned[cleaned_off[e]:cleaned_off[e] + cleaned_len[e]]``, ``row_entry[k]`` the entry of row
    ``k`` (the rows of a multi-allelic line share one text), ``cleaned_flags[e]`` 0 or 1 + the reason
    the host rendered it (``N.VEPOUT_REASONS``), ``cleaned_counts`` by ``N.VEPOUT_COUNTS``,
    ``identity_only`` the form of ``input``'s dict; else these are ``None``.  Built with
    ``allele_frequencies=True`` (K18d) it holds every row's ``allele_frequencies`` text, one per ALT allele:
    row ``k``'s is ``freq[freq_off[k]:freq_off[k] + freq_len[k]]``, ``freq_flags[e]`` 0 or 1 + the reason the
    host rendered line ``e``'s (``N.VEPFREQ_REASONS``), ``freq_counts`` by ``N.VEPFREQ_COUNTS``,
    ``match_refsnp`` whether the element was matched by ``ref_snp_id``; else these are ``None``."""
    ranking: object = None
    unranked: list = None
    _keep: tuple = ()  # K18a's arrays and the rank text, which the table's build read
    cleaned: torch.Tensor = None
    cleaned_off: torch.Tensor = None
    cleaned_len: torch.Tensor = None
    row_entry: torch.Tensor = None
    cleaned_flags: torch.Tensor = None
    cleaned_counts: Dict[str, int] = None
    identity_only: bool = False
    freq: torch.Tensor = None
    freq_off: torch.Tensor = None
    freq_len: torch.Tensor = None
    freq_flags: torch.Tensor = None
    freq_counts: Dict[str, int] = None
    match_refsnp: bool = False

    def freq_view(self) -> "N.VepFreqTable":
        """The C struct over the frequency texts (valid while the tensors are alive)."""
        return N.VepFreqTable(self.n_rows, N.ptr(self.freq), self.freq.numel(), N.ptr(self.freq_off),
                              N.ptr(self.freq_len))

    def cleaned_view(self) -> "N.VepOutputTable":
        """The C struct over the cleaned texts (valid while the tensors are alive)."""
        return N.VepOutputTable(self.cleaned_off.numel(), N.ptr(self.cleaned), self.cleaned.numel(),
                                N.ptr(self.cleaned_off), N.ptr(self.cleaned_len), N.ptr(self.row_entry))


@dataclass
class QcTable(LofTable):
    """What K17a makes of an ADSP QC pVCF (:meth:`Engine.qc_table_build`): :class:`LofTable`'s
    members for one row per ALT allele of every line, ``json`` holding each line's
    ``json.dumps({release: {"info": ..., "filter": ..., "qual": ..., "format": ...}})``;
    ``flags`` the rows' ``N.QC_*`` flags (``N.QC_PASS``: FILTER is ``PASS``); ``release`` the
    release key's bytes; ``counts`` by ``N.QC_COUNTS``."""
    release: bytes = b""

    def view(self) -> "N.QcTableView":
        if self.n_rows == 0:
            return N.QcTableView(self.release)
        return N.QcTableView(self.release, self.n_rows, N.ptr(self.rkeys), N.ptr(self.rkey_off), N.ptr(self.keyset),
                             self.keyset.numel(), N.ptr(self.json), self.json.numel(), N.ptr(self.json_off),
                             N.ptr(self.json_len), N.ptr(self.flags), N.ptr(self.hit))


@dataclass
class QcUpdateRows:
    """What K17b makes of an export of ``AnnotatedVDB.Variant`` (:meth:`Engine.qc_update_rows`):
    ``text`` holds the update rows (``pk<TAB>chr<label><TAB>true|\\N<TAB>json<LF>``, row ``i`` at
    ``row_off[i] .. row_off[i + 1]``; a row the host found to have QC values already has no
    bytes), ``n`` the rows with bytes, ``match`` the table row each was rendered from, ``flags``
    their ``N.QCUPD_*`` flags, ``counts`` the pass's counts by name (``N.QCUPD_COUNTS``)."""
    n: int
    text: torch.Tensor
    row_off: torch.Tensor
    match: torch.Tensor
    flags: torch.Tensor
    counts: Dict[str, int]


@dataclass
class TxtHeader:
    """The header of a tab-delimited annotation file as ``csv`` reads it
    (:func:`annotatedvdb_amd.text_update.read_header`): ``fields`` its names, ``skip_lines`` the
    slab's lines up to and including it, ``id_col`` the column named ``variant``, ``key_col`` the
    column that is looked up (``id_col``; the ``ref_snp_id`` column for refSNP ids)."""
    fields: List[str]
    skip_lines: int
    id_col: int
    key_col: int

    def extra(self):
        return (self.skip_lines, len(self.fields), self.id_col, self.key_col)


@dataclass
class TxtTable(LofTable):
    """What K19a makes of a tab-delimited annotation file (:meth:`Engine.txt_table_build`):
    :class:`LofTable`'s members for one row per data line, keyed by the looked-up id; ``json``
    holds each row's body ``<label><TAB><update values>`` (the label is the id up to its first
    ``:``; ``N.TXT_ROW_PK_CHROM`` in ``flags`` marks an id without one, whose chromosome comes from
    the primary key); ``header`` the :class:`TxtHeader`; ``counts`` by ``N.TXT_COUNTS``."""
    header: Optional[TxtHeader] = None

    def view(self) -> "N.TxtTableView":
        if self.n_rows == 0:
            return N.TxtTableView()
        return N.TxtTableView(self.n_rows, N.ptr(self.rkeys), N.ptr(self.rkey_off), N.ptr(self.keyset),
                              self.keyset.numel(), N.ptr(self.json), self.json.numel(), N.ptr(self.json_off),
                              N.ptr(self.json_len), N.ptr(self.flags), N.ptr(self.hit))


@dataclass
class TxtUpdateRows:
    """What K19b and K19c make (:meth:`Engine.txt_update_rows`, :meth:`Engine.txt_direct_rows`):
    ``text`` holds the ``n`` update rows (``pk<TAB>chr<label><TAB>values[<TAB>true]<LF>``, row ``i``
    at ``row_off[i] .. row_off[i + 1]``), ``match`` the table row each was rendered from (``None``
    for K19c), ``counts`` the pass's counts by name (``N.TXTUPD_COUNTS`` / ``N.TXTDIR_COUNTS``)."""
    n: int
    text: torch.Tensor
    row_off: torch.Tensor
    match: Optional[torch.Tensor]
    counts: Dict[str, int]


VCF_EXPORT_HEADER = b"#CHRM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"  # (sic) export_variant2vcf.py:26



@dataclass
class ExportVcf:
    """What K14 makes of an export of ``AnnotatedVDB.Variant`` (:meth:`Engine.export_vcf`):
    ``vcf_text`` holds the rows of all ``n_files`` VCF files back to back, without their
    header lines (valid row ``v`` at ``vcf_row_off[v] .. vcf_row_off[v + 1]``; a row whose
    key repeats an earlier one of its file has no bytes), ``invalid_text`` the rows of the
    invalid file (``pk<TAB>alg<LF>``) with ``invalid_row_off``, ``flags`` the valid rows'
    ``N.EXPVCF_*`` flags, ``counts`` the pass's counts by name (``N.EXPVCF_COUNTS``, and
    ``dropped``: the rows a repeated key removed)."""
    vcf_text: torch.Tensor
    vcf_row_off: torch.Tensor
    invalid_text: torch.Tensor
    invalid_row_off: torch.Tensor
    flags: torch.Tensor
    counts: Dict[str, int]
    n_files: int
    variants_per_file: int
    file_start: List[int]  # n_files + 1 offsets into vcf_text

    def file_span(self, k: int) -> Tuple[int, int]:
        """``(begin, end)`` of file ``k`` (1 .. ``n_files``) in ``vcf_text``."""
        if not 1 <= k <= self.n_files:
            raise IndexError(f"file {k} of {self.n_files}")
        return self.file_start[k - 1], self.file_start[k]

    def files(self, directory: str, chromosome: str) -> List[str]:
        """Writes ``<chromosome>_<k>.vcf`` (the header line, then the file's rows) for
        every file and ``<chromosome>_invalid.txt``, named as ``export_variant2vcf.py``
        names them (``:30,40``); returns the paths."""
        vcf = self.vcf_text.cpu().numpy()
        paths = []
        for k in range(1, self.n_files + 1):
            b, e = self.file_span(k)
            paths.append(os.path.join(directory, "%s_%d.vcf" % (chromosome, k)))
            with open(paths[-1], "wb") as fh:
                fh.write(VCF_EXPORT_HEADER)
                fh.write(vcf[b:e].tobytes())
        paths.append(os.path.join(directory, chromosome + "_invalid.txt"))
        with open(paths[-1], "wb") as fh:
            fh.write(self.invalid_text.cpu().numpy().tobytes())
        return paths


VCF_SPLIT_HEADER = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"  # split_vcf_by_chr.py:17


@dataclass
class SplitVcf:
    """What K15 makes of a slab of a whole-genome VCF (:meth:`Engine.split_vcf`): ``text``
    holds 26 streams back to back, the data lines of ``chr1.vcf`` ... ``chrM.vcf``
    (``CHROM_NAMES`` order) and, as stream 25, the lines no file takes (``unknown="keep"``
    only); stream ``c`` is ``text[stream_off[c]:stream_off[c + 1]]``.  ``counts``: ``lines``
    and ``bytes`` (26 each), ``comments``, ``host_lines`` (the lines whose stripped end the
    host decided); ``first_other``: the index of the first line of stream 25, or ``None``."""
    text: torch.Tensor
    stream_off: List[int]  # 27 offsets into text
    counts: Dict[str, object]
    first_other: Optional[int]

    def stream(self, c: int) -> torch.Tensor:
        """Stream ``c`` (0 .. 25) as a slice of ``text``."""
        if not 0 <= c < N.SPLIT_N_STREAMS:
            raise IndexError(f"stream {c} of {N.SPLIT_N_STREAMS}")
        return self.text[self.stream_off[c]:self.stream_off[c + 1]]

    @property
    def other_text(self) -> torch.Tensor:
        return self.stream(N.SPLIT_OTHER)

    def append_files(self, directory: str, first: bool) -> List[str]:
        """Appends every stream 0..24 to ``chr<label>.vcf`` in ``directory``; with ``first``
        the files are created and begin with the header line, as ``create_fh_dict``
        (split_vcf_by_chr.py:14-22) writes it.  Returns the 25 paths."""
        host = self.text[:self.stream_off[N.SPLIT_OTHER]].cpu().numpy()
        paths = []
        for c, label in enumerate(CHROM_NAMES[:N.SPLIT_OTHER]):
            paths.append(os.path.join(directory, "chr%s.vcf" % label))
            with open(paths[-1], "wb" if first else "ab") as fh:
                if first:
                    fh.write(VCF_SPLIT_HEADER)
                fh.write(host[self.stream_off[c]:self.stream_off[c + 1]].tobytes())
        return paths


def existing_contig_mask(contigs) -> int:
    """K12's contig mask: ``None`` keeps every row; otherwise one bit per label of
    ``contigs`` (``CHROM_NAMES`` index; bit 31 for any other label)."""
    if contigs is None:
        return N.EXIST_ALL_CONTIGS
    if isinstance(contigs, int):
        return contigs & 0xFFFFFFFF
    mask = 0
    for c in contigs:
        c = str(c)
        mask |= 1 << (CHROM_NAMES.index(c) if c in CHROM_NAMES else 31)
    return mask


_RS_RE = re.compile(r"^rs([1-9][0-9]{0,17})$")


class ExtIdInterner:
    """Maps external-id strings to the u64 ``ext_id`` keys the kernels compare.

    Canonical ``rs<N>`` ids map to ``N`` (N < 2^62); any other string gets
    ``2^63 | k`` for an interned index ``k``; ``None`` is 0.  Equal keys <=>
    equal strings, which is all the dedup contract needs."""

    def __init__(self):
        self._ids: Dict[str, int] = {}
        self._rev: List[str] = []

    def key(self, s: Optional[str]) -> int:
        if s is None:
            return 0
        m = _RS_RE.match(s)
        if m:
            return int(m.group(1))
        k = self._ids.get(s)
        if k is None:
            k = len(self._rev)
            self._ids[s] = k
            self._rev.append(s)
        return (1 << 63) | k

    def to_str(self, key: int) -> Optional[str]:
        if key == 0:
            return None
        if key >> 63:
            return self._rev[key & ((1 << 63) - 1)]
        return "rs%d" % key


def pack_records(chrom_codes: Sequence[int], pos: Sequence[int], refs: Sequence[bytes],
                 alts: Sequence[bytes], ext_ids: Optional[Sequence[int]] = None) -> RecordBatch:
    """Host-side SoA packing (numpy -> pinned CPU tensors)."""
    n = len(pos)
    rl = np.fromiter((len(r) for r in refs), dtype=np.int64, count=n)
    al = np.fromiter((len(a) for a in alts), dtype=np.int64, count=n)
    tot = rl + al
    off = np.zeros(n, dtype=np.int64)
    if n:
        np.cumsum(tot[:-1], out=off[1:])
    heap = b"".join(r + a for r, a in zip(refs, alts))
    heap_np = np.frombuffer(heap, dtype=np.uint8) if heap else np.zeros(1, dtype=np.uint8)
    ext = np.zeros(n, dtype=np.int64) if ext_ids is None else \
        np.asarray([int(x) if x < (1 << 63) else int(x) - (1 << 64) for x in ext_ids], dtype=np.int64)
    return RecordBatch(
        chrom=torch.from_numpy(np.asarray(chrom_codes, dtype=np.uint8)),
        pos=torch.from_numpy(np.asarray(pos, dtype=np.int64).astype(np.int32)),
        allele_off=torch.from_numpy(off),
        ref_len=torch.from_numpy(rl.astype(np.int32)),
        alt_len=torch.from_numpy(al.astype(np.int32)),
        heap=torch.from_numpy(heap_np.copy()),
        ext_id=torch.from_numpy(ext),
    )


def dedup_list_bytes(n: int, slack: int = 0) -> int:
    """Bytes of K3's list workspace for ``n`` records (``kDedupListHead`` in
    ``csrc/avdb_internal.hpp``: a 16 KiB head, then one u32 entry per record, rounded up
    to four) with room for ``slack`` more entries."""
    return 16384 + 4 * (((n + 3) & ~3) + slack)


def as_u32(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().view(np.uint32)


# avdb_vcf_line (include/avdb.h), 80 bytes
VCF_LINE_DTYPE = np.dtype([("start", "<u8"), ("len", "<u4"), ("n_fields", "<u4"), ("field", "<u4", (8,)),
                           ("field_end8", "<u4"), ("pos", "<u4"), ("ext_id", "<u8"), ("n_alt", "<u4"),
                           ("n_rec", "<u4"), ("flags", "<u4"), ("chrom", "u1"), ("pad", "u1", (3,))])
assert VCF_LINE_DTYPE.itemsize == 80

VCF_COMMENT = 0x001
VCF_FEW_FIELDS = 0x002
VCF_BAD_POS = 0x004
VCF_EXT_HOST = 0x008
VCF_ID_RS = 0x010
VCF_INFO_RS = 0x020
VCF_ID_METASEQ = 0x040
VCF_CHROM_HOST = 0x080
VCF_EMPTY = 0x100
VCF_ID_HOST = 0x200
VCF_HOST_FLAGS = VCF_BAD_POS | VCF_EXT_HOST | VCF_CHROM_HOST | VCF_ID_HOST
VCF_UNPARSED_FLAGS = VCF_FEW_FIELDS | VCF_EMPTY  # K0 stopped before the fields: no CHROM, POS, ID or records


def _stamp(*ts) -> tuple:
    """Identity + version of each tensor: what a keyed K2 hand-off is tied to.
    A weak reference (a freed tensor whose block the caching allocator hands to a
    new tensor at the same address does not match) and ``_version`` (an in-place
    edit of the batch between the producer and the consumer does not match)."""
    import weakref
    return tuple(None if t is None else (weakref.ref(t), t._version) for t in ts)


def _stamp_ok(stamp: tuple, *ts) -> bool:
    if stamp is None or len(stamp) != len(ts):
        return False
    for st, t in zip(stamp, ts):
        if st is None or t is None:
            if st is not None or t is not None:
                return False
        elif st[0]() is not t or t._version != st[1]:
            return False
    return True


@dataclass
class VcfBatch:
    """Output of ``Engine.vcf_tokenize``: device text, per-line table, records."""
    text: torch.Tensor
    n_lines: int
    lines: Optional[torch.Tensor]  # uint8[n_lines * 80] (VCF_LINE_DTYPE); None: vcf_tokenize(want_lines=False)
    rec_off: torch.Tensor        # int64[n_lines + 1]
    heap_off: torch.Tensor
    records: RecordBatch
    rec_line: torch.Tensor       # int32[n_rec]
    rec_alt: torch.Tensor

    def lines_host(self, rows=None) -> np.ndarray:
        """The line table on the host, as ``VCF_LINE_DTYPE`` records; ``rows`` (line
        indices) takes only those lines: gathered on the device, then one copy."""
        if self.lines is None:
            raise ValueError("this batch was tokenized without its line table (want_lines=False)")
        if self.n_lines == 0:
            return np.zeros(0, dtype=VCF_LINE_DTYPE)
        t = self.lines[: self.n_lines * VCF_LINE_DTYPE.itemsize]
        if rows is not None:
            t = t.view(self.n_lines, -1)[torch.as_tensor(rows, dtype=torch.int64, device=t.device)]
        return t.cpu().numpy().reshape(-1).view(VCF_LINE_DTYPE)

    def line_flags(self) -> torch.Tensor:
        """The table's ``flags`` column on the device (a strided int32 view)."""
        t = self.lines[: self.n_lines * VCF_LINE_DTYPE.itemsize].view(torch.int32)
        return t.view(self.n_lines, -1)[:, VCF_LINE_DTYPE.fields["flags"][1] // 4]


class _Timer:
    """Optional HIP-event pairs on the engine's stream (bench stage timing)."""

    def __init__(self, events: Optional[dict], device):
        self.events, self.device, self.cur = events, device, None

    def start(self, name):
        if self.events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.device))
            self.cur = (name, e)

    def stop(self):
        if self.events is not None and self.cur:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(self.device))
            self.events.setdefault(self.cur[0], []).append((self.cur[1], e))
            self.cur = None


@dataclass
class FormatResult:
    """Output of ``Engine.vcf_format`` (device tensors)."""
    copy: torch.Tensor           # uint8: COPY rows of every GPU-rendered line, in line order
    mapping: torch.Tensor        # uint8: .mapping lines
    copy_off: torch.Tensor       # int64[n_lines + 1]: start of each line's rows
    map_off: torch.Tensor        # int64[n_lines + 1]
    line_state: torch.Tensor     # uint8[n_lines]: LINE_GPU / LINE_HOST / LINE_SKIP
    counters: torch.Tensor


@dataclass
class KeyText:
    """Output of ``Engine.primary_keys`` (device tensors): key i is
    ``keys[key_off[i]:key_off[i+1]]`` when ``state[i] == KEY_OK``; path i is
    ``paths[path_off[i]:path_off[i+1]]`` (empty for an unmappable record).
    ``off32``: ``key_off`` / ``path_off`` are raw buffers in the narrow layout
    (AVDB_KEYS_OFF32: uint32 low words + a uint64 base per 4,096 records) —
    :meth:`key_offsets` / :meth:`path_offsets` give the int64 offsets either way."""
    ws: torch.Tensor
    key_off: torch.Tensor
    path_off: Optional[torch.Tensor]
    state: torch.Tensor
    keys: Optional[torch.Tensor]
    paths: Optional[torch.Tensor]
    off32: bool = False

    @staticmethod
    def _wide(t: torch.Tensor, n: int) -> torch.Tensor:
        lb = (4 * (n + 1) + 7) & ~7
        low = t[: 4 * (n + 1)].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        base = t[lb: lb + 8 * ((n >> 12) + 1)].view(torch.int64).repeat_interleave(4096)[: n + 1]
        return base + ((low - (base & 0xFFFFFFFF)) & 0xFFFFFFFF)

    def key_offsets(self, n: int) -> torch.Tensor:
        """int64 key offsets [n + 1] (device)."""
        return self._wide(self.key_off, n) if self.off32 else self.key_off[: n + 1]

    def path_offsets(self, n: int) -> Optional[torch.Tensor]:
        if self.path_off is None:
            return None
        return self._wide(self.path_off, n) if self.off32 else self.path_off[: n + 1]

    def host(self, n: int):
        """(keys, paths) as Python lists of str (None where not rendered).
        Raises ``ValueError`` if a text did not fit its buffer (a reused
        ``KeyText`` too small for this batch: state KEY_OVERFLOW / PATH_OVERFLOW)."""
        ko = self.key_offsets(n).cpu().numpy()
        kb = self.keys[: int(ko[n])].cpu().numpy().tobytes()
        st = self.state[:n].cpu().numpy()
        if ((st == N.KEY_OVERFLOW) | ((st & N.PATH_OVERFLOW) != 0)).any():
            raise ValueError("primary_keys: key/path text exceeded the reused KeyText buffers")
        keys = [kb[ko[i]:ko[i + 1]].decode() if st[i] == N.KEY_OK else None for i in range(n)]
        paths = None
        if self.paths is not None:
            po = self.path_offsets(n).cpu().numpy()
            pb = self.paths[: int(po[n])].cpu().numpy().tobytes()
            paths = [pb[po[i]:po[i + 1]].decode() or None for i in range(n)]
        return keys, paths


class SmallPrep:
    """K8 (``avdb_small_prep``) over one host-mapped pinned arena: the
    per-record / per-line drop-in path as one launch + one stream sync, no
    copies (the kernel reads the records and writes the results over PCIe).
    Batches that do not fit the arena return ``None`` (callers then use the
    multi-kernel path).

    A call of at most ``host_max`` records (one ``find_bin_index`` miss, one
    ``parse_variant`` line) runs K8h instead, ``avdb_small_prep_host``: the
    same record arithmetic compiled into the library's host code, over the same
    arena.  A launch plus a stream sync costs ~25 us on MI355X, more than the
    reference's whole per-line call; the kernels take every batch.
    ``AVDB_PERCALL=gpu`` (or ``mode='gpu'``) sends every call to K8,
    ``AVDB_PERCALL=host`` every call that fits to K8h."""

    HOST_MAX = 32

    def __init__(self, engine: "Engine", max_records: int = 4096, heap_bytes: int = 1 << 20,
                 text_bytes: Tuple[int, int, int] = (1 << 19, 1 << 19, 1 << 21)):
        self.eng = engine
        self.mode = os.environ.get("AVDB_PERCALL", "auto")  # auto | host | gpu
        self.host_max = self.HOST_MAX
        self.last_path = None  # "host" | "gpu": which entry served the last call
        self.R = int(max_records)
        self.H = int(heap_bytes)
        self.T = tuple(int(t) for t in text_bytes)
        # arena: the per-call SoA region (inputs then outputs of one call, packed
        # per call size by _layout: <= 62 bytes per record), the allele heap and
        # the three text streams
        self.scratch = 64 * (self.R + 1)
        regions = [("soa", self.scratch), ("heap", self.H)] + [("text%d" % k, self.T[k]) for k in range(3)]
        total = 0
        self.addr = {}
        offs = {}
        for name, nbytes in regions:
            total = (total + 63) & ~63
            offs[name] = total
            total += nbytes
        self._ptr = self._alloc(total)
        self._buf = np.ctypeslib.as_array((ctypes.c_uint8 * total).from_address(self._ptr))
        self._mv = memoryview(self._buf).cast("B")
        self._layouts = {}
        for name, off in offs.items():
            self.addr[name] = self._ptr + off
        self._heap0 = offs["heap"]
        self._text0 = [offs["text%d" % k] for k in range(3)]

    def _alloc(self, total: int) -> int:
        """The arena: pinned host memory mapped into the device (avdb_host_alloc);
        plain host memory for a host-only engine (K8h never reads it from a kernel)."""
        if self.eng.host_only:
            self._host_arena = np.zeros(total + 64, dtype=np.uint8)
            return (self._host_arena.ctypes.data + 63) & ~63
        p = ctypes.c_void_p()
        N.call("avdb_host_alloc", total, ctypes.byref(p))
        return p.value

    def close(self):
        if getattr(self, "_ptr", None):
            if not self.eng.host_only:
                self.eng.lib.avdb_host_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _layout(self, n: int, kind: int):
        """Per-call layout for ``n`` records (cached): the arrays of one call
        packed back to back at the start of the arena, a ``SmallBatch`` holding
        their pointers, and one ``struct`` each for all inputs and all outputs.
        kind: 0 intervals (end_in), 1 alleles, 2 alleles + ext_id."""
        key = (n, kind)
        lay = self._layouts.get(key)
        if lay is not None:
            return lay
        fmt_in, fmt_out = ["<"], ["<"]
        at = [0]
        ptr = {}

        def put(fmt, name, code, cnt, size):
            pad = (-at[0]) % 8
            if pad:
                fmt.append("%dx" % pad)
                at[0] += pad
            ptr[name] = self._ptr + at[0]
            fmt.append("%d%s" % (cnt, code))
            at[0] += cnt * size
        put(fmt_in, "chrom", "B", n, 1)
        put(fmt_in, "pos", "I", n, 4)
        if kind == 0:
            put(fmt_in, "end_in", "I", n, 4)
        else:
            put(fmt_in, "allele_off", "Q", n, 8)
            put(fmt_in, "ref_len", "I", n, 4)
            put(fmt_in, "alt_len", "I", n, 4)
            if kind == 2:
                put(fmt_in, "ext_id", "Q", n, 8)
        in_bytes = at[0] = (at[0] + 15) & ~15
        put(fmt_out, "end_out", "I", n, 4)
        put(fmt_out, "code", "I", n, 4)
        put(fmt_out, "status", "B", n, 1)
        if kind:
            put(fmt_out, "key_state", "B", n, 1)
            put(fmt_out, "disp_state", "B", n, 1)
        put(fmt_out, "off_out", "I", 3 * (n + 1), 4)
        put(fmt_out, "overflow", "I", 2, 4)
        if at[0] > self.scratch:
            return None
        b = N.SmallBatch()
        for name in ("chrom", "pos", "end_in", "allele_off", "ref_len", "alt_len", "ext_id", "end_out", "code",
                     "status", "key_state", "disp_state", "off_out", "overflow"):
            if name in ptr:
                setattr(b, name, ptr[name])
        b.heap = self.addr["heap"]
        for k in range(3):
            b.text_out[k] = self.addr["text%d" % k]
            b.text_cap[k] = self.T[k]
        b.n = n
        lay = (b, struct.Struct("".join(fmt_in)), struct.Struct("".join(fmt_out)), in_bytes)
        self._layouts[key] = lay
        return lay

    def run(self, chrom, pos, ends=None, refs: Optional[Sequence[bytes]] = None,
            alts: Optional[Sequence[bytes]] = None, ext=None, want: int = 1, max_seq_len: int = 50):
        """Returns a dict of results (lists) or ``None`` when the batch does not
        fit.  Text streams: ``path`` / ``key`` / ``display`` lists of str (None
        where not rendered).  All inputs of a call go into the arena with one
        ``struct.pack_into`` and all outputs come back with one ``unpack_from``
        (plus the allele bytes and the texts): a call of a few records costs a
        few microseconds of Python around the library call."""
        n = len(pos)
        if n > self.R:
            return None
        kind = 0 if refs is None else (2 if ext is not None else 1)
        lay = self._layout(n, kind)
        if lay is None:
            return None
        b, s_in, s_out, in_bytes = lay
        mv = self._mv
        if kind:
            rl = [len(x) for x in refs]
            al = [len(x) for x in alts]
            heap = b"".join([r + x for r, x in zip(refs, alts)])
            hb = len(heap)
            if hb > self.H:
                return None
            offs = [0] * n
            t = 0
            for i in range(n):
                offs[i] = t
                t += rl[i] + al[i]
            h0 = self._heap0
            mv[h0:h0 + hb] = heap
            b.heap_bytes = max(hb, 1)
            if kind == 2:
                s_in.pack_into(mv, 0, *chrom, *pos, *offs, *rl, *al, *ext)
            else:
                s_in.pack_into(mv, 0, *chrom, *pos, *offs, *rl, *al)
        else:
            s_in.pack_into(mv, 0, *chrom, *pos, *ends)
        b.max_seq_len, b.want = int(max_seq_len), int(want)
        on_host = self.mode == "host" or (self.mode == "auto" and n <= self.host_max) or self.eng.host_only
        if on_host:
            N.check("avdb_small_prep_host", self.eng.lib.avdb_small_prep_host(self.eng.ctx, ctypes.byref(b)))
        else:
            N.check("avdb_small_prep", self.eng.lib.avdb_small_prep(self.eng.ctx, ctypes.byref(b),
                                                                    self.eng._stream()))
            torch.cuda.current_stream(self.eng.device).synchronize()
        self.last_path = "host" if on_host else "gpu"
        r = s_out.unpack_from(mv, in_bytes)
        if r[-2] & want:  # overflow
            return None
        out = {"end": list(r[:n]), "code": list(r[n:2 * n]), "status": list(r[2 * n:3 * n])}
        k0 = 3 * n
        if kind:
            out["key_state"] = list(r[k0:k0 + n])
            out["disp_state"] = list(r[k0 + n:k0 + 2 * n])
            k0 += 2 * n
        for k, name in enumerate(("path", "key", "display")):
            if not (want >> k) & 1:
                continue
            o = r[k0 + k * (n + 1): k0 + (k + 1) * (n + 1)]
            t0 = self._text0[k]
            raw = bytes(mv[t0:t0 + o[n]]).decode("ascii")
            out[name] = [raw[o[i]:o[i + 1]] if o[i + 1] > o[i] else None for i in range(n)]
        return out


class ChromMap:
    """``avdb_chrom_map`` of a ChromosomeMap's ``source_id -> chromosome`` dict
    (chromosome_map_parser.py:51-91).  For each source id the host decides once
    what the reference's per-line code makes of it — ``update_chromosome`` then
    ``get_variant`` (xstr, 'MT' -> 'M', 'chr' removed, vcf_parser.py:117-155) —
    and gives the kernels the contig code, or 0xFF (the line is rendered by the
    host) when the result is not a canonical contig label, or when the source id
    is text Python would coerce to a number (a CHROM field equal to it becomes an
    int before the lookup and never matches: KeyError)."""

    def __init__(self, engine: "Engine", mapping: Dict):
        from .chromosomes import CHROM_NAMES as names, bin_index_chrom_code
        from .parsers import to_numeric
        self.eng, self.mapping = engine, mapping
        keys, codes = [], []
        for k, v in mapping.items():
            if not isinstance(k, str):
                continue  # a CHROM field is a str (or a number): never this key
            try:
                kb = k.encode("ascii")
            except UnicodeEncodeError:
                continue  # K0 flags non-ASCII lines for the host anyway
            chrom = "" if v is None else str(v)
            if chrom == "MT":
                chrom = "M"
            chrom = chrom.replace("chr", "")
            c = bin_index_chrom_code(chrom)
            ok = c < len(names) and names[c] == chrom and isinstance(to_numeric(k), str)
            keys.append(kb)
            codes.append(c if ok else 0xFF)
        self._create(keys, codes)

    @classmethod
    def for_split(cls, engine: "Engine", mapping: Dict) -> "ChromMap":
        """The map by the rule of ``split_vcf_by_chr.py:44-50`` (K15): the code of a
        source id is the index of ``mapping[id]`` among the 25 file labels when it is
        exactly one of them, else 0xFF (no file: the reference's ``KeyError``).  No
        'MT' -> 'M' step and no numeric coercion of the key: the script looks the text
        of the first field up as it is."""
        from .chromosomes import CHROM_NAMES as names
        self = cls.__new__(cls)
        self.eng, self.mapping = engine, mapping
        keys, codes = [], []
        for k, v in mapping.items():
            if not isinstance(k, str):
                continue
            keys.append(k.encode("utf-8"))
            codes.append(names.index(v) if isinstance(v, str) and v in names else 0xFF)
        self._create(keys, codes)
        return self

    def _create(self, keys, codes):
        engine = self.eng
        off = np.zeros(len(keys) + 1, dtype=np.uint64)
        if keys:
            off[1:] = np.cumsum([len(k) for k in keys])
        blob = np.frombuffer(b"".join(keys) or b"\0", dtype=np.uint8)
        cd = np.asarray(codes or [0], dtype=np.uint8)
        h = ctypes.c_void_p()
        N.call("avdb_chrom_map_create", engine.ctx, blob, off, len(keys), cd, ctypes.byref(h))
        self.handle = h.value
        self.n_keys = len(keys)

    def close(self):
        if getattr(self, "handle", None):
            self.eng.lib.avdb_chrom_map_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LineHost:
    """K5h (``avdb_vcf_line_host``): one VCF line -> its COPY rows and .mapping
    line, rendered by the library's host code with the kernels' own per-line
    definitions (K0 parse_line, K2 infer_end/classify, K5 format_line).  The
    loader's per-line ``parse_variant`` uses it: no GPU launch per line."""

    def __init__(self, engine: "Engine", cap: int = 1 << 16):
        self.eng = engine
        self.res = N.LineResult()
        self.opts = N.FormatOpts()
        self.rendered = 0  # lines this entry rendered (the rest went to the caller)
        self._grow(cap)

    def _grow(self, cap: int):
        self.cap = int(cap)
        self._copy = ctypes.create_string_buffer(self.cap)
        self._map = ctypes.create_string_buffer(self.cap)
        self._ca, self._ma = ctypes.addressof(self._copy), ctypes.addressof(self._map)

    def run(self, line: bytes, alg_id: bytes, max_seq_len: int = 50, adsp: bool = False, vcf_opts=None):
        """``(state, copy_text, mapping_text, result)``; the texts are None unless
        state == LINE_GPU (rendered).  ``vcf_opts``: header width / chromosome map."""
        o = self.opts
        o.alg_id, o.max_seq_len, o.flags = alg_id, max_seq_len, N.FORMAT_ADSP if adsp else 0
        r = self.res
        vo = ctypes.byref(vcf_opts) if vcf_opts is not None else None
        rc = self.eng.lib.avdb_vcf_line_host(self.eng.ctx, line, len(line), ctypes.byref(o), vo, self._ca, self.cap,
                                             self._ma, self.cap, ctypes.byref(r))
        if rc == N.AVDB_ERANGE:
            self._grow(2 * max(r.copy_bytes, r.map_bytes))
            rc = self.eng.lib.avdb_vcf_line_host(self.eng.ctx, line, len(line), ctypes.byref(o), vo, self._ca,
                                                 self.cap, self._ma, self.cap, ctypes.byref(r))
        N.check("avdb_vcf_line_host", rc)
        if r.state != N.LINE_GPU:
            return r.state, None, None, r
        self.rendered += 1
        return (r.state, ctypes.string_at(self._ca, r.copy_bytes).decode("ascii"),
                ctypes.string_at(self._ma, r.map_bytes).decode("ascii"), r)


# ---------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------
class Engine:
    """A context on one GPU: chromosome-length table + kernel entry points."""

    def __init__(self, device=None, lengths: Optional[Sequence[int]] = None, assembly: str = "GRCh38",
                 sequence_digests: Optional[Sequence[str]] = None):
        if device is None and os.environ.get("AVDB_DEVICE") == "host":
            device = "host"
        # "host": a host-only engine — only the library's per-call host entries
        # (K5h, K8h, K1h: the kernels' record arithmetic compiled for the host side)
        # work; every kernel entry raises NativeUnavailable.  Opt-in only
        # (device="host" or AVDB_DEVICE=host), never a silent fallback.
        self.host_only = device == "host"
        if not self.host_only:
            N.require_gpu()
        self.lib = N.load_library()
        if self.host_only:
            self.device = torch.device("cpu")
        else:
            if device is None:
                device = torch.cuda.current_device()
            self.device = torch.device("cuda", int(device) if not isinstance(device, torch.device)
                                       else (device.index or 0))
        self.lengths = list(lengths) if lengths is not None else length_table(assembly)
        arr = (ctypes.c_uint32 * len(self.lengths))(*self.lengths)
        h = ctypes.c_void_p()
        N.call("avdb_ctx_create", -1 if self.host_only else self.device.index, arr, len(self.lengths),
               ctypes.byref(h))
        self._ctx = h
        nb = ctypes.c_uint32()
        self._call("avdb_l8_bin_count", ctypes.byref(nb))
        self.n_l8 = int(nb.value)
        # what the last keyed K2 left for its consumers, each entry tied (by _stamp)
        # to the exact tensors it was computed from and taken by the one call it
        # was meant for: "totals" (K7's group totals in a KeyText's workspace),
        # "codes" (K4's long-record codes in a digest workspace), "marks" (K3's
        # first phase in a dedup workspace + keep).  Every record_prep call drops
        # all of them first.
        self._pending: Dict[str, tuple] = {}
        self.last_vcf_path = ""  # vcf_tokenize(want_lines=False): "local" (count-free) or "counted"
        # test hook: every output / workspace tensor the engine allocates is filled
        # with this byte first (None: torch.empty), so a check sees only what the
        # kernels wrote, never what an earlier pass left in a recycled block
        self.poison: Optional[int] = None
        if sequence_digests is not None:
            self.set_sequence_digests(sequence_digests)

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_small", None) is not None:
            self._small.close()
            self._small = None
        if getattr(self, "_ctx", None):
            self.lib.avdb_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def ctx(self):
        if not self._ctx:
            raise N.NativeUnavailable("engine closed")
        return self._ctx

    def _stream(self):
        if self.host_only:
            raise N.NativeUnavailable("a host-only engine (AVDB_DEVICE=host) runs the per-call host entries only; "
                                      "this batch entry is a gfx950 kernel and needs a GPU")
        return N.stream_handle(self.device)

    def _call(self, name: str, *args) -> int:
        """``N.call`` of a context entry."""
        return N.call(name, self.ctx, *args)

    def _launch(self, name: str, *args) -> int:
        """``N.call`` of a kernel entry: on the context, into the current stream."""
        return N.call(name, self.ctx, *args, self._stream())

    def small(self) -> SmallPrep:
        """The engine's K8 arena (created on first use)."""
        sp = getattr(self, "_small", None)
        if sp is None:
            sp = self._small = SmallPrep(self)
        return sp

    def chrom_map(self, mapping: Dict, key=None) -> "ChromMap":
        """A ChromosomeMap's ``source_id -> chromosome`` dict as a library map
        (device table for K0, host table for K5h), cached per ``key``."""
        cache = self.__dict__.setdefault("_chrom_maps", {})
        k = key if key is not None else id(mapping)
        cm = cache.get(k)
        if cm is None or cm.mapping is not mapping:
            cm = cache[k] = ChromMap(self, mapping)
        return cm

    def vcf_opts(self, min_fields: int = 0, chrom_map: Optional["ChromMap"] = None) -> "N.VcfOpts":
        return N.VcfOpts(min_fields, chrom_map.handle if chrom_map is not None else None)

    def line_host(self) -> LineHost:
        """The engine's K5h per-line renderer (created on first use)."""
        lh = getattr(self, "_line_host", None)
        if lh is None:
            lh = self._line_host = LineHost(self)
        return lh

    def set_sequence_digests(self, digests: Sequence[str]):
        if len(digests) != len(self.lengths) or any(len(d) != N.DIGEST_CHARS for d in digests):
            raise ValueError("need one 32-character refget digest per chromosome")
        blob = "".join(digests).encode("ascii")
        self._call("avdb_ctx_set_sequence_digests", blob, len(digests))

    # -- buffers -----------------------------------------------------------
    def empty(self, n, dtype):
        t = torch.empty(n, dtype=dtype, device=self.device)
        if self.poison is not None:
            t.view(torch.uint8).fill_(self.poison)
        return t

    def scratch(self, name: str, nbytes: int) -> torch.Tensor:
        """A workspace of at least ``nbytes`` bytes kept by the engine under ``name``
        and reused by later calls (grown when too small).  Every user runs on the
        engine's stream, so a later call's kernels are ordered after the earlier
        call's; with ``poison`` set it is refilled like a fresh buffer."""
        cache = self.__dict__.setdefault("_scratch", {})
        t = cache.get(name)
        if t is None or t.numel() < nbytes or t.device != self.device:
            cache[name] = None
            t = cache[name] = torch.empty(max(1, int(nbytes)), dtype=torch.uint8, device=self.device)
        if self.poison is not None:
            t.fill_(self.poison)
        return t

    def workspace(self, nbytes: int, given: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The caller's workspace when it holds ``nbytes``, else a fresh one."""
        return given if given is not None and given.numel() >= nbytes else self.empty(nbytes, torch.uint8)

    def _batch(self, b: RecordBatch) -> RecordBatch:
        """``b`` on the engine's device, its allele arrays checked."""
        b = b if b.device == self.device else b.to(self.device)
        self._check_alleles(b)
        return b

    def set_option(self, option: int, value: int):
        """``avdb_ctx_set_option`` (launch shape only: ``N.OPT_K4_GRID``)."""
        self._call("avdb_ctx_set_option", int(option), int(value))

    def new_histogram(self) -> torch.Tensor:
        return torch.zeros(self.n_l8, dtype=torch.int32, device=self.device)

    def new_counters(self) -> torch.Tensor:
        return torch.zeros(N.N_COUNTERS, dtype=torch.int64, device=self.device)

    def _dev(self, t: Optional[torch.Tensor]):
        if t is None:
            return None
        if t.device != self.device:
            t = t.to(self.device, non_blocking=True)
        return t.contiguous()

    # -- K1 ----------------------------------------------------------------
    def bin_assign(self, chrom: torch.Tensor, start: torch.Tensor, end: Optional[torch.Tensor] = None,
                   *, want_status: bool = True, hist: Optional[torch.Tensor] = None,
                   counters: Optional[torch.Tensor] = None,
                   out_code: Optional[torch.Tensor] = None,
                   out_status: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        chrom, start, end = self._dev(chrom), self._dev(start), self._dev(end)
        n = chrom.numel()
        if start.numel() != n or (end is not None and end.numel() != n):
            raise ValueError("chrom/start/end length mismatch")
        if chrom.dtype != torch.uint8 or start.element_size() != 4 or (end is not None and end.element_size() != 4):
            raise TypeError("chrom must be uint8, start/end 32-bit")
        code = out_code if out_code is not None else self.empty(n, torch.int32)
        status = None
        if want_status:
            status = out_status if out_status is not None else self.empty(n, torch.uint8)
        if hist is not None and hist.numel() != self.n_l8:
            raise ValueError("histogram must have n_l8 bins")
        self._launch("avdb_bin_assign", chrom, start, end, n, code, status, hist, counters)
        return code, status

    # -- K2 ----------------------------------------------------------------
    def record_prep(self, b: RecordBatch, *, want_lcp: bool = True, hist: Optional[torch.Tensor] = None,
                    counters: Optional[torch.Tensor] = None, keys: Optional["KeyText"] = None,
                    key_digest: bool = False, key_paths: bool = True, max_seq_len: int = 50,
                    digest_workspace: Optional[torch.Tensor] = None,
                    dedup_workspace: Optional[torch.Tensor] = None):
        """Returns ``(end, code, status, lcp)`` device tensors.  With ``keys`` (a
        one-pass ``KeyText`` from an earlier ``primary_keys`` on a same-sized
        batch) K2 also writes K7's group totals into its workspace
        (``avdb_record_prep_keyed``), so the next ``primary_keys(b, code,
        digest if key_digest, out=keys)`` skips its totals pass; with
        ``digest_workspace`` too (the K4 workspace the next ``vrs_digest(b,
        max_seq_len, workspace=...)`` gets) it classifies the long records for K4,
        and with ``dedup_workspace`` (the one the next ``pk_dedup(b, workspace=...)``
        gets) it runs K3's first phase, so that call only resolves the listed runs.
        Either workspace without ``keys`` runs the same K2 without K7's totals (a
        step with no key text, as C5's)."""
        b = self._batch(b)
        n = b.n
        self._pending.clear()
        end = self.empty(n, torch.int32)
        code = self.empty(n, torch.int32)
        status = self.empty(n, torch.uint8)
        lcp = self.empty(n, torch.int32) if want_lcp else None
        args = (*b.soa(), n, end, code, status, lcp, hist, counters)
        if keys is None and digest_workspace is None and dedup_workspace is None:
            self._launch("avdb_record_prep", *args)
            return end, code, status, lcp
        dws = digest_workspace
        if dws is not None:
            need = N.size("avdb_vrs_digest_workspace_size", n)
            if dws.numel() < need:
                raise ValueError("record_prep: digest_workspace needs %d bytes" % need)
        ddw = dedup_workspace
        keep = None
        if ddw is not None:
            keep = self.empty(max(4, n), torch.uint8)
        done = ctypes.c_int(0)
        self._launch("avdb_record_prep_keyed", *args, b.ext_id, int(max_seq_len), 1 if key_digest else 0,
                     1 if key_paths else 0, keys.ws if keys is not None else None,
                     keys.ws.numel() if keys is not None else 0, dws, dws.numel() if dws is not None else 0,
                     ddw, ddw.numel() if ddw is not None else 0, keep, ctypes.byref(done))
        # (tied to these exact tensors: another batch, a reallocated one or an
        # in-place edit recomputes)
        if done.value & N.KEYED_TOTALS:
            self._pending["totals"] = (_stamp(keys.ws, b.chrom, b.pos, b.ref_len, b.alt_len, b.ext_id,
                                              code if key_paths else None),
                                       keys, n, int(max_seq_len), bool(key_digest))
        if done.value & N.KEYED_LONG_CODES:
            self._pending["codes"] = (_stamp(dws, b.ref_len, b.alt_len), n, int(max_seq_len))
        if done.value & N.KEYED_DEDUP_MARKS:
            self._pending["marks"] = (_stamp(ddw, b.chrom, b.pos), n, keep)
        return end, code, status, lcp

    def keyed_prep(self, b: RecordBatch, kt: "KeyText", *, max_seq_len: int = 50, defer_digest: bool = True,
                   hist: Optional[torch.Tensor] = None, counters: Optional[torch.Tensor] = None,
                   digest_workspace: Optional[torch.Tensor] = None,
                   dedup_workspace: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
        """K2 + K7 in one pass (``avdb_keyed_prep``): ``(end, code, status, keep)``
        and ``kt`` filled with the keys and ltree paths (long keys' digests pending
        for :meth:`fill_digests` when ``defer_digest``).  With ``digest_workspace``
        (the one the next ``vrs_digest`` gets) it classifies the long records for K4;
        with ``dedup_workspace`` it runs K3's first phase (``keep`` = 1 and the listed
        runs; the next ``pk_dedup(b, workspace=...)`` resolves them), else ``keep`` is
        None.  ``workspace``: ``avdb_keyed_prep_workspace_size`` bytes (allocated
        when None)."""
        b = self._batch(b)
        n = b.n
        self._pending.clear()
        if kt.key_off.numel() < n + 1 or kt.state.numel() < max(1, n) or kt.keys is None or kt.off32:
            raise ValueError("keyed_prep: the KeyText holds fewer records (or narrow offsets)")
        ws = self.workspace(N.size("avdb_keyed_prep_workspace_size", n), workspace)
        end = self.empty(n, torch.int32)
        code = self.empty(n, torch.int32)
        status = self.empty(n, torch.uint8)
        dws, ddw = digest_workspace, dedup_workspace
        keep = self.empty(max(4, n), torch.uint8) if ddw is not None else None
        done = ctypes.c_int(0)
        self._launch("avdb_keyed_prep", *b.soa(), b.ext_id, n, int(max_seq_len), end, code, status, hist, counters,
                     ws, ws.numel(), dws, dws.numel() if dws is not None else 0, ddw,
                     ddw.numel() if ddw is not None else 0, keep, kt.key_off,
                     kt.path_off if kt.paths is not None else None, kt.keys, kt.keys.numel(), kt.paths,
                     kt.paths.numel() if kt.paths is not None else 0, kt.state,
                     N.KEYS_DIGEST_DEFERRED if defer_digest else 0, ctypes.byref(done))
        self.last_keyed_ws = ws
        if done.value & N.KEYED_LONG_CODES:
            self._pending["codes"] = (_stamp(dws, b.ref_len, b.alt_len), n, int(max_seq_len))
        if done.value & N.KEYED_DEDUP_MARKS:
            self._pending["marks"] = (_stamp(ddw, b.chrom, b.pos), n, keep, N.DEDUP_ONEPASS)
        return end, code, status, keep

    def keyed_prep_lookback_errors(self, workspace: torch.Tensor) -> int:
        """Look-back polls that gave up in the last ``keyed_prep`` on ``workspace``
        (a host sync; 0 expected)."""
        v = ctypes.c_uint32()
        self._call("avdb_keyed_prep_lookback_errors", workspace, ctypes.byref(v))
        return int(v.value)

    # -- K3 ----------------------------------------------------------------
    def pk_dedup(self, b: RecordBatch, *, grouped: bool = True,
                 counters: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        b = self._batch(b)
        n = b.n
        marks = self._pending.pop("marks", None)
        if (grouped and workspace is not None and marks is not None and marks[1] == n
                and _stamp_ok(marks[0], workspace, b.chrom, b.pos)):
            # the keyed K2 already wrote keep = 1 and listed the runs: resolve them
            keep = marks[2]
            flags = N.DEDUP_MARKED | (marks[3] if len(marks) > 3 else 0)
            self._launch("avdb_pk_dedup_ex", *b.soa(), b.ext_id, n, workspace, workspace.numel(), keep, counters,
                         flags)
            return keep[:n]
        keep = self.empty(n, torch.uint8)
        # grouped: the list of same-position records (two-phase run scan)
        ws_bytes = dedup_list_bytes(n) if grouped else N.size("avdb_pk_dedup_workspace_size", n)
        ws = self.workspace(ws_bytes, workspace)
        self._launch("avdb_pk_dedup", *b.soa(), b.ext_id, n, 1 if grouped else 0, ws, ws_bytes, keep, counters)
        return keep

    # -- K4 ----------------------------------------------------------------
    def vrs_digest(self, b: RecordBatch, max_seq_len: int = 50,
                   workspace: Optional[torch.Tensor] = None,
                   keys: Optional["KeyText"] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Returns ``(digests uint8[n,32], is_long uint8[n])``.  Only the rows
        with ``is_long`` set are written (the rest are unspecified: zero-filling
        32 bytes per record would cost more HBM traffic than the digests).
        ``keys``: the ``KeyText`` of a deferred ``primary_keys`` / ``keyed_prep``
        on this batch — the digests also go into its pending keys
        (``avdb_vrs_digest_keys``: no :meth:`fill_digests` pass)."""
        b = self._batch(b)
        n = b.n
        dig = self.empty(max(1, n) * N.DIGEST_CHARS, torch.uint8).view(-1, N.DIGEST_CHARS)[:n]
        is_long = self.empty(n, torch.uint8)
        need = N.size("avdb_vrs_digest_workspace_size", n)
        ws = self.workspace(need, workspace)
        # the keyed K2 classified this batch's records into this workspace
        codes = self._pending.pop("codes", None)
        ready = (codes is not None and codes[1:] == (n, int(max_seq_len))
                 and _stamp_ok(codes[0], ws, b.ref_len, b.alt_len))
        args = (*b.soa(), n, int(max_seq_len), ws, need, dig, is_long, N.DIGEST_CODES_READY if ready else 0)
        if keys is None:
            self._launch("avdb_vrs_digest_ex", *args)
        else:
            if keys.off32:
                raise ValueError("vrs_digest(keys=...): narrow key offsets are not accepted")
            self._launch("avdb_vrs_digest_keys", *args, keys.key_off, keys.keys, keys.state)
        return dig, is_long

    def sha512t24u(self, blobs: Sequence[bytes]) -> List[str]:
        n = len(blobs)
        if n == 0:
            return []
        lens = np.fromiter((len(x) for x in blobs), dtype=np.int64, count=n)
        off = np.zeros(n, dtype=np.int64)
        np.cumsum(lens[:-1], out=off[1:])
        data = b"".join(blobs) or b"\0"
        d_data = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(self.device)
        d_off = torch.from_numpy(off).to(self.device)
        d_len = torch.from_numpy(lens.astype(np.int32)).to(self.device)
        out = self.empty(n * N.DIGEST_CHARS, torch.uint8)
        self._launch("avdb_sha512t24u", d_data, d_off, d_len, n, out)
        raw = out.cpu().numpy().tobytes()
        return [raw[i * 32:(i + 1) * 32].decode("ascii") for i in range(n)]

    # -- K0: VCF text -> records ---------------------------------------------
    def vcf_tokenize(self, text, vcf_opts: Optional["N.VcfOpts"] = None, want_lines: bool = True,
                     count_free: bool = True) -> "VcfBatch":
        """Parse VCF data lines (bytes or a uint8 tensor) on the GPU into the
        record SoA (one row per ALT != '.') plus the per-line table.
        ``vcf_opts`` (:meth:`vcf_opts`): header width and chromosome map.
        ``want_lines=False``: no public line table (``VcfBatch.lines`` is None) — for
        callers that need only the records: the count-free path (avdb_vcf_parse_local:
        each parse window writes its lines to slots of its own, one scan of the window
        totals, avdb_vcf_emit_local), or, when a window holds more lines, records or allele
        bytes than its slots, count -> parse -> emit from 32-byte records in the parse
        workspace (also taken with ``count_free=False``)."""
        if not want_lines and count_free:
            vb, text = self._vcf_tokenize_local(text, vcf_opts)
            if vb is not None:
                self.last_vcf_path = "local"
                return vb
            # (a window overflowed its line slots: the counted path, on the text the
            # count-free attempt already put on the device)
        self.last_vcf_path = "counted"
        last_nl = None  # (device text: read with the newline count, one host sync, not two)
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = bytes(text)
            last_nl = text.endswith(b"\n") if text else True
        text_t = self._as_text(text)
        nb = int(text_t.numel())
        tp = text_t if nb else None
        ws0 = self.empty(N.size("avdb_vcf_count_workspace_size", nb), torch.uint8)  # (with the parse windows' counts)
        nl = torch.zeros(2, dtype=torch.int64, device=self.device)  # newlines, last byte
        self._launch("avdb_vcf_count_lines", tp, nb, ws0, ws0.numel(), nl)
        if last_nl is None and nb:
            nl[1:2].copy_(text_t[-1:])
        got = nl.cpu()
        n_nl = int(got[0])
        if last_nl is None:
            last_nl = nb == 0 or int(got[1]) == 10
        n_lines = n_nl + (0 if (last_nl or nb == 0) else 1)
        ws = self.empty(N.size("avdb_vcf_workspace_size", nb, n_lines), torch.uint8)
        lines = self.empty(max(1, n_lines) * VCF_LINE_DTYPE.itemsize, torch.uint8) if want_lines else None
        rec_off = self.empty(n_lines + 1, torch.int64)
        heap_off = self.empty(n_lines + 1, torch.int64)
        self._launch("avdb_vcf_parse_lines2", tp, nb, n_lines, ws0, ws0.numel(), ws, ws.numel(), lines, rec_off,
                     heap_off, ctypes.byref(vcf_opts) if vcf_opts is not None else None)
        if n_lines:
            tot = torch.stack([rec_off[n_lines], heap_off[n_lines]]).cpu().tolist()
        else:
            tot = [0, 0]
        n_rec = int(tot[0])
        b, rec_line, rec_alt, outs = self._tokenizer_outputs(n_rec, int(tot[1]))
        if n_rec and want_lines:
            self._launch("avdb_vcf_emit", tp, nb, n_lines, lines, rec_off, heap_off, *outs)
        elif n_rec:
            self._launch("avdb_vcf_emit_ws", tp, nb, n_lines, ws, ws.numel(), rec_off, heap_off, *outs)
        return VcfBatch(text=text_t, n_lines=n_lines, lines=lines, rec_off=rec_off, heap_off=heap_off,
                        records=b, rec_line=rec_line, rec_alt=rec_alt)

    def _tokenizer_outputs(self, n_rec: int, n_heap: int):
        """What a tokenizer's emit pass fills: ``(records, rec_line, rec_alt,`` the nine
        output arguments of ``avdb_vcf_emit*`` ``)``."""
        b = RecordBatch(chrom=self.empty(n_rec, torch.uint8), pos=self.empty(n_rec, torch.int32),
                        allele_off=self.empty(n_rec, torch.int64),
                        ref_len=self.empty(n_rec, torch.int32), alt_len=self.empty(n_rec, torch.int32),
                        heap=self.empty(max(1, n_heap), torch.uint8),
                        ext_id=self.empty(n_rec, torch.int64))
        rec_line = self.empty(n_rec, torch.int32)
        rec_alt = self.empty(n_rec, torch.int32)
        return b, rec_line, rec_alt, (b.chrom, b.pos, b.allele_off, b.ref_len, b.alt_len, b.ext_id, b.heap,
                                      rec_line, rec_alt)

    def _vcf_tokenize_local(self, text, vcf_opts):
        """vcf_tokenize(want_lines=False) without the count pass: (batch, device
        text), the batch None when a parse window overflowed its line slots (the
        caller then takes the counted path on the same device text).  The slot
        workspace (about 2.7x the text: line, record and heap slots, avdb.h) is the
        engine's, reused across calls."""
        text_t = self._as_text(text)
        nb = int(text_t.numel())
        tp = text_t if nb else None
        ws = self.scratch("vcf_local", N.size("avdb_vcf_local_workspace_size", nb))
        tot = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._launch("avdb_vcf_parse_local", tp, nb, ws, ws.numel(),
                     ctypes.byref(vcf_opts) if vcf_opts is not None else None, tot)
        n_lines, n_rec, n_heap, overflow = (int(v) for v in tot.cpu().tolist())
        if overflow:
            return None, text_t
        b, rec_line, rec_alt, outs = self._tokenizer_outputs(n_rec, n_heap)
        rec_off = self.empty(n_lines + 1, torch.int64)
        heap_off = self.empty(n_lines + 1, torch.int64)
        if n_rec == 0:  # (no line has a record: every offset is 0)
            rec_off.zero_()
            heap_off.zero_()
        else:
            self._launch("avdb_vcf_emit_local", tp, nb, ws, ws.numel(), rec_off, heap_off, *outs)
        return VcfBatch(text=text_t, n_lines=n_lines, lines=None, rec_off=rec_off, heap_off=heap_off,
                        records=b, rec_line=rec_line, rec_alt=rec_alt), text_t

    # -- K9: this rank's lines of a VCF text -----------------------------------
    def vcf_select(self, vb: "VcfBatch", assignment, rank: int, cut: int = 64_000_000) -> torch.Tensor:
        """The lines of ``vb`` that piece plan ``assignment`` gives to ``rank``
        (each + '\\n', file order) as a device text tensor."""
        from .shard import piece_table
        base, count, prank = piece_table(assignment, self.lengths, cut)
        n = vb.n_lines
        ws = self.empty(max(1, N.size("avdb_shard_workspace_size", n)), torch.uint8)
        sel = self.empty(n + 1, torch.int64)
        self._launch("avdb_vcf_select_lines", n, vb.lines, base, count, prank, len(prank), int(cut), int(rank),
                     ws, ws.numel(), sel)
        total = int(sel[n].item())
        out = self.empty(max(1, total), torch.uint8)
        if total:
            self._launch("avdb_vcf_select_copy", vb.text, vb.text.numel(), n, vb.lines, sel, out)
        return out[:total]

    # -- K5: COPY rows / .mapping lines / display attributes --------------------
    def vcf_format(self, vb: "VcfBatch", end: torch.Tensor, code: torch.Tensor, status: torch.Tensor,
                   digest: Optional[torch.Tensor] = None, keep: Optional[torch.Tensor] = None,
                   alg_id="", max_seq_len: int = 50,
                   counters: Optional[torch.Tensor] = None, events: Optional[dict] = None,
                   existing: Optional[tuple] = None, adsp: bool = False,
                   adsp_dup: Optional[torch.Tensor] = None) -> "FormatResult":
        """The load driver's COPY buffer and .mapping text for ``vb``'s lines
        (K5b: size pass, scans, one host sync for the totals, write pass)."""
        n = vb.n_lines
        self._stream()  # (a host-only engine stops here, before any argument check)
        tp = vb.text if vb.text.numel() else None
        opts =N.FormatOpts(str(alg_id).encode(), int(max_seq_len), N.FORMAT_ADSP if adsp else 0)
        if adsp_dup is not None:  # ADSP: records whose primary key is already loaded
            opts.adsp_dup = N.ptr(adsp_dup)
        if existing is not None:  # (match, kind, frag, frag_off) device tensors from keyset_probe
            m, k, fr, fo = existing
            opts.match, opts.match_kind, opts.frag, opts.frag_off = N.ptr(m), N.ptr(k), N.ptr(fr), N.ptr(fo)
        if len(opts.alg_id) >= N.MAX_ALG_ID:
            raise ValueError("algorithm id too long")
        ws = self.empty(N.size("avdb_format_workspace_size", n), torch.uint8)
        copy_off = self.empty(n + 1, torch.int64)
        map_off = self.empty(n + 1, torch.int64)
        state = self.empty(max(1, n), torch.uint8)
        if end.numel() == 0:  # no records in this batch: the kernels never read them
            end = code = self.empty(1, torch.int32)
            status = self.empty(1, torch.uint8)
        args = (tp, vb.text.numel(), n, vb.lines, vb.rec_off, end, code, status, digest, keep, ctypes.byref(opts))
        ev = _Timer(events, self.device)
        ev.start("format_size")
        self._launch("avdb_vcf_format_size", *args, ws, ws.numel(), copy_off, map_off, state)
        ev.stop()
        tot = torch.stack([copy_off[n], map_off[n]]).cpu().tolist()
        copy = self.empty(max(8, int(tot[0])), torch.uint8)
        mapping = self.empty(max(8, int(tot[1])), torch.uint8)
        ctr = counters if counters is not None else self.new_counters()
        ev.start("format_write")
        self._launch("avdb_vcf_format_write", *args, copy_off, map_off, state, copy, mapping, ctr)
        ev.stop()
        return FormatResult(copy=copy[: int(tot[0])], mapping=mapping[: int(tot[1])], copy_off=copy_off,
                            map_off=map_off, line_state=state[:n], counters=ctr)

    def display_attributes(self, b: RecordBatch, end: torch.Tensor):
        """K5a: json.dumps(get_display_attributes()) per record.  Returns
        ``(text uint8, off int64[n+1], state uint8[n])`` device tensors."""
        b = self._batch(b)
        n = b.n
        ws = self.empty(N.size("avdb_format_workspace_size", n), torch.uint8)
        off = self.empty(n + 1, torch.int64)
        state = self.empty(max(1, n), torch.uint8)
        end = self._dev(end)
        args = (b.chrom, b.pos, end, b.allele_off, b.ref_len, b.alt_len, b.heap, b.heap.numel(), n, ws, ws.numel(), off)
        self._launch("avdb_display_attributes", *args, None, state)
        total = int(off[n].item())
        out = self.empty(max(8, total), torch.uint8)
        if n:
            self._launch("avdb_display_attributes", *args, out, state)
        return out[:total], off, state[:n]

    # -- K7: primary keys + bin paths as text ------------------------------------
    def primary_keys(self, b: RecordBatch, code: Optional[torch.Tensor] = None,
                     digest: Optional[torch.Tensor] = None, max_seq_len: int = 50, *,
                     out: Optional["KeyText"] = None, onepass: bool = True,
                     defer_digest: bool = False) -> "KeyText":
        """``generate_primary_key`` (and, with ``code``, the ltree bin path) for
        every record of ``b`` as text on the device.  Without ``out`` the size
        pass is followed by one host read of the totals; passing a ``KeyText``
        from an earlier call on a same-shaped batch reuses its buffers (no host
        sync: a text that would end past a buffer is not written and its record's
        state says so — ``KEY_OVERFLOW`` for the key, ``PATH_OVERFLOW`` ORed in
        for the path; ``KeyText.host`` raises on either).  ``defer_digest`` (no
        ``digest``): long records' keys are laid out with their 32 digest
        characters left for :meth:`fill_digests` (state ``KEY_DIGEST_PENDING``),
        so this launch need not wait for K4."""
        b = self._batch(b)
        n = b.n
        self._stream()  # (a host-only engine stops here, before any argument check)
        code = self._dev(code)
        digest = self._dev(digest)
        if defer_digest and (digest is not None or not onepass):
            raise ValueError("primary_keys: defer_digest takes no digest (one-pass form)")
        if onepass:
            return self._primary_keys_onepass(b, code, digest, max_seq_len, out, defer_digest)
        if out is None:
            out = KeyText(ws=self.empty(N.size("avdb_format_workspace_size", n), torch.uint8),
                          key_off=self.empty(n + 1, torch.int64),
                          path_off=self.empty(n + 1, torch.int64) if code is not None else None,
                          state=self.empty(max(1, n), torch.uint8), keys=None, paths=None)
        if out.off32:
            raise ValueError("primary_keys: narrow offsets need the one-pass form")
        if out.key_off.numel() < n + 1 or out.state.numel() < max(1, n) or \
                (code is not None and (out.path_off is None or out.path_off.numel() < n + 1)):
            raise ValueError("primary_keys: the reused KeyText holds fewer records (or no paths)")
        args = (*b.soa(), b.ext_id, code, digest, n, int(max_seq_len), out.ws, out.ws.numel(), out.key_off,
                out.path_off)
        self._launch("avdb_primary_keys", *args, None, 0, None, 0, None)
        if out.keys is None:
            tot = torch.stack([out.key_off[n], out.path_off[n] if code is not None else out.key_off[n]]).cpu().tolist()
            out.keys = self.empty(max(8, int(tot[0])), torch.uint8)
            out.paths = self.empty(max(8, int(tot[1])), torch.uint8) if code is not None else None
        if n:
            self._launch("avdb_primary_keys", *args, out.keys, out.keys.numel(), out.paths,
                         out.paths.numel() if out.paths is not None else 0, out.state)
        return out

    def new_key_text(self, n: int, heap_bytes: int, paths: bool = True, off32: bool = False) -> "KeyText":
        """Buffers for one-pass K7 output over ``n`` records with ``heap_bytes`` of
        alleles (texts sized by ``avdb_primary_keys_bound``): what a keyed K2 writes
        its group totals into before the first ``primary_keys(..., out=...)``.
        ``off32``: the offsets in the narrow layout (AVDB_KEYS_OFF32, for exactly
        ``n`` records)."""
        ws_bytes = N.size("avdb_primary_keys_onepass_workspace_size", n)
        kc, pc = ctypes.c_size_t(), ctypes.c_size_t()
        N.call("avdb_primary_keys_bound", n, heap_bytes, ctypes.byref(kc), ctypes.byref(pc))
        if off32:
            ob = N.size("avdb_keys_off32_bytes", n)
            mk = lambda: self.empty(ob, torch.uint8)  # noqa: E731
        else:
            mk = lambda: self.empty(n + 1, torch.int64)  # noqa: E731
        return KeyText(ws=self.empty(ws_bytes, torch.uint8), key_off=mk(), path_off=mk() if paths else None,
                       state=self.empty(max(16, n), torch.uint8), keys=self.empty(int(kc.value), torch.uint8),
                       paths=self.empty(int(pc.value), torch.uint8) if paths else None, off32=off32)

    def fill_digests(self, b: RecordBatch, digest: torch.Tensor, kt: "KeyText"):
        """``avdb_primary_keys_fill_digests``: the digest characters of every key a
        ``primary_keys(..., defer_digest=True)`` left pending (``digest`` = this
        batch's ``vrs_digest`` output)."""
        b = b if b.device == self.device else b.to(self.device)
        if kt.off32:
            raise ValueError("fill_digests: narrow key offsets are not accepted")
        self._launch("avdb_primary_keys_fill_digests", b.chrom, b.pos, b.n, digest, kt.key_off, kt.keys, kt.state)
        return kt

    def _primary_keys_onepass(self, b: RecordBatch, code, digest, max_seq_len: int, out,
                              defer: bool = False) -> "KeyText":
        """K7 without a host round trip (``avdb_primary_keys_onepass``): per-group
        size totals, two small scans, then the write pass that recomputes each
        record's sizes, writes its offsets and the text; the text buffers are sized
        by ``avdb_primary_keys_bound``, so no host sync is needed even the first time."""
        n = b.n
        ws_bytes = N.size("avdb_primary_keys_onepass_workspace_size", n)
        if out is None:
            out = self.new_key_text(n, b.heap.numel(), paths=code is not None)
        if out.key_off.numel() < n + 1 or out.state.numel() < max(1, n) or \
                (code is not None and (out.path_off is None or out.path_off.numel() < n + 1 or out.paths is None)):
            raise ValueError("primary_keys: the reused KeyText holds fewer records (or no paths)")
        if out.off32:
            ob = N.size("avdb_keys_off32_bytes", n)
            if out.key_off.numel() < ob or (code is not None and out.path_off.numel() < ob):
                raise ValueError("primary_keys: the narrow offset buffers were made for fewer records")
        out.ws = self.workspace(ws_bytes, out.ws)
        # the keyed K2 wrote this batch's group totals into this KeyText's workspace
        # (sizes from these length / id arrays and, for the paths, these bin codes)
        tot = self._pending.pop("totals", None)
        ready = (tot is not None and tot[1] is out and tot[2:] == (n, int(max_seq_len), digest is not None or defer)
                 and _stamp_ok(tot[0], out.ws, b.chrom, b.pos, b.ref_len, b.alt_len, b.ext_id, code))
        flags = (N.KEYS_TOTALS_READY if ready else 0) | (N.KEYS_DIGEST_DEFERRED if defer else 0) | \
            (N.KEYS_OFF32 if out.off32 else 0)
        self._launch("avdb_primary_keys_onepass_ex", *b.soa(), b.ext_id, code, digest, n, int(max_seq_len), out.ws,
                     out.ws.numel(), out.key_off, out.path_off, out.keys, out.keys.numel(), out.paths,
                     out.paths.numel() if out.paths is not None else 0, out.state, flags)
        return out

    # -- K6: existing-variant key set ----------------------------------------
    def keyset_build(self, keys: torch.Tensor, key_off: torch.Tensor) -> torch.Tensor:
        """Hash table over the key strings (``keys`` bytes, ``key_off`` int64[n+1])."""
        keys, key_off = self._dev(keys), self._dev(key_off)
        n = key_off.numel() - 1
        table = self.empty(N.size("avdb_keyset_workspace_size", n), torch.uint8)
        self._launch("avdb_keyset_build", keys if keys.numel() else None, key_off, n, table, table.numel())
        return table

    def keyset_table(self, keys: torch.Tensor, key_off: torch.Tensor) -> torch.Tensor:
        """:meth:`keyset_build` where the engine lives: on a host-only engine the library's
        ``avdb_keyset_build_host`` builds the table (it answers every probe as the device's
        does, though not necessarily slot for slot)."""
        if not self.host_only:
            return self.keyset_build(keys, key_off)
        keys, key_off = self._dev(keys), self._dev(key_off)
        n = key_off.numel() - 1
        table = self.empty(N.size("avdb_keyset_workspace_size", n), torch.uint8)
        self._call("avdb_keyset_build_host", keys if keys.numel() else None, key_off, n, table, table.numel())
        return table

    def keyset_probe(self, table: torch.Tensor, keys: torch.Tensor, key_off: torch.Tensor, b: RecordBatch,
                     check_alt: bool = True, counters: Optional[torch.Tensor] = None):
        """``(match int32[n], kind uint8[n])``: first equal key of each record's
        metaseq id (then of the switched alleles with ``check_alt``)."""
        b = self._batch(b)
        n = b.n
        match = self.empty(max(1, n), torch.int32)
        kind = self.empty(max(1, n), torch.uint8)
        self._launch("avdb_keyset_probe", table, table.numel(), keys if keys.numel() else None, key_off,
                     key_off.numel() - 1, *b.soa(), n, 1 if check_alt else 0, match, kind, counters)
        return match[:n], kind[:n]

    def keyset_probe_text(self, table: torch.Tensor, keys: torch.Tensor, key_off: torch.Tensor,
                          q: torch.Tensor, q_off: torch.Tensor, n: int, skip: Optional[torch.Tensor] = None,
                          counters: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``match int32[n]``: first key equal to ``q[q_off[i]:q_off[i+1]]``, or -1."""
        match = self.empty(max(1, n), torch.int32)
        self._launch("avdb_keyset_probe_text", table, table.numel(), keys if keys.numel() else None, key_off,
                     key_off.numel() - 1, q if q.numel() else None, q_off, skip, n, match, counters)
        return match[:n]

    # -- text slabs (K10, K12) ---------------------------------------------------
    def _as_text(self, text) -> torch.Tensor:
        """Text (bytes-like, numpy ``uint8`` or a ``uint8`` tensor) as a dense tensor on
        the engine's device; no bytes give an empty tensor (NULL at a call)."""
        if isinstance(text, (bytes, bytearray, memoryview)):
            text = torch.from_numpy(np.frombuffer(bytes(text), dtype=np.uint8).copy()) if len(text) else \
                torch.zeros(0, dtype=torch.uint8)
        elif isinstance(text, np.ndarray):
            text = np.ascontiguousarray(text, dtype=np.uint8)
            text = torch.from_numpy(text if text.flags.writeable else text.copy())
        return self._dev(text)

    @staticmethod
    def _spans(start: torch.Tensor, length: torch.Tensor) -> torch.Tensor:
        """Flat indices of the spans ``[start[i], start[i] + length[i])``, concatenated."""
        first = torch.cumsum(length, 0) - length
        return torch.repeat_interleave(start - first, length) + torch.arange(int(length.sum()), device=start.device)

    def _count_lines(self, text: torch.Tensor) -> int:
        """Lines of a '\\n'-separated slab: newlines + (the text does not end in one)."""
        nb = text.numel()
        if nb == 0:
            return 0
        if self.host_only:
            return int((text == 10).sum()) + int(text[-1] != 10)
        ws = self.scratch("text_count", N.VCF_COUNT_WORKSPACE_BYTES)
        cnt = self.empty(1, torch.int64)
        self._launch("avdb_vcf_count_lines", text, nb, ws, ws.numel(), cnt)
        return int(cnt.item()) + int(text[-1].item() != 10)

    # -- K12: the key set's columns from an export --------------------------------
    def existing_table_build(self, text, contigs=None) -> "ExistingColumns":
        """K12: a slab of an export of ``AnnotatedVDB.Variant``
        (``metaseq_id<TAB>record_primary_key<TAB>bin_index[<TAB>...]`` lines; bytes,
        numpy ``uint8`` or a ``uint8`` tensor) -> :class:`ExistingColumns` on this
        engine's device, row for row what ``ExistingVariants.from_tsv`` builds.
        ``contigs``: labels whose rows to keep (``None``: all).  Three syncs: the line
        count, the size pass's counts (the blobs are allocated from them), the end.
        Rows whose fragment ``repr`` does not render verbatim (``frag_host``) have
        their two fields fetched and rendered here, and copied into their spans after
        the write pass.  On a host-only engine the library's host entries run the same
        per-line code."""
        return slab_passes.existing_table_build(self, text, contigs)

    # -- K13: CADD update rows from an export -------------------------------------
    def cadd_update_rows(self, text, snv, indel, chromosome=None, skip_existing: bool = True,
                         contigs=None) -> "CaddUpdateRows":
        """K13: a slab of an export in the reference's ``SELECT_SQL`` column order
        (``record_primary_key<TAB>metaseq_id<TAB>cadd_scores[<TAB>...]`` lines; bytes,
        numpy ``uint8`` or a ``uint8`` tensor) joined against the two CADD tables
        (:class:`~annotatedvdb_amd.cadd.CaddTable` or :class:`CaddColumns`, either may be
        ``None``) -> :class:`CaddUpdateRows` on this engine's device: the text of the
        tuples ``CADDUpdater.buffer_variants`` would append for the same records, in
        file order.  ``chromosome``: what ``set_chromosome`` takes (``None``: each row's
        ``chr`` + the label of its primary key); ``skip_existing``: records whose
        ``cadd_scores`` is not NULL (``\\N``, empty or absent) are counted ``skipped``;
        ``contigs``: labels of the metaseq ids whose rows to keep (``None``: all), as
        for :meth:`existing_table_build`.  Three syncs: the line count, the size pass's
        counts (the output is allocated from them), the end.  Rows the device leaves to
        the host (``host_rows``: a contig without a code, a position that is not plain
        digits, a table score the device does not parse) are rendered here with
        ``buffer_variants`` itself and copied into their spans after the write pass.
        On a host-only engine the library's host entries run the same per-line code."""
        return slab_passes.cadd_update_rows(self, text, snv, indel, chromosome, skip_existing, contigs)

    # -- K16: SnpEff LOF/NMD update rows ---------------------------------------------
    def lof_table_build(self, text) -> "LofTable":
        """K16a: a '\\n'-separated slab of the VCF SnpEff wrote (bytes, numpy ``uint8`` or a
        ``uint8`` tensor) -> :class:`LofTable` on this engine's device.  A line is read as
        ``load_annotation`` (``load_snpeff_lof.py:250-288``) reads it: ``rstrip()``ped; ``#``
        lines are comments; a line without ``;LOF=`` and ``;NMD=`` anywhere in it is
        unannotated; INFO is then looked up by key (the last item of a key wins) and a line
        with neither value counts ``no_values``.  Every other line gives one row per ALT
        allele, keyed ``chrom:pos:ref:alt`` (CHROM without ``chr``, ``MT`` as ``M``,
        ``str(int(POS))``), and one JSON text.  Of an id the VCF repeats the last record
        answers a probe (the reference keeps the last within one ``--numLookups`` batch).
        Lines outside the device subset (``host_lines``: DESIGN.md, K16) are rendered by
        :func:`annotatedvdb_amd.snpeff_lof.annotated_line` and copied into their spans after
        the write pass; an exception it raises is re-raised with the line number attached
        (``err.line``, 1-based, and a note).  A carriage return inside a line raises
        ``ValueError``.  Three syncs: the line count, the size pass's counts, the end.  On a
        host-only engine the library's host entries run the same per-line code."""
        return slab_passes.lof_table_build(self, text)

    def lof_update_rows(self, text, table: "LofTable", update_existing: bool = False,
                        contigs=None) -> "LofUpdateRows":
        """K16b: a slab of an export
        ``record_primary_key<TAB>metaseq_id<TAB>loss_of_function[<TAB>...]`` (K13's
        conventions: header line, ``\\r\\n``, fewer than two fields counted ``skipped_lines``,
        ``contigs``, a metaseq id without four parts raises) streamed against a
        :class:`LofTable` -> :class:`LofUpdateRows`: for every export row whose metaseq id
        is annotated the tuple ``__buffer_update_values`` appends
        (``vcf_variant_loader.py:197-217``) as ``pk<TAB>chr<label><TAB>json<LF>``, in export
        order; two primary keys of one variant both get a row (the reference's
        ``firstHitOnly=False`` lookup).  An id the table does not hold is counted
        ``not_annotated``; an annotated record whose third column is not NULL (``\\N``,
        empty or absent) is counted ``skipped`` and gets no row unless ``update_existing``
        (where the reference itself raises).  ``table.hit`` records the table
        rows matched, skipped records included.  Rows come out in export order.  Three syncs:
        the line count, the size pass's counts, the end.  On a host-only engine the library's
        host entries run the same per-line code."""
        return slab_passes.lof_update_rows(self, text, table, update_existing, contigs)

    # -- K18a: VEP consequences, ranked and sorted ---------------------------------------
    def vep_consequences(self, text, ranking) -> "VepConsequences":
        """K18a: a '\\n'-separated slab of VEP ``--json`` output (bytes, numpy ``uint8``, a ``uint8``
        tensor, or a path: plain, gzip or bgzip through :func:`annotatedvdb_amd.bgzf.read_whole`)
        and a ranking (:class:`~annotatedvdb_amd.vep_consequences.ConsequenceRanking`, or what it
        takes) -> :class:`~annotatedvdb_amd.vep_consequences.VepConsequences` on this engine's
        device: for every element of a line's four ``<type>_consequences`` arrays what
        ``VepJsonParser.adsp_rank_and_sort_consequences`` adds to it (``vep_parser.py:145-175``),
        and the order the elements end up in per type and allele.  Lines outside the device subset
        (``counts['host_lines']``, by reason in ``counts``: DESIGN.md, K18a) get blank rows, and
        :meth:`VepConsequences.ranked` answers them through
        :func:`~annotatedvdb_amd.vep_consequences.vep_line`.  Three syncs: the line count, the size
        pass's counts, the end.  On a host-only engine the library's host entries run the same
        per-block code."""
        return slab_passes.vep_consequences(self, text, ranking)

    # -- K18b: VEP consequence update rows ------------------------------------------------
    def vep_rows_table_build(self, text, ranking, vep_output: bool = False, identity_only: bool = False,
                             allele_frequencies: bool = False, match_refsnp: bool = False) -> "VepRowsTable":
        """K18b: VEP ``--json`` output (what :meth:`vep_consequences` takes) and a ranking ->
        :class:`VepRowsTable` on this engine's device: K18a's pass, then one row per ALT allele of the
        VCF line in every line's ``input``, keyed by its metaseq id ``chrom:pos:ref:alt``, its body what
        ``VEPVariantLoader.__parse_alt_alleles`` (``vep_variant_loader.py:153-213``) puts into
        ``adsp_most_severe_consequence`` and ``adsp_ranked_consequences`` for the normalised allele.
        Of an id two lines carry the last answers a probe.  Lines outside the device subset
        (``counts['host_lines']``, by reason in ``counts``: DESIGN.md, K18b) are rendered by
        :func:`annotatedvdb_amd.vep_rows.vep_rows_line` and copied into their spans after the write
        pass; an exception it raises is re-raised with the line number attached, except
        :class:`~annotatedvdb_amd.vep_consequences.UnrankedCombination`: such a line gives no rows
        and is listed in ``unranked``.  On a host-only engine the library's host entries run the
        same per-block code.

        ``vep_output=True`` (K18c) adds the cleaned result of every line, stored once per line:
        ``xstr(cleanResult)`` of ``__clean_result`` (``vep_variant_loader.py:112-123``), the line's
        object without ``colocated_variants`` and the four ``<type>_consequences`` members and with
        ``VcfEntryParser(input, identityOnly=identity_only).get_entry()`` in place of ``input``.  A
        line outside that pass's device subset (``cleaned_counts``) is rendered by
        :func:`annotatedvdb_amd.vep_rows.vep_output_line`.  With ``vep_output=False`` the table is
        K18b's, byte for byte.

        ``allele_frequencies=True`` (K18d) adds every row's ``allele_frequencies`` text:
        ``xstr(alleleFreq, nullStr='{}')`` of ``__parse_alt_alleles`` (``vep_variant_loader.py:85-109,
        126-142, 190-199``): the frequencies of the normalised ALT in the element of
        ``colocated_variants`` that ``VepJsonParser.get_frequencies`` takes (matched by ``ref_snp_id``
        with ``match_refsnp``, the reference's dbSNP datasource), regrouped by source, with the ALT's
        column of INFO ``FREQ`` merged in (not with ``identity_only``).  A line outside that pass's
        device subset (``freq_counts``) is rendered by
        :func:`annotatedvdb_amd.vep_rows.allele_frequencies_line`.  Without it the table is what it
        was, byte for byte."""
        return slab_passes.vep_rows_table_build(self, text, ranking, vep_output, identity_only, allele_frequencies,
                                                match_refsnp)

    def vep_update_rows(self, text, table: "VepRowsTable", alg_id: int, adsp: bool = False,
                        update_existing: bool = False, contigs=None) -> "LofUpdateRows":
        """K18b: a slab of an export ``record_primary_key<TAB>metaseq_id<TAB>vep_output[<TAB>...]``
        (:meth:`lof_update_rows`' conventions) streamed against a :class:`VepRowsTable` ->
        :class:`LofUpdateRows` whose rows are ``pk<TAB>chr<label><TAB>most severe<TAB>ranked<TAB>alg_id
        [<TAB>true]<LF>`` (``true`` with ``adsp``), in export order.  A record whose ``vep_output`` is
        not NULL is counted ``skipped`` and gets no row unless ``update_existing``
        (``has_attribute('vep_output', ...)`` with ``skip_existing``); an id the table lacks is
        counted ``not_annotated``; ``table.hit`` records the table rows matched.  A table built with
        ``vep_output=True`` (K18c) gives ``...<TAB>ranked<TAB>vep_output<TAB>alg_id...`` rows, written
        one wave per row; one built with ``allele_frequencies=True`` (K18d) gives
        ``pk<TAB>chr<label><TAB>allele_frequencies<TAB>most severe<TAB>ranked[<TAB>vep_output]<TAB>alg_id...``
        rows, ``updateValues``' order, written the same way."""
        return slab_passes.vep_update_rows(self, text, table, alg_id, adsp, update_existing, contigs)

    # -- K17: ADSP QC pVCF update rows --------------------------------------------------
    def qc_table_build(self, text, version: str, header_fields=None) -> "QcTable":
        """K17a: a '\\n'-separated slab of an ADSP QC pVCF (bytes, numpy ``uint8`` or a ``uint8``
        tensor) -> :class:`QcTable` on this engine's device.  A line is read as
        ``load_annotation`` (``update_from_qc_pvcf_file.py:226-258``) reads it: ``rstrip()``ped;
        ``#`` lines are comments; every other line gives one row per ALT allele, keyed
        ``chrom:pos:ref:alt`` as in :meth:`lof_table_build`, one JSON text
        ``{release: {"info": {...}, "filter": ..., "qual": ..., "format": ...}}`` as
        ``generate_update_values`` (``:117-149``) builds it, ``release`` being
        ``version.lower()``, and whether FILTER is ``PASS``.  Of an id the VCF repeats the last
        record answers a probe.  Lines outside the device subset (``host_lines``: DESIGN.md, K17)
        are rendered by :func:`annotatedvdb_amd.adsp_qc.qc_line` and copied into their spans
        after the write pass; an exception it raises is re-raised with the line number attached
        (``err.line``, 1-based, and a note).  ``header_fields`` other than the reference's
        default nine leave every line to the host.  A release that is not 1 to 64 printable
        ASCII bytes without ``"`` and ``\\`` raises ``ValueError``, as does a carriage return
        inside a line.  Three syncs, as :meth:`lof_table_build`; on a host-only engine the
        library's host entries run the same per-line code."""
        return slab_passes.qc_table_build(self, text, version, header_fields)

    def qc_update_rows(self, text, table: "QcTable", update_existing: bool = False, contigs=None) -> "QcUpdateRows":
        """K17b: a slab of an export ``record_primary_key<TAB>metaseq_id<TAB>adsp_qc[<TAB>...]``
        (K13's conventions, as :meth:`lof_update_rows`) streamed against a :class:`QcTable` ->
        :class:`QcUpdateRows`: for every export row whose metaseq id the QC file holds the tuple
        ``__buffer_update_values`` appends as ``pk<TAB>chr<label><TAB>true|\\N<TAB>json<LF>``, in
        export order.  An id the table does not hold is counted ``not_in_vcf``; a record that
        has QC values of this release already — its third column is not NULL and a key at depth
        1 of its JSON object equals the release — is counted ``skipped`` and gets no row unless
        ``update_existing``.  A column with a backslash in it, or that does not begin with
        ``{``, is settled here with ``json.loads`` (``host_rows``); one that is not JSON raises
        ``ValueError`` naming the export line.  ``table.hit`` records the table rows matched."""
        return slab_passes.qc_update_rows(self, text, table, update_existing, contigs)

    # -- K19: annotation update rows from a tab-delimited file --------------------------
    def txt_table_build(self, text, variant_id_type: str = "METASEQ") -> "TxtTable":
        """K19a: a '\\n'-separated slab of a tab-delimited file with a header (bytes, numpy
        ``uint8`` or a ``uint8`` tensor) -> :class:`TxtTable` on this engine's device.  The header
        is read on the host by ``csv`` from the slab's first bytes (one small copy); it must name a
        column ``variant`` and at least one, at most ``N.TXT_MAX_FIELDS - 1`` others, and for
        ``variant_id_type='REFSNP'`` a column ``ref_snp_id``, which is then the looked-up one
        (``set_current_variant``, ``txt_variant_loader.py:177-178``), else ``ValueError``.  A data
        line gives one row: its looked-up id as key and its update values, every header column but
        ``variant`` in header order, rendered once (``NULL`` and the fields a short row lacks as
        ``\\N``, fields beyond the header dropped, empty lines skipped).  Of an id the file
        repeats the last line answers a probe.  Lines outside the device subset (``host_lines``: a
        field that starts with ``"``, a byte above 0x7F, a field that is exactly ``\\N``) are
        rendered by :func:`annotatedvdb_amd.text_update.host_line` and copied into their spans
        after the write pass; an exception it raises carries the line number (``err.line``).  A
        carriage return inside a line raises ``ValueError``.  Three syncs and the header's copy;
        on a host-only engine the library's host entries run the same per-line code."""
        return slab_passes.txt_table_build(self, text, variant_id_type)

    def txt_update_rows(self, text, table: "TxtTable", id_type: str = "METASEQ", adsp: bool = False,
                        contigs=None) -> "TxtUpdateRows":
        """K19b: a slab of an export ``record_primary_key<TAB>metaseq_id<TAB>ref_snp_id[<TAB>...]``
        (K13's conventions, as :meth:`lof_update_rows`; the third column ``\\N``, empty or absent
        for none) streamed against a :class:`TxtTable` -> :class:`TxtUpdateRows`: for every export
        row whose id (``id_type``: ``METASEQ`` the second column, ``REFSNP`` the third) the file
        holds, the tuple ``__buffer_update_values`` appends (``txt_variant_loader.py:190-208``) as
        ``pk<TAB>chr<label><TAB>values[<TAB>true]<LF>`` (``true`` with ``adsp``), in export order;
        several primary keys of one id all get a row.  An id the table does not hold is counted
        ``not_in_file``.  ``table.hit`` records the table rows matched."""
        return slab_passes.txt_update_rows(self, text, table, id_type, adsp, contigs)

    def txt_direct_rows(self, text, adsp: bool = False) -> "TxtUpdateRows":
        """K19c: a slab of a tab-delimited file whose ``variant`` column holds primary keys ->
        :class:`TxtUpdateRows`, one row per data line in file order (the reference asks the
        database nothing for such a file).  The header, the update values and the host lines are
        :meth:`txt_table_build`'s; a host line's row is rendered by
        :func:`annotatedvdb_amd.text_update.host_line` and copied into its span."""
        return slab_passes.txt_direct_rows(self, text, adsp)

    # -- K14: the VCF files of an export ------------------------------------------
    def export_vcf(self, text, contigs=None, variants_per_file: int = 10_000_000) -> "ExportVcf":
        """K14: a slab of an export in the column order of ``export_variant2vcf.py``'s
        ``SELECT_SQL`` (``record_primary_key<TAB>metaseq_id<TAB>row_algorithm_id[<TAB>...]``
        lines; bytes, numpy ``uint8`` or a ``uint8`` tensor) -> :class:`ExportVcf` on this
        engine's device: the rows of the VCF files the reference's ``run`` writes for the
        same records, ``variants_per_file`` valid records to a file, and the rows of its
        invalid file.  ``contigs``: labels of the metaseq ids whose rows to keep
        (``None``: all), as for :meth:`existing_table_build`.  Three syncs: the line
        count, the size pass's counts (the outputs are allocated from them), the end.
        The reference keeps a file's rows in a dict keyed by primary key: rows of one
        file whose keys hash alike (found by sorting ``(file, pk_hash)``) have their key
        bytes fetched and compared here, and of true repeats the first is rendered here
        with the last one's metaseq id and the others are dropped; the VCF write pass
        then runs again.  Without such rows no row text comes to the host.  On a
        host-only engine the library's host entries run the same per-line code."""
        return slab_passes.export_vcf(self, text, contigs, variants_per_file)

    # -- K15: a whole-genome VCF split by chromosome ------------------------------
    def split_chrom_map(self, mapping: Dict) -> "ChromMap":
        """A ChromosomeMap's dict as the library map of K15's rule (:meth:`ChromMap.for_split`),
        cached per dict."""
        cache = self.__dict__.setdefault("_split_maps", {})
        cm = cache.get(id(mapping))
        if cm is None or cm.mapping is not mapping:
            cm = cache[id(mapping)] = ChromMap.for_split(self, mapping)
        return cm

    def split_vcf(self, text, chrom_map=None, unknown: str = "raise") -> "SplitVcf":
        """K15: a '\\n'-separated slab of a VCF (bytes, numpy ``uint8`` or a ``uint8``
        tensor) -> :class:`SplitVcf` on this engine's device: the lines
        ``split_vcf_by_chr.py``'s ``run`` prints to ``chr1.vcf`` ... ``chrM.vcf`` for the
        same text, per file and in file order.  ``chrom_map``: a :class:`ChromMap` made by
        :meth:`ChromMap.for_split` (or the ChromosomeMap's dict) when CHROM holds source
        ids, ``None`` when it holds the labels.  A line no file takes raises the
        reference's ``KeyError`` (``unknown="raise"``; the error's ``line`` is the line's
        1-based number in the slab) or goes to stream 25 (``unknown="keep"``).  Three
        syncs: the line count, the size pass's counts (the blob is allocated from them),
        the end.  Lines whose stripped end Python may see differently (a last byte of
        0x1C..0x1F or >= 0x80) are fetched and decided here by
        ``line.decode("utf-8").rstrip()``, whose ``UnicodeDecodeError`` propagates when no
        unplaced line comes before it; invalid UTF-8 elsewhere in a line is copied
        verbatim.  On a host-only engine the library's host entries run the same
        per-line code."""
        return slab_passes.split_vcf(self, text, chrom_map, unknown)

    # -- K10: CADD table and allele join ---------------------------------------
    def new_cadd_counters(self) -> torch.Tensor:
        """``{snv, indel, not_matched}`` (``N.CADD_CTR_*``), added to by :meth:`cadd_match`."""
        return torch.zeros(N.CADD_N_CTRS, dtype=torch.int64, device=self.device)

    def cadd_table_build(self, text) -> "CaddColumns":
        """K10a: a slab of uncompressed CADD TSV (bytes, numpy ``uint8`` or a ``uint8``
        tensor) -> the table's columns on this engine's device.  One sync (the line
        count) before the build, one after (the counts).  On a host-only engine the
        library's host entry runs the same per-line code."""
        return slab_passes.cadd_table_build(self, text)

    def cadd_match(self, snv: Optional["CaddColumns"], indel: Optional["CaddColumns"], b: RecordBatch,
                   counters: Optional[torch.Tensor] = None, out=None):
        """K10b: ``(row int32[n], kind uint8[n], raw float64[n], phred float64[n])`` of
        each record against the SNV or the indel table (either may be ``None``).
        ``raw`` / ``phred`` are written for matched records only (NaN elsewhere in
        buffers this call allocates; ``out``: the caller's four buffers, of which
        only the first ``n`` entries are touched).  ``counters``: see
        :meth:`new_cadd_counters`."""
        b = self._batch(b)
        n = b.n
        for t in (snv, indel):
            if t is not None and t.text.device != self.device:
                raise ValueError("CADD table lives on another device than this engine")
        if out is None:
            row, kind = self.empty(max(1, n), torch.int32), self.empty(max(1, n), torch.uint8)
            raw, phred = self.empty(max(1, n), torch.float64), self.empty(max(1, n), torch.float64)
            if self.poison is None:
                raw.fill_(float("nan"))
                phred.fill_(float("nan"))
        else:
            row, kind, raw, phred = out
            if min(t.numel() for t in out) < n or any(t.device != self.device for t in out):
                raise ValueError("out buffers must hold n entries on the engine's device")
        vs = snv.view() if snv is not None else None
        vi = indel.view() if indel is not None else None
        args = (ctypes.byref(vs) if vs is not None else None, ctypes.byref(vi) if vi is not None else None,
                *b.soa(), n, row, kind, raw, phred, counters)
        if self.host_only:
            self._call("avdb_cadd_match_host", *args)
        else:
            self._launch("avdb_cadd_match", *args)
        return row[:n], kind[:n], raw[:n], phred[:n]

    # -- K11: BGZF input ---------------------------------------------------------
    @staticmethod
    def _host_u8(data) -> np.ndarray:
        """``data`` (bytes-like, numpy ``uint8`` or a ``uint8`` tensor) as a contiguous host array, without a copy
        where it already is one."""
        if isinstance(data, torch.Tensor):
            if data.dtype != torch.uint8 or data.dim() != 1:
                raise TypeError("compressed data must be a 1-d uint8 tensor")
            return data.detach().cpu().contiguous().numpy()
        if isinstance(data, np.ndarray):
            if data.dtype != np.uint8 or data.ndim != 1:
                raise TypeError("compressed data must be a 1-d uint8 array")
            return np.ascontiguousarray(data)
        return np.frombuffer(data, dtype=np.uint8)

    def bgzf_index(self, data) -> "BgzfIndex":
        """``avdb_bgzf_index_host`` over the complete BGZF members at the head of
        ``data`` (host memory): see :class:`annotatedvdb_amd.bgzf.BgzfIndex`.  Raises
        ``bgzf.NotBgzf`` when the first member is gzip but not BGZF, ``bgzf.BgzfError``
        for a malformed member later in the chain."""
        from .bgzf import BgzfError, BgzfIndex, NotBgzf
        a = self._host_u8(data)
        nb = a.size
        ins, outs, at, total = [], [], 0, 0
        cap = max(16, min(nb // 26 + 1, 1 << 20))
        n, consumed, out_bytes = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_uint64()
        while True:
            in_off, out_off = np.empty(cap, dtype=np.uint64), np.empty(cap + 1, dtype=np.uint64)
            rc = N.call("avdb_bgzf_index_host", a.ctypes.data + at if nb else None, nb - at, cap, in_off, out_off,
                        ctypes.byref(n), ctypes.byref(consumed), ctypes.byref(out_bytes), check=False)
            if rc == N.AVDB_ENOTBGZF and at == 0:
                raise NotBgzf(N.last_error())
            if rc < 0:
                raise BgzfError("%s (the chain examined starts at offset %d)" % (N.last_error(), at))
            k = int(n.value)
            ins.append(in_off[:k] + np.uint64(at))
            outs.append(out_off[:k] + np.uint64(total))
            at += int(consumed.value)
            total += int(out_bytes.value)
            if k < cap:
                break
        outs.append(np.array([total], dtype=np.uint64))
        return BgzfIndex(np.concatenate(ins), np.concatenate(outs), at, total)

    def bgzf_inflate(self, data, index: Optional["BgzfIndex"] = None, raise_on_error: bool = True):
        """K11: the text of the BGZF members of ``data`` (bytes-like, numpy ``uint8`` or a
        ``uint8`` tensor; with ``index`` it may already be on the device) as a ``uint8``
        tensor on this engine's device: compressed bytes go up, the text stays in HBM.
        Without ``index`` every byte of ``data`` must belong to a complete member.  A
        member that fails (``N.BGZF_*``) raises ``bgzf.BgzfError``; with
        ``raise_on_error=False`` the call returns ``(text, status uint8[n_blocks],
        counts)`` instead, the ranges of failed members left as allocated.  On a
        host-only engine the library's host entry runs the same per-member code."""
        from .bgzf import BgzfError
        if index is None:
            host = self._host_u8(data)
            index = self.bgzf_index(host)
            if index.consumed != host.size:
                raise BgzfError("truncated BGZF data: %d bytes after the last complete member (offset %d)"
                                % (host.size - index.consumed, index.consumed))
            data = host
        if isinstance(data, torch.Tensor):
            comp = data
        else:
            a = self._host_u8(data)
            if not a.flags.writeable:  # (bytes: torch warns about a view nobody writes through)
                a = a.copy()
            comp = torch.from_numpy(a)
        if comp.dtype != torch.uint8 or comp.dim() != 1:
            raise TypeError("compressed data must be a 1-d uint8 tensor")
        comp = comp.to(self.device, non_blocking=True) if comp.device != self.device else comp
        if not comp.is_contiguous():
            comp = comp.contiguous()
        n, nb, total = index.n_blocks, comp.numel(), index.out_bytes
        in_off, out_off = np.ascontiguousarray(index.in_off, dtype=np.uint64), \
            np.ascontiguousarray(index.out_off, dtype=np.uint64)
        # sizes are checked here, before the call (the decoder checks them again per member)
        if in_off.size != n or out_off.size != n + 1:
            raise ValueError("index arrays must hold n_blocks and n_blocks + 1 entries")
        if n:
            sizes = np.diff(out_off.astype(np.int64))
            if int(out_off[0]) != 0 or int(out_off[-1]) != total or (sizes < 0).any() or (sizes > N.BGZF_MAX_OUT).any():
                raise ValueError("index out_off is not the exclusive sum of member sizes of at most 65536")
            if (np.diff(in_off.astype(np.int64)) < 26).any() or int(in_off[-1]) + 26 > nb:
                raise ValueError("index in_off does not lie inside the compressed data")
        out = self.empty(max(1, total), torch.uint8)
        status = self.empty(max(1, n), torch.uint8)
        counts = self.empty(N.BGZF_N_COUNTS, torch.int64)
        d_in = torch.from_numpy(in_off.view(np.int64)).to(self.device, non_blocking=True)
        d_out = torch.from_numpy(out_off.view(np.int64)).to(self.device, non_blocking=True)
        args = (comp if nb else None, nb, d_in if n else None, d_out, n, out, total, status, counts)
        if self.host_only:
            self._call("avdb_bgzf_inflate_host", *args)
        else:
            self._launch("avdb_bgzf_inflate", *args)
        cnt = counts.cpu().numpy().astype(np.uint64)  # (the sync: comp, d_in and d_out are done with)
        if not raise_on_error:
            return out[:total], status[:n], cnt
        if int(cnt[N.BGZF_COUNT_FAILED]):
            k = int(cnt[N.BGZF_COUNT_FIRST_FAILED])
            raise BgzfError.for_block(k, int(in_off[k]), int(status[k]), int(cnt[N.BGZF_COUNT_FAILED]))
        return out[:total]

    # -- formatting (host) ---------------------------------------------------
    def format_path(self, chrom_code: int, code: int) -> Optional[str]:
        buf = ctypes.create_string_buffer(N.MAX_PATH)
        rc = N.call("avdb_format_bin_path", self.ctx, chrom_code, code & 0xFFFFFFFF, buf, N.MAX_PATH, check=False)
        if rc < 0:
            return None
        return buf.raw[:rc].decode("ascii")

    def format_paths(self, chrom_codes: np.ndarray, codes: np.ndarray) -> List[Optional[str]]:
        """Host batch formatting of kernel outputs into ltree strings (None for
        unmappable rows)."""
        chrom_codes = np.ascontiguousarray(chrom_codes, dtype=np.uint8)
        codes = np.ascontiguousarray(codes).view(np.uint32)
        n = len(codes)
        cap = max(1, n * 88)
        out = np.empty(cap, dtype=np.uint8)
        offs = np.empty(n + 1, dtype=np.uint64)
        self._call("avdb_format_bin_paths", chrom_codes, codes, n, out, cap, offs)
        raw = out[: int(offs[n])].tobytes().decode("ascii")
        res: List[Optional[str]] = []
        for i in range(n):
            a, b = int(offs[i]), int(offs[i + 1])
            res.append(raw[a:b] if b > a else None)
        return res

    @staticmethod
    def _check_alleles(b: RecordBatch):
        if not b.has_alleles():
            raise ValueError("batch has no allele heap")
        if b.allele_off.dtype != torch.int64 or b.ref_len.element_size() != 4 or b.alt_len.element_size() != 4:
            raise TypeError("allele_off must be int64, ref_len/alt_len 32-bit")
        n = b.n
        for t in (b.pos, b.allele_off, b.ref_len, b.alt_len):
            if t.numel() != n:
                raise ValueError("record arrays must all have n entries")
        if b.ext_id is not None and b.ext_id.numel() != n:
            raise ValueError("ext_id must have n entries")


_ENGINES: Dict[int, Engine] = {}


def default_engine(device=None) -> Engine:
    """Process-wide engine per device (GRCh38 table); ``AVDB_DEVICE=host`` (with no
    device given) selects the host-only engine of the per-call entries."""
    if device is None and os.environ.get("AVDB_DEVICE") == "host":
        device = "host"
    if device == "host":
        eng = _ENGINES.get("host")
        if eng is None:
            eng = _ENGINES["host"] = Engine("host")
        return eng
    N.require_gpu()
    idx = torch.cuda.current_device() if device is None else int(device)
    eng = _ENGINES.get(idx)
    if eng is None:
        eng = Engine(idx)
        _ENGINES[idx] = eng
    return eng

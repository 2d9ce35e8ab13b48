"""CADD score annotation of loaded variants — the pass ``Load/bin/load_cadd_scores.py``
runs after ``load_vcf_file.py``.

The reference (``Util/lib/python/loaders/cadd_updater.py:187-221``) does, for
every variant, one tabix fetch at its position, a scan of the rows there, a
``ref`` / ``alt`` membership test and one buffered ``UPDATE ... SET cadd_scores``
value.  Here a CADD file (or one chromosome of it) is parsed once into a device
table (K10a, ``avdb_cadd_table_build``) and every batch of variants is a
sort-merge join against it on the GPU (K10b, ``avdb_cadd_match``): the indel table
when ``len(ref) > 1 or len(alt) > 1`` else the SNV table (``:189``), the first row
at the position, in file order, with ``ref in [R, A] and alt in [R, A]``
(``:202-204`` — deliberately that loose: a switched row matches).

A bgzip file read whole (``CaddTable.from_file(path)``) is inflated on the GPU (K11,
``bgzf.read_whole``) and the text handed to the table build where it lies: no host
copy of the text exists.  Tabix indexes are not read.  A whole-genome SNV file does
not fit in HBM: ``CaddTable.from_file(path, contigs=[...])`` keeps one chromosome's
lines while it reads, the way the reference's loop runs per chromosome; that filter
runs on the host, where bgzip files are multi-member gzip, so Python's ``gzip`` reads
them.

What stays with the caller, as in the reference it needs a database: the lookup
of a variant's primary key by metaseq id (``__get_variant_primary_key`` →
``is_duplicate``; here the records carry ``record_primary_key``, which is what
``SELECT_SQL`` of ``load_cadd_scores.py:29`` returns) and the ``UPDATE`` itself
(``update_variants``: ``execute_values`` over :meth:`CADDUpdater.update_buffer`).

A whole export of the variants (the rows ``SELECT_SQL`` returns, as ``COPY ... TO
STDOUT`` writes them) goes through :meth:`CADDUpdater.buffer_export` instead of
``buffer_variants``: K13 (``avdb_cadd_update_size`` / ``avdb_cadd_update_write``)
splits the lines, joins them against the tables and writes the update rows as text on
the GPU, the JSON of the two scores included: for every score text the table build
parses, ``json.dumps(float(text))`` is a rewrite of the text's own digits.  Only rows
the device does not decide (a contig without a code, a position that is not plain
digits, a table score left to ``float()``) are rendered by ``buffer_variants``' host
code.  ``annotatedvdb_amd.load_cadd_scores`` is the command-line driver over it.
"""

from __future__ import annotations

import json
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .chromosomes import CHROM_NAMES
from .engine import CaddColumns, pack_records

_CODE = {name: i for i, name in enumerate(CHROM_NAMES)}
_CODE["MT"] = _CODE["M"]  # a variant on 'MT' fetches 'MT', as one on 'M' does (cadd_updater.py:179)
UNKNOWN = 255


def _cadd_name(chrm: str) -> str:
    return "MT" if chrm == "M" else chrm  # cadd_updater.py:171,179


class CaddTable(object):
    """One CADD file (or the lines of some of its contigs) as a device table.

    Owns the text slab (the allele columns are offsets into it) and the column
    tensors; rows whose scores the device does not parse (exponents, 16 or more
    digits, ...) are patched once here with ``float()``; a file that is not in
    tabix order (a contig in two runs, a position that decreases) raises
    ``ValueError``."""

    def __init__(self, cols: CaddColumns, engine):
        self._engine = engine
        self.cols = cols
        self.counts = {name: int(cols.counts[k]) for name, k in (
            ("rows", N.CADD_COUNT_ROWS), ("score_host", N.CADD_COUNT_SCORE_HOST), ("bad", N.CADD_COUNT_BAD),
            ("order_violations", N.CADD_COUNT_ORDER_VIOLATIONS))}
        if self.counts["order_violations"]:
            raise ValueError("CADD table is not sorted as tabix requires: %d order violations (a contig in more "
                             "than one run, or a position that decreases)" % self.counts["order_violations"])
        self._slab: Optional[bytes] = None
        self._unknown: Optional[Dict[str, List[int]]] = None
        if self.counts["score_host"]:
            self._patch_scores()

    def __len__(self):
        return self.cols.n_rows

    @classmethod
    def from_text(cls, text: bytes, engine=None) -> "CaddTable":
        from .engine import default_engine
        engine = engine or default_engine()
        return cls(engine.cadd_table_build(text), engine)

    @classmethod
    def from_file(cls, path: str, contigs: Optional[Sequence[str]] = None, engine=None) -> "CaddTable":
        """A plain, gzip or bgzip CADD TSV.  ``contigs``: keep only the lines of
        these contigs (CADD labels: ``'1'`` .. ``'22'``, ``'X'``, ``'Y'``, ``'MT'``; ``'M'``
        and a ``chr`` prefix are accepted) while reading."""
        from . import bgzf
        if contigs is None:
            from .engine import default_engine
            engine = engine or default_engine()
            return cls.from_text(bgzf.read_whole(path, engine), engine)
        keep = set()
        for c in contigs:
            c = str(c)
            c = c[3:] if c.startswith("chr") else c
            keep.add(_cadd_name(c).encode() + b"\t")
        keep = tuple(keep)
        with bgzf.open_text(path) as fh:
            return cls.from_text(b"".join(ln for ln in fh if ln.startswith(keep)), engine)

    # ---- host-side pieces ---------------------------------------------------
    def slab(self) -> bytes:
        if self._slab is None:
            self._slab = self.cols.text.cpu().numpy().tobytes()
        return self._slab

    def _field(self, off: int, length: int) -> bytes:
        return self.slab()[off:off + length]

    def _patch_scores(self):
        """Scores flagged AVDB_CADD_ROW_SCORE_HOST, parsed as the reference does
        (``float(match[4])``, ``float(match[5])``, ``cadd_updater.py:205``)."""
        c = self.cols
        flags = c.flags.cpu().numpy()
        rows = np.nonzero(flags & N.CADD_ROW_SCORE_HOST)[0]
        alt_off, alt_len = c.alt_off.cpu().numpy(), c.alt_len.cpu().numpy()
        slab = self.slab()
        raw, phred = [], []
        for r in rows:
            a = int(alt_off[r]) + int(alt_len[r]) + 1
            e = slab.find(b"\n", a)
            f = slab[a:e if e >= 0 else len(slab)].split(b"\t")
            raw.append(float(f[0].decode("ascii", "replace")))
            phred.append(float(f[1].decode("ascii", "replace")))
        idx = torch.from_numpy(rows.astype(np.int64)).to(c.raw.device)
        c.raw[idx] = torch.tensor(raw, dtype=torch.float64).to(c.raw.device)
        c.phred[idx] = torch.tensor(phred, dtype=torch.float64).to(c.raw.device)

    def resolve_host(self, chrm: str, position: int, ref: str, alt: str) -> int:
        """Records the device leaves to the caller (``AVDB_CADD_HOST``: a contig
        without a code): the reference's lookup by contig name over this table's
        unknown-contig rows; the row index or -1."""
        if self._unknown is None:
            self._unknown = {}
            c = self.cols
            chrom, flags = c.chrom.cpu().numpy(), c.flags.cpu().numpy()
            ref_off = c.ref_off.cpu().numpy()
            slab = self.slab()
            for r in np.nonzero((chrom == UNKNOWN) & ((flags & N.CADD_ROW_BAD) == 0))[0]:
                s = slab.rfind(b"\n", 0, int(ref_off[r])) + 1
                name = slab[s:slab.find(b"\t", s)].decode("ascii", "replace")
                self._unknown.setdefault(name, []).append(int(r))
            self._host_cols = tuple(x.cpu().numpy() for x in (c.pos, c.ref_off, c.ref_len, c.alt_off, c.alt_len))
        rows = self._unknown.get(_cadd_name(chrm))
        if not rows:
            return -1
        pos, ref_off, ref_len, alt_off, alt_len = self._host_cols
        r8, a8 = ref.encode(), alt.encode()
        for r in rows:
            if int(pos[r]) != position:
                continue
            alleles = (self._field(int(ref_off[r]), int(ref_len[r])), self._field(int(alt_off[r]), int(alt_len[r])))
            if r8 in alleles and a8 in alleles:
                return r
        return -1


class CADDUpdater(object):
    """The reference ``CADDUpdater``'s observable surface, batch-wise and without a
    database: counters, chromosome, the update buffer of
    ``(record_primary_key, 'chr' + c, json.dumps(evidence))`` tuples that
    ``execute_values(cursor, CADD_UPDATE_SQL, buffer)`` takes.  The primary-key
    lookup by metaseq id and the ``UPDATE`` itself stay with the caller (module
    docstring)."""

    def __init__(self, snv: Optional[CaddTable] = None, indel: Optional[CaddTable] = None, engine=None):
        if engine is None:
            table = snv if snv is not None else indel
            if table is not None:
                engine = table._engine
            else:
                from .engine import default_engine
                engine = default_engine()
        self._engine = engine
        self._snv, self._indel = snv, indel
        self.__chromosome = None
        self._counters = {"line": 0, "variant": 0, "skipped": 0, "duplicates": 0, "update": 0,
                          "snv": 0, "indel": 0, "not_matched": 0}
        self._update_buffer: List[tuple] = []
        # rows buffer_export appended, not yet split into tuples: (index in _update_buffer they
        # stand before, number of rows, their text)
        self._export_rows: List[tuple] = []

    # ---- the reference's surface -----------------------------------------------
    def set_chromosome(self, chrm):
        self.__chromosome = str(chrm).replace("chr", "")

    def get_chromosome(self):
        return self.__chromosome

    def get_count(self, counter):
        return self._counters[counter]

    def increment_counter(self, counter):
        self._counters[counter] += 1

    def get_update_count(self, indels=False):
        return self.get_count("indel") if indels else self.get_count("snv")

    def get_total_update_count(self):
        return self.get_count("update") + self.get_count("not_matched") + self.get_count("skipped")

    def update_buffer(self, sizeOnly=False):
        """The buffered ``(pk, chrom, json)`` tuples, rows from :meth:`buffer_export`
        included (split into tuples at the first call that asks for them)."""
        if sizeOnly:
            return len(self._update_buffer) + sum(n for _, n, _ in self._export_rows)
        for at, _, text in reversed(self._export_rows):
            rows = text.decode("utf-8", "surrogateescape").split("\n")[:-1]
            self._update_buffer[at:at] = [tuple(r.split("\t")) for r in rows]
        self._export_rows = []
        return self._update_buffer

    def update_text(self) -> bytes:
        """The buffered rows as text, ``pk<TAB>chrom<TAB>json<LF>`` each, in buffer order."""
        parts, done = [], 0
        for at, _, text in self._export_rows + [(len(self._update_buffer), 0, b"")]:
            parts += [("\t".join(t) + "\n").encode("utf-8", "surrogateescape") for t in self._update_buffer[done:at]]
            parts.append(text)
            done = at
        return b"".join(parts)

    def reset_update_buffer(self):
        self._update_buffer = []
        self._export_rows = []

    def snv(self):
        return self._snv

    def indel(self):
        return self._indel

    # ---- batch entries -----------------------------------------------------------
    def match_batch(self, metaseq_ids: Sequence[str]):
        """``(row, kind, raw, phred)`` numpy arrays for ``chrom:pos:ref:alt`` ids:
        the matched row's index in its table (-1: none), ``N.CADD_NONE`` /
        ``CADD_SNV`` / ``CADD_INDEL``, and the two scores (NaN where unmatched).
        Records the device leaves to the host are resolved here, so no
        ``CADD_HOST`` is returned."""
        n = len(metaseq_ids)
        codes, pos, refs, alts, names = [], [], [], [], []
        for m in metaseq_ids:
            c, p, r, a = m.split(":")  # cadd_updater.py:188
            p = int(p)
            code = _CODE.get(c, UNKNOWN)
            if not 0 <= p < (1 << 32):
                code, p = UNKNOWN, 0
            codes.append(code)
            pos.append(p)
            refs.append(r.encode())
            alts.append(a.encode())
            names.append(c)
        if n == 0:
            return (np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros(0, np.float64), np.zeros(0, np.float64))
        b = pack_records(codes, pos, refs, alts)  # (pos of 2^31 and above wraps into the int32 column's bits)
        row, kind, raw, phred = self._engine.cadd_match(
            self._snv.cols if self._snv is not None else None, self._indel.cols if self._indel is not None else None, b)
        row, kind = row.cpu().numpy().copy(), kind.cpu().numpy().copy()
        raw, phred = raw.cpu().numpy().copy(), phred.cpu().numpy().copy()
        for i in np.nonzero(kind == N.CADD_HOST)[0]:
            r, a = refs[i].decode(), alts[i].decode()
            is_indel = len(r) > 1 or len(a) > 1
            t = self._indel if is_indel else self._snv
            k = -1
            if t is not None and names[i] not in _CODE:  # (a canonical contig is here for its position: no row)
                k = t.resolve_host(names[i], pos[i], r, a)
            row[i] = k
            kind[i] = N.CADD_NONE if k < 0 else (N.CADD_INDEL if is_indel else N.CADD_SNV)
            if k >= 0:
                raw[i] = float(t.cols.raw[k])
                phred[i] = float(t.cols.phred[k])
        return row, kind, raw, phred

    def buffer_variants(self, records: Iterable, skip_existing: bool = True):
        """``buffer_variant`` (``cadd_updater.py:187-221``) over a batch of records
        (mappings or namespaces with ``metaseq_id``, ``record_primary_key`` and
        optionally ``cadd_scores``): a record already annotated is counted
        ``skipped`` under ``skip_existing`` (``:192-196``, ``load_cadd_scores.py:114-117``);
        every other one appends its update tuple (``:121-130``) with the matched
        row's scores, or ``{}`` when no row matches, and moves the counters as
        ``:199-219`` do.  Returns the number of tuples appended."""
        todo = []
        for rec in records:
            get = rec.get if isinstance(rec, dict) else lambda k, d=None, rec=rec: getattr(rec, k, d)
            if skip_existing and get("cadd_scores") is not None:
                self.increment_counter("skipped")
                continue
            todo.append((get("metaseq_id"), get("record_primary_key")))
        if not todo:
            return 0
        _, kind, raw, phred = self.match_batch([m for m, _ in todo])
        chrm = None
        if self.__chromosome is not None:
            chrm = self.__chromosome if "chr" in self.__chromosome else "chr" + str(self.__chromosome)
        for (_, pk), k, x, y in zip(todo, kind.tolist(), raw.tolist(), phred.tolist()):
            if k == N.CADD_NONE:
                evidence = {}
                self.increment_counter("not_matched")
            else:
                evidence = {"CADD_raw_score": x, "CADD_phred": y}
                self.increment_counter("indel" if k == N.CADD_INDEL else "snv")
                self.increment_counter("update")
            c = chrm if chrm is not None else "chr" + str(pk.split(":")[0])
            self._update_buffer.append((pk, c, json.dumps(evidence)))
        return len(todo)

    def buffer_export(self, path_or_text, skip_existing: bool = True, contigs=None):
        """:meth:`buffer_variants` over a whole export (K13,
        :meth:`Engine.cadd_update_rows`): ``record_primary_key<TAB>metaseq_id<TAB>cadd_scores``
        lines, ``cadd_scores`` NULL as ``\\N``, empty or absent, given as a path (plain,
        gzip or bgzip) or as text (bytes, numpy ``uint8`` or a ``uint8`` tensor).
        ``contigs``: keep only the rows whose metaseq id carries one of these labels, so
        that one whole-table export serves every per-chromosome pass.  Moves ``snv``,
        ``indel``, ``update``, ``not_matched`` and ``skipped`` and appends the rows as
        ``buffer_variants`` would for the same records; returns their number."""
        if isinstance(path_or_text, str):
            from . import bgzf
            path_or_text = bgzf.read_whole(path_or_text, self._engine)
        rows = self._engine.cadd_update_rows(path_or_text, self._snv, self._indel, chromosome=self.__chromosome,
                                             skip_existing=skip_existing, contigs=contigs)
        c = rows.counts
        for name, k in (("snv", c["snv"]), ("indel", c["indel"]), ("update", c["snv"] + c["indel"]),
                        ("not_matched", c["not_matched"]), ("skipped", c["skipped"])):
            self._counters[name] += k
        if rows.n:
            self._export_rows.append((len(self._update_buffer), rows.n, rows.text.cpu().numpy().tobytes()))
        return rows.n

"""ADSP QC pVCF -> ``is_adsp_variant`` / ``adsp_qc`` update rows, without a database — the
counterpart of ``Load/bin/update_from_qc_pvcf_file.py``.

The reference walks the QC file on one host thread: every line is parsed (``VcfEntryParser``, the
whole INFO column into a dict with ``to_numeric`` on every value), its lookup ids
``chrom:pos:ref:alt`` go to a bulk SQL lookup 1,000 at a time, and for every hit
``generate_update_values`` (``:117-149``) renders ``{release: {"info": ..., "filter": ..., "qual":
..., "format": ...}}`` into the tuple ``(record_primary_key, 'chr' + chromosome, True | None, json)``
that ``__buffer_update_values`` (``vcf_variant_loader.py:172-219``) appends, unless the record has
QC values of this release already.  Here an export of the table stands in for the database, as for
the LOF pass (:mod:`annotatedvdb_amd.snpeff_lof`):

* K17a, :meth:`Engine.qc_table_build`: the QC file -> a device table of its alt alleles, their
  lookup ids hashed (K6), the JSON rendered once per line;
* K17b, :meth:`Engine.qc_update_rows`: the export
  (``record_primary_key<TAB>metaseq_id<TAB>adsp_qc``) streamed against that table -> the update
  rows as text.

:class:`QCUpdater` carries the reference loader's observable surface for this pass (counters, the
update buffer); :func:`qc_line` is the one Python path of a line the device leaves to the host.
Deviations are listed in DESIGN.md (K17).
"""

from __future__ import annotations

import json
from typing import List, Tuple

from .parsers import VcfEntryParser, _xstr

HEADER_FIELDS = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"]  # --vcfHeaderFields' default
UPDATE_FIELDS = ["is_adsp_variant", "adsp_qc"]  # initialize_loader:178


def qc_line(line: bytes, release: str, header_fields=None) -> Tuple[List[bytes], bytes, bool]:
    """One line of the QC file as the reference's loop treats it (``load_annotation:226-258`` and
    ``generate_update_values:117-149``): ``(lookup ids, one per ALT allele; the JSON of the
    ``adsp_qc`` update value; whether FILTER is PASS)``.  Raises what the reference raises for the
    line: ``IndexError`` (fewer fields than the header), ``ImportError`` (``parse_entry``'s own
    wrapper, a numeric INFO), ``ValueError`` (``Infinity found among QC scores``, bytes that are
    not UTF-8), ``AttributeError`` (a numeric ID or ALT), ``TypeError`` (a REF or ALT that reads
    as a number)."""
    text = line.decode("utf-8").rstrip()
    entry = VcfEntryParser(text, HEADER_FIELDS if header_fields is None else header_fields)
    variant = entry.get_variant()
    keys = [":".join((_xstr(variant["chromosome"]), _xstr(variant["position"]), variant["ref_allele"], alt))
            .encode("utf-8") for alt in variant["alt_alleles"]]
    filter_ = entry.get("filter")
    values = {release: {"info": entry.get("info"), "filter": filter_, "qual": entry.get("qual"),
                        "format": entry.get("format", raiseError=False)}}
    text = json.dumps(values)
    if "Infinity" in text:
        raise ValueError("Infinity found among QC scores")
    return keys, text.encode("utf-8"), filter_ == "PASS"


class QCUpdater(object):
    """The reference loader's observable surface for the ADSP QC pass, batch-wise and without a
    database, in the mould of :class:`~annotatedvdb_amd.snpeff_lof.LOFUpdater`: counters and the
    update buffer of ``(record_primary_key, 'chr' + c, True | None, json)`` tuples that
    ``execute_values(cursor, update_sql, buffer)`` takes with ``UPDATE_FIELDS``.  ``table``: a
    :class:`~annotatedvdb_amd.engine.QcTable`, or the QC file as a path (plain, gzip or bgzip) or
    text, with ``version`` (and ``header_fields``) as the reference's ``--version`` (and
    ``--vcfHeaderFields``)."""

    def __init__(self, table, version=None, engine=None, header_fields=None):
        from .engine import QcTable, default_engine
        if engine is None:
            engine = table.engine if isinstance(table, QcTable) else default_engine()
        self._engine = engine
        if not isinstance(table, QcTable):
            if version is None:
                raise ValueError("a version (the ADSP release) is needed to build the table")
            if isinstance(table, str):
                from . import bgzf
                table = bgzf.read_whole(table, engine)
            table = engine.qc_table_build(table, version, header_fields)
        self._table = table
        self._counters = {"line": table.counts["lines"] - table.counts["comment_lines"], "variant": 0, "update": 0,
                          "skipped": 0, "not_in_vcf": 0}
        self._update_buffer: List[tuple] = []
        self._export_rows: List[tuple] = []  # (index in _update_buffer they stand before, rows, text)

    def table(self):
        return self._table

    def get_datasource(self):
        return self._table.release.decode("ascii")

    def get_count(self, counter):
        return self._counters[counter]

    def increment_counter(self, counter):
        self._counters[counter] += 1

    @staticmethod
    def _tuple(row: str) -> tuple:
        pk, chrom, flag, js = row.split("\t", 3)
        return pk, chrom, True if flag == "true" else None, js

    @staticmethod
    def _row(t: tuple) -> bytes:
        return "\t".join((t[0], t[1], "true" if t[2] else "\\N", t[3])).encode("utf-8", "surrogateescape") + b"\n"

    def update_buffer(self, sizeOnly=False):
        """The buffered ``(pk, chrom, True | None, json)`` tuples (rows from :meth:`buffer_export`
        are split into tuples at the first call that asks for them)."""
        if sizeOnly:
            return len(self._update_buffer) + sum(n for _, n, _ in self._export_rows)
        for at, _, text in reversed(self._export_rows):
            rows = text.decode("utf-8", "surrogateescape").split("\n")[:-1]
            self._update_buffer[at:at] = [self._tuple(r) for r in rows]
        self._export_rows = []
        return self._update_buffer

    def update_text(self) -> bytes:
        """The buffered rows as text, ``pk<TAB>chrom<TAB>true|\\N<TAB>json<LF>`` each, in buffer order."""
        parts, done = [], 0
        for at, _, text in self._export_rows + [(len(self._update_buffer), 0, b"")]:
            parts += [self._row(t) for t in self._update_buffer[done:at]]
            parts.append(text)
            done = at
        return b"".join(parts)

    def reset_update_buffer(self):
        self._update_buffer = []
        self._export_rows = []

    def buffer_export(self, path_or_text, update_existing: bool = False, contigs=None) -> int:
        """The update rows of a whole export (K17b, :meth:`Engine.qc_update_rows`):
        ``record_primary_key<TAB>metaseq_id<TAB>adsp_qc`` lines, the third column the JSONB text as
        ``COPY`` writes it (NULL as ``\\N``, empty or absent), given as a path (plain, gzip or
        bgzip) or as text.  Moves ``update``, ``skipped`` and ``not_in_vcf``; returns the number of
        rows appended."""
        if isinstance(path_or_text, str):
            from . import bgzf
            path_or_text = bgzf.read_whole(path_or_text, self._engine)
        rows = self._engine.qc_update_rows(path_or_text, self._table, update_existing=update_existing,
                                           contigs=contigs)
        for name, k in (("update", rows.n), ("skipped", rows.counts["skipped"]),
                        ("not_in_vcf", rows.counts["not_in_vcf"])):
            self._counters[name] += k
        if rows.n:
            self._export_rows.append((len(self._update_buffer), rows.n, rows.text.cpu().numpy().tobytes()))
        return rows.n

    def _unmatched_rows(self):
        """(lookup id, its last row) of the ids no export row has matched, in file order; the rows' keys."""
        t = self._table
        if t.n_rows == 0:
            return [], []
        hit = t.hit.cpu().numpy()
        off = t.key_off.cpu().numpy()
        blob = t.keys.cpu().numpy().tobytes()
        keys = [blob[off[r]:off[r + 1]] for r in range(t.n_rows)]
        last = {k: r for r, k in enumerate(keys)}
        return [(k, r) for k, r in last.items() if not hit[r]], keys

    def unmatched(self) -> List[str]:
        """The lookup ids of the table no export row has matched so far, in file order (an id the
        file repeats once; its last record is the one that answers)."""
        return [k.decode("utf-8", "surrogateescape") for k, _ in self._unmatched_rows()[0]]

    def novel_lines(self) -> List[bytes]:
        """The distinct lines of the QC file, in file order, that hold an id no export row has
        matched so far: the variants the reference would insert (``parse_variant`` without flags)."""
        missing, keys = self._unmatched_rows()
        if not missing:
            return []
        ids = {k for k, _ in missing}
        t = self._table
        starts = sorted({int(s) for s, k in zip(t.line_start.cpu().tolist(), keys) if k in ids})
        text = t.text.cpu().numpy().tobytes()
        out = []
        for s in starts:
            e = text.find(b"\n", s)
            out.append(text[s:e if e >= 0 else len(text)].rstrip())
        return out

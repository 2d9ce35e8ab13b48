"""SnpEff LOF / NMD annotation -> ``loss_of_function`` update rows, without a database — the
counterpart of ``Load/bin/load_snpeff_lof.py``.

The reference walks the VCF SnpEff wrote on one host thread: a line without ``;LOF=`` and
``;NMD=`` is dropped, every other one is parsed (``VcfEntryParser``), its lookup ids
``chrom:pos:ref:alt`` go to a bulk SQL lookup 1,000 at a time, and for every hit
``generate_update_values`` (``:136-173``) renders ``{'LOF': [...], 'NMD': [...]}`` into the tuple
``(record_primary_key, 'chr' + chromosome, json)`` that ``__buffer_update_values``
(``vcf_variant_loader.py:172-219``) appends.  Here an export of the table stands in for the
database (as for the CADD pass, :mod:`annotatedvdb_amd.cadd`):

* K16a, :meth:`Engine.lof_table_build`: the VCF -> a device table of the annotated alt alleles,
  their lookup ids hashed (K6), the JSON rendered once per line;
* K16b, :meth:`Engine.lof_update_rows`: the export
  (``record_primary_key<TAB>metaseq_id<TAB>loss_of_function``) streamed against that table ->
  the update rows as text.

:class:`LOFUpdater` carries the reference loader's observable surface for this pass (counters, the
update buffer); :func:`parse_annotation_string` is a drop-in; :func:`annotated_line` is the one
Python path of a line the device leaves to the host.  Deviations are listed in DESIGN.md (K16).
"""

from __future__ import annotations

import json
from typing import List, Tuple

from .parsers import VcfEntryParser, _xstr

HEADER_FIELDS = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"]


def parse_annotation_string(valueStr):
    """Drop-in for ``parse_annotation_string`` (``load_snpeff_lof.py:112-134``):
    ``(SFI1|ENSG00000198089|30|0.17),(...)`` -> a list of dicts; ``None`` -> ``None``.  A value
    that is no string (a number, a bare flag's ``True``) raises ``AttributeError``, a group of
    fewer than four parts ``IndexError``, a count or fraction that does not parse ``ValueError``."""
    if valueStr is None:
        return None
    returnVal = []
    for a in valueStr.split(","):
        values = a.replace("(", "").replace(")", "").split("|")
        returnVal.append({"gene_symbol": values[0], "gene_id": values[1], "num_transcripts": int(values[2]),
                          "fraction_affected_transcripts": float(values[3])})
    return returnVal


def annotated_line(line: bytes, header_fields=None) -> Tuple[List[bytes], bytes]:
    """One annotated VCF line as the reference's loop treats it (``load_annotation:251-288`` and
    ``generate_update_values:146-165``): ``(lookup ids, one per ALT allele; the JSON of the
    update values)``, or ``([], b"")`` when INFO holds neither key.  Raises what the reference
    raises for the line: ``AttributeError`` (a numeric ID or ALT, a numeric or bare LOF value),
    ``IndexError`` (too few fields, a group of fewer than four parts), ``ValueError`` (a count or
    fraction that does not parse, bytes that are not UTF-8), ``TypeError`` (a REF or ALT that
    reads as a number), ``ImportError`` (``parse_entry``'s own wrapper)."""
    text = line.decode("utf-8").rstrip()
    entry = VcfEntryParser(text, HEADER_FIELDS if header_fields is None else header_fields)
    variant = entry.get_variant()
    keys = [":".join((_xstr(variant["chromosome"]), _xstr(variant["position"]), variant["ref_allele"], alt))
            .encode("utf-8") for alt in variant["alt_alleles"]]  # (the ids first, as load_annotation joins them)
    lof = parse_annotation_string(entry.get_info("LOF"))
    nmd = parse_annotation_string(entry.get_info("NMD"))
    if lof is None and nmd is None:
        return [], b""
    values = {}
    if lof is not None:
        values["LOF"] = lof
    if nmd is not None:
        values["NMD"] = nmd
    return keys, json.dumps(values).encode("utf-8")


class LOFUpdater(object):
    """The reference loader's observable surface for the ``loss_of_function`` pass, batch-wise
    and without a database, in the mould of :class:`~annotatedvdb_amd.cadd.CADDUpdater`:
    counters and the update buffer of ``(record_primary_key, 'chr' + c, json)`` tuples that
    ``execute_values(cursor, update_sql, buffer)`` takes.  ``table``: a
    :class:`~annotatedvdb_amd.engine.LofTable`, or the SnpEff VCF as a path (plain, gzip or
    bgzip) or text."""

    def __init__(self, table, engine=None):
        from .engine import LofTable, default_engine
        if engine is None:
            engine = table.engine if isinstance(table, LofTable) else default_engine()
        self._engine = engine
        if not isinstance(table, LofTable):
            if isinstance(table, str):
                from . import bgzf
                table = bgzf.read_whole(table, engine)
            table = engine.lof_table_build(table)
        self._table = table
        self._counters = {"line": table.counts["lines"] - table.counts["comment_lines"], "variant": 0, "update": 0,
                          "skipped": 0, "not_annotated": 0}
        self._update_buffer: List[tuple] = []
        self._export_rows: List[tuple] = []  # (index in _update_buffer they stand before, rows, text)

    def table(self):
        return self._table

    def get_count(self, counter):
        return self._counters[counter]

    def increment_counter(self, counter):
        self._counters[counter] += 1

    def update_buffer(self, sizeOnly=False):
        """The buffered ``(pk, chrom, json)`` tuples (rows from :meth:`buffer_export` are split
        into tuples at the first call that asks for them)."""
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

    def buffer_export(self, path_or_text, update_existing: bool = False, contigs=None) -> int:
        """The update rows of a whole export (K16b, :meth:`Engine.lof_update_rows`):
        ``record_primary_key<TAB>metaseq_id<TAB>loss_of_function`` lines, the third column NULL
        as ``\\N``, empty or absent, given as a path (plain, gzip or bgzip) or as text.  Moves
        ``update``, ``skipped`` and ``not_annotated``; returns the number of rows appended."""
        if isinstance(path_or_text, str):
            from . import bgzf
            path_or_text = bgzf.read_whole(path_or_text, self._engine)
        rows = self._engine.lof_update_rows(path_or_text, self._table, update_existing=update_existing,
                                            contigs=contigs)
        for name, k in (("update", rows.n), ("skipped", rows.counts["skipped"]),
                        ("not_annotated", rows.counts["not_annotated"])):
            self._counters[name] += k
        if rows.n:
            self._export_rows.append((len(self._update_buffer), rows.n, rows.text.cpu().numpy().tobytes()))
        return rows.n

    def unmatched(self) -> List[str]:
        """The lookup ids of the table no export row has matched so far, in file order (an id
        the VCF repeats once; its last record is the one that answers)."""
        t = self._table
        if t.n_rows == 0:
            return []
        hit = t.hit.cpu().numpy()
        off = t.key_off.cpu().numpy()
        blob = t.keys.cpu().numpy().tobytes()
        last = {}
        for r in range(t.n_rows):
            last[blob[off[r]:off[r + 1]]] = r
        return [k.decode("utf-8", "surrogateescape") for k, r in last.items() if not hit[r]]

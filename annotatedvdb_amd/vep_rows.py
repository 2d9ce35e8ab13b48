"""K18b: VEP results -> ``adsp_most_severe_consequence`` / ``adsp_ranked_consequences`` update rows,
without a database — two of the four JSON columns of ``Load/bin/load_vep_result.py`` on
``VEPVariantLoader`` (``vep_variant_loader.py:153-213``), and on request a third, ``vep_output`` (K18c:
the cleaned result, :func:`vep_output_line`) and the fourth, ``allele_frequencies`` (K18d:
:func:`allele_frequencies_line`).

The reference walks VEP's ``--json`` output on one host thread: per line a ``json.loads``, a
``VcfEntryParser`` of the top-level ``input`` string, the consequences ranked and sorted (K18a), and
per ALT allele a ``VariantAnnotator``, a primary-key lookup by metaseq id, and
``xstr(get_most_severe_consequence(normAlt))`` / ``xstr(get_allele_consequences(normAlt))``.  Here
an export of the table stands in for the database, as for K16:

* :meth:`Engine.vep_rows_table_build`: the JSON -> a device table of one row per ALT allele, its
  metaseq id hashed (K6), its two columns rendered from the elements' own bytes;
* :meth:`Engine.vep_update_rows`: the export (``record_primary_key<TAB>metaseq_id<TAB>vep_output``)
  streamed against that table -> the update rows as text.

:func:`vep_rows_line` is the reference's per-line pass in Python (the host path), :class:`VEPUpdater`
the loader's observable surface for these columns.  ``xstr(dict)`` is taken to be ``json.dumps``
(README, "json.dumps stand-in").  Deviations are listed in DESIGN.md (K18b).
"""

from __future__ import annotations

import json
from typing import List, Tuple

from .parsers import VcfEntryParser
from .variant_annotator import VariantAnnotator
from .vep_consequences import TYPE_KEYS, ConsequenceRanking, most_severe_of, rank_annotation

UPDATE_FIELDS = ["adsp_most_severe_consequence", "adsp_ranked_consequences", "row_algorithm_id"]
JSONB_UPDATE_FIELDS = ["adsp_most_severe_consequence", "adsp_ranked_consequences"]


def allele_consequences(ranked, allele):
    """``get_allele_consequences(allele)`` over :func:`~annotatedvdb_amd.vep_consequences.vep_line`'s
    result: ``{"<type>_consequences": [...]}`` for the types that hold the allele, or ``None``."""
    out = {}
    for key in TYPE_KEYS:
        conseqs = ranked.get(key)
        if conseqs is not None and allele in conseqs:
            out[key] = conseqs[allele]
    return out or None


def _xstr_json(value) -> str:
    return "{}" if value is None else json.dumps(value)


def vep_rows_line(line, ranking: ConsequenceRanking) -> List[Tuple[str, str, str]]:
    """One line (``bytes`` or ``str``) as ``parse_variant`` and ``__parse_alt_alleles`` treat it, for
    the two consequence columns: ``[(metaseq id, adsp_most_severe_consequence,
    adsp_ranked_consequences)]``, one per ALT allele of ``input``.  Only the first five fields of
    ``input`` are read (``identityOnly``: INFO matters to ``allele_frequencies`` alone).  Raises what
    the reference raises for the line: ``json.JSONDecodeError``, ``KeyError('input')``, ``IndexError``
    (fewer than five fields), ``AttributeError`` / ``ImportError`` / ``ValueError`` / ``TypeError`` of
    the VCF fields, what :func:`~annotatedvdb_amd.vep_consequences.vep_line` raises, and
    :class:`~annotatedvdb_amd.vep_consequences.UnrankedCombination` where it would re-rank."""
    annotation = json.loads(line)
    entry = VcfEntryParser(annotation["input"], identityOnly=True)
    variant = entry.get_variant(namespace=True)
    ranked = rank_annotation(annotation, ranking)
    rows = []
    for alt in variant.alt_alleles:
        annotator = VariantAnnotator(variant.ref_allele, alt, variant.chromosome, variant.position)
        _, norm_alt = annotator.get_normalized_alleles(snvDivMinus=True)
        rows.append((annotator.get_metaseq_id(), _xstr_json(most_severe_of(ranked, norm_alt)),
                     _xstr_json(allele_consequences(ranked, norm_alt))))
    return rows


def vep_output_line(line, identity_only: bool = False) -> str:
    """K18c's host path: ``xstr(cleanResult)`` of one line (``bytes`` or ``str``), the same text for every
    ALT allele.  ``parse_variant`` (``vep_variant_loader.py:262-296``) puts ``VcfEntryParser(input,
    identityOnly).get_entry()`` in place of the ``input`` string, ``__clean_result`` (``:112-123``) pops
    ``colocated_variants`` and the four ``<type>_consequences`` keys, and ``xstr(dict)`` is taken to be
    ``json.dumps``.  Raises what the reference raises before it: ``json.JSONDecodeError``,
    ``KeyError('input')``, ``IndexError`` (fewer fields than ``identity_only`` asks for: five, else eight),
    ``ImportError`` (an INFO that is a number)."""
    annotation = json.loads(line)
    entry = VcfEntryParser(annotation["input"], identityOnly=identity_only)
    annotation["input"] = entry.get_entry()
    annotation.pop("colocated_variants", None)
    for key in TYPE_KEYS:
        annotation.pop(key, None)
    return json.dumps(annotation)


def _deep_update(a: dict, b: dict) -> dict:
    """``deep_update`` as DESIGN.md (K18d) takes it: the recursive in-place merge, new keys appended."""
    for key, value in b.items():
        if isinstance(value, dict) and isinstance(a.get(key), dict):
            _deep_update(a[key], value)
        else:
            a[key] = value
    return a


def _group_frequencies_by_source(frequencies):
    """``VepJsonParser.__group_frequencies_by_source`` (``vep_parser.py:235-254``)."""
    if frequencies is None:
        return None
    result = {}
    for allele in frequencies:
        items = frequencies[allele].items()
        gnomad = {k: v for k, v in items if "gnomad" in k}
        esp = {k: v for k, v in items if k in ("aa", "ea")}
        genomes = {k: v for k, v in items if "gnomad" not in k and k not in ("aa", "ea")}
        for name, group in (("GnomAD", gnomad), ("1000Genomes", genomes), ("ESP", esp)):
            if group:
                result.setdefault(allele, {})[name] = group
    return result


def result_frequencies(annotation: dict, matching_variant_id=None):
    """``VepJsonParser.get_frequencies(matchingVariantId)['values']`` (``vep_parser.py:178-232``) of a parsed
    line, or ``None``."""
    if "colocated_variants" not in annotation:
        return None
    cv = annotation["colocated_variants"]
    chosen, found = None, False
    if len(cv) > 1:
        for covar in cv:
            if covar["allele_string"] != "COSMIC_MUTATION" and "frequencies" in covar:
                if matching_variant_id is None or covar["id"] == matching_variant_id:
                    chosen, found = covar, True
    elif "frequencies" in cv[0]:
        chosen, found = cv[0], True
    return _group_frequencies_by_source(chosen["frequencies"]) if found else None


def allele_frequencies_line(line, identity_only: bool = False, match_refsnp: bool = False) -> List[Tuple[str, str]]:
    """K18d's host path: ``[(metaseq id, xstr(alleleFreq, nullStr='{}'))]``, one per ALT allele of ``input``, of one
    line (``bytes`` or ``str``) as ``__parse_alt_alleles`` (``vep_variant_loader.py:153-199``) makes them: the
    frequencies of the normalised ALT in the element ``get_frequencies`` takes (``match_refsnp``: the one whose
    ``id`` is the variant's ``ref_snp_id``, the reference's dbSNP datasource), regrouped by source, and
    ``VcfEntryParser.get_frequencies(alt)`` (INFO ``FREQ``; none with ``identity_only``) merged into them in place,
    so that two ALTs with one normalised allele see each other's ``gmaf`` as they do there.  Raises what the
    reference raises: ``json.JSONDecodeError``, ``KeyError`` (``input``, ``allele_string``, ``id``), ``IndexError``
    (an empty ``colocated_variants``, fewer fields, fewer ``FREQ`` items than ALTs), ``AttributeError`` /
    ``TypeError`` (values that are not the containers or strings it expects), ``ImportError``."""
    annotation = json.loads(line)
    entry = VcfEntryParser(annotation["input"], identityOnly=identity_only)
    variant = entry.get_variant(dbSNP=match_refsnp, namespace=True)
    frequencies = result_frequencies(annotation, variant.ref_snp_id if match_refsnp else None)
    rows = []
    for alt in variant.alt_alleles:
        annotator = VariantAnnotator(variant.ref_allele, alt, variant.chromosome, variant.position)
        _, norm_alt = annotator.get_normalized_alleles(snvDivMinus=True)
        allele_freq = frequencies[norm_alt] if frequencies is not None and norm_alt in frequencies else None
        gmafs = entry.get_frequencies(alt)
        if allele_freq is None:
            allele_freq = gmafs
        elif gmafs is not None:
            allele_freq = _deep_update(allele_freq, gmafs)
        rows.append((annotator.get_metaseq_id(), _xstr_json(allele_freq)))
    return rows


def update_sql(adsp: bool = False, vep_output: bool = False, allele_frequencies: bool = False) -> str:
    """``initialize_update_sql`` (``vep_variant_loader.py:215-247``) over this pass's fields;
    ``vep_output``: the cleaned result's column too, before ``row_algorithm_id`` as in ``COPY_FIELDS``;
    ``allele_frequencies``: that column too, first behind the keys as there.  With both the statement is
    the reference's."""
    fields = list(UPDATE_FIELDS)
    if vep_output:
        fields.insert(fields.index("row_algorithm_id"), "vep_output")
    if allele_frequencies:
        fields.insert(0, "allele_frequencies")
    fields += ["is_adsp_variant"] if adsp else []
    sets = []
    for f in fields:
        if f in JSONB_UPDATE_FIELDS or f in ("vep_output", "allele_frequencies"):
            sets.append(f"{f} = jsonb_merge(COALESCE(v.{f} ,'{{}}'::jsonb), d.{f}::jsonb)")
        else:
            sets.append(f"{f} = d.{f}")
    cols = ",".join(["record_primary_key", "chromosome"] + fields)
    return ("UPDATE AnnotatedVDB.Variant v SET " + ", ".join(sets) + " FROM (VALUES %s) AS d(" + cols + ")"
            " WHERE v.chromosome = d.chromosome AND v.record_primary_key = d.record_primary_key")


class VEPUpdater(object):
    """The reference loader's observable surface for the two consequence columns, batch-wise and
    without a database, in the mould of :class:`~annotatedvdb_amd.snpeff_lof.LOFUpdater`: counters
    and the update buffer of ``(record_primary_key, 'chr' + c[, allele_frequencies], most severe, ranked[,
    vep_output], alg id[, 'true'])`` tuples (``vep_output``: K18c's column, ``allele_frequencies``: K18d's, the
    table built with them; ``dbsnp``: the reference's ``is_dbsnp()``, the element is matched by ``ref_snp_id``;
    ``identity_only``, by
    default ``adsp``, is the reference's ``identityOnly=self.is_adsp()``) that ``execute_values(cursor, update_sql, buffer)`` takes.  ``table``: a
    :class:`~annotatedvdb_amd.engine.VepRowsTable`, or the VEP output as a path (plain, gzip or
    bgzip) or text, with ``ranking`` (a :class:`ConsequenceRanking`, or what it takes)."""

    def __init__(self, table, ranking=None, alg_id: int = 0, adsp: bool = False, engine=None,
                 vep_output: bool = False, identity_only=None, allele_frequencies: bool = False, dbsnp: bool = False):
        from .engine import VepRowsTable, default_engine
        if engine is None:
            engine = table.engine if isinstance(table, VepRowsTable) else default_engine()
        self._engine = engine
        if not isinstance(table, VepRowsTable):
            if ranking is None:
                raise ValueError("a ranking is needed to build the table")
            # identityOnly=self.is_adsp() (vep_variant_loader.py:269)
            identity_only = bool(adsp) if identity_only is None else bool(identity_only)
            table = engine.vep_rows_table_build(table, ranking, vep_output=vep_output, identity_only=identity_only,
                                                allele_frequencies=allele_frequencies, match_refsnp=bool(dbsnp))
        elif vep_output and table.cleaned is None:
            raise ValueError("the table was built without vep_output")
        elif allele_frequencies and table.freq is None:
            raise ValueError("the table was built without allele_frequencies")
        self._vep_output = table.cleaned is not None
        self._allele_frequencies = table.freq is not None
        self._table = table
        self._alg_id, self._adsp = int(alg_id), bool(adsp)
        self._counters = {"line": table.counts["lines"], "variant": table.n_rows, "update": 0, "duplicates": 0,
                          "skipped": 0, "not_annotated": 0}
        self._update_buffer: List[tuple] = []
        self._export_rows: List[tuple] = []  # (index in _update_buffer they stand before, rows, text)

    def table(self):
        return self._table

    def get_count(self, counter):
        return self._counters[counter]

    def increment_counter(self, counter):
        self._counters[counter] += 1

    def update_sql(self) -> str:
        return update_sql(self._adsp, self._vep_output, self._allele_frequencies)

    def update_buffer(self, sizeOnly=False):
        """The buffered tuples (rows from :meth:`buffer_export` are split into tuples at the first
        call that asks for them)."""
        if sizeOnly:
            return len(self._update_buffer) + sum(n for _, n, _ in self._export_rows)
        for at, _, text in reversed(self._export_rows):
            rows = text.decode("utf-8", "surrogateescape").split("\n")[:-1]
            self._update_buffer[at:at] = [tuple(r.split("\t")) for r in rows]
        self._export_rows = []
        return self._update_buffer

    def update_text(self) -> bytes:
        """The buffered rows as text, tab-separated and ``<LF>``-ended, in buffer order."""
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
        """The update rows of a whole export (:meth:`Engine.vep_update_rows`):
        ``record_primary_key<TAB>metaseq_id<TAB>vep_output`` lines, the third column NULL as ``\\N``,
        empty or absent, given as a path (plain, gzip or bgzip) or as text.  Moves ``update``,
        ``skipped`` (the reference's ``duplicates``, moved as well) and ``not_annotated``; returns the
        number of rows appended."""
        if isinstance(path_or_text, str):
            from . import bgzf
            path_or_text = bgzf.read_whole(path_or_text, self._engine)
        rows = self._engine.vep_update_rows(path_or_text, self._table, self._alg_id, adsp=self._adsp,
                                            update_existing=update_existing, contigs=contigs)
        for name, k in (("update", rows.n), ("skipped", rows.counts["skipped"]),
                        ("duplicates", rows.counts["skipped"]), ("not_annotated", rows.counts["not_annotated"])):
            self._counters[name] += k
        if rows.n:
            self._export_rows.append((len(self._update_buffer), rows.n, rows.text.cpu().numpy().tobytes()))
        return rows.n

    def unmatched(self) -> List[str]:
        """The metaseq ids of the table no export row has matched so far, in file order (an id two
        lines carry once; its last line is the one that answers)."""
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

    def unranked(self) -> List[tuple]:
        """The lines that need a re-rank and gave no rows: ``(line number, id, combination)``."""
        return list(self._table.unranked)

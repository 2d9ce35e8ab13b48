"""Annotation update rows from a tab-delimited file, without a database — the counterpart of
``Load/bin/update_variant_annotation.py`` on ``TextVariantLoader``
(``Util/lib/python/loaders/txt_variant_loader.py``).

The reference reads the file with ``csv.DictReader(fh, delimiter='\\t')``: one column is named
``variant`` and holds a primary key, a metaseq id or a refSNP id (``--variantIdType``); every other
header column is a column of ``AnnotatedVDB.Variant`` to overwrite (``jsonb_merge`` for the JSONB
ones).  Per line it looks the id up in the database (not for primary keys) and appends the tuple
``(record_primary_key, 'chr' + c, value, ...[, True])`` (``__buffer_update_values``, ``:190-208``),
a value that is exactly ``NULL`` as ``None``.  Here an export of the table stands in for the
database, as for the other update passes:

* K19a, :meth:`Engine.txt_table_build`: the file -> a device table of its data lines, the looked-up
  ids hashed (K6), the update values rendered once per line;
* K19b, :meth:`Engine.txt_update_rows`: the export
  (``record_primary_key<TAB>metaseq_id<TAB>ref_snp_id``) streamed against that table -> the update
  rows as text;
* K19c, :meth:`Engine.txt_direct_rows`: a file of primary keys -> its rows, with neither.

For refSNP ids the reference looks up ``record['ref_snp_id']``, not ``record['variant']``
(``set_current_variant:177-178``): such a file needs a ``ref_snp_id`` column, which is also an
update field.  :class:`TextUpdater` carries the reference loader's observable surface for this pass;
:func:`host_line` is the one Python path of a line the device leaves to the host.  Deviations are
listed in DESIGN.md (K19).
"""

from __future__ import annotations

import csv
from typing import List, Optional, Tuple

from . import _native as N
from .loaders import ALLOWABLE_COPY_FIELDS  # noqa: F401 (the driver's check)

VARIANT_ID_TYPES = ["PRIMARY_KEY", "METASEQ", "REFSNP"]  # AnnotatedVDB.Util.database
# the jsonb columns of AnnotatedVDB.Variant among the allowable ones: an update merges into them
_JSONB_COLUMNS = frozenset(("adsp_most_severe_consequence", "adsp_qc", "adsp_ranked_consequences", "allele_frequencies",
                            "display_attributes", "gwas_flags", "loss_of_function", "other_annotation", "vep_output"))
# one SET item per column kind; {c}: the column
_SET_ITEM = {"jsonb": "{c} = jsonb_merge(COALESCE(v.{c} ,'{{}}'::jsonb), d.{c}::jsonb)",
             "ltree": "{c} = d.{c}::ltree",
             "plain": "{c} = d.{c}"}
_MATCH_PK = "v.record_primary_key = d.record_primary_key"
_MATCH_LEGACY_PK = ("LEFT(v.metaseq_id, 50) = split_part(d.record_primary_key, '_', 1) "
                    "AND (v.ref_snp_id = split_part(d.record_primary_key, '_', 2) "
                    "OR (v.ref_snp_id IS NULL AND split_part(d.record_primary_key, '_', 2) = ''))")
HEADER_WINDOW = 1 << 16  # the header is read from this many leading bytes of the slab


def read_header(head: bytes, variant_id_type: str = "METASEQ", text_bytes: Optional[int] = None):
    """The header of a file from its leading bytes, as ``csv.DictReader`` takes it (the first row
    ``csv`` returns) -> :class:`~annotatedvdb_amd.engine.TxtHeader`.  ``ValueError``: no header, no
    ``variant`` column (``updateFields.remove('variant')``), no other column, more than
    ``N.TXT_MAX_FIELDS`` columns, a name twice, no ``ref_snp_id`` column for refSNP ids."""
    from .engine import TxtHeader
    if variant_id_type not in VARIANT_ID_TYPES:
        raise ValueError(f"variant id type {variant_id_type!r}: one of {VARIANT_ID_TYPES}")
    lines = head.split(b"\n")
    if len(lines) == 1 and text_bytes is not None and text_bytes > len(head):
        raise ValueError(f"no line end in the first {len(head)} bytes: not a header")
    if not head:
        raise ValueError("an empty file has no header")
    reader = _rows((ln[:-1] if ln.endswith(b"\r") else ln).decode("utf-8") for ln in lines)
    fields = next(reader)
    if "variant" not in fields:
        raise ValueError(f"the header {fields!r} has no column 'variant'")
    if len(fields) < 2:
        raise ValueError("the header names no column to update beside 'variant'")
    if len(fields) > N.TXT_MAX_FIELDS:
        raise ValueError(f"the header has {len(fields)} columns ({N.TXT_MAX_FIELDS} are taken)")
    if len(set(fields)) != len(fields):
        raise ValueError(f"the header {fields!r} names a column twice")
    id_col = key_col = fields.index("variant")
    if variant_id_type == "REFSNP":
        if "ref_snp_id" not in fields:
            raise ValueError("refSNP ids are looked up by the column 'ref_snp_id' (set_current_variant), which the "
                             f"header {fields!r} lacks")
        key_col = fields.index("ref_snp_id")
    return TxtHeader(fields, reader.line_num, id_col, key_col)


def _rows(lines):
    """``csv.reader`` as ``update_annotation`` sets it up: the one place the dialect is chosen."""
    return csv.reader(lines, delimiter="\t")


def host_line(line: bytes, header) -> Tuple[bytes, Optional[bytes], bytes]:
    """One data line as the reference's loop treats it (``csv``, ``set_current_variant``,
    ``__buffer_update_values``): ``(looked-up id, chromosome label or None, update values)`` — the
    label is the ``variant`` field up to its first ``:``, ``None`` when it has none (the
    chromosome then comes from the primary key); the values are tab-joined, ``\\N`` for ``NULL``
    and for a field the row lacks.  Raises ``TypeError`` for a row without its ``variant`` field
    (the reference's ``':' in None``), ``ValueError`` for bytes that are not UTF-8, an empty or
    absent looked-up field, and a value the row text cannot carry: exactly ``\\N``, or holding a
    tab or a line end (a quoted field)."""
    if line.endswith(b"\r"):
        line = line[:-1]
    text = line.decode("utf-8")
    row = next(_rows([text]))
    n = len(header.fields)
    rec = list(row[:n]) + [None] * (n - len(row))
    variant = rec[header.id_col]
    if variant is None:
        raise TypeError("argument of type 'NoneType' is not iterable")  # ':' in variantId
    key = rec[header.key_col]
    if not key:
        raise ValueError(f"no {header.fields[header.key_col]!r} to look the row up by")
    values = []
    for f, v in enumerate(rec):
        if v is not None and (v == "\\N" or "\t" in v or "\n" in v or "\r" in v):
            raise ValueError(f"column {header.fields[f]!r} holds {v!r}, which the row text cannot carry")
        if f != header.id_col:
            values.append("\\N" if v is None or v == "NULL" else v)
    label = variant.split(":")[0].encode("utf-8") if ":" in variant else None
    return key.encode("utf-8"), label, "\t".join(values).encode("utf-8")


def update_sql(columns, adsp: bool = False, legacy_pk: bool = False) -> str:
    """``UPDATE ... FROM (VALUES %s)`` over ``(record_primary_key, chromosome, *columns[,
    is_adsp_variant])``: a jsonb column is merged, ``bin_index`` cast to ``ltree``, any other
    overwritten; ``legacy_pk`` matches rows of the ``Public`` schema by the parts of a legacy key."""
    kind = lambda c: "jsonb" if c in _JSONB_COLUMNS else "ltree" if c == "bin_index" else "plain"  # noqa: E731
    sets = ", ".join(_SET_ITEM[kind(c)].format(c=c) for c in columns) + " "
    values = ["record_primary_key", "chromosome", *columns]
    if adsp:
        sets += ", v.is_adsp_variant = d.is_adsp_variant "
        values.append("is_adsp_variant")
    return (f"UPDATE {'Public' if legacy_pk else 'AnnotatedVDB'}.Variant v SET {sets}"
            f"FROM (VALUES %s) AS d({','.join(values)}) "
            f"WHERE v.chromosome = d.chromosome AND {_MATCH_LEGACY_PK if legacy_pk else _MATCH_PK}")


def read_file_header(path: str, variant_id_type: str = "METASEQ"):
    """The header of the file at ``path`` (plain, gzip or bgzip) from its first bytes alone, so
    that a file with a bad header is refused before it is read whole."""
    import gzip
    with open(path, "rb") as fh:
        packed = fh.read(2) == b"\x1f\x8b"
    with (gzip.open(path, "rb") if packed else open(path, "rb")) as fh:
        head = fh.read(HEADER_WINDOW)
        more = fh.read(1)
    return read_header(head, variant_id_type, len(head) + len(more))


class TextUpdater(object):
    """The reference loader's observable surface for the generic annotation pass, batch-wise and
    without a database, in the mould of :class:`~annotatedvdb_amd.snpeff_lof.LOFUpdater`: counters
    and the update buffer of ``(record_primary_key, 'chr' + c, value, ...[, True])`` tuples that
    ``execute_values(cursor, update_sql, buffer)`` takes.  ``path_or_text``: the file as a path
    (plain, gzip or bgzip) or text; ``datasource`` ``ADSP`` appends ``is_adsp_variant``."""

    def __init__(self, path_or_text, variant_id_type: str, datasource: str = "dbSNP", engine=None):
        from .engine import default_engine
        if variant_id_type not in VARIANT_ID_TYPES:
            raise ValueError(f"variant id type {variant_id_type!r}: one of {VARIANT_ID_TYPES}")
        self._engine = engine if engine is not None else default_engine()
        if isinstance(path_or_text, str):
            from . import bgzf
            path_or_text = bgzf.read_whole(path_or_text, self._engine)
        self._text = self._engine._as_text(path_or_text)
        self._id_type = variant_id_type
        self._adsp = str(datasource).lower() == "adsp"
        self._table = None
        if variant_id_type == "PRIMARY_KEY":
            self._header = read_header(self._text[:HEADER_WINDOW].cpu().numpy().tobytes(), variant_id_type,
                                       self._text.numel())
            lines = 0
        else:
            self._table = self._engine.txt_table_build(self._text, variant_id_type)
            self._header = self._table.header
            lines = self._table.counts["entries"]
        self._counters = {"line": lines, "variant": 0, "duplicates": 0, "update": 0, "skipped": 0, "not_in_file": 0}
        self._update_buffer: List[tuple] = []
        self._export_rows: List[tuple] = []  # (index in _update_buffer they stand before, rows, text)
        self._update_sql = None

    def table(self):
        return self._table

    def header(self):
        return self._header

    def is_adsp(self):
        return self._adsp

    def update_fields(self) -> List[str]:
        """The header's columns without ``variant``, in header order."""
        return [f for i, f in enumerate(self._header.fields) if i != self._header.id_col]

    def build_update_sql(self, useLegacyPk=False) -> str:
        """The statement ``execute_values`` runs over the update buffer: the text the reference's
        ``build_update_sql`` gives for the same header, datasource and flag (pinned by the golden)."""
        self._update_sql = update_sql(self.update_fields(), self._adsp, bool(useLegacyPk))
        return self._update_sql

    def get_count(self, counter):
        return self._counters[counter]

    def increment_counter(self, counter):
        self._counters[counter] += 1

    def _tuple(self, row: str) -> tuple:
        t = tuple(None if v == "\\N" else v for v in row.split("\t"))
        return t[:-1] + (True,) if self._adsp else t

    def update_buffer(self, sizeOnly=False):
        """The buffered tuples, ``None`` for ``\\N`` and ``True`` for the ADSP flag (rows from
        :meth:`buffer_export` / :meth:`buffer_file` are split into tuples at the first call that
        asks for them)."""
        if sizeOnly:
            return len(self._update_buffer) + sum(n for _, n, _ in self._export_rows)
        for at, _, text in reversed(self._export_rows):
            rows = text.decode("utf-8", "surrogateescape").split("\n")[:-1]
            self._update_buffer[at:at] = [self._tuple(r) for r in rows]
        self._export_rows = []
        return self._update_buffer

    def update_text(self) -> bytes:
        """The buffered rows as text, ``pk<TAB>chrom<TAB>values[<TAB>true]<LF>`` each, in buffer order."""
        def line(t):
            return "\t".join("\\N" if v is None else "true" if v is True else v for v in t) + "\n"
        parts, done = [], 0
        for at, _, text in self._export_rows + [(len(self._update_buffer), 0, b"")]:
            parts += [line(t).encode("utf-8", "surrogateescape") for t in self._update_buffer[done:at]]
            parts.append(text)
            done = at
        return b"".join(parts)

    def reset_update_buffer(self):
        self._update_buffer = []
        self._export_rows = []

    def _append(self, rows) -> int:
        for name in ("variant", "duplicates", "update"):
            self._counters[name] += rows.n
        if rows.n:
            self._export_rows.append((len(self._update_buffer), rows.n, rows.text.cpu().numpy().tobytes()))
        return rows.n

    def buffer_export(self, path_or_text, contigs=None) -> int:
        """The update rows of a whole export (K19b, :meth:`Engine.txt_update_rows`):
        ``record_primary_key<TAB>metaseq_id<TAB>ref_snp_id`` lines, given as a path (plain, gzip or
        bgzip) or as text.  Moves ``variant``, ``duplicates``, ``update`` and ``not_in_file``;
        returns the number of rows appended.  A file of primary keys needs no export:
        :meth:`buffer_file`."""
        if self._table is None:
            raise ValueError("a file of primary keys needs no export: buffer_file()")
        if isinstance(path_or_text, str):
            from . import bgzf
            path_or_text = bgzf.read_whole(path_or_text, self._engine)
        rows = self._engine.txt_update_rows(path_or_text, self._table, self._id_type, adsp=self._adsp, contigs=contigs)
        self._counters["not_in_file"] += rows.counts["not_in_file"]
        return self._append(rows)

    def buffer_file(self) -> int:
        """The update rows of a file of primary keys (K19c, :meth:`Engine.txt_direct_rows`), in
        file order; returns the number of rows appended."""
        if self._table is not None:
            raise ValueError(f"{self._id_type} ids are looked up in an export: buffer_export()")
        rows = self._engine.txt_direct_rows(self._text, adsp=self._adsp)
        self._counters["line"] += rows.n
        return self._append(rows)

    def _id_groups(self):
        """Per table row, on the table's device: (the last row of its id, the first row of its id,
        the rows of its id).  The device's answer is K6's: every key probed in the table's own key
        set, which holds the keys in reverse row order and keeps the first of equal ones."""
        import torch
        t, n = self._table, self._table.n_rows
        rows = torch.arange(n, dtype=torch.int64, device=t.keys.device)
        if self._engine.host_only:  # (the host engine has no probe entry: the keys one by one)
            off, blob, seen = t.key_off.numpy(), t.keys.numpy().tobytes(), {}
            for r in range(n):
                seen[blob[off[r]:off[r + 1]]] = r
            last = torch.tensor([seen[blob[off[r]:off[r + 1]]] for r in range(n)], dtype=torch.int64)
        else:
            match = self._engine.keyset_probe_text(t.keyset, t.rkeys, t.rkey_off, t.keys, t.key_off, n)
            last = n - 1 - match.long()
        first = torch.full((n,), n, dtype=torch.int64, device=rows.device).scatter_reduce(0, last, rows, "amin")
        count = torch.zeros(n, dtype=torch.int64, device=rows.device).scatter_add(0, last, torch.ones_like(rows))
        return rows, last, first, count

    def _ids_of(self, pick, first) -> List[str]:
        """The ids of the rows ``pick`` (a mask), ordered by ``first``: only their bytes come to the host."""
        import torch
        t = self._table
        sel = torch.nonzero(pick).flatten()
        sel = sel[torch.argsort(first[sel])]
        if sel.numel() == 0:
            return []
        start, length = t.key_off[sel], t.key_off[sel + 1] - t.key_off[sel]
        blob = t.keys[self._engine._spans(start, length)].cpu().numpy().tobytes()
        out, at = [], 0
        for k in length.tolist():
            out.append(blob[at:at + k].decode("utf-8", "surrogateescape"))
            at += k
        return out

    def unmatched(self) -> List[str]:
        """The ids of the file no export row has matched so far, in file order (an id the file
        repeats once, where it first stands; its last line is the one that answers).  None for a
        file of primary keys.  The rows are picked on the device; only these ids come to the host."""
        if self._table is None or self._table.n_rows == 0:
            return []
        rows, last, first, _ = self._id_groups()
        return self._ids_of((last == rows) & (self._table.hit == 0), first)

    def repeated_ids(self) -> List[str]:
        """The ids the file holds more than once, in file order of their first line (picked on the
        device, as :meth:`unmatched`)."""
        if self._table is None or self._table.n_rows == 0:
            return []
        rows, last, first, count = self._id_groups()
        return self._ids_of((last == rows) & (count > 1), first)

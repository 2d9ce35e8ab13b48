"""Annotation update rows from a tab-delimited file — the counterpart of
``Load/bin/update_variant_annotation.py``, with an export of ``AnnotatedVDB.Variant`` in place of the
database (:mod:`annotatedvdb_amd.text_update`).

    python -m annotatedvdb_amd.update_variant_annotation --fileName gwas_flags.txt.gz \\
        --variantIdType METASEQ --export variant_export.tsv.gz [--datasource ADSP] \\
        [--outDir out] [--existingContigs 1,2] [--allowMissing]

``--fileName``, ``--variantIdType`` and ``--datasource`` are the reference's.  ``--export`` is
``COPY (SELECT record_primary_key, metaseq_id, ref_snp_id FROM AnnotatedVDB.Variant) TO ...`` (plain,
gzip or bgzip; a bgzip file is inflated on the GPU, K11); a file of primary keys needs none.
``--existingContigs`` keeps only the export rows of these chromosomes.  Written to ``--outDir``
(default: beside the file): ``<file>.updates``, the rows
``record_primary_key<TAB>chromosome<TAB>value...`` that ``execute_values(cursor, update_sql, ...)``
takes as tuples (``\\N`` for NULL), and ``<file>.update.sql``, the reference's UPDATE statement.
Header columns that are no column of the table (``ALLOWABLE_COPY_FIELDS``) are refused by name.  Ids
the export lacks go to ``<file>.unmatched`` and the run ends non-zero unless ``--allowMissing`` (the
reference can only raise there: inserting them is out of scope, as are ``--resumeAfter``,
``--failAt`` and ``--useDynamicPkSql``).
"""

from __future__ import annotations

import argparse
import os
import sys
from typing import Dict, Optional, Sequence

from .text_update import ALLOWABLE_COPY_FIELDS, VARIANT_ID_TYPES, TextUpdater, read_file_header


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="update rows of AnnotatedVDB.Variant from a "
                                 "tab-delimited file and an export of the table, on one GPU")
    ap.add_argument("--fileName", required=True, help="the tab-delimited file (plain, gzip or bgzip)")
    ap.add_argument("--variantIdType", required=True, choices=VARIANT_ID_TYPES)
    ap.add_argument("--export", help="record_primary_key<TAB>metaseq_id<TAB>ref_snp_id export (not for PRIMARY_KEY)")
    ap.add_argument("--datasource", choices=["dbSNP", "DBSNP", "dbsnp", "ADSP", "NIAGADS", "EVA"], default="dbSNP",
                    help="variant source: dbSNP, NIAGADS, ADSP, or EVA (European Variant Archive")
    ap.add_argument("--outDir", help="receives the outputs (default: the file's directory)")
    ap.add_argument("--existingContigs", help="comma separated chromosomes whose export rows to keep")
    ap.add_argument("--allowMissing", action="store_true", help="go on when an id of the file is not in the export")
    args = ap.parse_args(argv)
    if args.variantIdType != "PRIMARY_KEY" and not args.export:
        ap.error("--export is required unless --variantIdType is PRIMARY_KEY")
    return args


def main(argv: Optional[Sequence[str]] = None, engine=None) -> Dict[str, int]:
    """Runs the pass; returns the counters (``line``, ``update``, ``not_in_file``, ``missing``,
    ``repeated``).  With ids missing and no ``--allowMissing`` only ``<file>.unmatched`` is written."""
    args = parse_args(argv)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    header = read_file_header(args.fileName, args.variantIdType)  # (the first bytes only: a bad file is refused at once)
    refused = [f for f in header.fields if f != "variant" and f not in ALLOWABLE_COPY_FIELDS]
    if refused:
        raise ValueError("no column(s) of AnnotatedVDB.Variant: " + ", ".join(refused))
    updater = TextUpdater(args.fileName, args.variantIdType, args.datasource, engine)
    if args.variantIdType == "PRIMARY_KEY":
        updater.buffer_file()
    else:
        contigs = [c.replace("chr", "") for c in args.existingContigs.split(",")] if args.existingContigs else None
        updater.buffer_export(args.export, contigs=contigs)
    missing = updater.unmatched()
    base = os.path.join(args.outDir or os.path.dirname(os.path.abspath(args.fileName)), os.path.basename(args.fileName))
    if args.outDir:
        os.makedirs(args.outDir, exist_ok=True)
    if missing:
        with open(base + ".unmatched", "w", encoding="utf-8", errors="surrogateescape") as fh:
            fh.write("".join(m + "\n" for m in missing))
    if not missing or args.allowMissing:
        with open(base + ".updates", "wb") as fh:
            fh.write(updater.update_text())
        with open(base + ".update.sql", "w", encoding="utf-8") as fh:
            fh.write(updater.build_update_sql() + "\n")
    return {"line": updater.get_count("line"), "update": updater.get_count("update"),
            "not_in_file": updater.get_count("not_in_file"), "missing": len(missing),
            "repeated": len(updater.repeated_ids())}


def cli(argv: Optional[Sequence[str]] = None, engine=None) -> int:
    """The exit status of a run: 1 when ids of the file are missing from the export and
    ``--allowMissing`` was not given."""
    allow = "--allowMissing" in (sys.argv[1:] if argv is None else argv)
    return 1 if main(argv, engine)["missing"] and not allow else 0


if __name__ == "__main__":
    sys.exit(cli())

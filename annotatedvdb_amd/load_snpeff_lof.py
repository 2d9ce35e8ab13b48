"""``loss_of_function`` update rows from a SnpEff VCF — the counterpart of
``Load/bin/load_snpeff_lof.py``, with an export of ``AnnotatedVDB.Variant`` in place of the
database (:mod:`annotatedvdb_amd.snpeff_lof`).

    python -m annotatedvdb_amd.load_snpeff_lof --fileName chr1_1.snpeff.vcf.gz \\
        --export variant_export.tsv.gz --outFile lof_rows.tsv [--updateExistingValues] \\
        [--existingContigs 1,2] [--skipMissing]

``--fileName`` and ``--updateExistingValues`` are the reference's.  ``--export`` is
``COPY (SELECT record_primary_key, metaseq_id, loss_of_function FROM AnnotatedVDB.Variant) TO ...``
(plain, gzip or bgzip; a bgzip file is inflated on the GPU, K11); ``--existingContigs`` keeps only
the export rows of these chromosomes, so one whole-table export serves every per-chromosome VCF.
``--outFile`` receives the rows ``record_primary_key<TAB>chromosome<TAB>json`` that
``execute_values(cursor, update_sql, ...)`` takes as tuples.  An annotated variant no export row
matches ends the run, before anything is written, with the reference's
``ValueError('Variant not found in the database')`` (``generate_update_values:140-141``) naming the
first one; ``--skipMissing`` goes on without them.
"""

from __future__ import annotations

import argparse
from typing import Dict, Optional, Sequence


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="loss_of_function update rows from a SnpEff VCF "
                                 "and an export of AnnotatedVDB.Variant, on one GPU")
    ap.add_argument("--fileName", required=True, help="the VCF SnpEff wrote (plain, gzip or bgzip)")
    ap.add_argument("--export", required=True, help="record_primary_key<TAB>metaseq_id<TAB>loss_of_function export")
    ap.add_argument("--outFile", required=True, help="receives the update rows")
    ap.add_argument("--updateExistingValues", action="store_true",
                    help="update fields even if value exists; if flag not specificed will skip records that already "
                         "have values")
    ap.add_argument("--existingContigs", help="comma separated chromosomes whose export rows to keep")
    ap.add_argument("--skipMissing", action="store_true", help="go on when an annotated variant is not in the export")
    return ap.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None, engine=None) -> Dict[str, int]:
    """Runs the pass; returns the counters (``update``, ``skipped``, ``not_annotated``, ``missing``)."""
    args = parse_args(argv)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    from .snpeff_lof import LOFUpdater
    updater = LOFUpdater(args.fileName, engine)
    contigs = [c.replace("chr", "") for c in args.existingContigs.split(",")] if args.existingContigs else None
    updater.buffer_export(args.export, update_existing=args.updateExistingValues, contigs=contigs)
    missing = updater.unmatched()
    if missing and not args.skipMissing:
        err = ValueError("Variant not found in the database")
        if hasattr(err, "add_note"):
            err.add_note(f"{missing[0]} ({len(missing)} annotated variant(s) without an export row)")
        err.variant = missing[0]
        raise err
    with open(args.outFile, "wb") as fh:
        fh.write(updater.update_text())
    return {"update": updater.get_count("update"), "skipped": updater.get_count("skipped"),
            "not_annotated": updater.get_count("not_annotated"), "missing": len(missing)}


if __name__ == "__main__":
    main()

"""``is_adsp_variant`` / ``adsp_qc`` update rows from an ADSP QC pVCF — the counterpart of
``Load/bin/update_from_qc_pvcf_file.py``, with an export of ``AnnotatedVDB.Variant`` in place of
the database (:mod:`annotatedvdb_amd.adsp_qc`).

    python -m annotatedvdb_amd.update_from_qc_pvcf_file --fileName chr1.qc.vcf.gz --version 17K \\
        --export variant_export.tsv.gz --outFile qc_rows.tsv [--updateExistingValues] \\
        [--vcfHeaderFields '#CHROM,POS,...'] [--novelOut novel.vcf]

``--fileName``, ``--version``, ``--updateExistingValues`` and ``--vcfHeaderFields`` are the
reference's.  ``--export`` is
``COPY (SELECT record_primary_key, metaseq_id, annotation->'adsp_qc' FROM AnnotatedVDB.Variant) TO ...``
(plain, gzip or bgzip; a bgzip file is inflated on the GPU, K11).  ``--outFile`` receives the rows
``record_primary_key<TAB>chromosome<TAB>true|\\N<TAB>json`` that
``execute_values(cursor, update_sql, ...)`` takes as tuples for the fields ``is_adsp_variant`` and
``adsp_qc``.  The lines of the QC file whose variants no export row matches (the ones the
reference would insert) go to ``--novelOut`` as a VCF that ``load_vcf_file`` takes; without it
they are only counted.
"""

from __future__ import annotations

import argparse
from typing import Dict, Optional, Sequence


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="is_adsp_variant / adsp_qc update rows from an ADSP "
                                 "QC pVCF and an export of AnnotatedVDB.Variant, on one GPU")
    ap.add_argument("--fileName", required=True, help="the QC pVCF (plain, gzip or bgzip)")
    ap.add_argument("--export", required=True, help="record_primary_key<TAB>metaseq_id<TAB>adsp_qc export")
    ap.add_argument("--version", required=True, help="release version, e.g., 17K")
    ap.add_argument("--outFile", required=True, help="receives the update rows")
    ap.add_argument("--updateExistingValues", action="store_true",
                    help="update fields even if value exists; if flag not specificed will skip records that already "
                         "have values")
    ap.add_argument("--vcfHeaderFields", help="comma separated list of fields to include",
                    default="#CHROM,POS,ID,REF,ALT,QUAL,FILTER,INFO,FORMAT")
    ap.add_argument("--novelOut", help="receives the lines whose variants are not in the export, as a VCF")
    return ap.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None, engine=None) -> Dict[str, int]:
    """Runs the pass; returns the counters (``line``, ``update``, ``skipped``, ``not_in_vcf``, ``novel``)."""
    args = parse_args(argv)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    from .adsp_qc import QCUpdater
    fields = args.vcfHeaderFields.split(",")
    updater = QCUpdater(args.fileName, args.version, engine, header_fields=fields)
    updater.buffer_export(args.export, update_existing=args.updateExistingValues)
    novel = updater.novel_lines()
    with open(args.outFile, "wb") as fh:
        fh.write(updater.update_text())
    if args.novelOut:
        with open(args.novelOut, "wb") as fh:
            fh.write("\t".join(fields).encode("utf-8") + b"\n")
            for line in novel:
                fh.write(line + b"\n")
    return {"line": updater.get_count("line"), "update": updater.get_count("update"),
            "skipped": updater.get_count("skipped"), "not_in_vcf": updater.get_count("not_in_vcf"),
            "novel": len(novel)}


if __name__ == "__main__":
    main()

"""``adsp_most_severe_consequence`` / ``adsp_ranked_consequences`` update rows from VEP's JSON output —
the counterpart of ``Load/bin/load_vep_result.py`` for these two columns (K18b) and, with ``--vepOutput``,
for ``vep_output`` (K18c) and with ``--alleleFrequencies`` for ``allele_frequencies`` (K18d), with an export of ``AnnotatedVDB.Variant`` in place of the database
(:mod:`annotatedvdb_amd.vep_rows`).

    python -m annotatedvdb_amd.load_vep_result --fileName chr1.vep.json.gz --rankingFile ranking.txt \\
        --export variant_export.tsv.gz --outFile vep_rows.tsv --algInvocationId 42 [--datasource ADSP] \\
        [--updateExisting] [--existingContigs 1,2] [--skipMissing] [--vepOutput] [--alleleFrequencies]

``--fileName``, ``--rankingFile``, ``--updateExisting`` and ``--datasource`` are the reference's.
``--export`` is ``COPY (SELECT record_primary_key, metaseq_id, vep_output FROM AnnotatedVDB.Variant)
TO ...`` (plain, gzip or bgzip); ``--existingContigs`` keeps only the export rows of these
chromosomes.  ``--outFile`` receives the rows ``record_primary_key<TAB>chromosome[<TAB>allele_frequencies]<TAB>most
severe<TAB>ranked[<TAB>vep_output]<TAB>row_algorithm_id[<TAB>true]`` (``vep_output``, the cleaned result, with
``--vepOutput``; its ``input`` has the five identity fields for ``--datasource ADSP``, else all eight;
``allele_frequencies`` with ``--alleleFrequencies``: the element of ``colocated_variants`` is matched by the
variant's refSNP id for ``--datasource dbSNP``, and INFO ``FREQ`` is merged in unless the datasource is ADSP;
with both switches the rows are the reference's full ``updateValues`` and the statement its full one) that ``execute_values(cursor, update_sql, ...)``
takes as tuples, ``<outFile>.update.sql`` the statement, ``<outFile>.unranked`` the lines that need a
re-rank (``line<TAB>id<TAB>combination``; the run then ends with exit code 2).  A variant of the
file no export row matches ends the run, before anything is written, with the reference's
``KeyError`` (``__get_variant_primary_key``); ``--skipMissing`` goes on without them.
"""

from __future__ import annotations

import argparse
import sys
from typing import Optional, Sequence


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="VEP consequence update rows from VEP JSON and an "
                                 "export of AnnotatedVDB.Variant, on one GPU")
    ap.add_argument("--fileName", required=True, help="VEP --json output (plain, gzip or bgzip)")
    ap.add_argument("-r", "--rankingFile", required=True, help="full path to ADSP VEP consequence ranking file")
    ap.add_argument("--export", required=True, help="record_primary_key<TAB>metaseq_id<TAB>vep_output export")
    ap.add_argument("--outFile", required=True, help="receives the update rows")
    ap.add_argument("--updateExisting", action="store_true", help="update existing annotated results")
    ap.add_argument("--datasource", choices=["dbSNP", "DBSNP", "dbsnp", "ADSP", "NIAGADS", "EVA"], default="dbSNP",
                    help="variant source: dbSNP, NIAGADS, ADSP, or EVA")
    ap.add_argument("--algInvocationId", type=int, default=0, help="row_algorithm_id of the update rows")
    ap.add_argument("--existingContigs", help="comma separated chromosomes whose export rows to keep")
    ap.add_argument("--skipMissing", action="store_true", help="go on when a variant of the file is not in the export")
    ap.add_argument("--vepOutput", action="store_true", help="add the vep_output column (the cleaned result)")
    ap.add_argument("--alleleFrequencies", action="store_true",
                    help="add the allele_frequencies column (colocated_variants frequencies and INFO FREQ)")
    ap.add_argument("--device", default=None, help="GPU index, or 'host'")
    return ap.parse_args(argv)


def main(argv: Optional[Sequence[str]] = None, engine=None) -> int:
    """Runs the pass; returns the exit code (2: lines that need a re-rank were left out)."""
    args = parse_args(argv)
    if engine is None:
        from .engine import Engine
        engine = Engine(args.device if args.device in (None, "host") else int(args.device))
    from .vep_rows import VEPUpdater
    updater = VEPUpdater(args.fileName, args.rankingFile, alg_id=args.algInvocationId,
                         adsp=args.datasource.lower() == "adsp", engine=engine, vep_output=args.vepOutput,
                         allele_frequencies=args.alleleFrequencies, dbsnp=args.datasource.lower() == "dbsnp")
    contigs = [c.replace("chr", "") for c in args.existingContigs.split(",")] if args.existingContigs else None
    updater.buffer_export(args.export, update_existing=args.updateExisting, contigs=contigs)
    missing = updater.unmatched()
    if missing and not args.skipMissing:
        err = KeyError("No record for variant %s found in DB.  VEP Variant Loader does updates only.", missing[0])
        if hasattr(err, "add_note"):
            err.add_note(f"{len(missing)} variant(s) of the file without an export row")
        err.variant = missing[0]
        raise err
    with open(args.outFile, "wb") as fh:
        fh.write(updater.update_text())
    with open(args.outFile + ".update.sql", "w") as fh:
        fh.write(updater.update_sql() + "\n")
    unranked = updater.unranked()
    with open(args.outFile + ".unranked", "w") as fh:
        for line, vid, comb in unranked:
            print(line, vid, comb, sep="\t", file=fh)
    print(f"{updater.get_count('line')} lines, {updater.table().counts['host_lines']} on the host, "
          f"{updater.get_count('update')} rows, {updater.get_count('skipped')} skipped, "
          f"{updater.get_count('not_annotated')} not in the file, {len(missing)} missing, {len(unranked)} unranked",
          file=sys.stderr)
    return 2 if unranked else 0


if __name__ == "__main__":
    sys.exit(main())

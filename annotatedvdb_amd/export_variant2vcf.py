"""VCF export driver — the counterpart of ``Util/bin/export_variant2vcf.py``.

The reference runs, per chromosome, ``SELECT record_primary_key, metaseq_id,
row_algorithm_id FROM AnnotatedVDB.Variant WHERE chromosome = %s`` (``SELECT_SQL``,
``:23``) on one host thread each, and writes the records as ``chrN_<k>.vcf`` files of
10,000,000 variants with ID set to the primary key, the records whose metaseq id holds
a symbolic allele to ``chrN_invalid.txt`` (``run``, ``:38-102``).  Here the records come
from an export of those three columns (``COPY (SELECT record_primary_key, metaseq_id,
row_algorithm_id FROM AnnotatedVDB.Variant) TO STDOUT``; one whole-table export serves
every chromosome), and per chromosome the export's rows of that contig become the text of
the files on the GPU (K14, ``Engine.export_vcf``).

    python -m annotatedvdb_amd.export_variant2vcf --export variants.tsv.gz --chr all -o out

There is no database here: ``--gusConfigFile`` is refused.  ``--maxWorkers`` is accepted
and ignored (one process, one GPU).  ``--chr`` takes ``all``, ``autosome`` or a comma
separated list, as ``load_cadd_scores`` does.
"""

from __future__ import annotations

import argparse
import os
from typing import Dict, Optional, Sequence

from .load_cadd_scores import chromosome_list

VARIANTS_PER_FILE = 10000000  # export_variant2vcf.py:24


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="VCF files of the variants of an export of "
                                 "AnnotatedVDB.Variant, on one GPU")
    ap.add_argument("--export", required=True,
                    help="export of AnnotatedVDB.Variant: record_primary_key<TAB>metaseq_id<TAB>row_algorithm_id "
                         "lines; a plain, gzip or bgzip file")
    ap.add_argument("-o", "--outputDir", required=True, help="output directory")
    ap.add_argument("--chr", default="all", help="comma separated list of one or more chromosomes, or all / autosome")
    ap.add_argument("--variantsPerFile", type=int, default=VARIANTS_PER_FILE)
    ap.add_argument("--maxWorkers", type=int, default=10, help="accepted as in the reference, and ignored")
    ap.add_argument("--gusConfigFile", help="not supported: there is no database here")
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--veryVerbose", action="store_true")
    args = ap.parse_args(argv)
    if args.gusConfigFile:
        ap.error("--gusConfigFile is not supported: there is no database here; give the variants as --export")
    if args.variantsPerFile < 1:
        ap.error("--variantsPerFile must be at least 1")
    return args


def main(argv: Optional[Sequence[str]] = None, engine=None) -> Dict[str, Dict[str, int]]:
    """Runs the export; returns ``{chromosome: {valid, invalid, dropped, files}}``."""
    args = parse_args(argv)
    from . import bgzf
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    text = engine._as_text(bgzf.read_whole(args.export, engine))
    os.makedirs(args.outputDir, exist_ok=True)
    result = {}
    for c in chromosome_list(args.chr):
        chromosome = "chr" + c  # run(directory, chromosome='chr' + xstr(c)), export_variant2vcf.py:129
        out = engine.export_vcf(text, contigs=[c], variants_per_file=args.variantsPerFile)
        out.files(args.outputDir, chromosome)
        with open(os.path.join(args.outputDir, chromosome + ".log"), "w") as lfh:
            print("Processing " + chromosome, file=lfh)
            for k in range(1, out.n_files):  # export_variant2vcf.py:86
                print("Fetched %d records from %s. Writing to file %d" % (k * out.variants_per_file, chromosome, k),
                      file=lfh)
            print("Fetched %d valid records from %s. Writing residuals to file %d" % (  # :96
                out.counts["valid"], chromosome, out.n_files), file=lfh)
        result[c] = {"valid": out.counts["valid"], "invalid": out.counts["invalid"],
                     "dropped": out.counts["dropped"], "files": out.n_files}
    return result


if __name__ == "__main__":
    main()

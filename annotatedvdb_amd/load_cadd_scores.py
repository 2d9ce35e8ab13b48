"""CADD update driver — the counterpart of ``Load/bin/load_cadd_scores.py``.

The reference runs, per chromosome, ``SELECT record_primary_key, metaseq_id,
cadd_scores FROM AnnotatedVDB.Variant WHERE chromosome = %s`` (``SELECT_SQL``, ``:29``)
and for every record a tabix fetch, a row scan, a ``json.dumps`` and a buffered
``UPDATE`` value (``update_cadd_scores_by_query``, ``:81-160``).  Here the records come
from an export of those three columns (``COPY (SELECT record_primary_key, metaseq_id,
cadd_scores FROM AnnotatedVDB.Variant) TO STDOUT``; one whole-table export serves every
chromosome), and per chromosome the two CADD files' lines of that contig become device
tables (K10a) and the export's rows of that contig become update rows on the GPU (K13,
``CADDUpdater.buffer_export``).  There is no database here: the rows
``execute_values(cursor, CADD_UPDATE_SQL, buffer)`` would take are written to
``<outDir>/chr<c>.cadd_update.tsv`` as ``pk<TAB>chrom<TAB>json`` lines.

    python -m annotatedvdb_amd.load_cadd_scores -d cadd --export variants.tsv.gz --chr all --outDir out

Records that carry ``cadd_scores`` already are counted ``skipped``, as the reference's
query loop does whether or not ``--skipExisting`` is given (``:114-117``).  ``--vcfFile``
(update only the listed variants) needs the primary-key lookup by metaseq id, which
needs the database: it is refused.  One process, one GPU.
"""

from __future__ import annotations

import argparse
import logging
import os
from typing import Dict, List, Optional, Sequence

LOGGER = logging.getLogger("load_cadd_scores")
SNV_FILE = "whole_genome_SNVs.tsv.gz"             # cadd_updater.py: the reference's two file names
INDEL_FILE = "gnomad.genomes.r3.0.indel.tsv.gz"


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="CADD update rows for the variants of an export "
                                 "of AnnotatedVDB.Variant, on one GPU")
    ap.add_argument("-d", "--databaseDir", required=True,
                    help="directory containing %s and %s (either may be missing)" % (SNV_FILE, INDEL_FILE))
    ap.add_argument("--export", help="export of AnnotatedVDB.Variant: record_primary_key<TAB>metaseq_id<TAB>cadd_scores "
                                     "lines; a plain, gzip or bgzip file")
    ap.add_argument("--vcfFile", help="not supported: updating only the variants of a VCF file needs the database")
    ap.add_argument("--chr", default="all", help="comma separated list of one or more chromosomes, or all / autosome")
    ap.add_argument("--skipExisting", action="store_true",
                    help="accepted as in the reference; annotated records are skipped either way")
    ap.add_argument("--outDir", default=".")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    if args.vcfFile:
        ap.error("--vcfFile is not supported: it needs the primary-key lookup by metaseq id in the database; "
                 "give the variants as --export")
    if not args.export:
        ap.error("--export is required")
    return args


def chromosome_list(spec: str) -> List[str]:
    """``--chr`` as the reference parses it (``load_cadd_scores.py:294-300``)."""
    from .chromosomes import CHROM_NAMES
    if spec == "all":
        return list(CHROM_NAMES)
    if spec == "autosome":
        return [c for c in CHROM_NAMES if c not in ("X", "Y", "M", "MT")]
    return [c[3:] if c.startswith("chr") else c for c in spec.split(",") if c]


def main(argv: Optional[Sequence[str]] = None, engine=None) -> Dict[str, Dict[str, int]]:
    """Runs the pass; returns ``{chromosome: {records, snv, indel, not_matched, skipped, rows}}``."""
    args = parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO,
                        format="%(asctime)s %(funcName)s %(levelname)-8s %(message)s")
    from . import bgzf
    from .cadd import CADDUpdater, CaddTable
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    text = engine._as_text(bgzf.read_whole(args.export, engine))
    os.makedirs(args.outDir, exist_ok=True)
    paths = [os.path.join(args.databaseDir, name) for name in (SNV_FILE, INDEL_FILE)]
    result = {}
    for c in chromosome_list(args.chr):
        tables = []
        for path in paths:
            if os.path.exists(path):
                tables.append(CaddTable.from_file(path, contigs=[c], engine=engine))
                LOGGER.debug("chr%s: %d rows of %s", c, len(tables[-1]), path)
            else:
                tables.append(None)
                LOGGER.debug("chr%s: %s is missing", c, path)
        updater = CADDUpdater(tables[0], tables[1], engine)
        updater.set_chromosome("chr" + c)  # update_cadd_scores_by_query, load_cadd_scores.py:91-94
        n = updater.buffer_export(text, skip_existing=True, contigs=[c])
        out = os.path.join(args.outDir, "chr%s.cadd_update.tsv" % c)
        with open(out, "wb") as fh:
            fh.write(updater.update_text())
        counts = {name: updater.get_count(name) for name in ("snv", "indel", "not_matched", "skipped")}
        counts["rows"] = n
        counts["records"] = n + counts["skipped"]
        result[c] = counts
        LOGGER.info("chr%s: %s", c, " ".join((  # load_cadd_scores.py:148-152
            "Updated", "{:,}".format(counts["records"]), "variants", "- SNVS:", "{:,}".format(counts["snv"]),
            "- INDELs:", "{:,}".format(counts["indel"]), "- No match", "{:,}".format(counts["not_matched"]),
            "- Skipped", "{:,}".format(counts["skipped"]))))
        LOGGER.debug("chr%s: %d rows written to %s", c, n, out)
    return result


if __name__ == "__main__":
    main()

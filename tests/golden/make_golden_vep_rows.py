#!/usr/bin/env python3
"""Generate the K18b golden fixture by running the REFERENCE's own ``VepJsonParser``,
``VcfEntryParser`` and ``VariantAnnotator`` over synthetic VEP ``--json`` lines whose ``input`` and
consequence alleles agree (tests/vep_rows_common.py builds them).

Which of the two ways: ``VEPVariantLoader`` is not constructed (its constructor wants a database
handle, a validator and SeqRepo); ``parse_variant:262-296`` and ``__parse_alt_alleles:169-204`` are
RESTATED here around the reference's own classes, for the two consequence columns only:
``json.loads``, ``set_annotation(deepcopy(...))``, ``VcfEntryParser(get('input'), identityOnly=True)``
(the ADSP form: the five identity fields; INFO matters to ``allele_frequencies`` alone),
``get_variant(namespace=True)``, ``adsp_rank_and_sort_consequences()``, then per ALT allele
``VariantAnnotator(...)``, ``get_metaseq_id()``, ``get_normalized_alleles(snvDivMinus=True)``,
``get_most_severe_consequence(normAlt)`` and ``get_allele_consequences(normAlt)``.

Stand-ins: those of make_golden_vep.py (UNPINNED ``GenomicsDBData.Util``; a re-rank is recorded as
``rerank``), and ``xstr(dict, nullStr='{}')`` is ``json.dumps`` (README, "json.dumps stand-in").  The
database calls (``is_duplicate``, ``has_attribute``) are an export here; the expected update rows are
the loop's tuples joined against it by metaseq id, the last line of an id answering.

Runs where the reference checkout is (never on the GPU machine).  Writes vep_rows.tsv.gz:

  K<TAB>name<TAB>json                a ranking file's text (``fractional``; ``shipped`` is vep_ranking.tsv)
  L<TAB>name<TAB>kind or -<TAB>outcome<TAB>line<TAB>rows
                                     outcome ``ok`` (rows: ``[[metaseq id, most severe, ranked], ...]``,
                                     one per ALT), ``rerank`` or ``raise:<class>``
  E<TAB>json                         the export's text (over the ``shipped`` lines)
  U<TAB>adsp<TAB>update_existing<TAB>json
                                     the update rows' text for algorithm id vep_rows_common.ALG_ID
"""

from __future__ import annotations

import gzip
import io
import json
import os
import sys
import tempfile
from copy import deepcopy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_vep import NeedsRerank, load_reference  # noqa: E402
import vep_common as V  # noqa: E402
import vep_rows_common as R  # noqa: E402

N_LINES = 520
N_FRACTIONAL = 80


def xstr(value):
    return "{}" if value is None else json.dumps(value)


def parse_line(parser, VcfEntryParser, VariantAnnotator, line):
    parser.set_annotation(deepcopy(json.loads(line)))
    entry = VcfEntryParser(parser.get("input"), identityOnly=True)
    entry.update_chromosome(None)
    variant = entry.get_variant(dbSNP=False, namespace=True)
    parser.adsp_rank_and_sort_consequences()
    rows = []
    for alt in variant.alt_alleles:
        annotator = VariantAnnotator(variant.ref_allele, alt, variant.chromosome, variant.position)
        _, norm_alt = annotator.get_normalized_alleles(snvDivMinus=True)
        rows.append([annotator.get_metaseq_id(), xstr(parser.get_most_severe_consequence(norm_alt)),
                     xstr(parser.get_allele_consequences(norm_alt))])
    return rows


def run_lines(classes, ranking_path, lines, name, out):
    VepJsonParser, VcfEntryParser, VariantAnnotator = classes
    parser = VepJsonParser(ranking_path, rankConsequencesOnLoad=False)
    done = []
    for line, kind in lines:
        assert "\t" not in line and "\n" not in line
        rows = None
        try:
            rows = parse_line(parser, VcfEntryParser, VariantAnnotator, line)
            outcome, col = "ok", json.dumps(rows)
        except NeedsRerank:
            outcome, col = "rerank", ""
        except Exception as err:  # noqa: BLE001 (the class is the record)
            outcome, col = "raise:" + type(err).__name__, ""
        out.write("\t".join(["L", name, kind or "-", outcome, line, col]) + "\n")
        done.append(rows)
    return done


def update_text(rows_of_lines, export: bytes, adsp: bool, update_existing: bool) -> str:
    table = {}
    for rows in rows_of_lines:
        for key, ms, ranked in rows or ():
            table[key] = (ms, ranked)  # the last line of an id answers
    out = []
    for rec in export.decode("utf-8").split("\n")[:-1]:
        f = rec.split("\t")
        if len(f) < 2 or f[0] == "record_primary_key" or f[1] not in table:
            continue
        if not update_existing and len(f) > 2 and f[2] not in ("", "\\N"):
            continue
        ms, ranked = table[f[1]]
        t = [f[0], "chr" + f[1].split(":")[0], ms, ranked, str(R.ALG_ID)] + (["true"] if adsp else [])
        out.append("\t".join(t) + "\n")
    return "".join(out)


def main():
    VepJsonParser = load_reference()
    from AnnotatedVDB.Util.parsers import VcfEntryParser
    from AnnotatedVDB.Util.variant_annotator import VariantAnnotator
    classes = (VepJsonParser, VcfEntryParser, VariantAnnotator)
    rows = V.read_ranking_rows()
    with tempfile.TemporaryDirectory() as tmp, gzip.GzipFile(R.GOLDEN_FILE, "wb", mtime=0) as raw:
        out = io.TextIOWrapper(raw, encoding="utf-8", newline="\n")
        shipped = run_lines(classes, V.RANKING_FILE, R.golden_lines(rows, 20261023, N_LINES), "shipped", out)
        frac = os.path.join(tmp, "fractional.txt")
        with open(frac, "w") as fh:
            fh.write(V.ranking_text(V.FRACTIONAL_ROWS))
        out.write("K\tfractional\t%s\n" % json.dumps(V.ranking_text(V.FRACTIONAL_ROWS)))
        run_lines(classes, frac, R.golden_lines(V.FRACTIONAL_ROWS, 20261024, N_FRACTIONAL), "fractional", out)
        export = R.export_text([key for r in shipped for key, _, _ in r or ()])
        out.write("E\t%s\n" % json.dumps(export.decode("utf-8")))
        for adsp in (False, True):
            for upd in (False, True):
                out.write("U\t%d\t%d\t%s\n" % (adsp, upd, json.dumps(update_text(shipped, export, adsp, upd))))
        out.flush()
    print(R.GOLDEN_FILE, os.path.getsize(R.GOLDEN_FILE))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate the K18c golden fixture by running the REFERENCE's own ``VepJsonParser`` and
``VcfEntryParser`` over synthetic VEP ``--json`` lines whose ``input`` has eight fields
(tests/vep_output_common.py builds them).

Which of the two ways: as in make_golden_vep_rows.py, ``VEPVariantLoader`` is not constructed;
``parse_variant:262-296``, ``__clean_result:112-123`` and ``__parse_alt_alleles:169-204`` are RESTATED
here around the reference's own classes: ``json.loads``, ``set_annotation(deepcopy(...))``,
``VcfEntryParser(get('input'), identityOnly=...)``, ``update_chromosome(None)``,
``set('input', entry.get_entry())``, ``get_variant(namespace=True)``,
``adsp_rank_and_sort_consequences()``, then ``get_annotation(deepCopy=True)`` with
``colocated_variants`` and the four ``<type>_consequences`` keys popped, and per ALT allele the two
consequence columns.  Every line is run in both forms, ``identityOnly`` False and True.

Stand-ins: those of make_golden_vep.py and make_golden_vep_rows.py (``xstr(dict, nullStr='{}')`` is
``json.dumps``; ``to_numeric`` is the stub's).  The database calls are an export; the expected update
rows are the loop's tuples joined against it by metaseq id, the last line of an id answering, with
``identityOnly = adsp`` as ``parse_variant`` has it.

Runs where the reference checkout is (never on the GPU machine).  Writes vep_output.tsv.gz:

  L<TAB>kind or -<TAB>line<TAB>outcome<TAB>cleaned<TAB>rows<TAB>outcome<TAB>cleaned<TAB>rows
                                     the full form, then the identityOnly form: outcome ``ok`` (cleaned: the
                                     text as a JSON string; rows: ``[[metaseq id, most severe, ranked], ...]``),
                                     ``rerank`` or ``raise:<class>``
  E<TAB>json                         the export's text
  U<TAB>adsp<TAB>update_existing<TAB>json
                                     the update rows' text for algorithm id vep_output_common.ALG_ID
"""

from __future__ import annotations

import gzip
import io
import json
import os
import sys
from copy import deepcopy

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden_vep import NeedsRerank, load_reference  # noqa: E402
import vep_common as V  # noqa: E402
import vep_output_common as O  # noqa: E402
import vep_rows_common as R  # noqa: E402

N_LINES = 672


def xstr(value):
    return "{}" if value is None else json.dumps(value)


def parse_line(parser, VcfEntryParser, VariantAnnotator, line, identity_only):
    parser.set_annotation(deepcopy(json.loads(line)))
    entry = VcfEntryParser(parser.get("input"), identityOnly=identity_only)
    entry.update_chromosome(None)
    parser.set("input", entry.get_entry())
    variant = entry.get_variant(dbSNP=False, namespace=True)
    parser.adsp_rank_and_sort_consequences()
    clean = parser.get_annotation(deepCopy=True)
    clean.pop("colocated_variants", None)
    for ctype in V.TYPES:
        clean.pop(ctype + "_consequences", None)
    rows = []
    for alt in variant.alt_alleles:
        annotator = VariantAnnotator(variant.ref_allele, alt, variant.chromosome, variant.position)
        _, norm_alt = annotator.get_normalized_alleles(snvDivMinus=True)
        rows.append([annotator.get_metaseq_id(), xstr(parser.get_most_severe_consequence(norm_alt)),
                     xstr(parser.get_allele_consequences(norm_alt))])
    return xstr(clean), rows


def run_lines(classes, ranking_path, lines, out):
    VepJsonParser, VcfEntryParser, VariantAnnotator = classes
    parser = VepJsonParser(ranking_path, rankConsequencesOnLoad=False)
    done = {False: [], True: []}
    for line, kind in lines:
        assert "\t" not in line and "\n" not in line
        cols = ["L", kind or "-", line]
        for identity_only in (False, True):
            result = None
            try:
                result = parse_line(parser, VcfEntryParser, VariantAnnotator, line, identity_only)
                cols += ["ok", json.dumps(result[0]), json.dumps(result[1])]
            except NeedsRerank:
                cols += ["rerank", "", ""]
            except Exception as err:  # noqa: BLE001 (the class is the record)
                cols += ["raise:" + type(err).__name__, "", ""]
            done[identity_only].append(result)
        out.write("\t".join(cols) + "\n")
    return done


def update_text(results, export: bytes, adsp: bool, update_existing: bool) -> str:
    table = {}
    for result in results:
        if result is not None:
            for key, ms, ranked in result[1]:
                table[key] = (ms, ranked, result[0])
    return O.join_text(table, export, O.ALG_ID, adsp, update_existing)


def main():
    VepJsonParser = load_reference()
    from AnnotatedVDB.Util.parsers import VcfEntryParser
    from AnnotatedVDB.Util.variant_annotator import VariantAnnotator
    classes = (VepJsonParser, VcfEntryParser, VariantAnnotator)
    rows = V.read_ranking_rows()
    with gzip.GzipFile(O.GOLDEN_FILE, "wb", mtime=0) as raw:
        out = io.TextIOWrapper(raw, encoding="utf-8", newline="\n")
        done = run_lines(classes, V.RANKING_FILE, O.golden_lines(rows, 20261025, N_LINES), out)
        export = R.export_text([key for r in done[False] if r is not None for key, _, _ in r[1]])
        out.write("E\t%s\n" % json.dumps(export.decode("utf-8")))
        for adsp in (False, True):
            for upd in (False, True):
                out.write("U\t%d\t%d\t%s\n" % (adsp, upd, json.dumps(update_text(done[adsp], export, adsp, upd))))
        out.flush()
    print(O.GOLDEN_FILE, os.path.getsize(O.GOLDEN_FILE))


if __name__ == "__main__":
    main()

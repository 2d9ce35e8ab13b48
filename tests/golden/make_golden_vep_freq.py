#!/usr/bin/env python3
"""Generate the K18d golden fixture by running the REFERENCE's own ``VepJsonParser.get_frequencies``,
``VcfEntryParser.get_frequencies`` and ``VariantAnnotator`` over synthetic VEP ``--json`` lines
(tests/vep_freq_common.py builds them).

Which of the two ways: as in make_golden_vep_output.py, ``VEPVariantLoader`` is not constructed;
``parse_variant:262-296``, ``__get_result_frequencies:85-93``, ``__get_allele_frequencies:96-109``,
``__add_vcf_frequencies:126-142`` and ``__parse_alt_alleles:169-204`` are RESTATED here around the
reference's own classes: ``json.loads``, ``set_annotation(deepcopy(...))``, ``VcfEntryParser(get('input'),
identityOnly=...)``, ``update_chromosome(None)``, ``set('input', entry.get_entry())``,
``get_variant(dbSNP=..., namespace=True)``, ``adsp_rank_and_sort_consequences()``,
``get_frequencies(ref_snp_id or None)['values']``, the cleaned result, and per ALT allele
``frequencies.get(normAlt)`` merged with ``entry.get_frequencies(alt)`` and the two consequence columns.
Every line is run in four forms: ``identityOnly`` x matching by ``ref_snp_id`` (``is_dbsnp()``).

Stand-ins: those of make_golden_vep.py and make_golden_vep_rows.py (``xstr(dict, nullStr='{}')`` is
``json.dumps``; ``to_numeric`` is the stub's), with two of make_golden.py's shallow stubs overridden in the
loaded reference modules' namespaces before they are used, as DESIGN.md (K18d) takes them:
``AutoVivificationDict`` is a dict that creates missing keys, and ``deep_update(a, b)`` is the recursive
in-place merge (both values dicts: recurse; else ``a[k] = b[k]``; new keys appended).  The database calls are an
export; the expected update rows are the loop's tuples joined against it by metaseq id, the last line of an id
answering, for the reference's two datasources: dbSNP (all eight fields, matched by ``ref_snp_id``) and ADSP
(``identityOnly``, no match, ``is_adsp_variant``).

Runs where the reference checkout is (never on the GPU machine).  Writes vep_freq.tsv.gz:

  L<TAB>kind or -<TAB>line<TAB>(outcome<TAB>rows) x 4
                                     the forms of vep_freq_common.FORMS in turn: outcome ``ok`` (rows:
                                     ``[[metaseq id, allele_frequencies], ...]``), ``rerank`` or ``raise:<class>``
  E<TAB>json                         the export's text
  U<TAB>adsp<TAB>update_existing<TAB>vep_output<TAB>json
                                     the update rows' text for algorithm id vep_freq_common.ALG_ID
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
import vep_freq_common as F  # noqa: E402
import vep_rows_common as R  # noqa: E402

N_LINES = 616
HOST_EVERY = 11  # one line in eleven is a host case: every kind once, and at most one line in ten


class AutoVivificationDict(dict):
    def __missing__(self, key):
        value = self[key] = type(self)()
        return value


def deep_update(a, b):
    for key, value in b.items():
        if isinstance(value, dict) and isinstance(a.get(key), dict):
            deep_update(a[key], value)
        else:
            a[key] = value
    return a


def override_stubs():
    """The two names, wherever a loaded reference module (or the stub it imports them from) holds them."""
    for name, module in list(sys.modules.items()):
        if module is not None and name.split(".")[0] in ("AnnotatedVDB", "GenomicsDBData"):
            if hasattr(module, "AutoVivificationDict"):
                module.AutoVivificationDict = AutoVivificationDict
            if hasattr(module, "deep_update"):
                module.deep_update = deep_update


def xstr(value):
    return "{}" if value is None else json.dumps(value)


def parse_line(parser, VcfEntryParser, VariantAnnotator, line, identity_only, match_refsnp):
    parser.set_annotation(deepcopy(json.loads(line)))
    entry = VcfEntryParser(parser.get("input"), identityOnly=identity_only)
    entry.update_chromosome(None)
    parser.set("input", entry.get_entry())
    variant = entry.get_variant(dbSNP=match_refsnp, namespace=True)
    parser.adsp_rank_and_sort_consequences()
    frequencies = parser.get_frequencies(variant.ref_snp_id if match_refsnp else None)
    if frequencies is not None:
        frequencies = frequencies["values"]
    clean = parser.get_annotation(deepCopy=True)
    clean.pop("colocated_variants", None)
    for ctype in V.TYPES:
        clean.pop(ctype + "_consequences", None)
    rows = []
    for alt in variant.alt_alleles:
        annotator = VariantAnnotator(variant.ref_allele, alt, variant.chromosome, variant.position)
        _, norm_alt = annotator.get_normalized_alleles(snvDivMinus=True)
        allele_freq = None
        if frequencies is not None and norm_alt in frequencies:
            allele_freq = frequencies[norm_alt]
        gmafs = entry.get_frequencies(alt)
        if allele_freq is None:
            allele_freq = gmafs
        elif gmafs is not None:
            allele_freq = deep_update(allele_freq, gmafs)
        rows.append([annotator.get_metaseq_id(), xstr(allele_freq), xstr(parser.get_most_severe_consequence(norm_alt)),
                     xstr(parser.get_allele_consequences(norm_alt))])
    return xstr(clean), rows


def run_lines(classes, ranking_path, lines, out):
    VepJsonParser, VcfEntryParser, VariantAnnotator = classes
    parser = VepJsonParser(ranking_path, rankConsequencesOnLoad=False)
    done = {form: [] for form in F.FORMS}
    for line, kind in lines:
        assert "\t" not in line and "\n" not in line
        cols = ["L", kind or "-", line]
        for form in F.FORMS:
            result = None
            try:
                result = parse_line(parser, VcfEntryParser, VariantAnnotator, line, *form)
                cols += ["ok", json.dumps([r[:2] for r in result[1]])]
            except NeedsRerank:
                cols += ["rerank", ""]
            except Exception as err:  # noqa: BLE001 (the class is the record)
                cols += ["raise:" + type(err).__name__, ""]
            done[form].append(result)
        out.write("\t".join(cols) + "\n")
    return done


def update_text(results, export: bytes, adsp: bool, update_existing: bool, vep_output: bool) -> str:
    table = {}
    for result in results:
        if result is not None:
            for key, freq, ms, ranked in result[1]:
                table[key] = (freq, ms, ranked, result[0])
    return F.join_text(table, export, F.ALG_ID, adsp, update_existing, vep_output)


def main():
    VepJsonParser = load_reference()
    from AnnotatedVDB.Util.parsers import VcfEntryParser
    from AnnotatedVDB.Util.variant_annotator import VariantAnnotator
    override_stubs()
    classes = (VepJsonParser, VcfEntryParser, VariantAnnotator)
    rows = V.read_ranking_rows()
    lines = F.golden_lines(rows, 20261028, N_LINES, HOST_EVERY)
    with gzip.GzipFile(F.GOLDEN_FILE, "wb", mtime=0) as raw:
        out = io.TextIOWrapper(raw, encoding="utf-8", newline="\n")
        done = run_lines(classes, V.RANKING_FILE, lines, out)
        # the bound again, on what the reference itself answered: the host cases among the lines it takes
        for form in F.FORMS:
            taken = [kind for (_, kind), r in zip(lines, done[form]) if r is not None]
            hosts = sum(F.reason_of(kind, *form) is not None for kind in taken)
            assert 0 < 10 * hosts <= len(taken), (form, hosts, len(taken))
        export = R.export_text([key for r in done[(False, True)] if r is not None for key, *_ in r[1]])
        out.write("E\t%s\n" % json.dumps(export.decode("utf-8")))
        for adsp in (False, True):
            form = (True, False) if adsp else (False, True)  # ADSP: identityOnly; dbSNP: matched by ref_snp_id
            for upd in (False, True):
                for vo in (False, True):
                    out.write("U\t%d\t%d\t%d\t%s\n" % (adsp, upd, vo, json.dumps(update_text(done[form], export, adsp, upd, vo))))
        out.flush()
    print(F.GOLDEN_FILE, os.path.getsize(F.GOLDEN_FILE))


if __name__ == "__main__":
    main()

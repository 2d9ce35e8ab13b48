#!/usr/bin/env python3
"""Generate the K18a golden fixtures by running the REFERENCE's own ``VepJsonParser`` and
``ConsequenceParser`` (Util/lib/python/parsers/vep_parser.py, adsp_consequence_parser.py) over
synthetic VEP ``--json`` lines (tests/vep_common.py builds them).

Runs where the reference checkout is (never on the GPU machine); the tests read only the files it
writes:

  vep_ranking.tsv           the shipped ranking (Load/data/custom_consequence_ranking.txt) as
                            ``save_ranking_file`` would write it, ``consequence<TAB>rank`` in load
                            order: names and numbers only
  vep_consequences.tsv.gz   ``G<TAB>name<TAB>json``: ``get_rankings()`` of the ranking ``name`` as a
                            list of pairs; ``K<TAB>name<TAB>json``: a ranking file's text (the second,
                            small ranking with fractional and tied ranks); per line
                            ``L<TAB>name<TAB>host kind or -<TAB>outcome<TAB>line<TAB>ranked<TAB>most severe``:
                            outcome ``ok`` (``ranked``: the four ``<type>_consequences`` keys of
                            ``_annotation`` after ``adsp_rank_and_sort_consequences()``, ``most
                            severe``: ``get_most_severe_consequence`` per allele), ``raise:<class>``
                            (what the call raised), or ``rerank`` (the call reached
                            ``__update_rankings``)

Stand-ins (UNPINNED: ``GenomicsDBData.Util`` is not on this machine): ``alphabetize_string_list``
sorts the comma-separated terms, ``is_equivalent_list`` (make_golden.py) compares sorted lists,
``list_to_indexed_dict`` and ``is_overlapping_list`` exist only so that the modules import.  The
re-ranking is not pinned at all: ``__update_rankings`` is replaced by a function that raises, and
a line that reaches it is recorded as ``rerank``.  The parser is made once per ranking with
``rankConsequencesOnLoad=False`` and fed line after line, as ``load_vep_result.py`` feeds it.
"""

from __future__ import annotations

import gzip
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import REF, install_stubs  # noqa: E402
import vep_common as V  # noqa: E402

N_LINES = 2000
N_FRACTIONAL = 160


class NeedsRerank(Exception):
    pass


def load_reference():
    install_stubs()
    import GenomicsDBData.Util.list_utils as lu
    lu.alphabetize_string_list = lambda s: ",".join(sorted(s.split(",") if isinstance(s, str) else s))
    lu.list_to_indexed_dict = lambda values: {v: i + 1 for i, v in enumerate(values)}
    lu.is_overlapping_list = lambda a, b: bool(set(a) & set(b))
    from AnnotatedVDB.Util.parsers import ConsequenceParser, VepJsonParser

    def no_rerank(self, terms=None):
        raise NeedsRerank(terms)

    ConsequenceParser._ConsequenceParser__update_rankings = no_rerank
    return VepJsonParser


def shipped_rows():
    """The shipped file through the reference's own reader: load order is the rank."""
    VepJsonParser = load_reference()
    parser = VepJsonParser(os.path.join(REF, "Load", "data", "custom_consequence_ranking.txt"))
    return [(c, str(r)) for c, r in parser.get_consequence_parser().get_rankings().items()]


def run_lines(VepJsonParser, ranking_path, lines, name, out):
    parser = VepJsonParser(ranking_path, rankConsequencesOnLoad=False)
    out.write("G\t%s\t%s\n" % (name, json.dumps(list(parser.get_consequence_parser().get_rankings().items()))))
    keys = [t + "_consequences" for t in V.TYPES]
    host = 0
    for line, kind in lines:
        host += kind is not None
        assert "\t" not in line and "\n" not in line
        try:
            parser.set_annotation(json.loads(line))
            parser.adsp_rank_and_sort_consequences()
            ann = parser.get_annotation()
            ranked = {k: ann[k] for k in keys if k in ann}
            alleles = []
            for k in keys:
                for va in (ranked.get(k) or ()):
                    if va not in alleles:
                        alleles.append(va)
            severe = {va: parser.get_most_severe_consequence(va) for va in alleles}
            outcome, cols = "ok", [json.dumps(ranked), json.dumps(severe)]
        except NeedsRerank:
            outcome, cols = "rerank", ["", ""]
        except Exception as err:  # noqa: BLE001 (the class is the record)
            outcome, cols = "raise:" + type(err).__name__, ["", ""]
        out.write("\t".join(["L", name, kind or "-", outcome, line] + cols) + "\n")
    assert 0 < host and 9 * host <= len(lines) - host, (host, len(lines))


def main():
    VepJsonParser = load_reference()
    rows = shipped_rows()
    assert len(rows) == 293 and len({t for c, _ in rows for t in c.split(",")}) == 31, len(rows)
    with open(V.RANKING_FILE, "w") as fh:
        fh.write(V.ranking_text(rows))
    with tempfile.TemporaryDirectory() as tmp, gzip.GzipFile(V.GOLDEN_FILE, "wb", mtime=0) as raw:
        import io
        out = io.TextIOWrapper(raw, encoding="utf-8", newline="\n")
        run_lines(VepJsonParser, V.RANKING_FILE, V.golden_lines(rows, 20261021, N_LINES), "shipped", out)
        frac = os.path.join(tmp, "fractional.txt")
        with open(frac, "w") as fh:
            fh.write(V.ranking_text(V.FRACTIONAL_ROWS))
        out.write("K\tfractional\t%s\n" % json.dumps(V.ranking_text(V.FRACTIONAL_ROWS)))
        run_lines(VepJsonParser, frac, V.golden_lines(V.FRACTIONAL_ROWS, 20261022, N_FRACTIONAL), "fractional", out)
        out.flush()
    print(V.GOLDEN_FILE, os.path.getsize(V.GOLDEN_FILE))


if __name__ == "__main__":
    main()

"""Helpers of the K18a tests: the generator of synthetic VEP ``--json`` lines (the golden's and the
fuzz's), the golden's reader, and the comparison of a device result with the host entries'."""

import gzip
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
RANKING_FILE = os.path.join(GOLDEN, "vep_ranking.tsv")
GOLDEN_FILE = os.path.join(GOLDEN, "vep_consequences.tsv.gz")

TYPES = ("transcript", "regulatory_feature", "motif_feature", "intergenic")
# the second ranking of the golden: fractional and tied ranks (a user's own file)
FRACTIONAL_ROWS = [("stop_gained", "1"), ("missense_variant", "2.5"), ("synonymous_variant", "2.5"),
                   ("splice_region_variant,intron_variant", "2.75"), ("intron_variant", "3"),
                   ("regulatory_region_variant", "7"), ("TF_binding_site_variant", "7.0"),
                   ("upstream_gene_variant", "10"), ("intergenic_variant", "10"),
                   ("missense_variant,splice_region_variant", "2.25"), ("downstream_gene_variant", "0.5")]
# why the device leaves a line to the host (annotatedvdb_amd._native.VEP_REASONS), as the generator builds them
HOST_KINDS = ("whitespace", "not_object", "truncated", "depth", "duplicate_id", "duplicate_array", "no_allele",
              "two_term_arrays", "number_term", "escaped_key", "escaped_allele", "escaped_term", "utf8_allele",
              "repeated_term", "no_terms", "unknown_single", "unknown_beside_ranked", "two_unknown",
              "unknown_combination", "null_array", "too_many")
REASON_OF = {"whitespace": "whitespace", "not_object": "structure", "truncated": "structure", "depth": "depth",
             "duplicate_id": "duplicate_key", "duplicate_array": "duplicate_key", "no_allele": "element",
             "two_term_arrays": "element", "number_term": "element", "escaped_key": "element",
             "escaped_allele": "bytes", "escaped_term": "bytes", "utf8_allele": "bytes",
             "repeated_term": "repeated_term", "no_terms": "no_terms", "unknown_single": "unknown_term",
             "unknown_beside_ranked": "unknown_term", "two_unknown": "unknown_term",
             "unknown_combination": "unknown_combination", "null_array": "element", "too_many": "too_many"}


def read_ranking_rows(path=RANKING_FILE):
    with open(path) as fh:
        rows = [line.rstrip("\n").split("\t") for line in fh]
    return [(c, r) for c, r in rows[1:]]


def ranking_text(rows) -> str:
    return "consequence\trank\n" + "".join(f"{c}\t{r}\n" for c, r in rows)


def dumps(obj) -> str:
    return json.dumps(obj, separators=(",", ":"))


class LineGenerator:
    """Synthetic lines over the combinations of a ranking (``combos``: lists of terms)."""

    def __init__(self, combos, seed: int):
        self.combos = [list(c) for c in combos]
        self.singles = [c for c in self.combos if len(c) == 1]
        self.multis = [c for c in self.combos if len(c) > 1]
        self.rng = random.Random(seed)
        self.n = 0

    def terms(self):
        rng = self.rng
        c = list(rng.choice(self.multis if self.multis and rng.random() < 0.4 else self.singles))
        order = rng.randrange(3)  # both orders of one combination, and a shuffle
        if order == 0:
            c.sort()
        elif order == 1:
            c.sort(reverse=True)
        else:
            rng.shuffle(c)
        return c

    def element(self, ctype: str, allele: str, k: int):
        rng = self.rng
        el = {"variant_allele": allele, "consequence_terms": self.terms(), "impact": rng.choice(["HIGH", "MODIFIER", "LOW"])}
        if ctype == "transcript":
            el["gene_id"] = "ENSG%05d" % rng.randrange(300)
            el["transcript_id"] = "ENST%05d" % rng.randrange(300)
            if k % 3 == 0:  # a nested object with a key of the element's name, two levels down
                el["domains"] = [{"db": "Pfam", "name": "PF%03d" % rng.randrange(50), "variant_allele": "Z"}]
            if k % 4 == 1:
                el["flags"] = ["cds_start_NF"]
            if k % 5 == 2:
                el["hgvsp"] = 'p.("%d")\\' % rng.randrange(99)  # an escaped quote and a backslash in a value
        elif ctype == "regulatory_feature":
            el["regulatory_feature_id"] = "ENSR%05d" % rng.randrange(300)
            el["biotype"] = "promoter"
        elif ctype == "motif_feature":
            el["motif_feature_id"] = "ENSM%05d" % rng.randrange(300)
            el["motif_score_change"] = -0.022
        if rng.random() < 0.5:  # the keys in another order
            el = dict(reversed(list(el.items())))
        return el

    def obj(self, n_csq=None):
        """One line's object: all four types over the lines, multi-allelic sites, the alleles -, G and GT,
        the same allele in several types, alleles interleaved within an array."""
        rng = self.rng
        self.n += 1
        k = self.n
        alleles = [["G"], ["G", "GT"], ["-", "G"], ["GT", "-", "G"], ["T"], ["A", "C"]][k % 6]
        pos = 10000 + 7 * k
        vid = "rs%d" % (1000 + k)
        o = {"input": "\t".join(["1", str(pos), vid, "A", ",".join(alleles), ".", ".", "."]), "id": vid,
             "assembly_name": "GRCh38", "seq_region_name": "1", "start": pos, "end": pos, "strand": 1,
             "allele_string": "A/" + "/".join(alleles), "most_severe_consequence": "intron_variant"}
        colocated = [{"id": vid, "allele_string": "A/G", "variant_allele": "Q", "consequence_terms": ["not_a_term"],
                      "frequencies": {"G": {"af": 0.25, "gnomad": 0.125}}}]
        if k % 3 == 0:
            o["colocated_variants"] = colocated
        types = [t for i, t in enumerate(TYPES) if (k >> i) & 1 or (k % 16 == 0)] or ["intergenic"]
        for t in types:
            if n_csq is not None:
                n = n_csq if t == types[0] else 0
            else:
                n = 1 if t == "intergenic" else rng.randrange(1, 7 if t == "transcript" else 4)
            o[t + "_consequences"] = [self.element(t, rng.choice(alleles), k + j) for j in range(n)]
        if k % 3 == 1:
            o["colocated_variants"] = colocated
        if k % 7 == 0:  # an empty array: the key stays, with no alleles
            o.setdefault("motif_feature_consequences", [])
        return o

    def line(self, host_kind=None) -> str:
        """A line the device answers, or one of ``HOST_KINDS``."""
        if host_kind is None:
            return dumps(self.obj())
        rng = self.rng
        if host_kind == "too_many":
            return dumps(self.obj(n_csq=513))
        o = self.obj()
        first = next(t + "_consequences" for t in TYPES if o.get(t + "_consequences"))
        els = o[first]
        if host_kind == "whitespace":
            return json.dumps(o)
        if host_kind == "not_object":
            return dumps([o])
        if host_kind == "truncated":
            return dumps(o)[:-1]
        if host_kind == "depth":
            deep = "x"
            for _ in range(70):
                deep = [deep]
            o["deep"] = deep
            return dumps(o)
        if host_kind == "duplicate_id":
            return dumps(o)[:-1] + ',"id":"again"}'
        if host_kind == "duplicate_array":
            return dumps(o)[:-1] + "," + dumps({first: els[:1]})[1:]
        if host_kind == "no_allele":
            del els[-1]["variant_allele"]
        elif host_kind == "two_term_arrays":
            text = dumps(o)
            at = text.index('"%s"' % first)
            return text[:at] + text[at:].replace('"consequence_terms":[',
                                                 '"consequence_terms":["intron_variant"],"consequence_terms":[', 1)
        elif host_kind == "number_term":
            els[0]["consequence_terms"] = ["intron_variant", 5]
        elif host_kind == "escaped_key":
            return dumps(o).replace('"variant_allele":"%s"' % els[0]["variant_allele"],
                                    '"variant\\u005fallele":"%s"' % els[0]["variant_allele"])
        elif host_kind == "escaped_allele":
            a = els[0]["variant_allele"]
            text = dumps(o)
            at = text.index('"%s"' % first)
            return text[:at] + text[at:].replace('"variant_allele":"%s"' % a, '"variant_allele":"\\u00%02x%s"' % (ord(a[0]), a[1:]), 1)
        elif host_kind == "escaped_term":
            t = els[0]["consequence_terms"][0]
            text = dumps(o)
            at = text.index('"%s":' % first) + len(first) + 3
            return text[:at] + text[at:].replace('"%s"' % t, '"\\u00%02x%s"' % (ord(t[0]), t[1:]), 1)
        elif host_kind == "utf8_allele":
            els[0]["variant_allele"] = "é"
            return json.dumps(o, separators=(",", ":"), ensure_ascii=False)
        elif host_kind == "repeated_term":
            t = els[0]["consequence_terms"][0]
            els[0]["consequence_terms"] = [t, t]
        elif host_kind == "no_terms":
            els[0]["consequence_terms"] = []
        elif host_kind == "unknown_single":  # alone in its allele's list: rank None
            o[first] = [dict(els[0], variant_allele="N", consequence_terms=["not_a_term"])] + els
        elif host_kind == "unknown_beside_ranked":  # None beside an int: TypeError
            o[first] = els + [dict(els[0], consequence_terms=["not_a_term"])]
        elif host_kind == "two_unknown":
            o[first] = [dict(els[0], variant_allele="N", consequence_terms=["not_a_term"]),
                        dict(els[0], variant_allele="N", consequence_terms=["no_term_either"])] + els
        elif host_kind == "unknown_combination":
            els[-1]["consequence_terms"] = [self.singles[0][0], self.singles[-1][0], self.singles[1][0]]
        elif host_kind == "null_array":
            o[first] = None
        else:
            raise ValueError(host_kind)
        return dumps(o)


def combos_of(rows):
    return [c.split(",") for c, _ in rows]


def golden_lines(rows, seed: int, n: int):
    """``(line, host kind or None)``: one line in sixteen is a host case, the kinds in turn."""
    gen = LineGenerator(combos_of(rows), seed)
    out, h = [], 0
    for k in range(n):
        kind = None
        if k % 16 == 5:
            kind = HOST_KINDS[h % len(HOST_KINDS)]
            h += 1
        out.append((gen.line(kind), kind))
    # a line of exactly AVDB_VEP_MAX_CSQ consequences is still the device's
    out.append((dumps(gen.obj(n_csq=512)), None))
    return out


def read_golden(path=GOLDEN_FILE):
    """``{"rankings": {name: [[combination, rank], ...]}, "files": {name: ranking file text},
    "lines": [(ranking name, host kind or None, outcome, line bytes, ranked or None, most severe or None)]}``;
    outcome: ``ok``, ``rerank`` or ``raise:<class>``."""
    out = {"rankings": {}, "files": {}, "lines": []}
    with gzip.open(path, "rt", encoding="utf-8") as fh:
        for row in fh:
            f = row.rstrip("\n").split("\t")
            if f[0] == "G":
                out["rankings"][f[1]] = json.loads(f[2])
            elif f[0] == "K":
                out["files"][f[1]] = json.loads(f[2])
            elif f[0] == "L":
                ok = f[3] == "ok"
                out["lines"].append((f[1], None if f[2] == "-" else f[2], f[3], f[4].encode("utf-8"),
                                     json.loads(f[5]) if ok else None, json.loads(f[6]) if ok else None))
    return out


ARRAYS = ("n_csq", "flags", "types", "input_start", "input_len", "id_start", "id_len", "csq_off", "type", "order",
          "el_start", "el_len", "al_start", "al_len", "mask", "entry", "coding", "sorted", "head")


def assert_same_arrays(got, want):
    """Two VepConsequences (the device's and the host entries'), array for array."""
    assert got.n_lines == want.n_lines
    assert got.counts == want.counts
    for name in ARRAYS:
        a, b = getattr(got, name).cpu().numpy(), getattr(want, name).cpu().numpy()
        assert a.shape == b.shape, name
        if not np.array_equal(a, b):
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{name}[{at}]: {a[at]} != {b[at]}")


EDGE_PADS = range(0, 131)


def edge_line(k: int) -> str:
    """One line whose leading string value is padded by k bytes: over k = 0..130 every structural
    feature behind it lands on every lane and on both sides of a 64-byte edge: key names and their
    colons, the '[' of consequence_terms, an element's braces, an escaped quote, and an even and an
    odd run of backslashes before a quote."""
    o = {"pad": "x" * k, "input": "1\t5\trs5\tA\tG,GT", "id": "rs5",
         "colocated_variants": [{"variant_allele": "Q", "consequence_terms": ["not_a_term"]}],
         "transcript_consequences": [
             {"variant_allele": "G", "note": 'a"b', "even": "c\\", "odd": 'd\\"e',
              "consequence_terms": ["splice_region_variant", "missense_variant"], "domains": [{"variant_allele": "Z"}]},
             {"consequence_terms": ["intron_variant"], "variant_allele": "GT"},
             {"variant_allele": "G", "consequence_terms": ["stop_gained"], "flags": ["cds_start_NF"]}],
         "intergenic_consequences": [{"consequence_terms": ["intergenic_variant"], "variant_allele": "-"}]}
    return dumps(o)


def sized_line(nbytes: int) -> str:
    """A line of exactly ``nbytes`` bytes with one consequence."""
    o = {"pad": "", "id": "r", "intergenic_consequences": [{"variant_allele": "G", "consequence_terms": ["intron_variant"]}]}
    o["pad"] = "y" * (nbytes - len(dumps(o)))
    line = dumps(o)
    assert len(line) == nbytes, (len(line), nbytes)
    return line


def edge_lines():
    return [edge_line(k) for k in EDGE_PADS] + [sized_line(128), sized_line(192), '{"id":"r","pad":"%s"}' % ("z" * 45),
                                                '{"id":"r","pad":"%s"}' % ("z" * 109)]


def count_lines(rows, counts):
    """Lines with the given numbers of consequences (all in one array)."""
    gen = LineGenerator(combos_of(rows), 11)
    return [dumps(gen.obj(n_csq=n)) for n in counts]


def small_lines(n: int):
    return ['{"id":"v%d","intergenic_consequences":[{"variant_allele":"%s","consequence_terms":["intergenic_variant"]}]}'
            % (i, "ACGT"[i % 4]) for i in range(n)]


def slab(lines) -> bytes:
    return "".join(l + "\n" for l in lines).encode("utf-8")


def outcome_of(call):
    """A call's value, or the class it raises."""
    try:
        return call()
    except Exception as err:  # noqa: BLE001
        return type(err)


def assert_ranked_as_vep_line(res, lines, ranking, vep_line):
    for i, line in enumerate(lines):
        got, want = outcome_of(lambda: res.ranked(i)), outcome_of(lambda: vep_line(line, ranking))
        assert got == want, (i, line[:300])
        if isinstance(want, dict):
            for key in want:
                assert list(got[key] or ()) == list(want[key] or ())

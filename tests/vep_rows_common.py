"""Helpers of the K18b tests: the generator of VEP ``--json`` lines whose ``input`` and consequence
alleles agree (the golden's and the fuzz's), the golden's reader, edge-case lines for the element
renderer, and the comparison of a device table with the host entries'."""

import gzip
import json
import os

import numpy as np

import vep_common as V

GOLDEN_FILE = os.path.join(V.GOLDEN, "vep_rows.tsv.gz")
ALG_ID = 4242

# the new reasons a line is the host's (annotatedvdb_amd._native.VEPROWS_REASONS), as the generator builds them
NEW_HOST_KINDS = ("escaped_slash", "escaped_u", "exponent", "trailing_zero", "minus_zero", "utf8_value",
                  "backslash_ref", "no_input", "four_fields", "numeric_id")
HOST_KINDS = V.HOST_KINDS + NEW_HOST_KINDS
REASON_OF = dict(V.REASON_OF, escaped_slash="escape", escaped_u="escape", exponent="token", trailing_zero="token",
                 minus_zero="token", utf8_value="byte", backslash_ref="input_fields", no_input="no_input",
                 four_fields="input_fields", numeric_id="input_fields")

# (CHROM of input, REF, [(ALT, the allele VEP names it by)]): SNVs, a deletion to '-', an insertion,
# multi-allelic sites of mixed kinds, a deletion that keeps bases, chrM and MT
SITES = [("1", "A", [("G", "G")]),
         ("chr2", "AT", [("A", "-")]),
         ("3", "A", [("AGT", "GT")]),
         ("X", "A", [("G", "G"), ("AGT", "GT")]),
         ("chrM", "AT", [("A", "-"), ("AG", "G")]),
         ("MT", "A", [("C", "C"), ("T", "T")]),
         ("22", "ATG", [("ACG", "CG"), ("A", "-"), ("ATGA", "A")]),
         ("Y", "C", [("T", "T")])]


class RowsLineGenerator(V.LineGenerator):
    """Lines whose ``input`` is the VCF line the consequences' alleles come from."""

    def obj(self, n_csq=None):
        rng = self.rng
        self.n += 1
        k = self.n
        chrom, ref, alts = SITES[k % len(SITES)]
        pos = 20000 + 11 * (k % 200)  # (ids repeat over the file: the last line of an id answers)
        vid = "rs%d" % (5000 + k) if k % 5 else "."
        names = [name for _, name in alts]
        used = list(names)
        if k % 6 == 1 and len(used) > 1:
            used = used[:-1]  # an ALT no consequence mentions: both columns {}
        if k % 6 == 2:
            used = used + ["TTT"]  # a consequence allele no ALT normalises to
        fields = [chrom, ("00%d" % pos) if k % 9 == 0 else str(pos), vid, ref, ",".join(a for a, _ in alts)]
        if k % 4:
            fields += [".", "PASS", "RS=%d;FREQ=1000Genomes:0.9,0.1" % k]
        o = {"input": "\t".join(fields), "id": vid, "assembly_name": "GRCh38", "seq_region_name": chrom.replace("chr", ""),
             "start": pos, "end": pos, "strand": 1, "allele_string": ref + "/" + "/".join(a for a, _ in alts),
             "most_severe_consequence": "intron_variant"}
        if k % 3 == 0:
            o["colocated_variants"] = [{"id": vid, "allele_string": "A/G", "variant_allele": "Q",
                                        "consequence_terms": ["not_a_term"], "frequencies": {"G": {"af": 0.25}}}]
        types = [t for i, t in enumerate(V.TYPES) if (k >> i) & 1 or (k % 16 == 0)] or ["intergenic"]
        for t in types:
            if n_csq is not None:
                n = n_csq if t == types[0] else 0
                o[t + "_consequences"] = [self.element(t, used[0], k + j) for j in range(n)]
                continue
            n = 1 if t == "intergenic" else rng.randrange(1, 7 if t == "transcript" else 4)
            o[t + "_consequences"] = [self.element(t, rng.choice(used), k + j) for j in range(n)]  # interleaved
        if k % 7 == 0:
            o.setdefault("motif_feature_consequences", [])
        return o

    def element(self, ctype, allele, k):
        el = super().element(ctype, allele, k)
        if k % 4 == 2:  # numbers, literals and escapes the device copies
            el.update(sift_score=0.01, polyphen_score=1.0, cdna_start=123456789012345, distance=0, canonical=True,
                      appris=None, ccds=False, protein="p.Ala\tVal\n\r\b\f")
        return el

    def line(self, host_kind=None):
        if host_kind is None or host_kind in V.HOST_KINDS:
            return super().line(host_kind)
        o = self.obj()
        first = next(t + "_consequences" for t in V.TYPES if o.get(t + "_consequences"))
        el = o[first][0]
        if host_kind == "no_input":
            del o["input"]
            return V.dumps(o)
        if host_kind == "four_fields":
            o["input"] = "\t".join(o["input"].split("\t")[:4])
            return V.dumps(o)
        if host_kind == "numeric_id":
            f = o["input"].split("\t")
            f[2] = "12345"
            o["input"] = "\t".join(f)
            return V.dumps(o)
        if host_kind == "backslash_ref":
            f = o["input"].split("\t")
            return V.dumps(o).replace('\\t%s\\t' % f[3], '\\t\\u0041%s\\t' % f[3][1:], 1)
        if host_kind == "utf8_value":
            el["note"] = "café"
            return json.dumps(o, separators=(",", ":"), ensure_ascii=False)
        el["marker"] = "@@"
        text = V.dumps(o)
        value = {"escaped_slash": '"a\\/b"', "escaped_u": '"\\u0041"', "exponent": "1e-05", "trailing_zero": "0.10",
                 "minus_zero": "-0"}[host_kind]
        return text.replace('"@@"', value, 1)


def golden_lines(rows, seed: int, n: int):
    """``(line, host kind or None)``: one line in sixteen is a host case, the kinds in turn."""
    gen = RowsLineGenerator(V.combos_of(rows), seed)
    out, h = [], 0
    for k in range(n):
        kind = None
        if k % 16 == 5:
            kind = HOST_KINDS[h % len(HOST_KINDS)]
            h += 1
        out.append((gen.line(kind), kind))
    n_host = sum(kind is not None for _, kind in out)
    assert 10 * (len(out) - n_host) >= 9 * len(out), (n_host, len(out))  # at least nine in ten are the device's
    return out


def export_text(keys) -> bytes:
    """An export over the metaseq ids ``keys`` (in file order, repeats included): hits, misses, a
    record with ``vep_output`` set, two primary keys of one id, a header and a short line."""
    seen, lines = set(), ["record_primary_key\tmetaseq_id\tvep_output"]
    for i, k in enumerate(keys):
        if k in seen:
            continue
        seen.add(k)
        if i % 11 == 3:
            continue  # not in the export: the table row stays unmatched
        pk = k + ":rs%d" % i if i % 3 else k
        third = ["\\N", "", None, '{"id": "x"}'][i % 4] if i % 13 else '{"set": 1}'
        lines.append(pk + "\t" + k + ("" if third is None else "\t" + third))
        if i % 17 == 5:
            lines.append(pk + "_b\t" + k + "\t\\N")  # a second primary key of the id
        if i % 19 == 7:
            c, p, r, a = k.split(":")
            lines.append("%s:%d:%s:%s\t%s:%d:%s:%s\t\\N" % (c, int(p) + 100000, r, a, c, int(p) + 100000, r, a))  # a miss
    lines.append("short")
    return ("\n".join(lines) + "\n").encode("utf-8")


def read_golden(path=GOLDEN_FILE):
    """``{"lines": [(ranking name, host kind or None, outcome, line bytes, rows or None)], "export": bytes,
    "updates": {(adsp, update_existing): text}}``; outcome ``ok``, ``rerank`` or ``raise:<class>``; rows
    ``[[metaseq id, most severe, ranked], ...]``."""
    out = {"lines": [], "export": b"", "updates": {}, "files": {}}
    with gzip.open(path, "rt", encoding="utf-8", newline="\n") as fh:
        for row in fh:
            f = row.rstrip("\n").split("\t")
            if f[0] == "L":
                out["lines"].append((f[1], None if f[2] == "-" else f[2], f[3], f[4].encode("utf-8"),
                                     json.loads(f[5]) if f[3] == "ok" else None))
            elif f[0] == "K":
                out["files"][f[1]] = json.loads(f[2])
            elif f[0] == "E":
                out["export"] = json.loads(f[1]).encode("utf-8")
            elif f[0] == "U":
                out["updates"][(f[1] == "1", f[2] == "1")] = json.loads(f[3])
    return out


def loadable(golden, name):
    """The lines of ranking ``name`` a table build takes (``ok`` and ``rerank``), with their rows."""
    return [(line, kind, outcome, rows) for n, kind, outcome, line, rows in golden["lines"]
            if n == name and not outcome.startswith("raise")]


TABLE_ARRAYS = ("keys", "key_off", "rkeys", "rkey_off", "json", "json_off", "json_len", "line_start", "flags")


def assert_same_table(got, want):
    """Two VepRowsTable (the device's and the host entries'), array for array and byte for byte."""
    assert got.n_rows == want.n_rows
    assert got.counts == want.counts
    assert got.unranked == want.unranked
    for name in TABLE_ARRAYS:
        a, b = getattr(got, name).cpu().numpy(), getattr(want, name).cpu().numpy()
        assert a.shape == b.shape, name
        if not np.array_equal(a, b):
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{name}[{at}]: {a[at]} != {b[at]}")


def table_rows(t):
    """``[(metaseq id, most severe, ranked)]`` of a table, in row order."""
    keys, ko = t.keys.cpu().numpy().tobytes(), t.key_off.cpu().numpy()
    js, jo, jl = t.json.cpu().numpy().tobytes(), t.json_off.cpu().numpy(), t.json_len.cpu().numpy()
    out = []
    for r in range(t.n_rows):
        ms, ranked = js[jo[r]:jo[r] + jl[r]].decode("utf-8").split("\t")
        out.append((keys[ko[r]:ko[r + 1]].decode("utf-8"), ms, ranked))
    return out


def one_element_line(element_text: str, allele: str = "G", ref: str = "A", alt: str = "G") -> str:
    """A line with one transcript consequence whose text is ``element_text`` (compact JSON of an object
    that holds ``variant_allele`` and ``consequence_terms``)."""
    return ('{"input":"1\\t100\\trs1\\t%s\\t%s","id":"rs1","transcript_consequences":[%s]}' % (ref, alt, element_text))


def padded_element(k: int) -> str:
    """An element whose first string value is padded by k bytes: over k = 0..130 every structural ','
    and ':', an escaped quote, an even and an odd run of backslashes, numbers at their first byte and
    the closing '}' meet every lane and both sides of a 64-byte edge."""
    el = {"pad": "x" * k, "variant_allele": "G", "note": 'a"b', "even": "c\\", "odd": 'd\\"e', "colon": "k:v,w",
          "score": -0.022, "n": 12, "flag": True, "none": None, "consequence_terms": ["missense_variant"],
          "domains": [{"db": "Pfam", "name": "PF1"}]}
    return V.dumps(el)


def sized_element(nbytes: int) -> str:
    """An element of exactly ``nbytes`` input bytes."""
    term = min((c for c, _ in V.read_ranking_rows() if "," not in c), key=len)  # (the shortest ranked term)
    el = {"variant_allele": "G", "consequence_terms": [term], "p": ""}
    el["p"] = "y" * (nbytes - len(V.dumps(el)))
    text = V.dumps(el)
    assert len(text) == nbytes, (len(text), nbytes)
    return text


def order_line(n: int) -> str:
    """A line of n consequences on one allele (order numbers 0 .. n - 1)."""
    els = ",".join('{"variant_allele":"G","consequence_terms":["intron_variant"],"k":%d}' % i for i in range(n))
    return '{"input":"1\\t100\\trs1\\tA\\tG","id":"rs1","transcript_consequences":[%s]}' % els


def edge_lines():
    """The element renderer's edges: the padded element over 0..130, elements of exactly 63, 64, 65 and
    128 input bytes."""
    return [one_element_line(padded_element(k)) for k in range(131)] + \
        [one_element_line(sized_element(n)) for n in (63, 64, 65, 128)]


def order_lines():
    """Order numbers 9|10, 99|100 and 511 (the digit-count edges of the suffix), and 513 consequences (a host line)."""
    return [order_line(n) for n in (10, 11, 100, 101, 512, 513)]


def empty_row_lines():
    """A row without consequences beside one with; a line all of whose rows have none; a line without arrays;
    an ALT given twice; an empty ALT field."""
    el = '{"variant_allele":"G","consequence_terms":["intron_variant"]}'
    return [one_element_line(el, alt="G,T"), one_element_line(el, alt="C,T"),
            '{"input":"1\\t100\\trs1\\tA\\tG","id":"rs1"}', one_element_line(el, alt="G,G"), one_element_line(el, alt="")]


def small_lines(n: int):
    return ['{"input":"%s\\t%d\\t.\\tA\\t%s","id":"v%d","intergenic_consequences":[{"variant_allele":"%s",'
            '"consequence_terms":["intergenic_variant"]}]}' % (1 + i % 22, 100 + i, "CGT"[i % 3], i, "CGT"[i % 3])
            for i in range(n)]


def random_device_lines(rows, seed: int, n: int):
    gen = RowsLineGenerator(V.combos_of(rows), seed)
    return [gen.line() for _ in range(n)]


def expected_rows(lines, ranking):
    """What vep_rows_line gives for the lines, back to back (a line that needs a re-rank gives none)."""
    from annotatedvdb_amd.vep_consequences import UnrankedCombination
    from annotatedvdb_amd.vep_rows import vep_rows_line
    out = []
    for line in lines:
        try:
            out += [tuple(r) for r in vep_rows_line(line, ranking)]
        except UnrankedCombination:
            pass
    return out


def join_cases():
    """``(table lines, export, what to expect)`` of the small join: hit, miss, skipped, two keys of one id,
    and an id two lines carry (the second line's terms differ)."""
    def line(pos, term):
        return ('{"input":"1\\t%d\\trs1\\tA\\tG","id":"rs1","transcript_consequences":[{"variant_allele":"G",'
                '"consequence_terms":["%s"]}]}' % (pos, term))
    lines = [line(100, "intron_variant"), line(200, "missense_variant"), line(100, "stop_gained"),
             line(300, "intron_variant")]
    export = (b"pk_a\t1:100:A:G\t\\N\npk_b\t1:100:A:G\t\npk_c\t1:200:A:G\t{\"id\": 1}\npk_d\t1:999:A:G\t\\N\n"
              b"pk_e\t1:200:A:G\n")
    return lines, export

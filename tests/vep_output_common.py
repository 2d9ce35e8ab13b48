"""Helpers of the K18c tests: the generator of VEP ``--json`` lines whose ``input`` has eight fields with a
dbSNP-like INFO and whose top-level members come in every arrangement the cleaned result's kernel has to
get right, the golden's reader, edge-case lines for the member drop and the wave-per-row update write, and
the comparison of a device table's cleaned texts with the host entries'."""

import gzip
import json
import os

import numpy as np

import vep_common as V
import vep_rows_common as R

GOLDEN_FILE = os.path.join(V.GOLDEN, "vep_output.tsv.gz")
ALG_ID = R.ALG_ID
DROPPED = ("colocated_variants",) + tuple(t + "_consequences" for t in V.TYPES)

# the new reasons a line's cleaned text is the host's (annotatedvdb_amd._native.VEPOUT_REASONS), as the generator
# builds them; the reason depends on the form of ``input``'s dict: identityOnly reads five fields only
NEW_HOST_KINDS = ("kept_exponent", "kept_escape", "kept_utf8", "five_fields", "info_exponent", "qual_exponent",
                  "info_backslash", "info_repeat", "numeric_info", "allele_dot")
HOST_KINDS = R.HOST_KINDS + NEW_HOST_KINDS
_FULL = dict(kept_exponent="kept_text", kept_escape="kept_text", kept_utf8="kept_text", five_fields="eight_fields",
             info_exponent="input_value", qual_exponent="input_value", info_backslash="input_value",
             info_repeat="input_value", numeric_info="input_value", allele_dot="input_value")
_IDENTITY = dict(_FULL, five_fields=None, info_exponent=None, qual_exponent=None, info_backslash=None,
                 info_repeat=None, numeric_info=None)


def reason_of(kind, identity_only: bool):
    """The reason the cleaned text of a line of host kind ``kind`` is the host's, or None (the device's)."""
    if kind is None:
        return None
    if kind in R.REASON_OF:
        return R.REASON_OF[kind]
    return (_IDENTITY if identity_only else _FULL)[kind]


INFOS = ("RS=%(k)d;RSPOS=%(pos)d;dbSNPBuildID=144;SSR=0;SAO=0;VP=0x05000088000d000026000100;GENEINFO=SHOX#6473;WGT=1;"
         "VC=SNV;U3;INT;CFL;ASP;KGPhase3;CAF=0.9996,0.0003994;COMMON=0;TOPMED=0.99999203618756371,0.00000796381243628",
         ".",
         "RS=%(k)d;FREQ=1000Genomes:0.9,0.1|GnomAD:0.5,.;AF=0.25;NEG=-3;Z=0.0;DP=007;SMALL=0.00001234;VC=INT;R5",
         "AC=12;AN=200;SVTYPE=.;NOTE=a#b;K#1=v;BIG=12345678901234567890;F=1234567.125;ASP")


class OutputLineGenerator(R.RowsLineGenerator):
    """K18b's lines with eight (sometimes ten) fields in ``input``, kept members with nested arrays and
    objects, a dropped key's name inside a string and under ``colocated_variants``, and the members in turn:
    as they come, a dropped member first, one last, ``input`` in the middle and last, all five dropped
    members adjacent, none dropped, and a line that is only ``input``."""

    def obj(self, n_csq=None):
        o = super().obj(n_csq)
        k = self.n
        f = o["input"].split("\t")[:5]
        f += [(".", "100", "29.5", "0.001")[k % 4], ("PASS", ".", "q10;s50")[k % 3],
              INFOS[k % len(INFOS)] % {"k": k, "pos": 20000 + k}]
        if k % 10 == 3:
            f += ["GT", "0/1"]  # more than eight fields: ignored
        o["input"] = "\t".join(f)
        if k % 4 == 1:
            o["custom_annotations"] = {"panel": [1, 2.5, {"input": "not the input", "hits": [True, None, "x,y:z"]}],
                                       "colocated_variants": "a name that is no member here"}
        if k % 5 == 2:
            o["note"] = 'see "transcript_consequences": [] and ,"colocated_variants": in the text'
        if k % 3 == 0 and "colocated_variants" in o:
            o["colocated_variants"][0]["input"] = "1\t2\t3"
            o["colocated_variants"][0]["transcript_consequences"] = [{"x": 1}]
        how = k % 8 if n_csq is None else 0
        csq = {key: o.pop(key) for key in list(o) if key.endswith("_consequences")}
        col = o.pop("colocated_variants", None)
        if how == 1:  # a dropped member first
            return dict([("colocated_variants", col or [])] + list(o.items()) + list(csq.items()))
        if how == 2:  # a dropped member last, input in the middle
            inp = o.pop("input")
            rest = list(o.items())
            return dict(rest[:3] + [("input", inp)] + rest[3:] + list(csq.items()) + [("colocated_variants", col or [])])
        if how == 3:  # input last, the dropped members before it
            inp = o.pop("input")
            return dict(list(csq.items()) + list(o.items()) + [("input", inp)])
        if how == 4:  # all five dropped members, adjacent, between kept ones
            rest = list(o.items())
            five = {key: csq.get(key, []) for key in DROPPED[1:]}
            return dict(rest[:2] + [("colocated_variants", col or [])] + list(five.items()) + rest[2:])
        if how == 5:  # none dropped
            return o
        if how == 6:  # only input
            return {"input": o["input"]}
        if how == 7:  # dropped members first and last, kept ones between
            items = list(csq.items())
            return dict(items[:1] + list(o.items()) + items[1:] + ([("colocated_variants", col)] if col else []))
        out = dict(o)
        out.update(csq)
        if col is not None:
            out["colocated_variants"] = col
        return out

    def line(self, host_kind=None):
        if host_kind is None or host_kind in R.HOST_KINDS:
            while host_kind is not None and (self.n + 1) % 8 in (5, 6):
                self.n += 1  # (K18a's and K18b's kinds edit a consequence: not a line without any)
            return super().line(host_kind)
        o = self.obj()
        f = o["input"].split("\t")

        def with_input(fields):
            o["input"] = "\t".join(fields)
            return V.dumps(o)

        if host_kind == "five_fields":
            return with_input(f[:5])
        if host_kind == "info_exponent":
            return with_input(f[:7] + ["RS=5;END=1E5"])
        if host_kind == "qual_exponent":
            return with_input(f[:5] + ["1e3"] + f[6:8])
        if host_kind == "info_backslash":
            return with_input(f[:7] + ["RS=5;CSQ=a\\x2cb"])
        if host_kind == "info_repeat":
            return with_input(f[:7] + ["RS=5;AF=0.5;RS=6"])
        if host_kind == "numeric_info":
            return with_input(f[:7] + ["5"])
        if host_kind == "allele_dot":
            return with_input(f[:3] + ["A.", "G"] + f[5:8])
        if host_kind == "kept_utf8":
            o["remark"] = "café"
            return json.dumps(o, separators=(",", ":"), ensure_ascii=False)
        o["marker"] = "@@"
        return V.dumps(o).replace('"@@"', {"kept_exponent": "1e-05", "kept_escape": '"a\\/b"'}[host_kind], 1)


def golden_lines(rows, seed: int, n: int):
    """``(line, host kind or None)``: one line in sixteen is a host case, the kinds in turn."""
    gen = OutputLineGenerator(V.combos_of(rows), seed)
    out, h = [], 0
    for k in range(n):
        kind = None
        if k % 16 == 5:
            kind = HOST_KINDS[h % len(HOST_KINDS)]
            h += 1
        out.append((gen.line(kind), kind))
    n_host = sum(kind is not None for _, kind in out)
    assert 10 * n_host <= len(out), (n_host, len(out))  # host cases are at most one tenth of the lines
    return out


def read_golden(path=GOLDEN_FILE):
    """``{"lines": [(host kind or None, {identity_only: (outcome, cleaned text or None, rows or None)}, line bytes)],
    "export": bytes, "updates": {(adsp, update_existing): text}}``; outcome ``ok``, ``rerank`` or
    ``raise:<class>``; rows ``[[metaseq id, most severe, ranked], ...]``."""
    out = {"lines": [], "export": b"", "updates": {}}
    with gzip.open(path, "rt", encoding="utf-8", newline="\n") as fh:
        for row in fh:
            f = row.rstrip("\n").split("\t")
            if f[0] == "L":
                forms = {}
                for identity, at in ((False, 3), (True, 6)):
                    ok = f[at] == "ok"
                    forms[identity] = (f[at], json.loads(f[at + 1]) if ok else None, json.loads(f[at + 2]) if ok else None)
                out["lines"].append((None if f[1] == "-" else f[1], forms, f[2].encode("utf-8")))
            elif f[0] == "E":
                out["export"] = json.loads(f[1]).encode("utf-8")
            elif f[0] == "U":
                out["updates"][(f[1] == "1", f[2] == "1")] = json.loads(f[3])
    return out


def loadable(golden, identity_only: bool):
    """The lines a table build takes in the given form (``ok`` and ``rerank``):
    ``[(line, kind, outcome, cleaned, rows)]``."""
    return [(line, kind) + forms[identity_only] for kind, forms, line in golden["lines"]
            if not forms[identity_only][0].startswith("raise")]


CLEANED_ARRAYS = ("cleaned", "cleaned_off", "cleaned_len", "row_entry", "cleaned_flags")


def assert_same_cleaned(got, want):
    """The K18c members of two VepRowsTable (the device's and the host entries'), array for array."""
    R.assert_same_table(got, want)
    assert got.cleaned_counts == want.cleaned_counts
    for name in CLEANED_ARRAYS:
        a, b = getattr(got, name).cpu().numpy(), getattr(want, name).cpu().numpy()
        assert a.shape == b.shape, name
        if not np.array_equal(a, b):
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{name}[{at}]: {a[at]} != {b[at]}")


def cleaned_texts(t):
    """The cleaned text of every entry (line) of a table, in line order."""
    blob, off, ln = t.cleaned.cpu().numpy().tobytes(), t.cleaned_off.cpu().tolist(), t.cleaned_len.cpu().tolist()
    return [blob[a:a + n].decode("utf-8") for a, n in zip(off, ln)]


def row_cleaned(t):
    """The cleaned text every table row points at, in row order."""
    texts = cleaned_texts(t)
    return [texts[e] for e in t.row_entry.cpu().tolist()[:t.n_rows]]


INPUT8 = "1\\t100\\trs1\\tA\\tG\\t.\\tPASS\\tRS=1;ASP"
CSQ = '"transcript_consequences":[{"variant_allele":"G","consequence_terms":["intron_variant"]}]'


def padded_drop_line(k: int) -> str:
    """A kept string of k bytes in front of a dropped member, a kept one, ``input`` and another dropped member:
    over k = 0..130 every key quote, colon, member edge and the carry of "a kept member came before" meet
    every lane and both sides of a 64-byte edge."""
    return ('{"pad":"%s","colocated_variants":[{"id":"x\\"y","input":"1\\t2"}],"kept":{"a":[1,2.5,"c\\\\"],"b":null},'
            '"input":"%s","id":"rs1",%s,"end":7}' % ("x" * k, INPUT8, CSQ))


def padded_input_line(k: int) -> str:
    """The same with the dropped member first and the padding right in front of ``input``."""
    return '{%s,"pad":"%s","input":"%s","colocated_variants":[],"id":"rs1"}' % (CSQ, "y" * k, INPUT8)


def sized_member_line(nbytes: int, dropped: bool) -> str:
    """A line with a member of exactly ``nbytes`` bytes (key, colon and value), kept or dropped."""
    key = '"colocated_variants":' if dropped else '"kept_member":'
    member = key + '"' + "m" * (nbytes - len(key) - 2) + '"'
    assert len(member) == nbytes
    return '{"id":"rs1",%s,"input":"%s",%s}' % (member, INPUT8, CSQ)


def sized_line(nbytes: int) -> str:
    """A line of exactly ``nbytes`` bytes: only ``input`` and a padding member."""
    base = '{"input":"1\\t100\\t.\\tA\\tG\\t.\\t.\\t.","p":""}'
    line = base.replace('"p":""', '"p":"%s"' % ("z" * (nbytes - len(base))))
    assert len(line) == nbytes, (len(line), nbytes)
    return line


def three_block_drop_line() -> str:
    """A dropped member that spans three blocks, between two kept ones."""
    return '{"a":1,"colocated_variants":[{"long":"%s"}],"input":"%s","z":[2]}' % ("q" * 150, INPUT8)


def nested_line(depth: int) -> str:
    """A kept member nested ``depth`` levels deep (the top-level object is level 1)."""
    value = "1"
    for i in range(depth - 1):
        value = ("[%s]" if i % 2 else '{"k":%s}') % value
    return '{"input":"%s","deep":%s,"id":"rs1"}' % (INPUT8, value)


def edge_lines():
    return ([padded_drop_line(k) for k in range(131)] + [padded_input_line(k) for k in range(131)] +
            [sized_member_line(n, d) for n in (63, 64, 65, 128) for d in (False, True)] +
            [sized_line(64), sized_line(128), three_block_drop_line(), nested_line(V_MAX_DEPTH),
             '{"colocated_variants":[],%s,"input":"%s"}' % (CSQ, INPUT8),  # everything but input dropped
             '{"input":"%s"}' % INPUT8])


V_MAX_DEPTH = 64  # AVDB_VEP_MAX_DEPTH


def small_lines(n: int):
    return ['{"input":"%s\\t%d\\t.\\tA\\t%s\\t.\\t.\\tRS=%d","id":"v%d","intergenic_consequences":[{"variant_allele":"%s",'
            '"consequence_terms":["intergenic_variant"]}]}' % (1 + i % 22, 100 + i, "CGT"[i % 3], i, i, "CGT"[i % 3])
            for i in range(n)]


def random_device_lines(rows, seed: int, n: int):
    gen = OutputLineGenerator(V.combos_of(rows), seed)
    return [gen.line() for _ in range(n)]


def boundary_join_cases(ranking, alg_id: int, adsp: bool, identity_only: bool):
    """Twelve table lines and their export records: for the head, the body, the cleaned text and the tail of an
    update row in turn, a row in which that part ends 63, 64 and 65 bytes past a 64-byte boundary of the row
    (the primary key is padded: every later part moves with it).  Body and cleaned text are longer than a block.
    Returns ``(lines, export, [(part, bytes past the boundary)])``."""
    from annotatedvdb_amd.vep_rows import vep_output_line, vep_rows_line
    lines, recs, want = [], [], []
    for part in range(4):
        for past in (63, 64, 65):
            pos = 1000 + len(lines)
            line = ('{"input":"1\\t%d\\trs1\\tA\\tG\\t.\\tPASS\\tRS=1","id":"rs1","pad":"%s","transcript_consequences":'
                    '[{"variant_allele":"G","consequence_terms":["intron_variant"],"pad":"%s"}]}' % (pos, "c" * 70, "b" * 40))
            key = "1:%d:A:G" % pos
            (_, ms, ranked), = vep_rows_line(line, ranking)
            ends = [len(key) + 1 + len("\tchr1\t")]
            ends.append(ends[0] + len(ms) + 1 + len(ranked))
            ends.append(ends[1] + 1 + len(vep_output_line(line, identity_only)))
            ends.append(ends[2] + 1 + len(str(alg_id)) + (5 if adsp else 0) + 1)
            pk = key + ":" + "p" * ((past - ends[part]) % 64)
            assert (ends[part] + len(pk) - len(key) - 1) % 64 == past % 64
            lines.append(line)
            recs.append(pk + "\t" + key + "\t\\N\n")
            want.append((part, past))
    return lines, "".join(recs).encode("ascii"), want


def expected_update_text(lines, export: bytes, ranking, alg_id: int, adsp: bool, update_existing: bool,
                         identity_only: bool) -> str:
    """The update rows of the export against the lines, from vep_rows_line and vep_output_line."""
    from annotatedvdb_amd.vep_consequences import UnrankedCombination
    from annotatedvdb_amd.vep_rows import vep_output_line, vep_rows_line
    table = {}
    for line in lines:
        try:
            rows = vep_rows_line(line, ranking)
        except UnrankedCombination:
            continue
        cleaned = vep_output_line(line, identity_only)
        for key, ms, ranked in rows:
            table[key] = (ms, ranked, cleaned)
    return join_text(table, export, alg_id, adsp, update_existing)


def join_text(table, export: bytes, alg_id: int, adsp: bool, update_existing: bool) -> str:
    """``table``: metaseq id -> (most severe, ranked, cleaned), the last line of an id answering."""
    out = []
    for rec in export.decode("utf-8").split("\n")[:-1]:
        f = rec.split("\t")
        if len(f) < 2 or f[0] == "record_primary_key" or f[1] not in table:
            continue
        if not update_existing and len(f) > 2 and f[2] not in ("", "\\N"):
            continue
        ms, ranked, cleaned = table[f[1]]
        t = [f[0], "chr" + f[1].split(":")[0], ms, ranked, cleaned, str(alg_id)] + (["true"] if adsp else [])
        out.append("\t".join(t) + "\n")
    return "".join(out)

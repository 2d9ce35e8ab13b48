"""Helpers of the K18d tests: the seeded generator of VEP ``--json`` lines whose ``colocated_variants`` and INFO
``FREQ`` come in every arrangement the ``allele_frequencies`` kernels have to get right (on top of K18c's and
K18b's generators), the golden's reader, edge-case lines for the two walks and the wave-per-row update write,
and the comparison of a device table's frequency texts with the host entries'."""

import gzip
import json
import os

import numpy as np

import vep_common as V
import vep_output_common as O
import vep_rows_common as R

GOLDEN_FILE = os.path.join(V.GOLDEN, "vep_freq.tsv.gz")
ALG_ID = R.ALG_ID
FORMS = [(False, False), (False, True), (True, False), (True, True)]  # (identity_only, match_refsnp)

# The new host cases, as the generator builds them, and the reason (annotatedvdb_amd._native.VEPFREQ_REASONS) each
# is counted under: always, or by form.  A kind whose reason is None in a form is the device's there.
NEW_HOST_KINDS = ("cv_object", "cv_empty", "cv_string_element", "no_allele_string", "no_id", "dup_frequencies",
                  "dup_member", "cv_escape", "cv_utf8", "frequencies_null", "allele_number", "member_string",
                  "member_exponent", "members_65", "vep_gmaf", "seven_fields", "info_backslash", "rs_text",
                  "freq_bare", "freq_no_colon", "freq_hash", "freq_exponent", "freq_few", "same_allele")
HOST_KINDS = R.HOST_KINDS + NEW_HOST_KINDS
_ALWAYS = dict(cv_object="colocated", cv_empty="colocated", cv_string_element="colocated",
               no_allele_string="element_key", dup_frequencies="repeated_key", dup_member="repeated_key",
               cv_escape="colocated_bytes", cv_utf8="colocated_bytes", frequencies_null="not_object",
               allele_number="not_object", member_string="member_value", member_exponent="member_value",
               members_65="members", same_allele="same_allele")
_FULL_ONLY = dict(vep_gmaf="gmaf", seven_fields="info", info_backslash="info", freq_bare="freq_item",
                  freq_no_colon="freq_item", freq_hash="freq_item", freq_exponent="freq_number", freq_few="freq_number")


def reason_of(kind, identity_only: bool, match_refsnp: bool):
    """The reason a line of host kind ``kind`` is the host's in the given form, or None (the device's)."""
    if kind is None:
        return None
    if kind in R.REASON_OF:
        return R.REASON_OF[kind]
    if kind in _ALWAYS:
        return _ALWAYS[kind]
    if kind in _FULL_ONLY:
        return None if identity_only else _FULL_ONLY[kind]
    if kind == "no_id":  # covar['id'] is read only where an id is matched (the line's ID field holds one)
        return "element_key" if match_refsnp else None
    if kind == "rs_text":  # INFO RS is read only where an id is matched and the ID field has none
        return "info" if match_refsnp and not identity_only else None
    raise KeyError(kind)


GNOMAD = ("gnomade", "gnomade_afr", "gnomadg_nfe", "gnomad_sas", "gnomadg", "xgnomadx")
GENOMES = ("af", "afr", "amr", "eas", "eur", "sas", "aaa", "e")
ESP = ("aa", "ea")
VALUES = (0.25, 0.0312, 1, 0, 0.5, 1.234e-05, 3e-06, 6.573e-10, 0.999999, 0.0001, 12, 1.5e-300)


class FreqLineGenerator(O.OutputLineGenerator):
    """K18c's lines with ``colocated_variants`` absent and with 1, 2 and 3 elements, COSMIC elements first, last
    and alone, elements without ``frequencies``, the chosen one in each position, ids that match and do not match
    ``input``'s rs id or INFO ``RS``, allele keys ``-``, bases and insertions, multi-allelic lines where only some
    ALTs have frequencies, every combination of groups with members in mixed order, values in positional and
    exponent form, and INFO ``FREQ`` absent, with ``.`` and ``0`` columns, with the three group names (the nested
    merge) and with new names."""

    def members(self, mode: int):
        rng = self.rng
        pools = [(GNOMAD, GENOMES, ESP), (GNOMAD,), (GENOMES,), (ESP,), (), (GNOMAD, ESP), (GENOMES, ESP)][mode % 7]
        keys = [k for pool in pools for k in rng.sample(pool, rng.randrange(1, len(pool) + 1))]
        rng.shuffle(keys)  # the groups alternate member by member
        return {k: rng.choice(VALUES) for k in keys}

    def covar(self, vid, names, how, mode):
        """how: 'freq' (qualifies), 'nofreq', 'cosmic' (with frequencies)."""
        rng = self.rng
        el = {"id": vid, "start": 100, "allele_string": "COSMIC_MUTATION" if how == "cosmic" else "A/G", "strand": 1}
        if how != "nofreq":
            alleles = list(names) if rng.random() < 0.5 else names[:1]  # only some ALTs have frequencies
            if rng.random() < 0.3:
                alleles.insert(rng.randrange(len(alleles) + 1), "TTTT")  # an allele no ALT normalises to
            el["frequencies"] = {a: self.members(mode + i) for i, a in enumerate(alleles)}
            if rng.random() < 0.3:  # the three keys in another order, something nested between them
                el = {"frequencies": el["frequencies"], "pubmed": [1, 2], "var_synonyms": {"ClinVar": ["RCV1"]},
                      "allele_string": el["allele_string"], "id": el["id"], "end": 100}
        return el

    def obj(self, n_csq=None):
        o = super().obj(n_csq)
        k = self.n
        f = o["input"].split("\t")
        _, _, alts = R.SITES[k % len(R.SITES)]
        names = [name for _, name in alts]
        rs = 5000 + k
        own = f[2] if f[2] != "." else "rs%d" % rs  # the id get_refsnp gives: the ID field, else 'rs' + INFO RS
        other = "rs%d" % (rs + 1)
        # INFO: RS (the line's own number, or none), FREQ with one column per allele
        n_cols = len(alts) + 1
        def cols(i):
            vals = ["0.9"] + [("0.1", ".", "0", "0.00001234", "5", "0.25", "007", "1.")[(k + i + j) % 8] for j in range(n_cols - 1)]
            return ",".join(vals)
        pops = [[], ["GnomAD", "Korea1K"], ["1000Genomes", "ESP"], ["TOPMED"], ["GnomAD", "1000Genomes", "ESP", "dbGaP_PopFreq"],
                ["Estonian", "GnomAD"], ["ALSPAC"]][(k // 2) % 7]
        info = ["RS=%d" % rs] if k % 7 != 3 else []
        info += ["dbSNPBuildID=144", "VC=SNV", "ASP"]
        if pops:
            info.insert(2, "FREQ=" + "|".join("%s:%s" % (p, cols(i)) for i, p in enumerate(pops)))
        f[7] = ";".join(info)
        o["input"] = "\t".join(f)
        mode = k // 3
        arrangement = (k // 8) % 12
        c = lambda how, vid=own, m=mode: self.covar(vid, names, how, m)  # noqa: E731
        cv = {0: None,
              1: [c("freq")],
              2: [c("nofreq")],
              3: [c("cosmic")],
              4: [c("cosmic", "COSV1"), c("freq")],
              5: [c("freq"), c("cosmic", "COSV1")],
              6: [c("nofreq"), c("freq")],
              7: [c("freq"), c("cosmic", "COSV2"), c("nofreq", other)],
              8: [c("nofreq", other), c("freq"), c("cosmic", "COSV3")],
              9: [c("freq", other, mode + 1), c("nofreq"), c("freq")],
              10: [c("freq"), c("cosmic", "COSV4"), c("freq", other, mode + 2)],
              11: [c("nofreq"), c("cosmic", "COSV5")]}[arrangement]
        o.pop("colocated_variants", None)
        if cv is not None:
            items = list(o.items())
            at = (k // 5) % (len(items) + 1)  # first, in the middle and last
            o = dict(items[:at] + [("colocated_variants", cv)] + items[at:])
        return o

    def line(self, host_kind=None):
        if host_kind is None or host_kind in R.HOST_KINDS:
            return super().line(host_kind)
        while (self.n + 1) % 8 in (5, 6):
            self.n += 1  # (as K18c: a line with consequences)
        o = self.obj()
        f = o["input"].split("\t")
        own = f[2] if f[2] != "." else "rs1"
        o.pop("colocated_variants", None)
        fr = {a: {"af": 0.5, "gnomade": 0.25, "aa": 0.1} for a in ("G", "-", "GT", "C", "T", "CG", "A")}  # every site's ALTs
        good = {"id": own, "allele_string": "A/G", "frequencies": fr}

        def done(cv=None, fields=None, edit=None):
            if cv is not None:
                o["colocated_variants"] = cv
            if fields is not None:
                o["input"] = "\t".join(fields)
            text = V.dumps(o)
            return edit(text) if edit else text

        def info(value):
            return f[:7] + [value]

        n_cols = f[4].count(",") + 2
        col = ",".join(["0.5"] * n_cols)
        if host_kind == "cv_object":
            return done(good)
        if host_kind == "cv_empty":
            return done([])
        if host_kind == "cv_string_element":
            return done(["x"])  # ('frequencies' in "x" is False: no frequencies, and nothing raised)
        if host_kind == "no_allele_string":
            return done([good, {"id": "rs9", "frequencies": fr}])
        if host_kind == "no_id":
            return done([good, {"allele_string": "A/G", "frequencies": fr}], f[:2] + ["rs77"] + f[3:])
        if host_kind == "dup_frequencies":
            return done([good], edit=lambda t: t.replace('"frequencies":{', '"frequencies":{"T":{"af":0.1}},"frequencies":{', 1))
        if host_kind == "dup_member":
            return done([good], edit=lambda t: t.replace('{"af":0.5,', '{"af":0.5,"af":0.75,'))
        if host_kind == "cv_escape":
            return done([dict(good, note="@@")], edit=lambda t: t.replace('"@@"', '"a\\u0041"', 1))
        if host_kind == "cv_utf8":
            o["colocated_variants"] = [dict(good, note="café")]
            return json.dumps(o, separators=(",", ":"), ensure_ascii=False)
        if host_kind == "frequencies_null":
            return done([{"id": own, "allele_string": "A/G", "frequencies": None}])
        if host_kind == "allele_number":
            return done([dict(good, frequencies=dict(fr, TTT=0.5))])
        if host_kind == "member_string":
            return done([dict(good, frequencies={a: dict(m, src="x") for a, m in fr.items()})])
        if host_kind == "member_exponent":
            return done([dict(good, frequencies={a: dict(m, tiny="@@") for a, m in fr.items()})],
                        edit=lambda t: t.replace('"@@"', "1e-5"))
        if host_kind == "members_65":
            many = {"p%02d" % i: 0.5 for i in range(65)}
            return done([dict(good, frequencies={a: many for a in fr})])
        if host_kind == "vep_gmaf":
            return done([dict(good, frequencies={a: dict(m, gmaf=0.5) for a, m in fr.items()})],
                        info("RS=5;FREQ=1000Genomes:" + col))
        if host_kind == "seven_fields":
            return done([good], f[:7])
        if host_kind == "info_backslash":
            return done([good], info("RS=5;CSQ=a\\x2cb"))
        if host_kind == "rs_text":
            return done([good], f[:2] + ["."] + f[3:7] + ["RS=abc;ASP"])
        if host_kind == "freq_bare":
            return done([good], info("RS=5;FREQ"))
        if host_kind == "freq_no_colon":
            return done([good], info("RS=5;FREQ=GnomAD"))
        if host_kind == "freq_hash":
            return done([good], info("RS=5;FREQ=GnomAD#" + col))
        if host_kind == "freq_exponent":
            return done([good], info("RS=5;FREQ=GnomAD:" + ",".join(["1e-05"] * n_cols)))
        if host_kind == "freq_few":
            return done([good], info("RS=5;FREQ=GnomAD:0.9"))
        if host_kind == "same_allele":
            o = self.obj(1)  # (site 0 may not come up: the line is built from the ALT it has)
            f = o["input"].split("\t")
            first = f[4].split(",")[0]
            return done(None, f[:4] + [first + "," + first] + f[5:])
        raise KeyError(host_kind)


def golden_lines(rows, seed: int, n: int, every: int = 11):
    """``(line, host kind or None)``: one line in ``every`` is a host case, the kinds in turn."""
    gen = FreqLineGenerator(V.combos_of(rows), seed)
    out, h = [], 0
    for k in range(n):
        kind = None
        if k % every == 5:
            kind = HOST_KINDS[h % len(HOST_KINDS)]
            h += 1
        out.append((gen.line(kind), kind))
    assert h >= len(HOST_KINDS), (h, len(HOST_KINDS))  # every host kind at least once
    assert 10 * sum(kind is not None for _, kind in out) <= len(out)  # host cases are at most one tenth of the lines
    return out


def read_golden(path=GOLDEN_FILE):
    """``{"lines": [(host kind or None, {(identity_only, match_refsnp): (outcome, rows or None)}, line bytes)],
    "export": bytes, "updates": {(adsp, update_existing, vep_output): text}}``; outcome ``ok``, ``rerank`` or
    ``raise:<class>``; rows ``[[metaseq id, allele_frequencies, most severe, ranked, vep_output], ...]``."""
    out = {"lines": [], "export": b"", "updates": {}}
    with gzip.open(path, "rt", encoding="utf-8", newline="\n") as fh:
        for row in fh:
            f = row.rstrip("\n").split("\t")
            if f[0] == "L":
                forms = {}
                for i, form in enumerate(FORMS):
                    outcome = f[3 + 2 * i]
                    forms[form] = (outcome, json.loads(f[4 + 2 * i]) if outcome == "ok" else None)
                out["lines"].append((None if f[1] == "-" else f[1], forms, f[2].encode("utf-8")))
            elif f[0] == "E":
                out["export"] = json.loads(f[1]).encode("utf-8")
            elif f[0] == "U":
                out["updates"][(f[1] == "1", f[2] == "1", f[3] == "1")] = json.loads(f[4])
    return out


def loadable(golden, form):
    """The lines a table build takes in the given form (``ok`` and ``rerank``): ``[(line, kind, outcome, rows)]``."""
    return [(line, kind) + forms[form] for kind, forms, line in golden["lines"] if not forms[form][0].startswith("raise")]


FREQ_ARRAYS = ("freq", "freq_off", "freq_len", "freq_flags")


def assert_same_freq(got, want):
    """The K18d members of two VepRowsTable (the device's and the host entries'), array for array."""
    R.assert_same_table(got, want)
    assert got.freq_counts == want.freq_counts
    for name in FREQ_ARRAYS:
        a, b = getattr(got, name).cpu().numpy(), getattr(want, name).cpu().numpy()
        assert a.shape == b.shape, name
        if not np.array_equal(a, b):
            at = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{name}[{at}]: {a[at]} != {b[at]}")


def freq_texts(t):
    """The ``allele_frequencies`` text of every table row, in row order."""
    blob, off, ln = t.freq.cpu().numpy().tobytes(), t.freq_off.cpu().tolist(), t.freq_len.cpu().tolist()
    return [blob[a:a + n].decode("utf-8") for a, n in zip(off, ln)][:t.n_rows]


def expected_texts(lines, identity_only: bool, match_refsnp: bool):
    """What allele_frequencies_line gives for the lines, back to back."""
    from annotatedvdb_amd.vep_rows import allele_frequencies_line
    return [t for line in lines for _, t in allele_frequencies_line(line, identity_only, match_refsnp)]


# ---- edge-case lines --------------------------------------------------------------------------------
CSQ = O.CSQ


def member_text(n: int, alternate: bool = False) -> str:
    """An allele's object of n members: one group takes them all, or the three groups alternate member by member."""
    names = []
    for i in range(n):
        if not alternate or i % 3 == 0:
            names.append("gnomad%02d" % i)
        elif i % 3 == 1:
            names.append("p%02d" % i)
        else:
            names.append("aa" if i == 2 else "ea" if i == 5 else "q%02d" % i)
    return "{" + ",".join('"%s":%s' % (name, ("0.5", "1.234e-05", "1", "0.0312")[i % 4]) for i, name in enumerate(names)) + "}"


def padded_line(where: str, k: int, info: str = "RS=1;FREQ=GnomAD:0.9,0.1|Korea1K:0.8,0.2") -> str:
    """A line in which ``colocated_variants`` ('cv'), the chosen ``frequencies`` object ('fr') or the allele key
    ('key') begins k bytes into the line; the frequencies object spans more than three blocks."""
    inp = '"input":"1\\t100\\trs1\\tA\\tG\\t.\\tPASS\\t%s"' % info
    fr = '{"G":%s,"T":{"af":0.75,"gnomade":0.001},"C":{"eas":1}}' % member_text(14, True)
    assert len(fr) > 3 * 64
    head = '{"p":"'
    tail = '","colocated_variants":[{"frequencies":%s,"id":"rs1","allele_string":"A/G"}],' % fr
    mark = {"cv": '"colocated_variants"', "fr": '"frequencies":', "key": '"G":{'}[where]
    base = head + tail
    at = base.index(mark) + (len('"frequencies":') if where == "fr" else 0)
    pad = k - at
    assert pad >= 0, (where, k, at)
    line = head + "x" * pad + tail + inp + "," + CSQ + "}"
    assert line.index(mark) + (len('"frequencies":') if where == "fr" else 0) == k
    return line


def cosmic_split_line(k: int) -> str:
    """Two elements, the COSMIC one first, its ``"COSMIC_MUTATION"`` string beginning k bytes into the line: over
    k = 108..130 the string lies on both sides of a block edge and across it."""
    head = '{"p":"'
    tail = ('","colocated_variants":[{"frequencies":{"G":{"af":0.9}},"id":"COSV1","allele_string":"COSMIC_MUTATION"},'
            '{"allele_string":"A/G","id":"rs1","frequencies":{"G":{"af":0.1,"aa":0.2}}}],')
    at = len(head) + tail.index('"COSMIC_MUTATION"')
    line = head + "x" * (k - at) + tail + '"input":"1\\t100\\trs1\\tA\\tG\\t.\\tPASS\\tRS=1",' + CSQ + "}"
    assert line.index('"COSMIC_MUTATION"') == k
    return line


def members_line(n: int, alternate: bool = False, freq: bool = True) -> str:
    """An allele's object of n members (65: the host's)."""
    info = "RS=1;FREQ=GnomAD:0.9,0.1|ESP:0.8,0.25|New:0.7,0.3" if freq else "RS=1"
    return ('{"input":"1\\t100\\trs1\\tA\\tG\\t.\\tPASS\\t%s","colocated_variants":[{"id":"rs1","allele_string":"A/G",'
            '"frequencies":{"G":%s}}],%s}' % (info, member_text(n, alternate), CSQ))


def winner_line(n: int, winner: int) -> str:
    """n elements, the one that qualifies at place ``winner`` (the others: COSMIC, or without frequencies)."""
    els = []
    for i in range(n):
        if i == winner:
            els.append('{"id":"rs1","allele_string":"A/G","frequencies":{"G":{"af":0.%d,"gnomade":1e-05}}}' % (i + 1))
        elif i % 2:
            els.append('{"id":"COSV%d","allele_string":"COSMIC_MUTATION","frequencies":{"G":{"af":0.9}}}' % i)
        else:
            els.append('{"id":"rs%d","allele_string":"A/T"}' % (i + 2))
    return ('{"colocated_variants":[%s],"input":"1\\t100\\trs1\\tA\\tG\\t.\\tPASS\\tRS=1",%s}' % (",".join(els), CSQ))


def nested_line(depth: int) -> str:
    """A member of an element nested so that the line is ``depth`` levels deep."""
    value = "1"
    for i in range(depth - 3):
        value = ("[%s]" if i % 2 else '{"k":%s}') % value
    return ('{"input":"1\\t100\\trs1\\tA\\tG\\t.\\tPASS\\tRS=1","colocated_variants":[{"id":"rs1","deep":%s,'
            '"allele_string":"A/G","frequencies":{"G":{"af":0.5}}}],%s}' % (value, CSQ))


def empty_lines():
    """Rows whose text is ``{}``: no colocated_variants, no frequencies, another allele, an empty object, FREQ of
    zeros only; and two ALTs of which one has frequencies."""
    inp = '"input":"1\\t100\\trs1\\tA\\t%s\\t.\\tPASS\\t%s"'
    el = '"colocated_variants":[{"id":"rs1","allele_string":"A/G"%s}]'
    return ['{%s,%s}' % (inp % ("G", "RS=1"), CSQ),
            '{%s,%s,%s}' % (inp % ("G", "RS=1"), el % "", CSQ),
            '{%s,%s,%s}' % (inp % ("G", "RS=1"), el % ',"frequencies":{"T":{"af":1}}', CSQ),
            '{%s,%s,%s}' % (inp % ("G", "RS=1"), el % ',"frequencies":{"G":{}}', CSQ),
            '{%s,%s,%s}' % (inp % ("G", "RS=1;FREQ=GnomAD:1,0|X:.,."), el % ',"frequencies":{}', CSQ),
            '{%s,%s,%s}' % (inp % ("G,T", "RS=1;FREQ=GnomAD:0.9,0,0.1"), el % ',"frequencies":{"T":{"af":1}}', CSQ)]


def small_lines(n: int):
    return ['{"input":"%s\\t%d\\trs%d\\tA\\t%s\\t.\\t.\\tRS=%d;FREQ=GnomAD:0.9,0.%d","id":"v%d","colocated_variants":[{"id":"rs%d",'
            '"allele_string":"A/C","frequencies":{"%s":{"af":0.%d,"gnomade":%de-06,"ea":1}}}],"intergenic_consequences":'
            '[{"variant_allele":"%s","consequence_terms":["intergenic_variant"]}]}'
            % (1 + i % 22, 100 + i, i, "CGT"[i % 3], i, 1 + i % 9, i, i, "CGT"[i % 3], 1 + i % 9, 1 + i % 9, "CGT"[i % 3])
            for i in range(n)]


def edge_lines():
    return ([padded_line(w, k) for w in ("cv", "fr", "key") for k in (63, 64, 65)] +
            [padded_line("key", k, "RS=1") for k in (127, 128, 129)] +
            [cosmic_split_line(k) for k in range(108, 131)] +
            [members_line(n, alt, fq) for n in (1, 63, 64) for alt in (False, True) for fq in (False, True)] +
            [winner_line(n, w) for n in (1, 2, 3) for w in range(n)] + [nested_line(V_MAX_DEPTH)] + empty_lines())


V_MAX_DEPTH = O.V_MAX_DEPTH


def random_device_lines(rows, seed: int, n: int):
    gen = FreqLineGenerator(V.combos_of(rows), seed)
    return [gen.line() for _ in range(n)]


def boundary_join_cases(ranking, alg_id: int, adsp: bool, vep_output: bool):
    """Table lines and their export records: for the head, the frequency text, the body, the cleaned text (with
    ``vep_output``) and the tail of an update row in turn, a row in which that part ends 63, 64 and 65 bytes past
    a 64-byte boundary of the row (the primary key is padded: every later part moves with it).
    Returns ``(lines, export, [(part, bytes past the boundary)])``."""
    from annotatedvdb_amd.vep_rows import allele_frequencies_line, vep_output_line, vep_rows_line
    lines, recs, want = [], [], []
    for part in range(5 if vep_output else 4):
        for past in (63, 64, 65):
            pos = 1000 + len(lines)
            line = ('{"input":"1\\t%d\\trs1\\tA\\tG\\t.\\tPASS\\tRS=1;FREQ=New:0.5,0.25","id":"rs1","pad":"%s","colocated_variants":'
                    '[{"id":"rs1","allele_string":"A/G","frequencies":{"G":%s}}],"transcript_consequences":'
                    '[{"variant_allele":"G","consequence_terms":["intron_variant"],"pad":"%s"}]}'
                    % (pos, "c" * 70, member_text(9, True), "b" * 40))
            key = "1:%d:A:G" % pos
            (_, ms, ranked), = vep_rows_line(line, ranking)
            (_, freq), = allele_frequencies_line(line, adsp, False)
            ends = [len(key) + 1 + len("\tchr1\t")]
            ends.append(ends[-1] + len(freq) + 1)
            ends.append(ends[-1] + len(ms) + 1 + len(ranked))
            if vep_output:
                ends.append(ends[-1] + 1 + len(vep_output_line(line, adsp)))
            ends.append(ends[-1] + 1 + len(str(alg_id)) + (5 if adsp else 0) + 1)
            pk = key + ":" + "p" * ((past - ends[part]) % 64)
            assert (ends[part] + len(pk) - len(key) - 1) % 64 == past % 64
            lines.append(line)
            recs.append(pk + "\t" + key + "\t\\N\n")
            want.append((part, past))
    return lines, "".join(recs).encode("ascii"), want


def join_text(table, export: bytes, alg_id: int, adsp: bool, update_existing: bool, vep_output: bool) -> str:
    """``table``: metaseq id -> (allele_frequencies, most severe, ranked, cleaned), the last line of an id answering."""
    out = []
    for rec in export.decode("utf-8").split("\n")[:-1]:
        f = rec.split("\t")
        if len(f) < 2 or f[0] == "record_primary_key" or f[1] not in table:
            continue
        if not update_existing and len(f) > 2 and f[2] not in ("", "\\N"):
            continue
        freq, ms, ranked, cleaned = table[f[1]]
        t = [f[0], "chr" + f[1].split(":")[0], freq, ms, ranked] + ([cleaned] if vep_output else []) + [str(alg_id)] + \
            (["true"] if adsp else [])
        out.append("\t".join(t) + "\n")
    return "".join(out)


def expected_update_text(lines, export: bytes, ranking, alg_id: int, adsp: bool, update_existing: bool,
                         identity_only: bool, match_refsnp: bool, vep_output: bool) -> str:
    """The update rows of the export against the lines, from the three per-line functions."""
    from annotatedvdb_amd.vep_consequences import UnrankedCombination
    from annotatedvdb_amd.vep_rows import allele_frequencies_line, vep_output_line, vep_rows_line
    table = {}
    for line in lines:
        try:
            rows = vep_rows_line(line, ranking)
        except UnrankedCombination:
            continue
        cleaned = vep_output_line(line, identity_only)
        freqs = allele_frequencies_line(line, identity_only, match_refsnp)
        for (key, ms, ranked), (_, freq) in zip(rows, freqs):
            table[key] = (freq, ms, ranked, cleaned)
    return join_text(table, export, alg_id, adsp, update_existing, vep_output)

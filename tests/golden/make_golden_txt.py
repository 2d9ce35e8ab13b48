#!/usr/bin/env python3
"""Generate the K19 golden fixture by running the REFERENCE's own code of the generic annotation
update over generated text: ``TextVariantLoader.set_current_variant``, ``__get_current_variant_id``,
``__buffer_update_values`` and the update branch of ``parse_variant``
(Util/lib/python/loaders/txt_variant_loader.py), fed through ``csv.DictReader(fh, delimiter='\\t')``
from a text-mode file with ``updateFields.remove('variant')``, as ``update_annotation``
(Load/bin/update_variant_annotation.py:80-90) feeds them.

Runs where the reference checkout is (never on the GPU machine); the tests read only the file it
writes:

  text_update.tsv.gz  per id type ``F<TAB>idtype<TAB>nbytes`` then the file's text and a newline;
                      ``X<TAB>nbytes`` then the export text and a newline;
                      ``H<TAB>idtype<TAB>host<TAB>data``: the generator's own count of data lines
                      outside the device subset, and of all data lines;
                      per update tuple ``U<TAB>idtype<TAB>datasource<TAB>line<TAB>json list``
                      (line: the 1-based file line the tuple came from; ``None`` and ``True`` as
                      JSON has them), in the order the reference appended them;
                      ``M<TAB>idtype<TAB>id`` per looked-up id without a hit, in file order;
                      per one-line case ``E<TAB>case<TAB>idtype<TAB>exception<TAB>nbytes<TAB>json
                      list`` followed by the header and the line and a newline (exception: the
                      class the reference raised, ``-`` for none);
                      ``Q<TAB>json header<TAB>datasource<TAB>legacy<TAB>sql``: the statement the
                      reference's own ``build_update_sql(useLegacyPk)`` sets for a header's update
                      fields (the three files' headers and one with ``bin_index`` and plain
                      columns), on a fresh loader each, legacy 0 or 1.

What is worked around, the loader being stale: the instance is built past the
broken ``__init__`` (``__new__``, then ``VariantLoader.__init__`` with the arity it has, then the
setters ``initialize_loader`` and ``update_annotation`` call); ``is_duplicate(id, returnPK=True)``,
which the base class does not take, is answered from the generated export, once per primary key of
the id (K16's rule: every primary key of an annotated id updates); an id without a hit is recorded
and not parsed, since the insert branch reads attributes ``set_current_variant`` never sets.  What
is stubbed: make_golden.install_stubs().
"""

from __future__ import annotations

import csv
import gzip
import json
import os
import random
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402,F401
from make_golden import REF, install_stubs  # noqa: E402,F401

LABELS = [str(i) for i in range(1, 23)] + ["X", "Y", "M"]
BASES = "ACGT"
HEADERS = {  # `variant` first, in the middle, last
    "METASEQ": ["variant", "gwas_flags", "is_adsp_variant", "other_annotation", "allele_frequencies"],
    "REFSNP": ["gwas_flags", "ref_snp_id", "variant", "other_annotation"],
    "PRIMARY_KEY": ["gwas_flags", "other_annotation", "is_multi_allelic", "variant"],
}


def flags_json(rng):
    return json.dumps({"NG%05d" % rng.randint(1, 99999): {"p_value": "%.1e" % rng.random(), "is_gws": rng.random() < .5}})


def value(rng, col):
    r = rng.random()
    if r < .08:
        return "NULL"
    if r < .12:
        return rng.choice(["NULLx", "null", "xNULL", "Null"])
    if r < .18:
        return ""
    if col in ("is_adsp_variant", "is_multi_allelic"):
        return rng.choice(["true", "false"])
    if col == "allele_frequencies":
        return json.dumps({"1000Genomes": {"afr": round(rng.random(), 4)}})
    return flags_json(rng)


def file_text(id_type):
    """(text, ids looked up in file order, host lines, data lines)"""
    rng = random.Random({"METASEQ": 11, "REFSNP": 12, "PRIMARY_KEY": 13}[id_type])
    header = HEADERS[id_type]
    lines = ["\t".join(header)]
    ids, host, data = [], 0, 0
    pos = 10000
    for k in range(1500):
        c = LABELS[(k // 60) % 25]
        pos += rng.choice([1, 3, 17, 40])
        metaseq = "%s:%d:%s:%s" % (c, pos, rng.choice(BASES), rng.choice(BASES))
        rs = "rs%d" % (pos * 7)
        if k % 97 == 96 and ids:  # a repeated id
            metaseq, rs = ids[-5][1], ids[-5][2]
        rec = {}
        for col in header:
            rec[col] = value(rng, col)
        if id_type == "METASEQ":
            rec["variant"] = look = metaseq
        elif id_type == "REFSNP":
            rec["variant"] = metaseq if k % 3 else rs  # with and without ':'
            rec["ref_snp_id"] = look = rs
        else:
            rec["variant"] = look = [metaseq + ":" + rs, metaseq, rs, "chr" + metaseq][k % 4 if k % 16 == 2 or k % 4 < 2 else 0]
        if k % 23 == 5:  # the share left to the host: quoting and non-ASCII
            col = [h for h in header if h not in ("variant", "ref_snp_id")][k % 2]
            rec[col] = ['"quoted value"', '"say ""hi"""', "café", '"NULL"', '""'][(k // 23) % 5]
        fields = [rec[h] for h in header]
        if k % 29 == 7:  # a short row (never without its ids)
            keep = max(header.index("variant"), header.index("ref_snp_id") if "ref_snp_id" in header else 0) + 1
            fields = fields[:max(keep, len(fields) - 1 - k % 2)]
        if k % 31 == 9:
            fields += ["beyond", "the header"]
        outside = any(f.startswith('"') or not f.isascii() for f in fields)  # (a short row may have lost the field)
        line = "\t".join(fields) + ("\r" if k % 7 == 3 else "")
        lines.append(line)
        ids.append((look, metaseq, rs))
        data += 1
        host += outside
        if k % 200 == 150:
            lines.append("" if k % 400 == 150 else "\r")  # empty lines: csv skips them
    text = "\n".join(lines) + ("\n" if id_type != "REFSNP" else "")  # one file without its final newline
    assert host * 10 < data, (host, data)
    return text.encode("utf-8"), ids, host, data


def export_text(all_ids):
    rows, seen = ["record_primary_key\tmetaseq_id\tref_snp_id"], set()
    rng = random.Random(20261021)
    for k, (_, metaseq, rs) in enumerate(all_ids):
        if metaseq in seen or k % 9 == 4:  # (left out: not in the database)
            continue
        seen.add(metaseq)
        if k % 5 == 0:  # two primary keys of one variant
            rows += ["%s:%s\t%s\t%s" % (metaseq, rs, metaseq, rs), "%s:%s9\t%s\t%s" % (metaseq, rs, metaseq, rs)]
        elif k % 5 == 1:
            rows.append("%s\t%s%s" % (metaseq, metaseq, ["\t\\N", "\t", ""][k % 3]))  # no refSNP id
        else:
            rows.append("%s:%s\t%s\t%s" % (metaseq, rs, metaseq, rs))
        if k % 3 == 0:
            m = "%s:%d:%s:%s" % (rng.choice(LABELS), rng.randint(1, 10 ** 6), rng.choice(BASES), rng.choice(BASES))
            rows.append("%s\t%s\t\\N" % (m, m))
    return ("\n".join(rows) + "\n").encode()


CASES = [  # (case, id type, header, line)
    ("plain", "METASEQ", "variant\tgwas_flags", "1:100:A:G\t{\"a\": 1}"),
    ("null", "METASEQ", "variant\tgwas_flags\tother_annotation", "1:100:A:G\tNULL\tNULLx"),
    ("lower_null", "METASEQ", "variant\tgwas_flags", "1:100:A:G\tnull"),
    ("empty_field", "METASEQ", "variant\tgwas_flags\tother_annotation", "1:100:A:G\t\tx"),
    ("short_row", "METASEQ", "variant\tgwas_flags\tother_annotation", "1:100:A:G\tx"),
    ("long_row", "METASEQ", "variant\tgwas_flags", "1:100:A:G\tx\ty\tz"),
    ("id_only", "METASEQ", "variant\tgwas_flags", "1:100:A:G"),
    ("variant_last", "METASEQ", "gwas_flags\tvariant", "x\t1:100:A:G"),
    ("variant_missing", "METASEQ", "gwas_flags\tvariant", "x"),
    ("quoted", "METASEQ", "variant\tgwas_flags", "1:100:A:G\t\"a b\""),
    ("quoted_null", "METASEQ", "variant\tgwas_flags", "1:100:A:G\t\"NULL\""),
    ("quote_inside", "METASEQ", "variant\tgwas_flags", "1:100:A:G\ta\"b\"c"),
    ("doubled_quote", "METASEQ", "variant\tgwas_flags", "1:100:A:G\t\"a\"\"b\""),
    ("non_ascii", "METASEQ", "variant\tgwas_flags", "1:100:A:G\tcafé"),
    ("crlf", "METASEQ", "variant\tgwas_flags", "1:100:A:G\tx\r"),
    ("blank_field_line", "METASEQ", "variant\tgwas_flags", " "),
    ("pk_with_colon", "PRIMARY_KEY", "variant\tgwas_flags", "1:100:A:G:rs5\tx"),
    ("pk_without_colon", "PRIMARY_KEY", "variant\tgwas_flags", "rs5\tx"),
    ("pk_chr_prefix", "PRIMARY_KEY", "variant\tgwas_flags", "chr1:100:A:G\tx"),
    ("pk_leading_colon", "PRIMARY_KEY", "variant\tgwas_flags", ":100\tx"),
    ("refsnp_variant_metaseq", "REFSNP", "variant\tref_snp_id\tgwas_flags", "1:100:A:G\trs5\tx"),
    ("refsnp_variant_rs", "REFSNP", "variant\tref_snp_id\tgwas_flags", "rs5\trs5\tx"),
    ("refsnp_no_column", "REFSNP", "variant\tgwas_flags", "rs5\tx"),
]


def main():
    install_stubs()
    from AnnotatedVDB.Util.loaders import TextVariantLoader, VariantLoader

    class Loader(TextVariantLoader):
        answer = None

        def is_duplicate(self, variantId, returnPK=False):  # the database's answer, from the export
            return self.answer

    def new_loader(id_type, datasource):
        loader = Loader.__new__(Loader)
        VariantLoader.__init__(loader, datasource)
        loader.set_update_existing(True)
        loader.set_variant_id_type(id_type)
        if loader._update_buffer is None:
            loader._update_buffer = []
        return loader

    def run(text, id_type, datasource, answers):
        """update_annotation's loop (:80-90) over the text -> (tuples with their lines, ids without a hit)"""
        loader = new_loader(id_type, datasource)
        out, missing = [], []
        with tempfile.NamedTemporaryFile("wb", suffix=".txt", delete=False) as tmp:
            tmp.write(text)
        try:
            with open(tmp.name, "r", encoding="utf-8") as fhandle:
                reader = csv.DictReader(fhandle, delimiter="\t")
                updateFields = list(reader.fieldnames)
                updateFields.remove("variant")
                loader.set_update_fields(updateFields)
                for row in reader:
                    if id_type == "PRIMARY_KEY":
                        pks = [None]  # (never asked)
                    else:
                        look = row["ref_snp_id"] if id_type == "REFSNP" else row["variant"]
                        pks = answers.get(look)
                        if not pks:
                            loader.set_current_variant(row)  # (what the reference does before it asks)
                            missing.append(look)
                            continue
                    for pk in pks:
                        loader.answer = pk
                        before = len(loader.update_buffer())
                        loader.parse_variant(row)
                        out += [(reader.line_num, t) for t in loader.update_buffer()[before:]]
        finally:
            os.unlink(tmp.name)
        assert loader.get_count("update") == len(out)
        return out, missing

    texts = {t: file_text(t) for t in ("METASEQ", "REFSNP", "PRIMARY_KEY")}
    export = export_text(texts["METASEQ"][1] + texts["REFSNP"][1])
    by_metaseq, by_rs = {}, {}
    for row in export.decode().split("\n")[1:-1]:
        f = row.split("\t")
        by_metaseq.setdefault(f[1], []).append(f[0])
        if len(f) > 2 and f[2] not in ("", "\\N"):
            by_rs.setdefault(f[2], []).append(f[0])
    answers = {"METASEQ": by_metaseq, "REFSNP": by_rs, "PRIMARY_KEY": {}}
    blob = [b"X\t%d\n" % len(export) + export + b"\n"]
    for id_type, (text, _, host, data) in texts.items():
        blob.append(b"F\t%s\t%d\n" % (id_type.encode(), len(text)) + text + b"\n")
        blob.append(("H\t%s\t%d\t%d\n" % (id_type, host, data)).encode())
        for datasource in ("dbSNP", "ADSP"):
            tuples, missing = run(text, id_type, datasource, answers[id_type])
            for line, t in tuples:
                blob.append(("U\t%s\t%s\t%d\t%s\n" % (id_type, datasource, line, json.dumps(list(t)))).encode())
            print(id_type, datasource, len(tuples), "tuples,", len(missing), "ids without a hit,", host, "of", data,
                  "lines outside the device subset")
        seen = set()
        for m in missing:
            if m not in seen:
                blob.append(("M\t%s\t%s\n" % (id_type, m)).encode())
            seen.add(m)
    for case, id_type, header, line in CASES:
        raw = (header + "\n" + line + "\n").encode("utf-8")
        raised, tuples = "-", []
        try:
            tuples, _ = run(raw, id_type, "dbSNP", type("Any", (dict,), {"get": lambda self, k: ["PK:" + str(k)]})())
        except Exception as e:  # the class is the record
            raised = type(e).__name__
        blob.append(("E\t%s\t%s\t%s\t%d\t%s\n" % (case, id_type, raised, len(raw),
                                                  json.dumps([list(t) for _, t in tuples]))).encode() + raw + b"\n")
        print("%-26s %-12s %-12s %s" % (case, id_type, raised, [t for _, t in tuples]))
    for header in list(HEADERS.values()) + [["bin_index", "variant", "position", "gwas_flags", "is_multi_allelic"],
                                            ["variant", "vep_output"]]:
        for datasource in ("dbSNP", "ADSP"):
            for legacy in (0, 1):
                loader = new_loader("METASEQ", datasource)  # (ADSP: the call appends to the loader's update fields)
                loader.set_update_fields([h for h in header if h != "variant"])
                loader.build_update_sql(bool(legacy))
                sql = loader._update_sql
                assert "\t" not in sql and "\n" not in sql
                blob.append(("Q\t%s\t%s\t%d\t%s\n" % (json.dumps(header), datasource, legacy, sql)).encode())
    path = os.path.join(HERE, "text_update.tsv.gz")
    with open(path, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(b"".join(blob))
    print("text_update.tsv.gz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 400 * 1024


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate the K16 golden fixture by running the REFERENCE's own code of the SnpEff LOF/NMD pass
over generated text: ``VcfEntryParser`` and ``get_variant``, the line prefilter of
``load_annotation`` as written (Load/bin/load_snpeff_lof.py:251-288), ``generate_update_values``
(:136-173) and a real ``VCFVariantLoader`` set up as ``initialize_loader`` sets it up
(``set_update_fields(['loss_of_function'])``, ``set_update_value_generator``,
``set_update_existing(True)``), driven by ``parse_variant(entry, flags)`` as ``load`` (:34-53)
drives it.  The bulk SQL lookup is answered from the generated export: id -> every row with that
metaseq id (``firstHitOnly=False``).

Runs where the reference checkout is (never on the GPU machine); the tests read only the file it
writes:

  snpeff_lof.tsv.gz   ``V<TAB>nbytes`` then the VCF text and a newline; ``X<TAB>nbytes`` then the
                      export text and a newline; ``H<TAB>n`` the generator's own count of annotated
                      lines outside the device subset; per update tuple of ``update_buffer()``
                      ``U<TAB>mode<TAB>pk<TAB>chrom<TAB>json`` (mode 0: the reference's evident
                      intent without --updateExistingValues, 1: with it); ``M<TAB>id`` per lookup
                      id with values and without a hit; per one-line case
                      ``E<TAB>case<TAB>exception<TAB>nbytes<TAB>ids<TAB>json`` followed by the
                      line's bytes and a newline (exception: the class the reference raised, ``-``
                      for none; ids: the lookup ids joined by ``,``; json: the update value of a hit)

The script is loaded by path (its ``__main__`` block raises NotImplementedError and is not run)
and its module global ``args`` set.  ``args.udpateExisting`` (sic) is the attribute the script
reads at :153; argparse would only ever set ``updateExistingValues``, so the script as shipped
raises AttributeError for every variant that has a value.  The attribute is set here so that the
branch's evident intent is what the fixture records.  What is stubbed: make_golden.install_stubs()
and ``niagads.utils.dict`` / ``sys`` / ``list`` (names the script imports and the functions run
never call).  The reference appends one tuple per ALT allele of the line for every hit
(``__parse_alt_alleles`` loops over the alts inside ``parse_variant``); the tuples are recorded as
they come, repeats included.
"""

from __future__ import annotations

import gzip
import importlib.util
import json
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from make_golden import REF, install_stubs  # noqa: E402

HEADER = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO"]
LABELS = [str(i) for i in range(1, 23)] + ["X", "Y", "M"]
BASES = "ACGT"
GENES = ["SFI1", "PRAME", "TTN", "BRCA2", "A1BG-AS1", "C1orf112", "HLA-DRB1", "MT-ND1"]


def group(rng, frac=None, count=None, extra=False):
    g = rng.choice(GENES)
    count = str(rng.randint(1, 40)) if count is None else count
    frac = rng.choice(["0.17", "0.57", "1.00", "0.50", "0.05", "0.333", "1", "0.0001", "0.00001"]) if frac is None else frac
    return "(%s|ENSG%011d|%s|%s%s)" % (g, rng.randint(1, 300000), count, frac, "|more|parts" if extra else "")


def value(rng, **kw):
    return ",".join(group(rng, **kw) for _ in range(rng.choice([1, 1, 1, 2, 3])))


def vcf_text():
    """(text, number of annotated lines, number of them outside the device subset, the ids)."""
    rng = random.Random(20261020)
    lines = ["##fileformat=VCFv4.2", "##SnpEffVersion=\"5.1\"", "\t".join(HEADER)]
    annotated = host = 0
    ids = []
    pos = 10000
    for k in range(1600):
        c = LABELS[(k // 70) % 25]
        pos += rng.choice([1, 3, 17, 40])
        ref = rng.choice(BASES) if k % 5 else "".join(rng.choice(BASES) for _ in range(rng.randint(2, 6)))
        alts = [a for a in BASES if a != ref[0]]
        rng.shuffle(alts)
        alts = alts[:1] if k % 4 else alts[:rng.randint(2, 3)]
        chrom = c
        if k % 13 == 0:
            chrom = "chr" + c
        elif c == "M" and k % 2:
            chrom = "MT"
        vid = "%s:%d:%s:%s" % (c, pos, ref, alts[0]) if k % 3 else ("rs%d" % (pos * 3) if k % 2 else ".")
        info = ["ANN=%s|missense_variant|MODERATE|%s" % (alts[0], rng.choice(GENES)), "AC=%d" % rng.randint(1, 9)]
        outside = False
        kind = k % 5 if k % 4 == 1 or k % 7 == 0 else -1  # about a third of the lines annotated
        if kind in (0, 3):
            info.append("LOF=" + value(rng))
        if kind in (1, 3):
            info.append("NMD=" + value(rng))
        if kind == 2:
            info += ["LOF=" + value(rng), "NMD=" + value(rng), "LOF=" + value(rng)]  # a repeated key: the last wins
        if kind == 4:
            info.append("LOF=" + value(rng, extra=True))  # parts beyond the fourth
        if kind >= 0 and k % 35 == 0:  # the share left to the host: at most one annotated line in ten
            odd = (k // 35) % 6
            tail = [value(rng, frac=".5"), value(rng, frac="1e-5"), value(rng, count=" 3 "), value(rng, count="+7"),
                    value(rng).replace("|ENSG", "\\x59B|ENSG", 1), value(rng).replace("|ENSG", "#2|ENSG", 1)][odd]
            info.append("NMD=" + tail)
            outside = True
        if kind >= 0 and k % 35 == 7:
            info[-1] = info[-1].replace("(", "((", 1).replace("|ENSG", ")|ENSG", 1)  # stray parentheses (device)
        if kind >= 0 and k % 35 == 14:
            info[-1] = "LOF=" + group(rng, count="014")  # a count with a leading zero (device)
        fields = [chrom, str(pos), vid, ref, ",".join(alts), ".", ".", ";".join(info)]
        if k % 11 == 0:
            fields += ["GT", "0/1"]
        line = "\t".join(fields) + ["", "", "\r", " ", "\t"][k % 5]
        if ";LOF=" in line or ";NMD=" in line:
            annotated += 1
            host += outside
            ids += ["%s:%d:%s:%s" % (c, pos, ref, a) for a in alts]
        lines.append(line)
        if k % 300 == 299:
            lines.append("# a comment in the middle")
    # the same id annotated twice: the last record answers
    lines.append("7\t5000\t.\tA\tG\t.\t.\tAC=1;LOF=(FIRST|ENSG1|1|0.25)")
    lines.append("7\t5000\t.\tA\tG\t.\t.\tAC=1;LOF=(LAST|ENSG2|2|0.75)")
    ids += ["7:5000:A:G"]
    annotated += 2
    # an INFO that begins with LOF=, let through by ;NMD=
    lines.append("8\t6000\t.\tC\tT\t.\t.\tLOF=(HEAD|ENSG3|3|0.5);AC=2;NMD=(TAIL|ENSG4|4|0.25)")
    ids += ["8:6000:C:T"]
    annotated += 1
    # ;LOF= only in a sample column: parsed, no values
    lines.append("8\t6001\t.\tC\tT\t.\t.\tAC=2\tGT;LOF=x\t0/1")
    # an INFO that begins with LOF= and nothing else lets through: not looked at
    lines.append("8\t6002\t.\tC\tT\t.\t.\tLOF=(ONLY|ENSG5|5|0.5)")
    assert host * 10 <= annotated, (host, annotated)
    return ("\n".join(lines) + "\n").encode(), annotated, host, ids


def export_text(ids):
    """An export over some of the annotated ids (two primary keys for some, values already there
    for some) and ids SnpEff did not annotate; some annotated ids are left out."""
    rng = random.Random(20261021)
    rows = ["record_primary_key\tmetaseq_id\tloss_of_function"]
    seen = set()
    for k, i in enumerate(ids):
        if i in seen or k % 9 == 4:  # (left out: not in the database)
            continue
        seen.add(i)
        col = ["\\N", "", None, '{"LOF": []}'][(k // 6) % 4] if k % 6 == 0 else "\\N"
        pks = [i + ":rs%d" % (k + 1), i + ":rs%d" % (k + 100000)] if k % 5 == 0 else [i if k % 2 else i + ":rs%d" % k]
        for pk in pks:
            rows.append("\t".join([pk, i] + ([] if col is None else [col])))
        if k % 3 == 0:
            c = rng.choice(LABELS)
            m = "%s:%d:%s:%s" % (c, rng.randint(1, 10 ** 6), rng.choice(BASES), rng.choice(BASES))
            rows.append("%s\t%s\t\\N" % (m, m))
    return ("\n".join(rows) + "\n").encode()


CASES = [  # (case, line)
    ("plain", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(SFI1|ENSG00000198089|30|0.17)"),
    ("multi_alt", "1\t100\t.\tA\tG,T,AC\t.\t.\tAC=1;NMD=(PRAME|ENSG00000185686|14|0.57)"),
    ("two_annotations", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5),(C|D|2|0.25)"),
    ("both", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5);NMD=(C|D|2|0.25)"),
    ("nmd_before_lof", "1\t100\t.\tA\tG\t.\t.\tAC=1;NMD=(C|D|2|0.25);LOF=(A|B|1|0.5)"),
    ("info_begins_with_lof", "1\t100\t.\tA\tG\t.\t.\tLOF=(A|B|1|0.5);NMD=(C|D|2|0.25)"),
    ("lof_in_sample_column", "1\t100\t.\tA\tG\t.\t.\tAC=1\tGT;LOF=1\t0/1"),
    ("repeated_key", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5);LOF=(C|D|2|0.25)"),
    ("flag_then_value", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF;LOF=(C|D|2|0.25)"),
    ("extra_parts", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5|x|y)"),
    ("stray_parentheses", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=((A)|B(|1|0.5))"),
    ("inner_parenthesis_in_count", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1(4|0.5)"),
    ("chr_prefix", "chr1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("mt", "MT\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("chr_mt", "chrMT\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("chrom_leading_zero", "01\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("scaffold", "NT_187361.1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("pos_leading_zero", "1\t0100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("pos_not_digits", "1\t1e2\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("fraction_1.00", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|1.00)"),
    ("fraction_0.50", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.50)"),
    ("fraction_.5", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|.5)"),
    ("fraction_1e-5", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|1e-5)"),
    ("fraction_0.00001", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.00001)"),
    ("fraction_nan", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|nan)"),
    ("fraction_text", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|half)"),
    ("count_spaces", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B| 3 |0.5)"),
    ("count_plus", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|+7|0.5)"),
    ("count_leading_zero", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|014|0.5)"),
    ("count_float", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1.5|0.5)"),
    ("escaped_comma", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A\\x2cA2|B|1|0.5)"),
    ("escaped_slash", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A\\x59A2|B|1|0.5)"),
    ("hash", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A#1|B|1|0.5)"),
    ("quote", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A\"1|B|1|0.5)"),
    ("non_ascii_gene", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A\u00e9|B|1|0.5)"),
    ("numeric_id", "1\t100\t12345\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("float_id", "1\t100\t1e5\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("pk_id", "1\t100\t1:100:A:G:rs5\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("rs_id", "1\t100\trs5\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("ref_nan", "1\t100\t.\tNAN\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("alt_inf", "1\t100\t.\tA\tInf\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("alt_nan_in_list", "1\t100\t.\tA\tNAN,G\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("alt_star", "1\t100\t.\tA\tG,*\t.\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("lof_number", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=5"),
    ("lof_flag", "1\t100\t.\tA\tG\t.\t.\tAC=1;NMD=(A|B|1|0.5);LOF"),
    ("lof_empty", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF="),
    ("three_parts", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1)"),
    ("trailing_comma", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5),"),
    ("seven_fields", "1\t100\t.\tA\tG\t.\tAC=1;LOF=(A|B|1|0.5)"),
    ("trailing_blanks", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5) \t\r"),
    ("sample_columns", "1\t100\t.\tA\tG\t.\t.\tAC=1;LOF=(A|B|1|0.5)\tGT\t0/1"),
]


def main():
    install_stubs()
    make_golden._mod("niagads.utils.dict", print_dict=lambda d, pretty=False: json.dumps(d, default=str))
    make_golden._mod("niagads.utils.sys", warning=lambda *a, **k: None, print_args=lambda a, pretty=True: str(a),
                     die=make_golden._die, get_opener=None, is_binary_file=None)
    make_golden._mod("niagads.utils.list", chunker=None)
    spec = importlib.util.spec_from_file_location("avdb_ref_load_snpeff_lof",
                                                  os.path.join(REF, "Load/bin/load_snpeff_lof.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)  # __name__ != "__main__": the main block is not run
    from AnnotatedVDB.Util.loaders import VCFVariantLoader
    from AnnotatedVDB.Util.parsers import VcfEntryParser

    def new_loader():
        loader = VCFVariantLoader(None)
        loader.initialize_pk_generator("GRCh38", "/nonexistent")
        loader.initialize_bin_indexer(None)
        loader._alg_invocation_id = "1"
        loader.set_update_fields(["loss_of_function"])
        loader.set_update_value_generator(ref.generate_update_values)
        loader.set_update_existing(True)
        return loader

    def lookups_of(text):
        """load_annotation's loop (:250-288) over the text's lines, --resumeAfter unset."""
        lookups = {}
        for line in text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n"):
            line = line.decode("utf-8")
            line = line.rstrip()
            if line.startswith("#"):
                continue
            if ';LOF=' not in line and ';NMD=' not in line:
                continue
            entry = VcfEntryParser(line, HEADER, debug=True, loader=None)
            currentVariant = entry.get_variant()
            for alt in currentVariant['alt_alleles']:
                id = ':'.join((ref.xstr(currentVariant['chromosome']), ref.xstr(currentVariant['position']),
                               currentVariant['ref_allele'], alt))
                lookups[id] = entry
        return lookups

    def response_of(export):
        """The bulk lookup's answer (firstHitOnly=False): id -> every export row of that metaseq id."""
        out = {}
        for row in export.decode().split("\n")[1:-1]:
            f = row.split("\t")
            lof = None if len(f) < 3 or f[2] in ("", "\\N") else json.loads(f[2])
            out.setdefault(f[1], []).append({"record_primary_key": f[0], "annotation": {"loss_of_function": lof}})
        return out

    def run(lookups, response, update_existing):
        """load (:34-53) without the variants the lookup misses (they raise at :140-141)."""
        ref.args = types.SimpleNamespace(debug=False, verbose=False, udpateExisting=update_existing, commitAfter=10 ** 9)
        loader = new_loader()
        missing = []
        for variant in lookups:
            if response.get(variant) is None:
                entry = lookups[variant]  # (a line with neither value has nothing to update: not recorded)
                if entry.get_info('LOF') is not None or entry.get_info('NMD') is not None:
                    missing.append(variant)
                continue
            for hit in response[variant]:
                loader.parse_variant(lookups[variant], {'record_primary_key': hit['record_primary_key'],
                                                        'loss_of_function': hit['annotation']['loss_of_function']})
        return loader.update_buffer(), missing, loader.get_count('update'), loader.get_count('skipped')

    vcf, annotated, host, ids = vcf_text()
    export = export_text(ids)
    lookups, response = lookups_of(vcf), response_of(export)
    blob = [b"V\t%d\n" % len(vcf) + vcf + b"\n", b"X\t%d\n" % len(export) + export + b"\n", b"H\t%d\n" % host]
    for mode in (0, 1):
        tuples, missing, n_upd, n_skip = run(lookups, response, bool(mode))
        for t in tuples:
            assert len(t) == 3 and all("\t" not in x and "\n" not in x for x in t), t
            blob.append(("U\t%d\t%s\n" % (mode, "\t".join(t))).encode())
        print("mode", mode, len(tuples), "tuples,", n_upd, "updated,", n_skip, "skipped,", len(missing), "missing")
    blob += [("M\t%s\n" % m).encode() for m in missing]
    print(annotated, "annotated lines,", host, "outside the device subset,", len(lookups), "ids")
    for case, line in CASES:
        raw = (line + "\n").encode("utf-8")
        ids_, js, raised = "", "", "-"
        try:
            lk = lookups_of(raw)
            ids_ = ",".join(lk)
            ref.args = types.SimpleNamespace(debug=False, verbose=False, udpateExisting=True)
            loader = new_loader()
            for variant in lk:
                loader.parse_variant(lk[variant], {'record_primary_key': variant, 'loss_of_function': None})
                break
            buf = loader.update_buffer()
            js = buf[0][2] if buf else ""
        except Exception as e:  # the class is the record
            raised = type(e).__name__
        blob.append(("E\t%s\t%s\t%d\t%s\t%s\n" % (case, raised, len(raw), ids_, js)).encode() + raw + b"\n")
        print("%-28s %-16s %s %s" % (case, raised, ids_, js[:60]))
    path = os.path.join(HERE, "snpeff_lof.tsv.gz")
    with open(path, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(b"".join(blob))
    print("snpeff_lof.tsv.gz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "split_vcf.tsv.gz"))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate the K17 golden fixture by running the REFERENCE's own code of the ADSP QC pVCF pass
over generated text: ``VcfEntryParser`` and ``get_variant``, the loop of ``load_annotation`` as
written (Load/bin/update_from_qc_pvcf_file.py:226-258), ``generate_update_values`` (:117-149) and a
real ``VCFVariantLoader`` set up as ``initialize_loader`` (:178-188) sets it up
(``set_update_fields(['is_adsp_variant', 'adsp_qc'])``, ``set_update_value_generator``,
``set_update_existing(True)``), driven by ``parse_variant(entry, flags)`` as ``load`` (:34-58)
drives it.  The bulk SQL lookup is answered from the generated export: id -> every row with that
metaseq id (``firstHitOnly=False``), its ``adsp_qc`` the export's third column read as ``COPY``
wrote it.

Runs where the reference checkout is (never on the GPU machine); the tests read only the file it
writes:

  adsp_qc.tsv.gz   ``V<TAB>nbytes`` then the VCF text and a newline; ``X<TAB>nbytes`` then the
                   export text and a newline; ``R<TAB>version``; ``H<TAB>n<TAB>lines`` the
                   generator's own count of data lines outside the device subset and of data lines;
                   per update tuple of ``update_buffer()``
                   ``U<TAB>mode<TAB>pk<TAB>chrom<TAB>true|\\N<TAB>json`` (mode 0: without
                   --updateExistingValues, 1: with it); ``S<TAB>mode<TAB>n`` the loader's skipped
                   counter; ``M<TAB>id`` per lookup id without a hit; per one-line case
                   ``E<TAB>case<TAB>exception<TAB>nbytes<TAB>ids<TAB>true|\\N<TAB>json`` followed by
                   the line's bytes and a newline (exception: the class the reference raised, ``-``
                   for none)

The script is loaded by path (its ``__main__`` block is not run) and its module global ``args``
set.  As shipped it cannot run: it builds ``VCFVariantLoader(..., logFileName=...)`` and calls
``loader.log``, neither of which exists, and an id without a hit reaches
``generate_update_values`` with flags that lack ``record_primary_key`` (KeyError at :127).  Its
functions are intact and are what runs here; ids without a hit are recorded, not parsed, and the
loader is given a ``log`` that does nothing, so that the Infinity branch (:142-145) ends in the
``ValueError`` it is written to raise and not in the ``AttributeError`` of the missing method.  The
reference appends one tuple per ALT allele of the hit's line (``__parse_alt_alleles`` loops over
the alts inside ``parse_variant``); the tuples are recorded as they come, repeats included.
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

VERSION = "17K"
HEADER = ["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"]
LABELS = [str(i) for i in range(1, 23)] + ["X", "Y", "M"]
BASES = "ACGT"
FILTERS = ["PASS", "PASS", ".", "VQSRTrancheSNP99.80to100.00"]
# INFO items outside the device subset (the host's), one line in sixteen takes one
HOST_ITEMS = ["AF=1e-5", "AC=+5", "AF=0.1234567890123456", "MQ=nan", "DP=12;DP=14", "culprit=MQ\\x2cFS",
              "GENE=A\\x59B", "BIG=12345678901234567890.5", "X= 5", "N=1_000", "VQSLOD=-", "EMPTY="]
# ... and inside it
DEVICE_ITEMS = ["BaseQRankSum=-1.234", "Z=-0", "Z=-0.0", "Z=0.00", "Z=-00", "F=0.123456789012345", "F=123456789012.345",
                "SMALL=0.00001", "SMALL=-0.000012", "N30=123456789012345678901234567890", "N30=-00123456789012345678901234567890",
                "LIST=1,2,3", "LIST=0.5,0.25", "GENE=APOE#1", "HUGE=100000000000000000.0", "HALF=.5", "FIVE=5.",
                "ID=007", "DOT=.", "TEXT=a b", "K#1=2"]


def vcf_text():
    """(text, data lines, the ones outside the device subset, the ids in file order)."""
    rng = random.Random(20261022)
    lines = ["##fileformat=VCFv4.2", "##source=ADSP QC", "\t".join(HEADER) + "\tS1\tS2"]
    data = host = 0
    ids = []
    pos = 20000
    for k in range(1500):
        c = LABELS[(k // 60) % 25]
        pos += rng.choice([1, 2, 9, 31])
        ref = rng.choice(BASES) if k % 5 else "".join(rng.choice(BASES) for _ in range(rng.randint(2, 6)))
        alts = [a for a in BASES if a != ref[0]]
        rng.shuffle(alts)
        alts = alts[:1] if k % 4 else alts[:rng.randint(2, 3)]
        if k % 97 == 0:
            alts.append("*")
        chrom = c
        if k % 13 == 0:
            chrom = "chr" + c
        elif c == "M" and k % 2:
            chrom = "MT"
        vid = "." if k % 3 else "rs%d" % (pos * 3)
        qual = [".", str(rng.randint(30, 9999)), "%d.%02d" % (rng.randint(30, 9999), rng.randint(0, 99))][k % 3]
        filt = FILTERS[k % 4]
        info = ["AC=%d" % rng.randint(1, 99), "AF=%s" % rng.choice(["0.00123", "0.5", "1.00", "0.000", "0.00004"]),
                "AN=%d" % rng.randint(100, 35000), "DP=%d" % rng.randint(1000, 999999),
                "ExcessHet=%d.%04d" % (rng.randint(0, 9), rng.randint(0, 9999)), "FS=%d.%03d" % (rng.randint(0, 60), rng.randint(0, 999)),
                "MQ=60.00", "QD=%d.%02d" % (rng.randint(0, 35), rng.randint(0, 99)), "SOR=%d.%03d" % (rng.randint(0, 4), rng.randint(0, 999)),
                "VQSLOD=%s%d.%02d" % (rng.choice(["", "-"]), rng.randint(0, 20), rng.randint(0, 99)),
                "culprit=%s" % rng.choice(["MQ", "FS", "QD", "SOR"])]
        if k % 3 == 0:
            info.append("DB")
        if k % 7 == 0:
            info.insert(3, "POSITIVE_TRAIN_SITE")
        if k % 2 == 0:
            info.insert(rng.randint(0, len(info)), DEVICE_ITEMS[(k // 2) % len(DEVICE_ITEMS)])
        outside = k % 16 == 5
        if outside:
            info.insert(rng.randint(0, len(info)), HOST_ITEMS[(k // 16) % len(HOST_ITEMS)])
        text = ";".join(info)
        if k % 29 == 0:
            text += ";"  # an empty item from a trailing ';'
        if k % 211 == 0:
            text, outside = "DB", False  # one flag only
        fields = [chrom, str(pos), vid, ref, ",".join(alts), qual, filt, text, "GT:AD:DP" if k % 3 else "GT"]
        if k % 3 == 0:
            fields += ["0/1:12,9:21", "./.:0,0:0"]
        lines.append("\t".join(fields) + ["", "", "\r", " ", "\t"][k % 5])
        data += 1
        host += outside
        ids += ["%s:%d:%s:%s" % (c, pos, ref, a) for a in alts]
        if k % 300 == 299:
            lines.append("# a comment in the middle")
    # the same id twice: the last record answers
    lines.append("7\t5000\t.\tA\tG\t50\tLowQual\tAC=1;AF=0.1\tGT")
    lines.append("7\t5000\t.\tA\tG\t60\tPASS\tAC=2;AF=0.2\tGT")
    ids += ["7:5000:A:G"]
    data += 2
    assert host * 10 <= data, (host, data)
    return ("\n".join(lines) + "\n").encode(), data, host, ids


def copy_escape(s: str) -> str:
    return s.replace("\\", "\\\\").replace("\t", "\\t").replace("\n", "\\n")


def copy_unescape(s: str) -> str:
    out, i = [], 0
    while i < len(s):
        if s[i] == "\\" and i + 1 < len(s):
            i += 1
            out.append({"t": "\t", "n": "\n", "r": "\r", "b": "\b", "f": "\f", "v": "\v"}.get(s[i], s[i]))
        else:
            out.append(s[i])
        i += 1
    return "".join(out)


def export_text(ids):
    """An export over most of the ids (two primary keys for some; QC of this release, of another
    release only, and with an escaped string in the column for some) and ids the QC file does not
    hold; some ids are left out."""
    rng = random.Random(20261023)
    release = VERSION.lower()
    this = json.dumps({release: {"info": {"AC": 1}, "filter": "PASS", "qual": None, "format": "GT"}})
    both = json.dumps({"r3": {"info": {"AC": 2}, "filter": ".", "qual": 5, "format": None}, release: {"info": {}}})
    other = json.dumps({"r3": {"info": {release: 1, "note": release}, "filter": release, "qual": 5, "format": None},
                        "label": release})
    longer = json.dumps({release + "_r2": {"info": {}}, "x": [release, {release: 1}]})
    escaped = json.dumps({"r3": {"info": {"note": 'a "quoted" ' + release + ' \\ text'}}})
    escaped_this = json.dumps({release: {"info": {"note": 'tab\there "q"'}}})
    cols = ["\\N", "", None, this, other, both, longer, copy_escape(escaped), copy_escape(escaped_this), "null"]
    rows = ["record_primary_key\tmetaseq_id\tadsp_qc"]
    seen = set()
    for k, i in enumerate(ids):
        if i in seen or k % 9 == 4:  # (left out: not in the database)
            continue
        seen.add(i)
        col = cols[(k // 4) % len(cols)] if k % 4 == 0 else "\\N"
        pks = [i + ":rs%d" % (k + 1), i + ":rs%d" % (k + 100000)] if k % 5 == 0 else [i if k % 2 else i + ":rs%d" % k]
        for pk in pks:
            rows.append("\t".join([pk, i] + ([] if col is None else [col])))
        if k % 3 == 0:
            c = rng.choice(LABELS)
            m = "%s:%d:%s:%s" % (c, rng.randint(1, 10 ** 6), rng.choice(BASES), rng.choice(BASES))
            rows.append("%s\t%s\t\\N" % (m, m))
    return ("\n".join(rows) + "\n").encode()


BASE = "1\t100\t.\tA\tG\t50\tPASS\t%s\tGT:DP"
VALUES = ["5", "-5", "007", "-007", "0", "-0", "-00", "0.0", "-0.0", "0.00", "-.0", ".5", "5.", "-5.", ".", "-", "",
          "+5", "1e5", "1E-5", "-1e5", "1_000", " 5", "5 ", "inf", "-inf", "Infinity", "nan", "NaN", "-nan", "iNf",
          "0.00001", "0.0001", "-0.00001", "0.000012345", "123456789012345", "1234567890123456", "0.123456789012345",
          "0.1234567890123456", "123456789012345.0", "1234567890123456.0", "12345678901234567890.0",
          "1000000000000000.0", "10000000000000000.0", "100000000000000000000.0", "0.000000000000000000001",
          "123456789012345678901234567890", "-123456789012345678901234567890", "00000000000000000001.5",
          "1.50000000000000000000", "PASS", "a", "e", "1,2", "0x1F", "--5", "5-", "1.2.3", "tiny", "fin", "A#B"]
CASES = [  # (case, line)
    ("plain", BASE % "AC=1;AF=0.5;DB"),
    ("multi_alt", "1\t100\t.\tA\tG,T,AC\t.\t.\tAC=1,2,3\tGT"),
    ("sample_columns", BASE % "AC=1" + "\t0/1:3\t1/1:4"),
    ("nine_fields_exactly", "1\t100\t.\tA\tG\t.\t.\tAC=1\t."),
    ("chr_prefix", "chr1\t100\t.\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("mt", "MT\t100\t.\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("chr_mt", "chrMT\t100\t.\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("scaffold", "NT_187361.1\t100\t.\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("pos_leading_zero", "1\t0100\t.\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("pos_not_digits", "1\t1e2\t.\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("rs_id", "1\t100\trs5\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("numeric_id", "1\t100\t12345\tA\tG\t.\tPASS\tAC=1\tGT"),
    ("ref_nan", "1\t100\t.\tNAN\tG\t.\tPASS\tAC=1\tGT"),
    ("alt_inf", "1\t100\t.\tA\tInf\t.\tPASS\tAC=1\tGT"),
    ("alt_star", "1\t100\t.\tA\tG,*\t.\tPASS\tAC=1\tGT"),
    ("eight_fields", "1\t100\t.\tA\tG\t.\tPASS\tAC=1"),
    ("empty_line", ""),
    ("info_number", "1\t100\t.\tA\tG\t.\tPASS\t5\tGT"),
    ("info_float_word", "1\t100\t.\tA\tG\t.\tPASS\tnan\tGT"),
    ("info_dot", "1\t100\t.\tA\tG\t.\tPASS\t.\tGT"),
    ("info_empty", "1\t100\t.\tA\tG\t.\tPASS\t\tGT"),
    ("info_infinity", BASE % "AF=inf"),
    ("info_infinity_text", BASE % "NOTE=Infinity_and_beyond"),
    ("filter_infinity", "1\t100\t.\tA\tG\t.\tinf\tAC=1\tGT"),
    ("filter_lower_pass", "1\t100\t.\tA\tG\t.\tpass\tAC=1\tGT"),
    ("filter_hash", "1\t100\t.\tA\tG\t.\tq#10\tAC=1\tGT#X"),
    ("qual_float", "1\t100\t.\tA\tG\t50.00\tPASS\tAC=1\tGT"),
    ("qual_negative", "1\t100\t.\tA\tG\t-1\tPASS\tAC=1\tGT"),
    ("format_number", "1\t100\t.\tA\tG\t.\tPASS\tAC=1\t12"),
    ("format_empty", "1\t100\t.\tA\tG\t.\tPASS\tAC=1\t\t0/1"),
    ("flag_only", BASE % "DB"),
    ("trailing_semicolon", BASE % "AC=1;"),
    ("double_semicolon", BASE % "AC=1;;DB"),
    ("repeated_key", BASE % "AC=1;DP=2;AC=3"),
    ("repeated_flag", BASE % "DB;AC=1;DB"),
    ("flag_then_value", BASE % "DB;DB=1"),
    ("repeated_after_hash", BASE % "K#1=1;K:1=2"),
    ("equals_in_value", BASE % "EXPR=a=b"),
    ("empty_key", BASE % "=5"),
    ("escaped_comma", BASE % "L=1\\x2c2"),
    ("escaped_slash", BASE % "G=A\\x59B"),
    ("hash", BASE % "G=A#1;K#2=x"),
    ("quote", BASE % "G=\"q\""),
    ("backslash", BASE % "G=a\\b"),
    ("non_ascii", BASE % "G=caf\u00e9"),
    ("control_byte", BASE % "G=a\x01b"),
    ("del_byte", BASE % "G=a\x7fb"),
    ("trailing_blanks", BASE % "AC=1" + " \t\r"),
] + [("value_%02d" % i, BASE % ("V=" + v)) for i, v in enumerate(VALUES)] \
  + [("qual_value_%02d" % i, "1\t100\t.\tA\tG\t%s\t.\tAC=1\tGT" % v) for i, v in enumerate(VALUES) if "\t" not in v and v.strip() == v and v]


def main():
    install_stubs()
    make_golden._mod("niagads.utils.dict", print_dict=lambda d, pretty=False: json.dumps(d, default=str))
    make_golden._mod("niagads.utils.sys", warning=lambda *a, **k: None, print_args=lambda a, pretty=True: str(a),
                     die=make_golden._die, get_opener=None, is_binary_file=None)
    make_golden._mod("niagads.utils.list", chunker=None)
    spec = importlib.util.spec_from_file_location("avdb_ref_update_from_qc_pvcf_file",
                                                  os.path.join(REF, "Load/bin/update_from_qc_pvcf_file.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)  # __name__ != "__main__": the main block is not run
    from AnnotatedVDB.Util.loaders import VCFVariantLoader
    from AnnotatedVDB.Util.parsers import VcfEntryParser

    def new_loader():
        loader = VCFVariantLoader(VERSION)
        loader.initialize_pk_generator("GRCh38", "/nonexistent")
        loader.initialize_bin_indexer(None)
        loader._alg_invocation_id = "1"
        loader.log = lambda *a, **k: None  # (the method the script expects and the class lacks)
        loader.set_update_fields(["is_adsp_variant", "adsp_qc"])
        loader.set_update_value_generator(ref.generate_update_values)
        loader.set_update_existing(True)
        return loader

    def lookups_of(text):
        """load_annotation's loop (:226-258) over the text's lines, --resumeAfter unset."""
        lookups = {}
        for line in text.split(b"\n")[:-1] if text.endswith(b"\n") else text.split(b"\n"):
            line = line.decode("utf-8")
            line = line.rstrip()
            if line.startswith("#"):
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
            qc = None if len(f) < 3 or f[2] in ("", "\\N") else json.loads(copy_unescape(f[2]))
            out.setdefault(f[1], []).append({"record_primary_key": f[0], "is_adsp_variant": None,
                                             "annotation": {"adsp_qc": qc}})
        return out

    def run(lookups, response, update_existing):
        """load (:34-58) without the variants the lookup misses (they raise KeyError at :127)."""
        ref.args = types.SimpleNamespace(debug=False, verbose=False, updateExistingValues=update_existing,
                                         version=VERSION, commitAfter=10 ** 9)
        args = ref.args
        loader = new_loader()
        missing = []
        for variant in lookups:
            if response.get(variant) is None:
                missing.append(variant)
                continue
            for hit in response[variant]:
                updateFlags = {'record_primary_key': hit['record_primary_key'],
                               'is_adsp_variant': hit['is_adsp_variant'],
                               'adsp_qc': hit['annotation']['adsp_qc'] is not None and args.version.lower() in hit['annotation']['adsp_qc']}
                loader.parse_variant(lookups[variant], updateFlags)
        return loader.update_buffer(), missing, loader.get_count('update'), loader.get_count('skipped')

    def flag_text(v):
        assert v is True or v is None, v
        return "true" if v else "\\N"

    vcf, data, host, ids = vcf_text()
    export = export_text(ids)
    lookups, response = lookups_of(vcf), response_of(export)
    blob = [b"V\t%d\n" % len(vcf) + vcf + b"\n", b"X\t%d\n" % len(export) + export + b"\n",
            b"R\t%s\n" % VERSION.encode(), b"H\t%d\t%d\n" % (host, data)]
    for mode in (0, 1):
        tuples, missing, n_upd, n_skip = run(lookups, response, bool(mode))
        for t in tuples:
            assert len(t) == 4 and all("\t" not in x and "\n" not in x for x in (t[0], t[1], t[3])), t
            blob.append(("U\t%d\t%s\t%s\t%s\t%s\n" % (mode, t[0], t[1], flag_text(t[2]), t[3])).encode())
        blob.append(b"S\t%d\t%d\n" % (mode, n_skip))
        print("mode", mode, len(tuples), "tuples,", n_upd, "updated,", n_skip, "skipped,", len(missing), "missing")
    blob += [("M\t%s\n" % m).encode() for m in missing]
    print(data, "data lines,", host, "outside the device subset,", len(lookups), "ids")
    for case, line in CASES:
        raw = (line + "\n").encode("utf-8")
        ids_, js, flag, raised = "", "", "", "-"
        try:
            lk = lookups_of(raw)
            ids_ = ",".join(lk)
            ref.args = types.SimpleNamespace(debug=False, verbose=False, updateExistingValues=True, version=VERSION)
            loader = new_loader()
            for variant in lk:
                loader.parse_variant(lk[variant], {'record_primary_key': variant, 'is_adsp_variant': None,
                                                   'adsp_qc': False})
                break
            buf = loader.update_buffer()
            flag, js = flag_text(buf[0][2]), buf[0][3]
        except Exception as e:  # the class is the record
            raised = type(e).__name__
        assert "\t" not in js and "\n" not in js, js
        blob.append(("E\t%s\t%s\t%d\t%s\t%s\t%s\n" % (case, raised, len(raw), ids_, flag, js)).encode() + raw + b"\n")
        print("%-28s %-16s %s %s %s" % (case, raised, ids_, flag, js[:70]))
    path = os.path.join(HERE, "adsp_qc.tsv.gz")
    with open(path, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(b"".join(blob))
    print("adsp_qc.tsv.gz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main()

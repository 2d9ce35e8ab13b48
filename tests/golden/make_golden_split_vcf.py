#!/usr/bin/env python3
"""Generate the K15 golden fixture by running the REFERENCE's own ``create_fh_dict()``,
``run()`` and ``close_fh_dict()`` (Util/bin/split_vcf_by_chr.py:14-52) over generated
whole-genome VCF text, each run from a gzip file into a temporary directory.

Runs where the reference checkout is (never on the GPU machine); the tests read only the
file it writes:

  split_vcf.tsv.gz   per run ``I<TAB>run<TAB>map<TAB>nbytes`` (map: 1 when the run used
                     chrmap_grch38.tsv) followed by the input text's nbytes bytes and a
                     newline, then for every file the run produced
                     ``F<TAB>run<TAB>name<TAB>nbytes`` followed by the file's bytes and a
                     newline; then per one-line case
                     ``E<TAB>case<TAB>exception<TAB>map<TAB>nbytes`` followed by the
                     line's bytes and a newline (exception: the class the reference
                     raised, ``-`` for none)

The reference script is loaded by path and its module globals ``args``, ``chrmMap`` and
``fhDict`` set, as its main block sets them.  What is stubbed (no GenomicsDBData package
here): ``GenomicsDBData.Util.utils`` (``warning`` prints nothing, ``xstr`` is ``str``
with None as the empty string, ``create_dir`` is ``os.makedirs``; ``print_dict``,
``execute_cmd``, ``die`` and ``get_opener`` are not called by the functions run).
"""

from __future__ import annotations

import gzip
import importlib.util
import os
import random
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, install_stubs  # noqa: E402

LABELS = [str(i) for i in range(1, 23)] + ["X", "Y", "M"]
CHRMAP = os.path.join(HERE, "chrmap_grch38.tsv")
BASES = "ACGT"


def accessions():
    """label -> the source id chrmap_grch38.tsv maps to chr<label> (its first 25 rows)."""
    out = {}
    with open(CHRMAP) as fh:
        next(fh)
        for line in fh:
            sid, chrom = line.split("\t")[:2]
            out.setdefault(chrom.replace("chr", ""), sid)
    return {c: out[c] for c in LABELS}


def data_line(rng, chrom, pos, k):
    """One data line: 8 fields mostly, 9+ now and then; the tails rstrip() removes on some."""
    ref = rng.choice(BASES) if k % 5 else "".join(rng.choice(BASES) for _ in range(rng.randint(2, 9)))
    alt = rng.choice([b for b in BASES if b != ref[0]])
    fields = [chrom, str(pos), "rs%d" % (pos * 7 + k), ref, alt, ".", ".", "VC=SNV" if k % 4 else "VC=DIV;GNO"]
    if k % 11 == 0:
        fields += ["GT", "0/1", "1/1"]
    line = "\t".join(fields)
    line += ["", "", "", "", "\r", " ", "\t", " \t \r", "\t\t"][k % 9]
    return line


def run1_text():
    """Labels as CHROM: all 25 contigs, sorted; comments at the top and in the middle; the
    last line without its newline."""
    rng = random.Random(20261020)
    lines = ["##fileformat=VCFv4.2", "##source=make_golden_split_vcf", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    k = 0
    for c in LABELS:
        n = {"1": 750, "2": 300, "Y": 3, "M": 40}.get(c, 90)
        pos = 10000
        for i in range(n):
            pos += rng.choice([1, 2, 7, 30])
            lines.append(data_line(rng, c, pos, k))
            k += 1
            if k % 400 == 0:
                lines.append("# a comment in the middle \t")
                lines.append("#")
    return ("\n".join(lines)).encode()


def run2_text():
    """RefSeq accessions as CHROM (mapped through chrmap_grch38.tsv), contigs interleaved."""
    rng = random.Random(20261021)
    acc = accessions()
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    pos = {c: 5000 for c in LABELS}
    for k in range(2900):
        c = LABELS[k % 25] if k % 3 else rng.choice(LABELS)  # line by line, with random breaks
        pos[c] += rng.choice([1, 3, 11])
        chrom = "7" if c == "7" and k % 2 else acc[c]  # the map holds the plain key 7 too
        lines.append(data_line(rng, chrom, pos[c], k))
        if k == 1500:
            lines.append("##late header\r")
    return ("\n".join(lines) + "\n").encode()


CASES = [  # (case, line bytes, with the map)
    ("chr_prefix", b"chr1\t100\trs1\tA\tC\t.\t.\t.\n", False),
    ("mt", b"MT\t100\trs1\tA\tC\t.\t.\t.\n", False),
    ("empty_line", b"\n", False),
    ("blank_line", b" \t \r\n", False),
    ("lower_x", b"x\t100\trs1\tA\tC\t.\t.\t.\n", False),
    ("leading_zero", b"01\t100\trs1\tA\tC\t.\t.\t.\n", False),
    ("key_with_blank", b"1 \t100\trs1\tA\tC\t.\t.\t.\n", False),
    ("label_ok", b"X\t\t\t\n", False),
    ("unmapped_accession", b"NW_003315950.2\t100\trs1\tA\tC\t.\t.\t.\n", True),
    ("mapped_to_scaffold", b"NT_187361.1\t100\trs1\tA\tC\t.\t.\t.\n", True),
    ("mapped_to_mt", b"J01415.2\t100\trs1\tA\tC\t.\t.\t.\n", True),
    ("label_under_map", b"1\t100\trs1\tA\tC\t.\t.\t.\n", True),
    ("mapped_ok", b"CM000685.2\t100\trs1\tA\tC\t.\t.\t.\n", True),
    ("lone_ff_at_end", b"1\t100\trs1\tA\tC\t.\t.\tX\xff\n", False),
    ("lone_ff_in_comment", b"#note \xff\n", False),
    ("unit_separator_tail", b"1\t100\trs1\tA\tC\t.\t.\t.\x1f\n", False),
    ("nbsp_tail", b"1\t100\trs1\tA\tC\t.\t.\t.\xc2\xa0\n", False),
    ("nel_tail", b"1\t100\trs1\tA\tC\t.\t.\t.\xc2\x85 \n", False),
]


def main():
    install_stubs()
    utils = sys.modules["GenomicsDBData.Util.utils"]
    utils.warning = lambda *a, **k: None
    utils.create_dir = lambda d: os.makedirs(d, exist_ok=True)
    for name in ("print_dict", "execute_cmd", "die", "get_opener"):
        if not hasattr(utils, name):
            setattr(utils, name, None)
    spec = importlib.util.spec_from_file_location("avdb_ref_split_vcf_by_chr",
                                                  os.path.join(REF, "Util/bin/split_vcf_by_chr.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)  # __name__ != "__main__": the main block is not run

    def reference_run(text, with_map):
        """{name: bytes} of the files the reference wrote, and the exception class it raised (or None)."""
        with tempfile.TemporaryDirectory() as d:
            src = os.path.join(d, "in.vcf.gz")
            with gzip.open(src, "wb") as fh:
                fh.write(text)
            out = os.path.join(d, "out")
            ref.args = types.SimpleNamespace(fileName=src, outputDir=out, chromosomeMap=CHRMAP if with_map else None)
            ref.chrmMap = ref.ChromosomeMap(CHRMAP) if with_map else None
            utils.create_dir(out)
            ref.fhDict = {}
            ref.create_fh_dict()
            raised = None
            try:
                ref.run()
            except Exception as e:  # the class is the record
                raised = type(e).__name__
            ref.close_fh_dict()
            files = {}
            for name in sorted(os.listdir(out)):
                with open(os.path.join(out, name), "rb") as fh:
                    files[name] = fh.read()
            return files, raised

    blob = []
    for run, text, with_map in (("run1", run1_text(), False), ("run2", run2_text(), True)):
        files, raised = reference_run(text, with_map)
        assert raised is None and len(files) == 25, (run, raised)
        blob.append(b"I\t%s\t%d\t%d\n" % (run.encode(), with_map, len(text)) + text + b"\n")
        for name, data in files.items():
            blob.append(b"F\t%s\t%s\t%d\n" % (run.encode(), name.encode(), len(data)) + data + b"\n")
        print(run, text.count(b"\n"), "newlines,", sum(len(v) for v in files.values()), "bytes out")
    for case, line, with_map in CASES:
        _, raised = reference_run(line, with_map)
        blob.append(b"E\t%s\t%s\t%d\t%d\n" % (case.encode(), (raised or "-").encode(), with_map, len(line)) + line + b"\n")
        print("%-22s %s" % (case, raised))
    path = os.path.join(HERE, "split_vcf.tsv.gz")
    with open(path, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(b"".join(blob))
    print("split_vcf.tsv.gz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 110 * 1024


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate the CADD golden fixtures by running the REFERENCE's own
``CADDUpdater.buffer_variant`` (Util/lib/python/loaders/cadd_updater.py:187-221)
over generated variants, the way ``Load/bin/load_cadd_scores.py:109-120`` drives it.

Runs where the reference checkout is (never on the GPU machine); the tests read
only the three files it writes:

  cadd_snv.tsv.gz       the SNV table: 3 alts per position, %.6f / %.3f scores
  cadd_indel.tsv.gz     the indel table: several rows per position, alleles to 60 bp
  cadd_expected.tsv.gz  class, chromosome setting, metaseq_id, record_primary_key,
                        cadd_scores, then the tuple the reference buffered (three
                        empty columns for a skipped record); the last line holds
                        the reference's final counters

What is stubbed (no database, no pysam here): ``pysam.TabixFile`` is an in-memory
table whose ``fetch(chrom, start, end, parser)`` returns, in file order, the rows
with ``start < pos <= end`` and raises ``ValueError`` for a contig the file lacks,
as pysam does; ``is_duplicate`` returns the record's own primary key; the
validator's ``has_attr`` returns ``None``.
"""

from __future__ import annotations

import gzip
import json
import os
import random
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import install_stubs  # noqa: E402

SNV_FILE = "whole_genome_SNVs.tsv.gz"
INDEL_FILE = "gnomad.genomes.r3.0.indel.tsv.gz"
HEADER = "## CADD GRCh38-v1.6 (c) University of Washington, Hudson-Alpha Institute for Biotechnology and Berlin " \
         "Institute of Health 2013-2020. All rights reserved.\n#Chrom\tPos\tRef\tAlt\tRawScore\tPHRED\n"
BASES = "ACGT"
SNV_CONTIGS = ["1", "21", "22", "X", "MT"]   # file order; the table lacks Y
INDEL_CONTIGS = ["1", "21", "22", "X"]       # ... and the indel table lacks MT too
TABLES = {}                                  # file name -> {contig: [row tuples]}


class TabixFile:
    def __init__(self, path):
        self.rows = TABLES[os.path.basename(path)]

    def fetch(self, chrom, start, end, parser=None):
        if chrom not in self.rows:
            raise ValueError("could not create iterator for region '%s:%d-%d'" % (chrom, start + 1, end))
        return [r for r in self.rows[chrom] if start < int(r[1]) <= end]


def score(rng):
    x = rng.choice([rng.uniform(-2.0, 8.0), rng.uniform(-0.001, 0.001), -0.0000001, 0.0, rng.uniform(-0.5, 0.5)])
    return "%.6f" % x, "%.3f" % rng.choice([rng.uniform(0.0, 40.0), rng.uniform(0.0, 1.0), 0.0])


def seq(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def gen_snv(rng):
    table = {}
    for c in SNV_CONTIGS:
        rows, pos = [], rng.randint(10000, 10100) if c != "MT" else 3
        for _ in range(400):
            ref = rng.choice(BASES)
            for alt in BASES:
                if alt != ref:
                    rows.append((c, str(pos), ref, alt) + score(rng))
            pos += rng.choice([1, 1, 1, 2, 3, 7, 40]) if c != "MT" else rng.choice([1, 2, 5])
        table[c] = rows
    return table


def gen_indel(rng):
    table = {}
    for c in INDEL_CONTIGS:
        rows, pos = [], rng.randint(10000, 10100)
        while len(rows) < 760:
            anchor = rng.choice(BASES)
            here = []
            for _ in range(rng.choice([1, 1, 2, 3, 4, 6])):
                tail = seq(rng, rng.choice([1, 1, 2, 3, 5, 9, 17, 33, 59]))
                pair = (anchor + tail, anchor) if rng.random() < 0.5 else (anchor, anchor + tail)
                here.append(pair)
                if rng.random() < 0.35 and len(tail) > 1:  # a sibling equal up to the last byte, and a prefix of it
                    last = rng.choice([b for b in BASES if b != tail[-1]])
                    sib = anchor + tail[:-1] + last
                    here.append((sib, anchor) if pair[1] == anchor else (anchor, sib))
                    pre = anchor + tail[:-1]
                    here.append((pre, anchor) if pair[1] == anchor else (anchor, pre))
            seen = set()
            for ref, alt in here:
                if (ref, alt) not in seen:
                    seen.add((ref, alt))
                    rows.append((c, str(pos), ref, alt) + score(rng))
            pos += rng.choice([1, 2, 3, 11, 50])
        table[c] = rows
    return table


def table_text(table, contigs):
    return HEADER + "".join("\t".join(r) + "\n" for c in contigs for r in table[c])


def mutate_last(rng, s):
    return s[:-1] + rng.choice([b for b in BASES if b != s[-1]])


def gen_variants(rng, snv, indel):
    """(class, contig, pos, ref, alt) drawn from the tables' rows and perturbed."""
    out = []
    name = {"MT": "M"}

    def add(cls, c, pos, ref, alt):
        out.append((cls, name.get(c, c), int(pos), ref, alt))

    for kind, table, contigs in (("snv", snv, SNV_CONTIGS), ("indel", indel, INDEL_CONTIGS)):
        rows = [r for c in contigs for r in table[c]]
        for cls, n in (("exact", 640), ("switched", 400), ("ref_eq_alt", 130), ("absent_pos", 160),
                       ("before_first", 110), ("after_last", 110), ("absent_contig", 110), ("last_byte", 130),
                       ("prefix", 130)):
            for _ in range(n):
                c, pos, ref, alt = rng.choice(rows)[:4]
                have = {int(r[1]) for r in table[c]}
                if cls == "exact":
                    add(kind + "_" + cls, c, pos, ref, alt)
                elif cls == "switched":
                    add(kind + "_" + cls, c, pos, alt, ref)
                elif cls == "ref_eq_alt":
                    x = rng.choice([ref, alt])
                    if kind == "indel" and len(x) == 1:
                        x = ref if len(ref) > 1 else alt  # len 1 twice would be looked up in the SNV table
                    add(kind + "_" + cls, c, pos, x, x)
                elif cls == "absent_pos":
                    p = int(pos) + 1
                    while p in have:
                        p += 1
                    add(kind + "_" + cls, c, p, ref, alt)
                elif cls == "before_first":
                    add(kind + "_" + cls, c, max(1, min(have) - rng.randint(1, 2)), ref, alt)
                elif cls == "after_last":
                    add(kind + "_" + cls, c, max(have) + rng.randint(1, 1000), ref, alt)
                elif cls == "absent_contig":
                    add(kind + "_" + cls, rng.choice(["Y", "Y", "M"] if kind == "indel" else ["Y"]), pos, ref, alt)
                elif cls == "last_byte":
                    if kind == "snv":  # (every other base is a row of its own: an allele no row has)
                        add(kind + "_" + cls, c, pos, ref, "N")
                    elif len(ref) > 1:
                        add(kind + "_" + cls, c, pos, mutate_last(rng, ref), alt)
                    else:
                        add(kind + "_" + cls, c, pos, ref, mutate_last(rng, alt))
                elif cls == "prefix":
                    if kind == "snv":  # a one-base allele against the indel table's longer ones and back
                        add(kind + "_" + cls, c, pos, ref, alt + rng.choice(BASES))
                    elif len(ref) > 1:
                        add(kind + "_" + cls, c, pos, rng.choice([ref[:-1], ref + rng.choice(BASES)]), alt)
                    else:
                        add(kind + "_" + cls, c, pos, ref, rng.choice([alt[:-1], alt + rng.choice(BASES)]))
    return out


def main():
    rng = random.Random(20251019)
    snv, indel = gen_snv(rng), gen_indel(rng)
    TABLES[SNV_FILE], TABLES[INDEL_FILE] = snv, indel
    variants = gen_variants(rng, snv, indel)
    counts = {}
    for v in variants:
        counts[v[0]] = counts.get(v[0], 0) + 1
    for k in sorted(counts):
        print("%-22s %d" % (k, counts[k]))
    assert min(counts.values()) >= 100, counts

    install_stubs()
    pysam = sys.modules["pysam"]
    pysam.TabixFile = TabixFile
    pysam.asTuple = lambda: None
    from AnnotatedVDB.Util.loaders.cadd_updater import CADDUpdater

    class Validator:
        def has_attr(self, field, pk, returnVal=True):
            return None

    loader = CADDUpdater("/nonexistent")
    loader._variant_validator = Validator()
    loader._skip_existing = True
    current = {}
    loader.is_duplicate = lambda metaseqId, returnMatch=False: [{"primary_key": current["pk"]}]

    # load_cadd_scores.py runs with or without a chromosome: the first pass leaves it
    # unset (chromosome from the primary key, cadd_updater.py:126-127), then one pass
    # per chromosome as update_cadd_scores_by_query(chromosome) does (:92-96)
    order = {c: i for i, c in enumerate(["22", "X", "M", "Y", "1", "21"])}
    variants.sort(key=lambda v: (order[v[1]], v[2], v[3], v[4], v[0]))
    lines = []
    setting = ""
    for k, (cls, c, pos, ref, alt) in enumerate(variants):
        if c in ("1", "21") and setting != "chr" + c:
            setting = "chr" + c
            loader.set_chromosome(setting)
        metaseq = "%s:%d:%s:%s" % (c, pos, ref, alt)
        pk = metaseq if rng.random() < 0.6 else metaseq + ":rs%d" % rng.randint(1, 10 ** 9)
        scores = None
        if rng.random() < 0.05:
            scores = rng.choice([{}, {"CADD_raw_score": 1.25, "CADD_phred": 10.5}])
        record = {"record_primary_key": pk, "metaseq_id": metaseq, "cadd_scores": scores}
        current["pk"] = pk
        before = loader.update_buffer(sizeOnly=True)
        if record["cadd_scores"] is not None:      # load_cadd_scores.py:114-117
            loader.increment_counter("skipped")
            got = ("", "", "")
        else:
            loader.set_current_variant(record)     # :119-120
            loader.buffer_variant()
            assert loader.update_buffer(sizeOnly=True) == before + 1
            got = loader.update_buffer()[-1]
        lines.append("\t".join((cls, setting, metaseq, pk, "" if scores is None else json.dumps(scores)) + tuple(got)))
    final = {k: loader.get_count(k) for k in ("snv", "indel", "not_matched", "update", "skipped")}
    print("variants", len(variants), "counters", final)
    lines.append("#counters\t" + json.dumps(final))

    def write(name, text):
        with open(os.path.join(HERE, name), "wb") as fh:
            with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
                gz.write(text.encode())
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")

    write("cadd_snv.tsv.gz", table_text(snv, SNV_CONTIGS))
    write("cadd_indel.tsv.gz", table_text(indel, INDEL_CONTIGS))
    write("cadd_expected.tsv.gz", "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

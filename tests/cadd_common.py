"""Shared by test_cadd_host.py and test_gpu_cadd.py: the CADD golden (written by
tests/golden/make_golden_cadd.py from the reference's own CADDUpdater) and a
pure-Python restatement of the reference's ``match`` and ``buffer_variant``
(Util/lib/python/loaders/cadd_updater.py:175-221), which test_cadd_host.py pins
to that golden before any test leans on it."""

import gzip
import json
import os

import numpy as np
import torch

from conftest import GOLDEN
from annotatedvdb_amd import _native as N
from annotatedvdb_amd.engine import RecordBatch

_cache = {}


def golden():
    """``(snv_text, indel_text, records, counters)``; a record is a dict of the
    expected file's columns (``expected``: the buffered tuple, or None if skipped)."""
    if "g" not in _cache:
        snv = gzip.open(os.path.join(GOLDEN, "cadd_snv.tsv.gz"), "rb").read()
        indel = gzip.open(os.path.join(GOLDEN, "cadd_indel.tsv.gz"), "rb").read()
        recs, counters = [], None
        for line in gzip.open(os.path.join(GOLDEN, "cadd_expected.tsv.gz"), "rt"):
            f = line.rstrip("\n").split("\t")
            if f[0] == "#counters":
                counters = json.loads(f[1])
                continue
            recs.append({"cls": f[0], "chromosome": f[1], "metaseq_id": f[2], "record_primary_key": f[3],
                         "cadd_scores": json.loads(f[4]) if f[4] else None,
                         "expected": None if f[4] else (f[5], f[6], f[7])})
        _cache["g"] = (snv, indel, recs, counters)
    return _cache["g"]


# ---- the restatement ---------------------------------------------------------
def parse_table(text: bytes):
    """{contig: [fields]} in file order — what a TabixFile over the text serves."""
    rows = {}
    for line in text.decode().split("\n"):
        if line and not line.startswith("#"):
            f = line.split("\t")
            rows.setdefault(f[0], []).append(f)
    return rows


def ref_match(snv, indel, metaseq_id):
    """cadd_updater.py:188-214: ``(table name or None, matched row fields or None)``."""
    chrm, position, ref, alt = metaseq_id.split(":")
    is_indel = len(ref) > 1 or len(alt) > 1
    table = indel if is_indel else snv
    cadd_chr = "MT" if chrm == "M" else chrm
    for row in table.get(cadd_chr, ()):  # (a missing contig: pysam's ValueError -> [])
        if int(row[1]) == int(position) and ref in (row[2], row[3]) and alt in (row[2], row[3]):
            return ("indel" if is_indel else "snv"), row
    return None, None


def ref_buffer(snv, indel, records):
    """load_cadd_scores.py:109-120 + buffer_variant over records carrying the
    golden's ``chromosome`` setting: ``(tuples, counters)``."""
    out, ctr = [], {"snv": 0, "indel": 0, "not_matched": 0, "update": 0, "skipped": 0}
    for r in records:
        if r["cadd_scores"] is not None:
            ctr["skipped"] += 1
            continue
        which, row = ref_match(snv, indel, r["metaseq_id"])
        if row is None:
            evidence = {}
            ctr["not_matched"] += 1
        else:
            evidence = {"CADD_raw_score": float(row[4]), "CADD_phred": float(row[5])}
            ctr[which] += 1
            ctr["update"] += 1
        pk = r["record_primary_key"]
        chrm = r.get("chromosome") or "chr" + pk.split(":")[0]
        out.append((pk, chrm, json.dumps(evidence)))
    return out, ctr


# ---- helpers over the package --------------------------------------------------
def run_updater(updater, records):
    """Feed the golden's records to a package CADDUpdater the way the reference's
    driver would: one buffer_variants call per chromosome setting."""
    i = 0
    while i < len(records):
        j = i
        while j < len(records) and records[j]["chromosome"] == records[i]["chromosome"]:
            j += 1
        if records[i]["chromosome"]:
            updater.set_chromosome(records[i]["chromosome"])
        updater.buffer_variants(records[i:j])
        i = j
    return list(updater.update_buffer()), {k: updater.get_count(k)
                                            for k in ("snv", "indel", "not_matched", "update", "skipped")}


CODE = {str(i + 1): i for i in range(22)}
CODE.update({"X": 22, "Y": 23, "M": 24, "MT": 24})


def batch_of(metaseq_ids, residue=None):
    """A CPU RecordBatch of ``chrom:pos:ref:alt`` ids; with ``residue``, junk bytes
    in front of record i's alleles put its heap offset at ``residue[i]`` mod 8."""
    chrom, pos, off, rl, al, heap = [], [], [], [], [], bytearray()
    for i, m in enumerate(metaseq_ids):
        c, p, r, a = m.split(":")
        while residue is not None and len(heap) % 8 != residue[i]:
            heap += b"#"
        chrom.append(CODE.get(c, 255))
        pos.append(int(p))
        off.append(len(heap))
        rl.append(len(r))
        al.append(len(a))
        heap += (r + a).encode()
    heap = bytes(heap) or b"\0"
    return RecordBatch(chrom=torch.tensor(chrom, dtype=torch.uint8), pos=torch.tensor(pos, dtype=torch.int32),
                       allele_off=torch.tensor(off, dtype=torch.int64), ref_len=torch.tensor(rl, dtype=torch.int32),
                       alt_len=torch.tensor(al, dtype=torch.int32),
                       heap=torch.from_numpy(np.frombuffer(heap, dtype=np.uint8).copy()))


def expect_arrays(snv_text, indel_text, metaseq_ids):
    """What cadd_match must give for these ids, by the restatement: row index in
    its table (-1), kind, raw and phred (NaN where unmatched)."""
    tabs = {"snv": parse_table(snv_text), "indel": parse_table(indel_text)}
    index = {}
    for name, t in tabs.items():
        k = 0
        for line in (snv_text if name == "snv" else indel_text).decode().split("\n"):
            if line and not line.startswith("#"):
                index.setdefault((name, line), k)  # the first of identical lines
                k += 1
    n = len(metaseq_ids)
    row, kind = np.full(n, -1, np.int32), np.zeros(n, np.uint8)
    raw, phred = np.full(n, np.nan), np.full(n, np.nan)
    for i, m in enumerate(metaseq_ids):
        which, r = ref_match(tabs["snv"], tabs["indel"], m)
        if r is not None:
            row[i] = index[(which, "\t".join(r))]
            kind[i] = N.CADD_SNV if which == "snv" else N.CADD_INDEL
            raw[i], phred[i] = float(r[4]), float(r[5])
    return row, kind, raw, phred


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)

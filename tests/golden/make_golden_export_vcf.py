#!/usr/bin/env python3
"""Generate the K14 golden fixture by running the REFERENCE's own ``run()``
(Util/bin/export_variant2vcf.py:38-102, with its ``print_file``, :29-35) over generated
records, one chromosome at a time, into a temporary directory.

Runs where the reference checkout is (never on the GPU machine); the tests read only the
file it writes:

  export_vcf.tsv.gz   the input rows, ``R<TAB>pk<TAB>metaseq_id<TAB>row_algorithm_id``
                      (``\\N``: NULL), in cursor order; then for every chromosome every
                      file ``run()`` produced, ``F<TAB>chromosome<TAB>name<TAB>nbytes``
                      followed by the file's nbytes bytes and a newline

The reference script is loaded by path and its module constants set:
``VARIANTS_PER_FILE = 1000``, ``ITERATION_SIZE = 250`` and ``args``.

What is stubbed (no database, no niagads package here): ``niagads.utils.sys.warning``
prints its arguments joined by blanks to ``file`` (the real one's prefix is not on this
machine, so the tests pin only the counts of the log's closing line);
``niagads.utils.list.qw`` splits on blanks; ``niagads.utils.reg_ex.matches(pattern,
value)`` is ``re.search(pattern, value) is not None``; ``Database.named_cursor`` yields,
for ``execute(SELECT_SQL, [chromosome])``, the rows of that chromosome as dicts, the way
a ``RealDictCursor`` does.
"""

from __future__ import annotations

import contextlib
import gzip
import importlib.util
import os
import random
import re
import sys
import tempfile
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF, install_stubs  # noqa: E402

BASES = "ACGT"
CHROMOSOMES = ["1", "2", "X", "Y", "M"]  # the order the rows are stored in; Y has none
ROWS = {}                                # 'chr' + label -> [record dicts], in cursor order


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def warning(*args, file=sys.stderr, flush=False, **kw):
    if file is not sys.stderr:
        print(*args, file=file, flush=flush)


class Cursor:
    def __init__(self):
        self.itersize = None
        self.rows = []

    def execute(self, sql, params):
        assert "record_primary_key, metaseq_id, row_algorithm_id" in sql
        self.rows = ROWS.get(params[0], [])

    def __iter__(self):
        return iter(dict(r) for r in self.rows)


class Database:
    def __init__(self, config=None):
        pass

    def connect(self):
        pass

    def close(self):
        pass

    @contextlib.contextmanager
    def named_cursor(self, name, cursorFactory=None):
        assert cursorFactory == "RealDictCursor"
        yield Cursor()


def seq(rng, n):
    return "".join(rng.choice(BASES) for _ in range(n))


def digest(rng):
    return "".join(rng.choice("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_-") for _ in range(32))


def plain(rng, c, pos):
    """A valid record: SNVs mostly, short indels, now and then a key with an rsid."""
    ref = rng.choice(BASES) if rng.random() < 0.8 else seq(rng, rng.randint(2, 12))
    alt = rng.choice([b for b in BASES if b != ref[0]]) if rng.random() < 0.8 else seq(rng, rng.randint(2, 12))
    ms = "%s:%d:%s:%s" % (c, pos, ref, alt)
    pk = ms if rng.random() < 0.7 else ms + ":rs%d" % rng.randint(1, 10 ** 9)
    return {"record_primary_key": pk, "metaseq_id": ms, "row_algorithm_id": rng.choice([None, 1, 17, 2405])}


def invalid(rng, c, pos, k):
    """A record whose metaseq id holds I, R, D or N: each letter alone, symbolic alleles,
    an N deep inside a long allele."""
    ref, alt = [("A", "I"), ("R", "G"), ("C", "D"), ("N", "T"), ("A", "<DEL>"), ("G", "<INS>"), ("T", "<DUP>"),
                ("C", "<CNV>"), (seq(rng, 150) + "N" + seq(rng, 90), "A"), ("A", seq(rng, 40) + "N"),
                ("ACGTN", "ACG"), ("A", "<INV>")][k % 12]
    ms = "%s:%d:%s:%s" % (c, pos, ref, alt)
    pk = ms if len(ms) < 60 else "%s:%d:%s" % (c, pos, digest(rng))
    return {"record_primary_key": pk, "metaseq_id": ms, "row_algorithm_id": rng.choice([None, 3, 99])}


def chromosome_rows(rng, c, n_valid, n_invalid):
    """``n_valid`` valid and ``n_invalid`` invalid records of contig ``c``, positions ascending."""
    marks = [0] * n_valid + [1] * n_invalid
    rng.shuffle(marks)
    rows, pos, k = [], rng.randint(10000, 20000), 0
    for m in marks:
        pos += rng.choice([1, 1, 2, 5, 40])
        if m:
            rows.append(invalid(rng, c, pos, k))
            k += 1
        else:
            rows.append(plain(rng, c, pos))
    return rows


def valid_index(rows):
    """Indices into ``rows`` of the valid records, in order (valid record v is rows[index[v]])."""
    return [i for i, r in enumerate(rows) if not re.search("I|R|D|N", r["metaseq_id"])]


def repeat(rows, v_from, v_to, other_id=True):
    """Valid record ``v_to`` takes the key of valid record ``v_from`` (its own metaseq id kept, or a changed one)."""
    at = valid_index(rows)
    src, dst = rows[at[v_from]], rows[at[v_to]]
    dst["record_primary_key"] = src["record_primary_key"]
    if not other_id:
        dst["metaseq_id"] = src["metaseq_id"]


def generate():
    rng = random.Random(20261014)
    # chr1: 2,600 valid records in three files of 1,000, with repeated keys
    rows = chromosome_rows(rng, "1", 2600, 60)
    repeat(rows, 10, 500)                    # a pair inside file 1, another metaseq id
    repeat(rows, 20, 21, other_id=False)     # a pair of neighbours, the same id
    repeat(rows, 1200, 1500)                 # threefold inside file 2
    repeat(rows, 1200, 1999)
    repeat(rows, 999, 1000)                  # a pair that straddles the boundary of files 1 and 2
    repeat(rows, 1990, 2010)                 # ... and of files 2 and 3, further apart
    repeat(rows, 300, 2300)                  # the same key in files 1 and 3
    bad = [i for i, r in enumerate(rows) if re.search("I|R|D|N", r["metaseq_id"])]
    rows[bad[5]]["record_primary_key"] = rows[bad[4]]["record_primary_key"]       # two invalid rows, one key
    rows[valid_index(rows)[700]]["record_primary_key"] = rows[bad[0]]["record_primary_key"]  # a valid row with an invalid row's key
    rows[bad[7]]["record_primary_key"] = rows[valid_index(rows)[50]]["record_primary_key"]   # and the other way round
    ROWS["chr1"] = rows
    # chr2: exactly 2,000 valid records: the third file holds the header alone
    ROWS["chr2"] = chromosome_rows(rng, "2", 2000, 25)
    # chrX: digest-form keys with long metaseq ids, NULL algorithm ids
    rows = chromosome_rows(rng, "X", 90, 13)
    for i in valid_index(rows)[::3]:
        c, pos = rows[i]["metaseq_id"].split(":")[:2]
        rows[i]["metaseq_id"] = "%s:%s:%s:%s" % (c, pos, seq(rng, rng.randint(51, 400)), seq(rng, rng.choice([1, 70])))
        rows[i]["record_primary_key"] = "%s:%s:%s" % (c, pos, digest(rng))
        rows[i]["row_algorithm_id"] = None
    ROWS["chrX"] = rows
    ROWS["chrM"] = chromosome_rows(rng, "M", 7, 1)
    for c in CHROMOSOMES:
        for r in ROWS.get("chr" + c, []):
            assert len(r["metaseq_id"].split(":")) == 4, r  # (the reference dies on any other)


def main():
    generate()
    install_stubs()
    _module("niagads.utils.sys", warning=warning, print_args=lambda a, pretty=True: str(a), execute_cmd=None)
    _module("niagads.utils.list", qw=lambda s, returnTuple=False: tuple(s.split()) if returnTuple else s.split())
    _module("niagads.utils.reg_ex", matches=lambda pattern, value: re.search(pattern, value) is not None)
    sys.modules["niagads.db.postgres"].Database = Database
    spec = importlib.util.spec_from_file_location("avdb_ref_export_variant2vcf",
                                                  os.path.join(REF, "Util/bin/export_variant2vcf.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)  # __name__ != "__main__": the main block is not run
    ref.args = types.SimpleNamespace(gusConfigFile=None)
    ref.VARIANTS_PER_FILE = 1000
    ref.ITERATION_SIZE = 250

    out = []
    for c in CHROMOSOMES:
        for r in ROWS.get("chr" + c, []):
            alg = r["row_algorithm_id"]
            out.append(("R\t%s\t%s\t%s\n" % (r["record_primary_key"], r["metaseq_id"],
                                             "\\N" if alg is None else alg)).encode())
    for c in CHROMOSOMES:
        with tempfile.TemporaryDirectory() as d:
            ref.run(d, "chr" + c)
            for name in sorted(os.listdir(d)):
                with open(os.path.join(d, name), "rb") as fh:
                    data = fh.read()
                out.append(b"F\tchr%s\t%s\t%d\n" % (c.encode(), name.encode(), len(data)) + data + b"\n")
                print("chr%s %-18s %8d bytes" % (c, name, len(data)))
    path = os.path.join(HERE, "export_vcf.tsv.gz")
    with open(path, "wb") as fh:
        with gzip.GzipFile(fileobj=fh, mode="wb", mtime=0, filename="") as gz:
            gz.write(b"".join(out))
    print("export_vcf.tsv.gz", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()

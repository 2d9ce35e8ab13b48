"""Shared by test_export_vcf_host.py and test_gpu_export_vcf.py (K14, the VCF files of a
variant export): the golden's rows and files, a pure-Python restatement of the
reference's loop with its dict (Util/bin/export_variant2vcf.py:29-35,63-97) over an
export's lines, a seeded export fuzz, the engine's output as numpy arrays, and the two
library entries called directly."""

import functools
import gzip
import os
import re

import numpy as np

from annotatedvdb_amd import _native as N
from cadd_update_common import CANON, split_lines

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_LINE = b"record_primary_key\tmetaseq_id\trow_algorithm_id"
VCF_HEADER = b"#CHRM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
GOLDEN_CHROMOSOMES = ["1", "2", "X", "Y", "M"]
GOLDEN_PER_FILE = 1000


@functools.lru_cache(maxsize=None)
def golden():
    """``(rows, files)``: the input rows ``(pk, metaseq_id, alg or None)`` as bytes, in
    cursor order, and ``{chromosome: {file name: bytes}}`` as the reference wrote them."""
    with gzip.open(os.path.join(HERE, "golden", "export_vcf.tsv.gz"), "rb") as fh:
        data = fh.read()
    rows, files, at = [], {}, 0
    while at < len(data):
        end = data.index(b"\n", at)
        f = data[at:end].split(b"\t")
        at = end + 1
        if f[0] == b"R":
            rows.append((f[1], f[2], None if f[3] == b"\\N" else f[3]))
        else:
            assert f[0] == b"F"
            n = int(f[3])
            files.setdefault(f[1].decode(), {})[f[2].decode()] = data[at:at + n]
            at += n + 1
    return rows, files


def export_line(pk, ms, alg=None, null=b"\\N") -> bytes:
    """One COPY-text line of the export; ``alg``: None (NULL, spelled ``null``: ``\\N``,
    empty, or ``None`` for no third field at all) or the value."""
    pk, ms = (x.encode() if isinstance(x, str) else x for x in (pk, ms))
    if alg is None:
        return pk + b"\t" + ms + (b"" if null is None else b"\t" + null)
    return pk + b"\t" + ms + b"\t" + (alg if isinstance(alg, bytes) else str(alg).encode())


def golden_export(vary_null=True) -> bytes:
    """The golden's rows as one export with a header line; NULL in its three spellings by turns."""
    spell = (b"\\N", b"", None)
    lines = [HEADER_LINE]
    for i, (pk, ms, alg) in enumerate(golden()[0]):
        lines.append(export_line(pk, ms, alg, spell[i % 3] if vary_null else b"\\N"))
    return b"\n".join(lines) + b"\n"


def ref_export(text, contigs=None, variants_per_file=10_000_000):
    """The reference's loop over an export: ``(files, invalid, counters)``; ``files`` is the
    list of the VCF files' bytes without their header lines, ``invalid`` the invalid
    file's.  A valid metaseq id that does not split into four raises ``ValueError`` as
    ``chr, pos, ref, alt = metaseqId.split(':')`` does."""
    keep = None if contigs is None else {c if c in CANON else None for c in contigs}
    ctr = {"valid": 0, "invalid": 0, "skipped_lines": 0, "filtered": 0, "dropped": 0}
    files, invalid, variants = [], [], {}

    def print_file():
        out = []
        for pk, ms in variants.items():
            c, p, r, a = ms.split(b":")
            out.append(b"\t".join((c, p, pk, r, a, b".", b".", b".")) + b"\n")
        files.append(b"".join(out))

    for line in split_lines(text):
        f = line.split(b"\t")
        if len(f) < 2 or f[0] == b"record_primary_key":
            ctr["skipped_lines"] += 1
            continue
        pk, ms = f[0], f[1]
        label = ms.split(b":")[0].decode("latin-1")
        if keep is not None and (label if label in CANON else None) not in keep:
            ctr["filtered"] += 1
            continue
        alg = b"None" if len(f) < 3 or f[2] in (b"", b"\\N") else f[2]
        if re.search(b"I|R|D|N", ms):
            invalid.append(pk + b"\t" + alg + b"\n")
            ctr["invalid"] += 1
            continue
        ctr["valid"] += 1
        ctr["dropped"] += pk in variants
        variants[pk] = ms
        if ctr["valid"] % variants_per_file == 0:
            print_file()
            variants = {}
    print_file()  # residuals
    return files, b"".join(invalid), ctr


_ALGS = (None, None, b"1", b"17", b"2405", b"x y", b"back\\slash")


def fuzz_export(rng, ids, n_lines, long_allele=None, repeats=0.0):
    """An export of exactly ``n_lines`` lines over the metaseq ids ``ids``: valid and
    invalid rows, NULL as ``\\N``, as an empty field and as a missing field, extra columns,
    keys with an rsid, without a ':' and empty, headers, empty and one-field lines, CRLF,
    the last line with or without its newline.  ``long_allele``: now and then an id whose
    alleles are that long (one in four of them invalid).  ``repeats``: the share of rows
    that take an earlier row's key."""
    lines, keys = [], []
    for _ in range(n_lines):
        k = rng.random()
        if k < 0.04:
            lines.append(rng.choice((b"", HEADER_LINE, b"one field", b"\r")))
            continue
        m = rng.choice(ids)
        c, p = m.split(":")[:2]
        if long_allele and rng.random() < 0.02:
            body = "".join(rng.choice("ACGT") for _ in range(long_allele))
            if rng.random() < 0.25:
                body = body[:long_allele // 2] + "N" + body[long_allele // 2 + 1:]
            m = "%s:%s:%s:%s" % (c, p, body, rng.choice(("A", body[:long_allele // 3])))
        elif rng.random() < 0.1:
            m = "%s:%s:%s:%s" % (c, p, rng.choice(("A", "N", "R")), rng.choice(("<DEL>", "I", "<INS>", "D", "ACGTNACGT")))
        pk = rng.choice((m, m, m + ":rs%d" % rng.randint(1, 10 ** 9), "rs%d" % rng.randint(1, 999), ""))
        if len(pk) > 200:
            pk = "%s:%s:%032x" % (c, p, rng.getrandbits(128))
        if keys and rng.random() < repeats:
            pk = rng.choice(keys)
        keys.append(pk)
        k = rng.random()
        alg = rng.choice(_ALGS)
        if k < 0.6:
            line = export_line(pk, m, alg, rng.choice((b"\\N", b"", None)))
        elif k < 0.8:
            line = export_line(pk, m, alg, b"\\N") + b"\textra\t\tcolumns"
        else:
            line = export_line(pk, m, alg, b"")
        if rng.random() < 0.1:
            line += b"\r"
        lines.append(line)
    if not lines:
        return b""
    text = b"\n".join(lines)
    # (a last line that is empty needs its newline to be a line at all, and a last '\r' its '\n')
    return text + b"\n" if lines[-1] in (b"", b"\r") or text.endswith(b"\r") or rng.random() < 0.5 else text


def fuzz_ids(rng, n=300):
    """Metaseq ids on canonical and other contigs (all valid: ACGT alleles)."""
    out = []
    for _ in range(n):
        c = rng.choice(("1", "1", "2", "7", "22", "X", "M", "MT", "GL9", "chr1"))
        ref = "".join(rng.choice("ACGT") for _ in range(rng.choice((1, 1, 1, 2, 9, 60))))
        alt = "".join(rng.choice("ACGT") for _ in range(rng.choice((1, 1, 1, 3, 30))))
        out.append("%s:%d:%s:%s" % (c, rng.randint(1, 250000000), ref, alt))
    return out


def files_of(res):
    """An ExportVcf's VCF files (without headers) and its invalid file, as bytes."""
    vcf = res.vcf_text.cpu().numpy().tobytes()
    return [vcf[slice(*res.file_span(k))] for k in range(1, res.n_files + 1)], res.invalid_text.cpu().numpy().tobytes()


def check_against_ref(res, text, contigs=None, variants_per_file=10_000_000):
    """The engine's result against the restatement: files, invalid file, counts, offsets."""
    files, invalid, ctr = ref_export(text, contigs, variants_per_file)
    got_files, got_invalid = files_of(res)
    assert got_files == files and got_invalid == invalid, (text[:200], contigs)
    assert {k: res.counts[k] for k in ctr} == ctr, (res.counts, ctr)
    off = res.vcf_row_off.cpu().numpy()
    assert len(off) == ctr["valid"] + 1 and off[0] == 0 and off[-1] == sum(map(len, files)) == res.counts["vcf_bytes"]
    ioff = res.invalid_row_off.cpu().numpy()
    assert len(ioff) == ctr["invalid"] + 1 and ioff[0] == 0 and ioff[-1] == len(invalid) == res.counts["invalid_bytes"]
    assert res.n_files == len(files) == ctr["valid"] // variants_per_file + 1
    return files, invalid, ctr


def as_arrays(res):
    """An ExportVcf (host or device) as numpy."""
    return {"vcf_text": res.vcf_text.cpu().numpy().copy(), "vcf_row_off": res.vcf_row_off.cpu().numpy().copy(),
            "invalid_text": res.invalid_text.cpu().numpy().copy(),
            "invalid_row_off": res.invalid_row_off.cpu().numpy().copy(), "flags": res.flags.cpu().numpy().copy(),
            "counts": dict(res.counts), "n_files": res.n_files, "file_start": list(res.file_start)}


def assert_same(got, want, what=""):
    for name in ("counts", "n_files", "file_start"):
        assert got[name] == want[name], (what, name, got[name], want[name])
    for name in ("vcf_row_off", "invalid_row_off", "flags", "vcf_text", "invalid_text"):
        x, y = got[name], want[name]
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        if not np.array_equal(x, y):
            k = int(np.nonzero(x != y)[0][0])
            raise AssertionError("%s: %s differs first at %d: %r != %r" % (what, name, k, x[k], y[k]))


def raw_size(eng, text, mask=N.EXIST_ALL_CONTIGS):
    """The size entry called directly on ``eng`` (host or device): the row lists as numpy
    (cut to their rows), the counts, and what the write entry needs again."""
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    row_start, pk_hash, inv_start = (eng.empty(m, torch.int64) for _ in range(3))
    pk_len, ms_len, out_len, inv_pk_len, inv_out_len = (eng.empty(m, torch.int32) for _ in range(5))
    fl = eng.empty(m, torch.uint8)
    counts = eng.empty(N.EXPVCF_N_COUNTS, torch.int64)
    if eng.host_only:
        run, suffix, tail = eng._call, "_host", ()
    else:
        ws = eng.scratch("export_vcf", N.size("avdb_export_vcf_workspace_size", nb, n_lines))
        run, suffix, tail = eng._launch, "", (ws, ws.numel())
    run("avdb_export_vcf_size" + suffix, t if nb else None, nb, n_lines, mask, row_start, pk_len, ms_len, out_len, fl,
        pk_hash, inv_start, inv_pk_len, inv_out_len, counts, *tail)
    cnt = dict(zip(N.EXPVCF_COUNTS, counts.cpu().tolist()))
    nv, ni = cnt["valid"], cnt["invalid"]
    state = {"t": t, "nb": nb, "n_lines": n_lines, "suffix": suffix, "tail": tail,
             "vcf": (row_start, pk_len, ms_len, out_len, fl), "invalid": (inv_start, inv_pk_len, None, inv_out_len, None)}
    arrays = {"row_start": row_start[:nv], "pk_len": pk_len[:nv], "ms_len": ms_len[:nv], "out_len": out_len[:nv],
              "flags": fl[:nv], "pk_hash": pk_hash[:nv], "inv_start": inv_start[:ni], "inv_pk_len": inv_pk_len[:ni],
              "inv_out_len": inv_out_len[:ni]}
    return {k: v.cpu().numpy().copy() for k, v in arrays.items()}, cnt, state


def raw_write(eng, state, which, n_rows, cap, pad=64, sentinel=0xA5):
    """The write entry of one stream called directly, the output ``pad`` bytes longer than
    ``cap`` with ``pad`` more in front, all filled with ``sentinel``:
    ``(rc, front pad, out, totals, row_off)``."""
    import torch
    buf = torch.full((pad + cap + pad,), sentinel, dtype=torch.uint8, device=eng.device)
    out = buf[pad:]  # (pad is a multiple of 8: the output stays 8-byte aligned)
    row_off = eng.empty(n_rows + 1, torch.int64)
    totals = eng.empty(2, torch.int64)
    name = "avdb_export_vcf_write" + state["suffix"]
    cols = state["vcf" if which == N.EXPVCF_STREAM_VCF else "invalid"]
    args = (state["t"] if state["nb"] else None, state["nb"], state["n_lines"], which, n_rows, *cols, out, cap, row_off,
            totals, *state["tail"])
    rc = N.call(name, eng.ctx, *args, check=False) if eng.host_only else \
        N.call(name, eng.ctx, *args, eng._stream(), check=False)
    b = buf.cpu().numpy()
    return rc, b[:pad], b[pad:], totals.cpu().tolist(), row_off.cpu().numpy()

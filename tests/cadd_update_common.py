"""Shared by test_cadd_update_host.py and test_gpu_cadd_update.py (K13, the CADD update
rows rendered from an export): the golden's records as exports, a pure-Python
restatement of the reference's query loop and ``buffer_variant``
(Load/bin/load_cadd_scores.py:109-120, Util/lib/python/loaders/cadd_updater.py:121-130,
187-221) over an export's lines, a seeded export fuzz, and the engine's output as
numpy arrays."""

import json

import numpy as np

import cadd_common as C
from annotatedvdb_amd import _native as N

CANON = {str(i + 1) for i in range(22)} | {"X", "Y", "M"}
HEADER_LINE = b"record_primary_key\tmetaseq_id\tcadd_scores"


def export_line(pk, metaseq_id, scores=None) -> bytes:
    """One COPY-text line of the export; ``scores``: None (NULL) or the JSON value."""
    third = "\\N" if scores is None else json.dumps(scores)
    return ("%s\t%s\t%s" % (pk, metaseq_id, third)).encode()


def golden_exports():
    """``[(chromosome or None, export text, records)]``: the golden's records, in file
    order, one export per run of one chromosome setting."""
    _, _, recs, _ = C.golden()
    out, i = [], 0
    while i < len(recs):
        j = i
        while j < len(recs) and recs[j]["chromosome"] == recs[i]["chromosome"]:
            j += 1
        text = b"".join(export_line(r["record_primary_key"], r["metaseq_id"], r["cadd_scores"]) + b"\n"
                        for r in recs[i:j])
        out.append((recs[i]["chromosome"] or None, text, recs[i:j]))
        i = j
    return out


def golden_text():
    """The rows the reference buffered for the golden's records, as K13 writes them."""
    _, _, recs, _ = C.golden()
    return "".join("\t".join(r["expected"]) + "\n" for r in recs if r["expected"] is not None).encode()


def split_lines(text: bytes):
    """The export's lines as K13 takes them: '\\n'-separated, one '\\r' before a '\\n' stripped."""
    lines = text.split(b"\n")
    ended = [True] * (len(lines) - 1) + [False]
    if lines[-1] == b"":
        lines, ended = lines[:-1], ended[:-1]
    return [ln[:-1] if nl and ln.endswith(b"\r") else ln for ln, nl in zip(lines, ended)]


def ref_export(snv_text, indel_text, text, chromosome=None, skip_existing=True, contigs=None):
    """The reference's loop over an export: ``(rows, counters)``; rows are the buffered
    ``(pk, chrom, json)`` tuples.  A metaseq id that does not split into four raises
    ``ValueError`` as ``chrm, position, ref, alt = metaseq_id.split(':')`` does."""
    snv, indel = C.parse_table(snv_text), C.parse_table(indel_text)
    rows, ctr = [], {"rows": 0, "skipped_lines": 0, "skipped": 0, "snv": 0, "indel": 0, "not_matched": 0}
    keep = None if contigs is None else {c if c in CANON else None for c in contigs}
    chrm = None
    if chromosome is not None:  # set_chromosome, then buffer_update_values
        label = str(chromosome).replace("chr", "")
        chrm = label if "chr" in label else "chr" + label
    for line in split_lines(text):
        f = line.split(b"\t")
        if len(f) < 2 or f[0] == b"record_primary_key":
            ctr["skipped_lines"] += 1
            continue
        pk, m = f[0].decode(), f[1].decode()
        label = m.split(":")[0]
        if keep is not None and (label if label in CANON else None) not in keep:
            ctr["skipped_lines"] += 1
            continue
        scores = None if len(f) < 3 or f[2] in (b"", b"\\N") else f[2]
        if skip_existing and scores is not None:
            ctr["skipped"] += 1
            continue
        which, row = C.ref_match(snv, indel, m)
        if row is None:
            evidence = {}
            ctr["not_matched"] += 1
        else:
            evidence = {"CADD_raw_score": float(row[4]), "CADD_phred": float(row[5])}
            ctr[which] += 1
        rows.append((pk, chrm if chrm is not None else "chr" + pk.split(":")[0], json.dumps(evidence)))
    ctr["rows"] = len(rows)
    return rows, ctr


def rows_text(rows) -> bytes:
    return "".join("\t".join(r) + "\n" for r in rows).encode()


_SCORES = ({"CADD_raw_score": 0.5, "CADD_phred": 12.1}, {}, {"CADD_raw_score": -1e-05, "CADD_phred": 0.0})


def fuzz_export(rng, ids, n_lines, long_allele=None):
    """An export of exactly ``n_lines`` lines over the metaseq ids ``ids``: NULL as
    ``\\N``, as an empty field and as a missing field, annotated records, extra columns,
    keys with an rsid and without a ':', headers, empty and one-field lines, CRLF, the
    last line with or without its newline.  ``long_allele``: now and then an id whose
    alleles are that long."""
    lines = []
    for _ in range(n_lines):
        k = rng.random()
        if k < 0.04:
            lines.append(rng.choice((b"", HEADER_LINE, b"one field", b"\r")))
            continue
        m = rng.choice(ids)
        if long_allele and rng.random() < 0.02:
            c, p = m.split(":")[:2]
            m = "%s:%s:%s:%s" % (c, p, C._bases(rng, long_allele), C._bases(rng, rng.choice((1, long_allele))))
        pk = rng.choice((m, m, m + ":rs%d" % rng.randint(1, 10 ** 9), "rs%d" % rng.randint(1, 999), ""))
        k = rng.random()
        if k < 0.5:
            line = b"%s\t%s\t\\N" % (pk.encode(), m.encode())
        elif k < 0.6:
            line = b"%s\t%s\t" % (pk.encode(), m.encode())
        elif k < 0.7:
            line = b"%s\t%s" % (pk.encode(), m.encode())
        elif k < 0.8:
            line = b"%s\t%s\t\\N\textra\t\tcolumns" % (pk.encode(), m.encode())
        elif k < 0.85:
            line = b"%s\t%s\t\t{}" % (pk.encode(), m.encode())
        else:
            line = export_line(pk, m, rng.choice(_SCORES))
        if rng.random() < 0.1:
            line += b"\r"
        lines.append(line)
    if not lines:
        return b""
    text = b"\n".join(lines)
    # (a last line that is empty needs its newline to be a line at all, and a last '\r' its '\n')
    return text + b"\n" if lines[-1] in (b"", b"\r") or text.endswith(b"\r") or rng.random() < 0.5 else text


def as_arrays(rows):
    """A CaddUpdateRows (host or device) as numpy: text, row_off, kind, flags, counts."""
    return {"text": rows.text.cpu().numpy().copy(), "row_off": rows.row_off.cpu().numpy().copy(),
            "kind": rows.kind.cpu().numpy().copy(), "flags": rows.flags.cpu().numpy().copy(),
            "counts": dict(rows.counts), "n": rows.n}


def assert_same_rows(got, want, what=""):
    assert got["n"] == want["n"] and got["counts"] == want["counts"], (what, got["counts"], want["counts"])
    for name in ("row_off", "kind", "flags", "text"):
        x, y = got[name], want[name]
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        if not np.array_equal(x, y):
            k = int(np.nonzero(x != y)[0][0])
            raise AssertionError("%s: %s differs first at %d: %r != %r" % (what, name, k, x[k], y[k]))


def raw_passes(eng, text, snv_t, indel_t, chrom=b"", mask=N.EXIST_ALL_CONTIGS, flags=N.CADDUPD_SKIP_EXISTING,
               cap=None, pad=64, sentinel=0xA5):
    """The two library entries called directly on ``eng`` (host or device), the output
    buffer ``pad`` bytes longer than ``cap`` (default: what the size pass asks for) and
    filled with ``sentinel``: ``(rc of the write pass, counts, out buffer, totals, cap)``."""
    import ctypes
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    views = [x.cols.view() if x is not None else None for x in (snv_t, indel_t)]
    shared = (*[ctypes.byref(v) if v is not None else None for v in views], chrom or None, len(chrom))
    row_start = eng.empty(m, torch.int64)
    pk_len, out_len, match = (eng.empty(m, torch.int32) for _ in range(3))
    kind, fl = eng.empty(m, torch.uint8), eng.empty(m, torch.uint8)
    counts = eng.empty(N.CADDUPD_N_COUNTS, torch.int64)
    if eng.host_only:
        run, suffix, tail = eng._call, "_host", ()
    else:
        ws = eng.scratch("cadd_update", N.size("avdb_cadd_update_workspace_size", nb, n_lines))
        run, suffix, tail = eng._launch, "", (ws, ws.numel())
    run("avdb_cadd_update_size" + suffix, t if nb else None, nb, n_lines, *shared, mask, flags, row_start, pk_len,
        kind, match, out_len, fl, counts, *tail)
    cnt = dict(zip(N.CADDUPD_COUNTS, counts.cpu().tolist()))
    cap = cnt["out_bytes"] if cap is None else cap
    out = torch.full((cap + pad,), sentinel, dtype=torch.uint8, device=eng.device)
    row_off = eng.empty(cnt["rows"] + 1, torch.int64)
    totals = eng.empty(2, torch.int64)
    name = "avdb_cadd_update_write" + suffix
    args = (t if nb else None, nb, n_lines, cnt["rows"], *shared, row_start, pk_len, kind, match, out_len, fl, out,
            cap, row_off, totals, *tail)
    rc = N.call(name, eng.ctx, *args, check=False) if eng.host_only else \
        N.call(name, eng.ctx, *args, eng._stream(), check=False)
    return rc, cnt, out.cpu().numpy(), totals.cpu().tolist(), cap

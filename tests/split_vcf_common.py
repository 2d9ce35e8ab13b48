"""Shared by test_split_vcf_host.py and test_gpu_split_vcf.py (K15, a whole-genome VCF
split by chromosome): the golden's runs and files, a pure-Python restatement of the
library's per-line rule (Util/bin/split_vcf_by_chr.py:37-50 on bytes), generated slabs, and
the two library entries called directly."""

import functools
import gzip
import os

import numpy as np

from annotatedvdb_amd import _native as N
from annotatedvdb_amd.chromosomes import CHROM_NAMES

HERE = os.path.dirname(os.path.abspath(__file__))
CHRMAP = os.path.join(HERE, "golden", "chrmap_grch38.tsv")
HEADER = b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
LABELS = [c.encode() for c in CHROM_NAMES]
NEAR_LABELS = [b"0", b"01", b"23", b"chr1", b"MT", b"x", b"1 ", b"", b"y", b"m", b"100", b"2a", b"XY"]
WS = b" \t\n\r\x0b\x0c"
HOST_TAILS = [bytes([c]) for c in range(0x1C, 0x20)] + [b"\xc2\x85", b"\xc2\xa0"]
OTHER, NONE, HOST = N.SPLIT_OTHER, N.SPLIT_NONE, N.SPLIT_LINE_HOST


@functools.lru_cache(maxsize=None)
def golden():
    """``(runs, cases)``: ``runs[name] = (text, with_map, {file name: bytes})`` as the reference
    read and wrote them; ``cases = [(case, exception name or None, with_map, line bytes)]``."""
    with gzip.open(os.path.join(HERE, "golden", "split_vcf.tsv.gz"), "rb") as fh:
        data = fh.read()
    runs, cases, at = {}, [], 0
    while at < len(data):
        end = data.index(b"\n", at)
        f = data[at:end].split(b"\t")
        n = int(f[-1])
        body = data[end + 1:end + 1 + n]
        at = end + 1 + n + 1
        if f[0] == b"I":
            runs[f[1].decode()] = (body, f[2] == b"1", {})
        elif f[0] == b"F":
            runs[f[1].decode()][2][f[2].decode()] = body
        else:
            assert f[0] == b"E"
            cases.append((f[1].decode(), None if f[2] == b"-" else f[2].decode(), f[3] == b"1", body))
    return runs, cases


@functools.lru_cache(maxsize=None)
def chrmap():
    """chrmap_grch38.tsv as ChromosomeMap reads it: source id -> chromosome without ``chr``."""
    from annotatedvdb_amd.parsers import ChromosomeMap
    return ChromosomeMap(CHRMAP).chromosome_map()


def split_lines(text: bytes):
    """``[(start, line bytes without the newline)]`` of a slab, as K0 counts its lines."""
    out, at = [], 0
    while at < len(text):
        k = text.find(b"\n", at)
        end = len(text) if k < 0 else k
        out.append((at, text[at:end]))
        at = end + 1
    return out


def ref_split(text: bytes, mapping=None):
    """The library's rule restated: per line ``code``, ``line_start``, ``out_len`` (bit 31: the
    host decides), the counts, and after that ``stream_off`` and the blob of the write pass."""
    code, start, out_len = [], [], []
    for s, line in split_lines(text):
        stored = line.rstrip(WS)
        host = HOST if stored and (0x1C <= stored[-1] <= 0x1F or stored[-1] >= 0x80) else 0
        start.append(s)
        if stored.startswith(b"#"):
            code.append(NONE)
            out_len.append(host)
            continue
        key = stored.split(b"\t")[0]
        if mapping is None:
            c = LABELS.index(key) if key in LABELS else OTHER
        else:
            label = mapping.get(key.decode("latin-1")) if all(b < 0x80 for b in key) else None
            c = CHROM_NAMES.index(label) if label in CHROM_NAMES else OTHER
        code.append(c)
        out_len.append((len(stored) + 1) | host)
    return (np.array(code, np.uint8), np.array(start, np.uint64), np.array(out_len, np.uint32)) + \
        ref_write(text, code, start, out_len)


def ref_counts(code, out_len):
    cnt = [0] * N.SPLIT_N_COUNTS
    cnt[N.SPLIT_COUNT_FIRST_OTHER] = (1 << 64) - 1
    for i, (c, ol) in enumerate(zip(code, out_len)):
        cnt[N.SPLIT_COUNT_HOST_LINES] += bool(int(ol) & HOST)
        if c == NONE:
            cnt[N.SPLIT_COUNT_COMMENTS] += 1
            continue
        cnt[N.SPLIT_COUNT_LINES + c] += 1
        cnt[N.SPLIT_COUNT_BYTES + c] += int(ol) & ~HOST
        if c == OTHER:
            cnt[N.SPLIT_COUNT_FIRST_OTHER] = min(cnt[N.SPLIT_COUNT_FIRST_OTHER], i)
    return cnt


def ref_write(text, code, start, out_len):
    """``(counts, stream_off, blob, dst_off)`` of the per-line arrays."""
    streams = [[] for _ in range(N.SPLIT_N_STREAMS)]
    where = []
    for c, s, ol in zip(code, start, out_len):
        n = int(ol) & ~HOST
        if c < N.SPLIT_N_STREAMS and n:
            where.append((int(c), sum(len(x) for x in streams[c])))
            streams[c].append(text[int(s):int(s) + n - 1] + b"\n")
        else:
            where.append(None)
    blobs = [b"".join(x) for x in streams]
    off = np.zeros(N.SPLIT_N_STREAMS + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in blobs])
    dst = np.array([(1 << 64) - 1 if w is None else int(off[w[0]]) + w[1] for w in where], np.uint64)
    return ref_counts(code, out_len), off, b"".join(blobs), dst


def vcf_line(chrom: bytes, k: int, length=None) -> bytes:
    """A data line of CHROM ``chrom``; ``length``: its bytes after the CHROM field and its tab."""
    tail = b"%d\trs%d\tA\tC\t.\t.\tK=%d" % (1000 + k, k, k)
    if length is not None:
        tail = (tail + b";" + b"ACGT" * (length // 4 + 1))[:length]
    return chrom + b"\t" + tail


def slab_of(chroms, lengths=None, comments=(), newline_at_end=True) -> bytes:
    """One line per entry of ``chroms`` (bytes keys); lines whose index is in ``comments`` are
    comment lines instead; ``lengths``: per line, or None."""
    lines = []
    for i, c in enumerate(chroms):
        if i in comments:
            lines.append(b"#comment %d" % i)
        else:
            lines.append(vcf_line(c, i, None if lengths is None else lengths[i]))
    return b"\n".join(lines) + (b"\n" if newline_at_end and lines else b"")


def edge_slabs():
    """``[(name, text)]``: every line class of the rule."""
    out = [("empty", b""), ("one_line_no_newline", b"1\t5\trs1\tA\tC"), ("one_newline", b"\n"),
           ("comments_only", b"##a\n#b\t\n#\n"),
           ("labels", b"".join(vcf_line(c, i) + b"\n" for i, c in enumerate(LABELS))),
           ("near_labels", b"".join(vcf_line(c, i) + b"\n" for i, c in enumerate(NEAR_LABELS))),
           ("bare_keys", b"\n".join(LABELS + NEAR_LABELS)),
           ("whitespace_only", b" \n\t\t\n \r\n\x0b\x0c\n\r\n   "),
           ("label_and_tabs", b"X\t\t\t\n1\t \t\r\nY \n M\n"),
           ("hash_after_blank", b" #not a comment\n\t#nor this\n#comment\n# \n"),
           ("long_unknown_key", b"K" * 300 + b"\t1\n" + b"1\t2\n" + b"Z" * 300 + b"\n"),
           ("cr_lf", b"1\t5\r\n2\t6\r\r\n#c\r\n3\t7\r"),
           ("mid_line_cr", b"1\t5\rx\n2\r\t6\n")]
    for t in HOST_TAILS:
        name = t.hex()
        out.append(("tail_" + name, b"1\t5\tA" + t + b"\n2\t7" + t + b" \t\r\n" + t + b"\n#c" + t + b"\nchr1" + t))
        out.append(("mid_" + name, b"1\t5" + t + b"A\n" + t + b"2\t7\n1" + t + b"\t9\n"))
    out.append(("invalid_utf8_mid_line", b"1\t5\t\xff\xfeA\n2\t\xc2\t7\n"))
    out.append(("lone_ff_tail", b"1\t5\tA\xff\n"))
    return out


def map_slab(mapping, n=400, seed=5):
    """Lines keyed by the map's source ids, by unknown ids and by labels (which the map does not hold)."""
    import random
    rng = random.Random(seed)
    keys = [k.encode() for k in mapping] + [b"NW_003315950.2", b"1", b"X", b"", b"NC_000001.1", b"NC_000001.111"]
    return b"".join(vcf_line(rng.choice(keys), i) + b"\n" for i in range(n))


# ---- the two entries called directly -----------------------------------------------------
def raw_size(eng, text, chrom_map=None):
    """The size entry called directly on ``eng`` (host or device): ``(code, line_start,
    out_len, counts)`` as numpy and what the write entry needs again."""
    import torch
    t = eng._as_text(text)
    nb, n_lines = t.numel(), eng._count_lines(t)
    m = max(1, n_lines)
    code = eng.empty(m, torch.uint8)
    line_start = eng.empty(m, torch.int64)
    out_len = eng.empty(m, torch.int32)
    counts = eng.empty(N.SPLIT_N_COUNTS, torch.int64)
    if eng.host_only:
        run, suffix, tail = eng._call, "_host", ()
    else:
        ws = eng.scratch("split_vcf", N.size("avdb_vcf_split_workspace_size", nb, n_lines))
        run, suffix, tail = eng._launch, "", (ws, ws.numel())
    run("avdb_vcf_split_size" + suffix, t if nb else None, nb, n_lines, chrom_map.handle if chrom_map else None, code,
        line_start, out_len, counts, *tail)
    state = {"t": t, "nb": nb, "n_lines": n_lines, "suffix": suffix, "tail": tail, "code": code,
             "line_start": line_start, "out_len": out_len}
    return (code[:n_lines].cpu().numpy().copy(), line_start[:n_lines].cpu().numpy().astype(np.uint64),
            out_len[:n_lines].cpu().numpy().astype(np.uint32), [int(x) for x in counts.cpu().numpy().astype(np.uint64)],
            state)


def raw_write(eng, state, cap, pad=64, sentinel=0xA5, want_dst=True):
    """The write entry called directly, the output ``pad`` bytes longer than ``cap`` with ``pad``
    more in front, all filled with ``sentinel``: ``(rc, front pad, out, totals, stream_off, dst_off)``."""
    import torch
    buf = torch.full((pad + cap + pad,), sentinel, dtype=torch.uint8, device=eng.device)
    out = buf[pad:]
    n = state["n_lines"]
    stream_off = eng.empty(N.SPLIT_N_STREAMS + 1, torch.int64)
    dst_off = eng.empty(max(1, n), torch.int64) if want_dst else None
    totals = eng.empty(2, torch.int64)
    name = "avdb_vcf_split_write" + state["suffix"]
    args = (state["t"] if state["nb"] else None, state["nb"], n, state["code"], state["line_start"], state["out_len"], out,
            cap, stream_off, dst_off, totals, *state["tail"])
    rc = N.call(name, eng.ctx, *args, check=False) if eng.host_only else \
        N.call(name, eng.ctx, *args, eng._stream(), check=False)
    b = buf.cpu().numpy()
    return (rc, b[:pad], b[pad:], [int(x) for x in totals.cpu().numpy().astype(np.uint64)],
            stream_off.cpu().numpy().astype(np.uint64),
            dst_off[:n].cpu().numpy().astype(np.uint64) if want_dst else None)


def check_against_ref(eng, text, mapping=None, chrom_map=None, what=""):
    """Both entries of ``eng`` on ``text`` against the restatement, array for array; the blob
    in a sentinel-filled buffer of exact capacity.  Returns the restatement's result."""
    code, start, out_len, cnt, off, blob, dst = ref_split(text, mapping)
    g_code, g_start, g_len, g_cnt, st = raw_size(eng, text, chrom_map)
    assert np.array_equal(g_code, code), (what, "code", g_code.tolist(), code.tolist())
    assert np.array_equal(g_start, start), (what, "line_start")
    assert np.array_equal(g_len, out_len), (what, "out_len", g_len.tolist(), out_len.tolist())
    assert g_cnt == cnt, (what, "counts", g_cnt, cnt)
    cap = len(blob)
    rc, front, out, totals, g_off, g_dst = raw_write(eng, st, cap)
    assert rc == 0 and totals == [cap, 0], (what, rc, totals)
    assert np.array_equal(g_off, off), (what, "stream_off", g_off.tolist(), off.tolist())
    assert np.array_equal(g_dst, dst), (what, "dst_off")
    assert out[:cap].tobytes() == blob, (what, "blob")
    assert (front == 0xA5).all() and (out[cap:] == 0xA5).all(), (what, "sentinels")
    return code, start, out_len, cnt, off, blob, dst


def same_on_both(dev_eng, host_eng, text, dev_map=None, host_map=None, what=""):
    """Device against host entries, array for array and blob for blob, on sentinel-filled buffers."""
    h_code, h_start, h_len, h_cnt, h_st = raw_size(host_eng, text, host_map)
    d_code, d_start, d_len, d_cnt, d_st = raw_size(dev_eng, text, dev_map)
    assert np.array_equal(d_code, h_code), (what, "code")
    assert np.array_equal(d_start, h_start), (what, "line_start")
    assert np.array_equal(d_len, h_len), (what, "out_len")
    assert d_cnt == h_cnt, (what, "counts", d_cnt, h_cnt)
    cap = sum(h_cnt[N.SPLIT_COUNT_BYTES:N.SPLIT_COUNT_BYTES + N.SPLIT_N_STREAMS])
    h = raw_write(host_eng, h_st, cap)
    d = raw_write(dev_eng, d_st, cap)
    assert d[0] == h[0] == 0 and d[3] == h[3] == [cap, 0], (what, d[0], d[3], h[3])
    assert np.array_equal(d[4], h[4]), (what, "stream_off")
    assert np.array_equal(d[5], h[5]), (what, "dst_off")
    assert (d[1] == 0xA5).all() and (d[2][cap:] == 0xA5).all(), (what, "sentinels")
    if not np.array_equal(d[2], h[2]):
        k = int(np.nonzero(d[2] != h[2])[0][0])
        raise AssertionError("%s: blob differs first at byte %d of %d" % (what, k, cap))
    return h_code, h_len, h_cnt, h[2][:cap].tobytes(), d_st

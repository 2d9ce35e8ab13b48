"""The passes over a '\\n'-separated text slab behind :class:`~annotatedvdb_amd.engine.Engine`:
K10a ``cadd_table_build``, K12 ``existing_table_build``, K13 ``cadd_update_rows``, K14
``export_vcf``, K15 ``split_vcf``, K16 ``lof_table_build`` / ``lof_update_rows``, K17
``qc_table_build`` / ``qc_update_rows``, K18a ``vep_consequences``, K18b ``vep_rows_table_build`` /
``vep_update_rows`` (with K18c's ``vep_output`` and K18d's ``allele_frequencies`` columns on request) and K19 ``txt_table_build`` /
``txt_update_rows`` / ``txt_direct_rows``.

The two-pass ones have one shape: line count -> size pass -> its counts to the host (second
sync) -> the rows the device leaves to the host rendered here -> outputs allocated -> write
pass -> the host-rendered rows copied into their spans -> totals checked (third sync).
:class:`SlabPass` holds what that shape needs from every pass; the functions below hold what
differs.  The ``Engine`` methods of the same names carry the contracts and delegate here.
"""

from __future__ import annotations

import ctypes
from typing import List

import numpy as np
import torch

from . import _native as N
from . import engine as E
from .chromosomes import CHROM_NAMES

_FILE_SALT = -7046029254386353131  # 0x9E3779B97F4A7C15 as int64: folds a row's file number into its key hash (K14)


class SlabPass:
    """One slab on the engine's device, its line count (a sync), and the library's entries
    for it: the ``_host`` ones on a host-only engine, else the device ones with the
    engine's scratch workspace ``scratch_name``, sized by ``workspace_size_entry``."""

    def __init__(self, engine, text, scratch_name: str, workspace_size_entry: str):
        self.engine = engine
        self.text = engine._as_text(text)
        self.nb = self.text.numel()
        self.n_lines = engine._count_lines(self.text)
        self.m = max(1, self.n_lines)  # entries of a per-line array: none is empty
        self.tp = self.text if self.nb else None
        if engine.host_only:
            self._run, self.suffix, self._tail = engine._call, "_host", ()
        else:
            ws = engine.scratch(scratch_name, N.size(workspace_size_entry, self.nb, self.n_lines))
            self._run, self.suffix, self._tail = engine._launch, "", (ws, ws.numel())

    def cols(self, *dtypes) -> List[torch.Tensor]:
        """Per-line (or per-row) arrays for the entries to fill."""
        return [self.engine.empty(self.m, dt) for dt in dtypes]

    def call(self, entry: str, *args):
        return self._run(entry + self.suffix, *args, *self._tail)

    def counts(self, tensor: torch.Tensor, names=None):
        """A pass's counts on the host (a sync): a dict by ``names``, or a list."""
        vals = [int(x) for x in tensor.cpu().numpy().astype(np.uint64)]
        return vals if names is None else dict(zip(names, vals))

    def rows_bytes(self, start: torch.Tensor, length: torch.Tensor) -> List[bytes]:
        """The text's spans ``[start[i], start[i] + length[i])``: one gather, one copy to the host."""
        raw = self.text[self.engine._spans(start, length)].cpu().numpy().tobytes()
        out, at = [], 0
        for n in length.tolist():
            out.append(raw[at:at + n])
            at += n
        return out

    def lengths(self, rendered: List[bytes]) -> torch.Tensor:
        return torch.tensor([len(x) for x in rendered], dtype=torch.int64).to(self.engine.device)

    def splice(self, out: torch.Tensor, off_at_rows: torch.Tensor, rendered: List[bytes]) -> torch.Tensor:
        """Host-rendered rows into their spans of ``out``, which start at ``off_at_rows``; their lengths."""
        new_len = self.lengths(rendered)
        blob = torch.from_numpy(np.frombuffer(b"".join(rendered), dtype=np.uint8).copy()).to(self.engine.device)
        out[self.engine._spans(off_at_rows, new_len)] = blob
        return new_len

    def check_totals(self, entry: str, got, want, what: str):
        """``got``: a write pass's totals, the last one its count of capacities exceeded;
        ``want``: the bytes the outputs were allocated with (an int for one stream)."""
        if isinstance(want, int):
            want, text = [want], f"{what} of {got[0]} bytes do not fit the {want} the size pass gave"
        else:
            text = f"{what} {got[:-1]} do not fit the sizes the size pass gave"
        if got[-1] or got[:-1] != want:
            raise N.NativeError(entry + self.suffix, N.AVDB_ERANGE, text)

    @staticmethod
    def raise_lone_cr(n: int, advice: str):
        raise ValueError(f"{n} carriage return(s) in the export that no newline follows: Python's "
                         f"text mode ends a line there and the device {advice}")

    def raise_bad_metaseq(self, row_start, flags, bit: int, n_rows: int, count: int):
        first = int(row_start[:n_rows][(flags[:n_rows] & bit) != 0][0])
        line = int((self.text[:first] == 10).sum()) + 1
        raise ValueError(f"line {line} of the export: the metaseq id does not have the four parts "
                         f"chrom:pos:ref:alt ({count} such line(s))")


def _lines_to_next(sp: SlabPass, rows, start, n: int) -> torch.Tensor:
    """Bytes from the starts of ``rows`` (indices into ``start[:n]``) to the next entry's start, or the text's end."""
    nxt = torch.where(rows + 1 < n, start[torch.clamp(rows + 1, max=max(n - 1, 0))],
                      torch.full_like(start[rows], sp.nb))
    return nxt - start[rows]


def cadd_table_build(engine, text):
    sp = SlabPass(engine, text, "cadd_build", "avdb_cadd_workspace_size")
    cols = sp.cols(torch.uint8, torch.int32, torch.int64, torch.int32, torch.int64, torch.int32, torch.float64,
                   torch.float64, torch.uint8)
    first_row = engine.empty(N.CADD_N_CONTIGS, torch.int32)
    end_row = engine.empty(N.CADD_N_CONTIGS, torch.int32)
    counts = engine.empty(N.CADD_N_COUNTS, torch.int64)
    sp.call("avdb_cadd_table_build", sp.tp, sp.nb, sp.n_lines, *cols, first_row, end_row, counts)
    cnt = counts.cpu().numpy().astype(np.uint64)
    n_rows = int(cnt[N.CADD_COUNT_ROWS])
    return E.CaddColumns(sp.text, n_rows, *[c[:n_rows] for c in cols], first_row, end_row, cnt)


def existing_table_build(engine, text, contigs=None):
    sp = SlabPass(engine, text, "existing_build", "avdb_existing_workspace_size")
    key_len, pk_len, frag_len, flags, row_off = sp.cols(torch.int32, torch.int32, torch.int32, torch.uint8, torch.int64)
    counts = engine.empty(N.EXIST_N_COUNTS, torch.int64)
    sp.call("avdb_existing_size", sp.tp, sp.nb, sp.n_lines, E.existing_contig_mask(contigs), key_len, pk_len, frag_len,
            flags, row_off, counts)
    cnt = sp.counts(counts, N.EXIST_COUNTS)
    if cnt["lone_cr"]:
        sp.raise_lone_cr(cnt["lone_cr"], "build does not; load this export with ExistingVariants.from_tsv "
                                         "(--existingHost)")
    n = cnt["rows"]
    frag_bytes = cnt["frag_bytes"]
    host_rows = rendered = None
    if cnt["frag_host"]:
        # the rows repr() escapes in: their pk and bin bytes ("pk<TAB>bin") to the host
        host_rows = torch.nonzero(flags[:n] & N.EXIST_FRAG_HOST).flatten()
        kl, pl = key_len[host_rows].long(), pk_len[host_rows].long()
        fl = frag_len[host_rows].long()
        span = fl - 36 + 1  # len(pk) + 1 + len(bin): the fixed text of a fragment is 36 bytes
        rendered = [repr({"primary_key": b[:p].decode("utf-8"), "bin_index": b[p + 1:].decode("utf-8")}).encode("utf-8")
                    for p, b in zip(pl.tolist(), sp.rows_bytes(row_off[host_rows] + kl + 1, span))]
        frag_bytes += sum(map(len, rendered)) - int(fl.sum())
        frag_len[host_rows] = sp.lengths(rendered).to(torch.int32)
    keys = engine.empty(max(1, cnt["key_bytes"]), torch.uint8)
    pks = engine.empty(max(1, cnt["pk_bytes"]), torch.uint8)
    frag = engine.empty(max(1, frag_bytes), torch.uint8)
    key_off, pk_off, frag_off = (engine.empty(n + 1, torch.int64) for _ in range(3))
    totals = engine.empty(4, torch.int64)
    sp.call("avdb_existing_write", sp.tp, sp.nb, sp.n_lines, n, key_len, pk_len, frag_len, flags, row_off, keys,
            cnt["key_bytes"], key_off, pks, cnt["pk_bytes"], pk_off, frag, frag_bytes, frag_off, totals)
    if rendered is not None:
        sp.splice(frag, frag_off[host_rows], rendered)
    sp.check_totals("avdb_existing_write", totals.cpu().tolist(), [cnt["key_bytes"], cnt["pk_bytes"], frag_bytes],
                    "blob totals")
    return E.ExistingColumns(n, keys, key_off, pks, pk_off, frag, frag_off, flags[:n], cnt)


def cadd_update_rows(engine, text, snv, indel, chromosome=None, skip_existing: bool = True, contigs=None):
    from .cadd import CADDUpdater, CaddTable  # (cadd imports the engine)
    tabs = [t if t is None or isinstance(t, CaddTable) else CaddTable(t, engine) for t in (snv, indel)]
    for t in tabs:
        if t is not None and t.cols.text.device != engine.device:
            raise ValueError("CADD table lives on another device than this engine")
    views = [t.cols.view() if t is not None else None for t in tabs]
    vp = [ctypes.byref(v) if v is not None else None for v in views]
    chrom = None
    if chromosome is not None:
        label = str(chromosome).replace("chr", "")  # set_chromosome, then buffer_update_values' prefix
        chrom = (label if "chr" in label else "chr" + label).encode("utf-8")
        if not 0 < len(chrom) <= N.CADDUPD_CHROM_MAX:
            raise ValueError(f"chromosome text of {len(chrom)} bytes (1 .. {N.CADDUPD_CHROM_MAX} taken)")
    shared = (*vp, chrom, len(chrom) if chrom else 0)
    sp = SlabPass(engine, text, "cadd_update", "avdb_cadd_update_workspace_size")
    row_start, pk_len, out_len, match, kind, flags = sp.cols(torch.int64, torch.int32, torch.int32, torch.int32,
                                                             torch.uint8, torch.uint8)
    counts = engine.empty(N.CADDUPD_N_COUNTS, torch.int64)
    sp.call("avdb_cadd_update_size", sp.tp, sp.nb, sp.n_lines, *shared, E.existing_contig_mask(contigs),
            N.CADDUPD_SKIP_EXISTING if skip_existing else 0, row_start, pk_len, kind, match, out_len, flags, counts)
    cnt = sp.counts(counts, N.CADDUPD_COUNTS)
    if cnt["lone_cr"]:
        sp.raise_lone_cr(cnt["lone_cr"], "pass does not; feed this export to CADDUpdater.buffer_variants record by "
                                         "record")
    n = cnt["rows"]
    if cnt["bad"]:
        sp.raise_bad_metaseq(row_start, flags, N.CADDUPD_BAD, n, cnt["bad"])
    out_bytes = cnt["out_bytes"]
    host_rows = rendered = None
    if cnt["host_rows"]:
        host_rows = torch.nonzero(flags[:n] & N.CADDUPD_ROW_HOST).flatten()
        recs = []
        # a row's span: its line, and the skipped lines behind it
        for b in sp.rows_bytes(row_start[host_rows], _lines_to_next(sp, host_rows, row_start, n)):
            f = b.split(b"\n", 1)[0]
            f = (f[:-1] if f.endswith(b"\r") and len(f) < len(b) else f).split(b"\t")
            recs.append({"record_primary_key": f[0].decode("utf-8", "surrogateescape"),
                         "metaseq_id": f[1].decode("utf-8", "surrogateescape")})
        u = CADDUpdater(tabs[0], tabs[1], engine)
        if chromosome is not None:
            u.set_chromosome(chromosome)
        u.buffer_variants(recs, skip_existing=False)
        rendered = [("\t".join(t) + "\n").encode("utf-8", "surrogateescape") for t in u.update_buffer()]
        kinds = []
        for rec, t in zip(recs, u.update_buffer()):
            _, _, r, a = rec["metaseq_id"].split(":")
            kinds.append(N.CADD_NONE if t[2] == "{}" else N.CADD_INDEL if len(r) > 1 or len(a) > 1 else N.CADD_SNV)
        for name in ("snv", "indel", "not_matched"):
            cnt[name] += u.get_count(name)
        out_bytes += sum(map(len, rendered))
        out_len[host_rows] = sp.lengths(rendered).to(torch.int32)
        kind[host_rows] = torch.tensor(kinds, dtype=torch.uint8).to(engine.device)
    cnt["out_bytes"] = out_bytes
    out_text = engine.empty(max(1, out_bytes), torch.uint8)
    row_off = engine.empty(n + 1, torch.int64)
    totals = engine.empty(2, torch.int64)
    sp.call("avdb_cadd_update_write", sp.tp, sp.nb, sp.n_lines, n, *shared, row_start, pk_len, kind, match, out_len,
            flags, out_text, out_bytes, row_off, totals)
    if rendered is not None:
        sp.splice(out_text, row_off[host_rows], rendered)
    sp.check_totals("avdb_cadd_update_write", totals.cpu().tolist(), out_bytes, "rows")
    return E.CaddUpdateRows(n, out_text[:out_bytes], row_off, kind[:n], flags[:n], cnt)


def export_vcf(engine, text, contigs=None, variants_per_file: int = 10_000_000):
    vpf = int(variants_per_file)
    if vpf < 1:
        raise ValueError("variants_per_file must be at least 1")
    sp = SlabPass(engine, text, "export_vcf", "avdb_export_vcf_workspace_size")
    row_start, pk_hash, inv_start = sp.cols(*[torch.int64] * 3)
    pk_len, ms_len, out_len, inv_pk_len, inv_out_len, flags = sp.cols(*[torch.int32] * 5, torch.uint8)
    counts = engine.empty(N.EXPVCF_N_COUNTS, torch.int64)
    sp.call("avdb_export_vcf_size", sp.tp, sp.nb, sp.n_lines, E.existing_contig_mask(contigs), row_start, pk_len,
            ms_len, out_len, flags, pk_hash, inv_start, inv_pk_len, inv_out_len, counts)
    cnt = sp.counts(counts, N.EXPVCF_COUNTS)
    if cnt["lone_cr"]:
        sp.raise_lone_cr(cnt["lone_cr"], "pass does not")
    nv, ni = cnt["valid"], cnt["invalid"]
    if cnt["bad"]:
        sp.raise_bad_metaseq(row_start, flags, N.EXPVCF_BAD, nv, cnt["bad"])
    n_files = nv // vpf + 1
    # rows of one file whose keys hash alike: neighbours after one sort of the hash with the file folded in
    # (equal (file, hash) pairs give equal sort keys; the host compare below sorts out any other)
    order = same = None
    n_cand = torch.zeros(1, dtype=torch.int64, device=engine.device)
    if nv > 1:
        key = pk_hash[:nv]
        if n_files > 1:
            key = key + torch.div(torch.arange(nv, device=engine.device), vpf, rounding_mode="floor") * _FILE_SALT
        skey, order = torch.sort(key)
        same = skey[1:] == skey[:-1]
        n_cand = same.sum().view(1)
    cnt["dropped"] = 0
    file_rows = torch.arange(n_files, device=engine.device) * vpf

    def write(which, n, cols, nbytes):
        out = engine.empty(max(1, nbytes), torch.uint8)
        row_off = engine.empty(n + 1, torch.int64)
        totals = engine.empty(2, torch.int64)
        sp.call("avdb_export_vcf_write", sp.tp, sp.nb, sp.n_lines, which, n, *cols, out, nbytes, row_off, totals)
        return out, row_off, totals

    vcf_cols = (row_start, pk_len, ms_len, out_len, flags)
    vcf, vcf_off, vcf_tot = write(N.EXPVCF_STREAM_VCF, nv, vcf_cols, cnt["vcf_bytes"])
    inv, inv_off, inv_tot = write(N.EXPVCF_STREAM_INVALID, ni, (inv_start, inv_pk_len, None, inv_out_len, None),
                                  cnt["invalid_bytes"])
    end = torch.cat([vcf_tot, inv_tot, n_cand, vcf_off[file_rows]]).cpu().tolist()
    sp.check_totals("avdb_export_vcf_write", end[0:2], cnt["vcf_bytes"], "VCF rows")
    sp.check_totals("avdb_export_vcf_write", end[2:4], cnt["invalid_bytes"], "invalid rows")
    file_start = end[5:]
    if end[4]:
        member = torch.zeros(nv, dtype=torch.bool, device=engine.device)
        member[order[1:][same]] = True
        member[order[:-1][same]] = True
        rows = torch.nonzero(member).flatten()  # in file order
        pl = pk_len[rows].long()
        groups = {}  # (file, key bytes) -> [(row, metaseq id)]
        for r, p, b in zip(rows.tolist(), pl.tolist(), sp.rows_bytes(row_start[rows], pl + 1 + ms_len[rows].long())):
            groups.setdefault((r // vpf, b[:p]), []).append((r, b[p + 1:]))
        first, rendered, dropped = [], [], []
        for (_, pk), g in groups.items():
            if len(g) > 1:  # variants[primaryKey] = metaseqId: the first one's place, the last one's id
                c, p, r, a = g[-1][1].split(b":")
                first.append(g[0][0])
                rendered.append(b"\t".join((c, p, pk, r, a, b".", b".", b".")) + b"\n")
                dropped += [x[0] for x in g[1:]]
        if first:
            first_t, dropped_t = (torch.tensor(x, dtype=torch.int64, device=engine.device) for x in (first, dropped))
            cnt["vcf_bytes"] += sum(map(len, rendered)) - int(out_len[first_t].sum()) - int(out_len[dropped_t].sum())
            cnt["dropped"] = len(dropped)
            flags[first_t] |= N.EXPVCF_ROW_HOST
            flags[dropped_t] |= N.EXPVCF_DROPPED
            out_len[first_t] = sp.lengths(rendered).to(torch.int32)
            out_len[dropped_t] = 0
            vcf, vcf_off, vcf_tot = write(N.EXPVCF_STREAM_VCF, nv, vcf_cols, cnt["vcf_bytes"])
            sp.splice(vcf, vcf_off[first_t], rendered)
            end = torch.cat([vcf_tot, vcf_off[file_rows]]).cpu().tolist()
            sp.check_totals("avdb_export_vcf_write", end[0:2], cnt["vcf_bytes"], "VCF rows")
            file_start = end[2:]
    file_start = [int(x) for x in file_start] + [cnt["vcf_bytes"]]
    return E.ExportVcf(vcf[:cnt["vcf_bytes"]], vcf_off, inv[:cnt["invalid_bytes"]], inv_off, flags[:nv], cnt, n_files,
                       vpf, file_start)


def split_vcf(engine, text, chrom_map=None, unknown: str = "raise"):
    if unknown not in ("raise", "keep"):
        raise ValueError("unknown must be 'raise' or 'keep'")
    if isinstance(chrom_map, dict):
        chrom_map = engine.split_chrom_map(chrom_map)
    sp = SlabPass(engine, text, "split_vcf", "avdb_vcf_split_workspace_size")
    n_lines = sp.n_lines
    code, line_start, out_len = sp.cols(torch.uint8, torch.int64, torch.int32)
    counts = engine.empty(N.SPLIT_N_COUNTS, torch.int64)
    handle = chrom_map.handle if chrom_map is not None else None
    sp.call("avdb_vcf_split_size", sp.tp, sp.nb, n_lines, handle, code, line_start, out_len, counts)
    cnt = sp.counts(counts)
    n_of = cnt[N.SPLIT_COUNT_LINES:N.SPLIT_COUNT_LINES + N.SPLIT_N_STREAMS]
    b_of = cnt[N.SPLIT_COUNT_BYTES:N.SPLIT_COUNT_BYTES + N.SPLIT_N_STREAMS]
    comments, host_lines = cnt[N.SPLIT_COUNT_COMMENTS], cnt[N.SPLIT_COUNT_HOST_LINES]
    first_other = cnt[N.SPLIT_COUNT_FIRST_OTHER] if n_of[N.SPLIT_OTHER] else None
    mapping = chrom_map.mapping if chrom_map is not None else None

    def stream_of_key(key: str) -> int:
        label = key if mapping is None else mapping.get(key)
        return CHROM_NAMES.index(label) if isinstance(label, str) and label in CHROM_NAMES else N.SPLIT_OTHER

    decode_error = None  # (line, the UnicodeDecodeError) of the first line whose decode raises
    if host_lines:
        rows = torch.nonzero(out_len[:n_lines] < 0).flatten()  # bit 31: N.SPLIT_LINE_HOST
        old_code, old_len = code[rows].cpu().tolist(), (out_len[rows] & 0x7FFFFFFF).cpu().tolist()
        new_code, new_len = [], []
        for i, (r, line) in enumerate(zip(rows.tolist(), sp.rows_bytes(line_start[rows],
                                                                       _lines_to_next(sp, rows, line_start, n_lines)))):
            try:
                line = line.decode("utf-8").rstrip()
            except UnicodeDecodeError as e:
                if decode_error is None:
                    decode_error = (r, e)
                new_code.append(old_code[i])
                new_len.append(old_len[i])
                continue
            if line.startswith("#"):
                c, ln = N.SPLIT_NONE, 0
            else:
                c, ln = stream_of_key(line.split("\t")[0]), len(line.encode("utf-8")) + 1
            new_code.append(c)
            new_len.append(ln)
            if old_code[i] < N.SPLIT_N_STREAMS:
                n_of[old_code[i]] -= 1
                b_of[old_code[i]] -= old_len[i]
            else:
                comments -= 1
            if c < N.SPLIT_N_STREAMS:
                n_of[c] += 1
                b_of[c] += ln
            else:
                comments += 1
        code[rows] = torch.tensor(new_code, dtype=torch.uint8).to(engine.device)
        out_len[rows] = torch.tensor(new_len, dtype=torch.int32).to(engine.device)
        others = torch.nonzero(code[:n_lines] == N.SPLIT_OTHER).flatten()
        first_other = int(others[0]) if others.numel() else None
    if decode_error is not None and (unknown == "keep" or first_other is None or decode_error[0] < first_other):
        raise decode_error[1]
    if first_other is not None and unknown == "raise":
        b = int(line_start[first_other])
        line = sp.text[b:b + int(out_len[first_other] & 0x7FFFFFFF) - 1].cpu().numpy().tobytes()
        key = line.decode("utf-8", "replace").split("\t")[0]
        err = KeyError(key if mapping is None or key not in mapping else mapping[key])
        err.line = first_other + 1
        if hasattr(err, "add_note"):
            err.add_note(f"line {err.line} of the slab: no chr<label>.vcf takes it")
        raise err
    total = sum(b_of)
    out = engine.empty(max(1, total), torch.uint8)
    stream_off = engine.empty(N.SPLIT_N_STREAMS + 1, torch.int64)
    totals = engine.empty(2, torch.int64)
    sp.call("avdb_vcf_split_write", sp.tp, sp.nb, n_lines, code, line_start, out_len, out, total, stream_off, None,
            totals)
    end = torch.cat([totals, stream_off]).cpu().tolist()
    sp.check_totals("avdb_vcf_split_write", end[0:2], total, "lines")
    cnt = {"lines": n_of, "bytes": b_of, "comments": comments, "host_lines": host_lines}
    return E.SplitVcf(out[:total], [int(x) for x in end[2:]], cnt, first_other)


def _line_number(sp: SlabPass, offset: int) -> int:
    """The 1-based number of the line that starts at ``offset``."""
    return int((sp.text[:offset] == 10).sum()) + 1


def _alt_table_build(engine, text, name: str, count_names, extra, host_line, all_host: bool = False,
                     what: str = "VCF", row_json: bool = False, keep=None):
    """The table build K16a, K17a and K19a share: entry ``avdb_<name>_size`` / ``_write`` with ``extra``
    arguments behind the line (and row) counts, one row per ALT allele of every entry (K19a: one row
    per entry), one JSON text (K19a: body) per entry; ``what`` names the file in messages.  ``host_line(line bytes, cnt)`` renders a line the device leaves to the host (flag 1 of
    its entry): ``(lookup ids, JSON, row flag bits)``.  ``all_host``: every entry is such a line.
    ``row_json`` (K18b): a row has a JSON text of its own; ``host_line(line bytes, cnt, offset of the line)``
    then returns one text per lookup id, and an entry's JSON is its rows' back to back.  ``keep`` (K18c): a dict
    that receives the entries' columns as ``keep["ents"]`` and their number as ``keep["n_entries"]``.
    Returns :class:`~annotatedvdb_amd.engine.LofTable`'s members, in its order."""
    sp = SlabPass(engine, text, name, f"avdb_{name}_workspace_size")
    ent_start, ent_alts, ent_key, ent_json, ent_flags = sp.cols(torch.int64, torch.int32, torch.int32, torch.int32,
                                                                torch.uint8)
    ents = (ent_start, ent_alts, ent_key, ent_json, ent_flags)
    counts = engine.empty(len(count_names), torch.int64)
    sp.call(f"avdb_{name}_size", sp.tp, sp.nb, sp.n_lines, *extra, *ents, counts)
    cnt = sp.counts(counts, count_names)
    if cnt["lone_cr"]:
        raise ValueError(f"{cnt['lone_cr']} carriage return(s) inside lines of the {what}: Python's text mode ends a "
                         "line there and the device pass does not")
    ne = cnt["entries"]
    if keep is not None:
        keep.update(ents=ents, n_entries=ne)
    if all_host and ne:
        ent_flags[:ne] |= 1
        for col in (ent_alts, ent_key, ent_json):
            col[:ne] = 0
        cnt.update(rows=0, key_bytes=0, json_bytes=0, host_lines=ne)
    host = None
    if cnt["host_lines"]:
        # the lines outside the device subset: their text to the host, rendered in file order
        host = torch.nonzero(ent_flags[:ne] & 1).flatten()
        host_keys, host_json, host_bits, host_row_json = [], [], [], []
        for at, b in zip(ent_start[host].tolist(), sp.rows_bytes(ent_start[host], _lines_to_next(sp, host, ent_start, ne))):
            try:
                keys, js, bits = host_line(b.split(b"\n", 1)[0], cnt, at) if row_json else \
                    host_line(b.split(b"\n", 1)[0], cnt)
            except Exception as err:
                err.line = _line_number(sp, at)
                if hasattr(err, "add_note"):
                    err.add_note(f"line {err.line} of the {what}")
                raise
            host_keys.append(keys)
            host_json.append(b"".join(js) if row_json else js)
            host_bits.append(bits)
            host_row_json.append([len(x) for x in js] if row_json else None)
        alts = [len(k) for k in host_keys]
        kb = [sum(map(len, k)) for k in host_keys]
        cnt["rows"] += sum(alts)
        cnt["key_bytes"] += sum(kb)
        cnt["json_bytes"] += sum(map(len, host_json))
        ent_alts[host] = torch.tensor(alts, dtype=torch.int32).to(engine.device)
        ent_key[host] = torch.tensor(kb, dtype=torch.int32).to(engine.device)
        ent_json[host] = sp.lengths(host_json).to(torch.int32)
    n, key_bytes, json_bytes = cnt["rows"], cnt["key_bytes"], cnt["json_bytes"]
    keys = engine.empty(max(1, key_bytes), torch.uint8)
    json_blob = engine.empty(max(1, json_bytes), torch.uint8)
    key_off = engine.empty(n + 1, torch.int64)
    json_off, line_start = (engine.empty(max(1, n), torch.int64) for _ in range(2))
    json_len = engine.empty(max(1, n), torch.int32)
    flags = engine.empty(max(1, n), torch.uint8)
    totals = engine.empty(4, torch.int64)
    sp.call(f"avdb_{name}_write", sp.tp, sp.nb, sp.n_lines, ne, n, *extra, *ents, keys, key_bytes, key_off, json_blob,
            json_bytes, json_off, json_len, line_start, flags, totals)
    if host is not None and host.numel():
        def starts(lengths):  # where each entry's share of a blob (or its rows) begins
            return torch.cumsum(lengths[:ne].long(), 0) - lengths[:ne].long()
        koff, joff, roff = (starts(x)[host] for x in (ent_key, ent_json, ent_alts))
        sp.splice(keys, koff, [b"".join(k) for k in host_keys])
        sp.splice(json_blob, joff, host_json)
        rows_at, offs, bits_at, joffs = [], [], [], []
        for first, base, jbase, ks, bits, jl in zip(roff.tolist(), koff.tolist(), joff.tolist(), host_keys, host_bits,
                                                    host_row_json):
            for a, k in enumerate(ks):
                rows_at.append(first + a)
                offs.append(base)
                bits_at.append(bits)
                base += len(k)
                if row_json:  # a row's own span of its entry's JSON
                    joffs.append(jbase)
                    jbase += jl[a]
        if rows_at:
            at = torch.tensor(rows_at, dtype=torch.int64).to(engine.device)
            key_off[at] = torch.tensor(offs, dtype=torch.int64).to(engine.device)
            if any(bits_at):
                flags[at] |= torch.tensor(bits_at, dtype=torch.uint8).to(engine.device)
            if row_json:
                json_off[at] = torch.tensor(joffs, dtype=torch.int64).to(engine.device)
                json_len[at] = torch.tensor([x for jl in host_row_json for x in jl], dtype=torch.int32).to(engine.device)
    got = totals.cpu().tolist()
    if got[3] or got[:3] != [key_bytes, json_bytes, n]:
        raise N.NativeError(f"avdb_{name}_write" + sp.suffix, N.AVDB_ERANGE,
                            f"totals {got[:3]} do not fit the sizes the size pass gave")
    # K6 keeps the first of equal keys: over the keys in reverse row order that is the last record of an id
    lens = (key_off[1:] - key_off[:-1]).flip(0)
    rkey_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=engine.device), torch.cumsum(lens, 0)])
    rkeys = keys[engine._spans(key_off[:-1].flip(0), lens)] if n else keys[:0]
    keyset = engine.keyset_table(rkeys, rkey_off)
    hit = torch.zeros(max(1, n), dtype=torch.uint8, device=engine.device)
    return (engine, sp.text, n, keys[:key_bytes], key_off, rkeys, rkey_off, keyset, json_blob[:json_bytes],
            json_off[:n], json_len[:n], line_start[:n], flags[:n], hit[:n] if n else hit[:0], cnt)


def lof_table_build(engine, text):
    from .snpeff_lof import annotated_line

    def host_line(line, cnt):
        keys, js = annotated_line(line)
        if not js:  # neither value: the line contributes nothing
            keys = []
            cnt["no_values"] += 1
        return keys, js, 0

    return E.LofTable(*_alt_table_build(engine, text, "lof_table", N.LOF_COUNTS, (), host_line))


def qc_release(version) -> bytes:
    """The release key of a ``--version``: lower-cased, as ``get_datasource`` gives it
    (``variant_loader.py:98``); the bytes the device writes and compares."""
    release = str(version).lower().encode("utf-8")
    if not 0 < len(release) <= N.QC_RELEASE_MAX or any(c < 0x20 or c > 0x7E or c in b'"\\' for c in release):
        raise ValueError(f"version {version!r}: 1 to {N.QC_RELEASE_MAX} printable ASCII characters without "
                         "'\"' and '\\' are taken")
    return release


def qc_table_build(engine, text, version, header_fields=None):
    from .adsp_qc import HEADER_FIELDS, qc_line
    release = qc_release(version)
    fields = None if header_fields is None else list(header_fields)
    plain = fields is None or [f.lower().replace("#", "") for f in fields] == \
        [f.lower().replace("#", "") for f in HEADER_FIELDS]

    def host_line(line, cnt):
        keys, js, passed = qc_line(line, release.decode("ascii"), fields)
        cnt["pass"] += passed
        return keys, js, N.QC_PASS if passed else 0

    # (a release that holds "Infinity" makes generate_update_values raise for every line: the host's too)
    parts = _alt_table_build(engine, text, "qc_table", N.QC_COUNTS, (release, len(release)), host_line,
                             not plain or b"Infinity" in release)
    return E.QcTable(*parts, release)


def vep_consequences(engine, text, ranking):
    import os
    from . import bgzf
    from .vep_consequences import ConsequenceRanking, VepConsequences
    if not isinstance(ranking, ConsequenceRanking):
        ranking = ConsequenceRanking(ranking)
    if isinstance(text, (str, os.PathLike)):
        text = bgzf.read_whole(os.fspath(text), engine)
    tab = ranking.table(engine)
    sp = SlabPass(engine, text, "vep_index", "avdb_vep_index_workspace_size")
    n_csq, flags, types, in_start, in_len, id_start, id_len = sp.cols(torch.int32, torch.uint8, torch.uint8, torch.int64,
                                                                      torch.int32, torch.int64, torch.int32)
    counts = engine.empty(N.VEP_N_COUNTS, torch.int64)
    sp.call("avdb_vep_index_size", sp.tp, sp.nb, sp.n_lines, tab.ref, n_csq, flags, types, in_start, in_len, id_start,
            id_len, counts)
    cnt = sp.counts(counts, N.VEP_COUNTS)
    total = cnt["consequences"]
    per_line = n_csq[:sp.n_lines].long()
    csq_off = torch.zeros(sp.m, dtype=torch.int64, device=engine.device)
    csq_off[:sp.n_lines] = torch.cumsum(per_line, 0) - per_line
    cols = [engine.empty(max(1, total), dt) for dt in (torch.uint8, torch.int32, torch.int64, torch.int32, torch.int64,
                                                       torch.int32, torch.int64, torch.int32, torch.uint8, torch.int32,
                                                       torch.uint8)]
    totals = engine.empty(2, torch.int64)
    sp.call("avdb_vep_index_write", sp.tp, sp.nb, sp.n_lines, tab.ref, n_csq, flags, csq_off, total, *cols, totals)
    got = totals.cpu().tolist()
    if got != [total, 0]:
        raise N.NativeError("avdb_vep_index_write" + sp.suffix, N.AVDB_ERANGE,
                            f"{got[0]} rows written, {got[1]} line(s) that differ from the size pass's {total} rows")
    return VepConsequences(engine, sp.text, ranking, sp.n_lines, cnt,
                           (n_csq, flags, types, in_start, in_len, id_start, id_len, csq_off), cols)


def _vep_cleaned(engine, text, view, ent_flags, row_line_start, identity_only: bool):
    """K18c: the cleaned result of every line of the slab K18b's table was built from, once per line: the size
    pass, the lines it leaves to the host rendered by :func:`~annotatedvdb_amd.vep_rows.vep_output_line`, the
    offsets, the write pass, the host texts copied into their spans.  ``view``: K18b's ``VepRowsIn``;
    ``ent_flags``: its entries' flags (entry e is line e); ``row_line_start``: the table rows' line starts.
    Returns ``(blob, off, len, row_entry, flags, counts)``."""
    from .vep_rows import vep_output_line
    sp = SlabPass(engine, text, "vep_output", "avdb_vep_output_workspace_size")
    nl = sp.n_lines
    line_start, out_len, dict_at, dict_len, flags = sp.cols(torch.int64, torch.int32, torch.int32, torch.int32,
                                                            torch.uint8)
    counts = engine.empty(N.VEPOUT_N_COUNTS, torch.int64)
    fl = N.VEPOUT_IDENTITY_ONLY if identity_only else 0
    vp = ctypes.byref(view)
    sp.call("avdb_vep_output_size", sp.tp, sp.nb, nl, vp, ent_flags, fl, line_start, out_len, dict_at, dict_len, flags,
            counts)
    cnt = sp.counts(counts, N.VEPOUT_COUNTS)
    device_bytes = cnt["out_bytes"]
    host, rendered = None, []
    if cnt["host_lines"]:
        host = torch.nonzero(flags[:nl]).flatten()
        for at, b in zip(line_start[host].tolist(),
                         sp.rows_bytes(line_start[host], _lines_to_next(sp, host, line_start, nl))):
            try:
                rendered.append(vep_output_line(b.split(b"\n", 1)[0], identity_only).encode("utf-8"))
            except Exception as err:
                err.line = _line_number(sp, at)
                err.counts = cnt  # (the size pass's counts by reason: what sent the line here)
                if hasattr(err, "add_note"):
                    err.add_note(f"line {err.line} of the VEP output")
                raise
        out_len[host] = sp.lengths(rendered).to(torch.int32)
        cnt["out_bytes"] += sum(map(len, rendered))
    total = cnt["out_bytes"]
    lens = out_len[:nl].long()
    off = torch.zeros(sp.m, dtype=torch.int64, device=engine.device)
    off[:nl] = torch.cumsum(lens, 0) - lens
    blob = engine.empty(max(1, total), torch.uint8)
    totals = engine.empty(2, torch.int64)
    sp.call("avdb_vep_output_write", sp.tp, sp.nb, nl, vp, fl, off, out_len, dict_at, dict_len, flags, blob, total, totals)
    if host is not None and host.numel():
        sp.splice(blob, off[host], rendered)
    got = totals.cpu().tolist()
    if got != [device_bytes, 0]:
        raise N.NativeError("avdb_vep_output_write" + sp.suffix, N.AVDB_ERANGE,
                            f"{got[0]} bytes written, {got[1]} line(s) that differ from the size pass's {device_bytes} bytes")
    if nl and row_line_start.numel():
        row_entry = (torch.searchsorted(line_start[:nl].contiguous(), row_line_start.contiguous(), right=True) - 1).to(torch.int32)
    else:
        row_entry = torch.zeros(max(1, row_line_start.numel()), dtype=torch.int32, device=engine.device)
    return blob[:total], off[:nl], out_len[:nl], row_entry, flags[:nl], cnt


def _vep_freq(engine, text, view, ents, n_rows: int, identity_only: bool, match_refsnp: bool):
    """K18d: the ``allele_frequencies`` text of every row of the table K18b built from the slab: the size pass,
    the lines it leaves to the host rendered by :func:`~annotatedvdb_amd.vep_rows.allele_frequencies_line`, the
    offsets, the write pass, the host texts copied into their rows' spans.  ``view``: K18b's ``VepRowsIn``;
    ``ents``: its entries' columns (entry e is line e).  Returns ``(blob, off, len, flags, counts)``."""
    from .vep_rows import allele_frequencies_line
    sp = SlabPass(engine, text, "vep_freq", "avdb_vep_freq_workspace_size")
    nl = sp.n_lines
    ent_start, ent_alts, _, _, ent_flags = ents
    alts = ent_alts[:nl].long()
    row0 = torch.zeros(sp.m, dtype=torch.int64, device=engine.device)
    row0[:nl] = torch.cumsum(alts, 0) - alts
    fr_start, fr_len, fq_start, fq_len, flags = sp.cols(torch.int64, torch.int32, torch.int64, torch.int32, torch.uint8)
    freq_len = torch.zeros(max(1, n_rows), dtype=torch.int32, device=engine.device)
    counts = engine.empty(N.VEPFREQ_N_COUNTS, torch.int64)
    fl = (N.VEPFREQ_IDENTITY_ONLY if identity_only else 0) | (N.VEPFREQ_MATCH_REFSNP if match_refsnp else 0)
    vp = ctypes.byref(view)
    sp.call("avdb_vep_freq_size", sp.tp, sp.nb, nl, n_rows, vp, ent_start, ent_alts, ent_flags, row0, fl, fr_start, fr_len,
            fq_start, fq_len, flags, freq_len, counts)
    cnt = sp.counts(counts, N.VEPFREQ_COUNTS)
    device_bytes = cnt["out_bytes"]
    rows_at, rendered = [], []
    if cnt["host_lines"]:
        host = torch.nonzero(flags[:nl]).flatten()
        for at, first, n, b in zip(ent_start[host].tolist(), row0[host].tolist(), alts[host].tolist(),
                                   sp.rows_bytes(ent_start[host], _lines_to_next(sp, host, ent_start, nl))):
            if n == 0:  # (a line K18b lists as unranked: it has no rows)
                continue
            try:
                texts = [t.encode("utf-8") for _, t in allele_frequencies_line(b.split(b"\n", 1)[0], identity_only,
                                                                              match_refsnp)]
                if len(texts) != n:
                    raise ValueError(f"{len(texts)} ALT alleles where the table has {n} rows")
            except Exception as err:
                err.line = _line_number(sp, at)
                err.counts = cnt  # (the size pass's counts by reason: what sent the line here)
                if hasattr(err, "add_note"):
                    err.add_note(f"line {err.line} of the VEP output")
                raise
            rows_at += range(first, first + n)
            rendered += texts
        if rows_at:
            rows_at = torch.tensor(rows_at, dtype=torch.int64).to(engine.device)
            freq_len[rows_at] = sp.lengths(rendered).to(torch.int32)
            cnt["rows"] += len(rendered)
            cnt["out_bytes"] += sum(map(len, rendered))
    total = cnt["out_bytes"]
    lens = freq_len[:n_rows].long()
    off = torch.zeros(max(1, n_rows), dtype=torch.int64, device=engine.device)
    off[:n_rows] = torch.cumsum(lens, 0) - lens
    blob = engine.empty(max(1, total), torch.uint8)
    totals = engine.empty(2, torch.int64)
    sp.call("avdb_vep_freq_write", sp.tp, sp.nb, nl, n_rows, vp, ent_alts, row0, fr_start, fr_len, fq_start, fq_len, flags,
            off, freq_len, blob, total, totals)
    if len(rendered):
        sp.splice(blob, off[rows_at], rendered)
    got = totals.cpu().tolist()
    if got != [device_bytes, 0]:
        raise N.NativeError("avdb_vep_freq_write" + sp.suffix, N.AVDB_ERANGE,
                            f"{got[0]} bytes written, {got[1]} row(s) that differ from the size pass's {device_bytes} bytes")
    return blob[:total], off[:n_rows], freq_len[:n_rows], flags[:nl], cnt


def vep_rows_table_build(engine, text, ranking, vep_output: bool = False, identity_only: bool = False,
                         allele_frequencies: bool = False, match_refsnp: bool = False):
    import json
    import os
    from . import bgzf
    from .vep_consequences import ConsequenceRanking, UnrankedCombination
    from .vep_rows import vep_rows_line
    if not isinstance(ranking, ConsequenceRanking):
        ranking = ConsequenceRanking(ranking)
    if isinstance(text, (str, os.PathLike)):
        text = bgzf.read_whole(os.fspath(text), engine)
    text = engine._as_text(text)
    csq = vep_consequences(engine, text, ranking)  # K18a, as it is
    # the rank of every entry as json.dumps prints it: the device copies it, and never formats a float
    rank_text = [json.dumps(r).encode("ascii") for r in ranking.ranks]
    off = np.zeros(len(rank_text) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(t) for t in rank_text], dtype=np.uint64)
    blob = engine._as_text(b"".join(rank_text) or b"\0")
    rank_off = torch.from_numpy(off.view(np.int32)).to(engine.device)
    n_total = csq.counts["consequences"]
    el_rlen = engine.empty(max(1, n_total), torch.int32)
    view = N.VepRowsIn(len(rank_text), n_total, N.ptr(blob), int(off[-1]), N.ptr(rank_off),
                       *[N.ptr(getattr(csq, a)) for a in ("flags", "n_csq", "csq_off", "input_start", "input_len", "type",
                                                          "order", "el_start", "el_len", "al_start", "al_len", "entry",
                                                          "coding", "sorted")], N.ptr(el_rlen))
    unranked = []

    def host_line(line, cnt, at):
        try:
            rows = vep_rows_line(line, ranking)
        except UnrankedCombination as err:  # the reference re-ranks here: no rows, and the line is reported
            try:
                vid = json.loads(line).get("id")
            except (ValueError, AttributeError):
                vid = None
            unranked.append((int((text[:at] == 10).sum()) + 1, vid if isinstance(vid, str) else "", err.combination))
            return [], [], 0
        return ([k.encode("utf-8") for k, _, _ in rows],
                [(ms + "\t" + ranked).encode("utf-8") for _, ms, ranked in rows], 0)

    kept = {} if vep_output or allele_frequencies else None
    parts = _alt_table_build(engine, text, "vep_rows_table", N.VEPROWS_COUNTS, (ctypes.byref(view),), host_line,
                             what="VEP output", row_json=True, keep=kept)
    table = E.VepRowsTable(*parts, ranking, unranked, (csq, blob, rank_off, el_rlen))
    if vep_output:
        (table.cleaned, table.cleaned_off, table.cleaned_len, table.row_entry, table.cleaned_flags,
         table.cleaned_counts) = _vep_cleaned(engine, text, view, kept["ents"][4], table.line_start, identity_only)
        table.identity_only = bool(identity_only)
    if allele_frequencies:
        (table.freq, table.freq_off, table.freq_len, table.freq_flags, table.freq_counts) = _vep_freq(
            engine, text, view, kept["ents"], table.n_rows, identity_only, match_refsnp)
        table.identity_only, table.match_refsnp = bool(identity_only), bool(match_refsnp)
    return table


def vep_update_rows(engine, text, table, alg_id: int, adsp: bool = False, update_existing: bool = False, contigs=None):
    if table.text.device != engine.device:
        raise ValueError("the VEP rows table lives on another device than this engine")
    alg_id = int(alg_id)
    if not 0 <= alg_id < 1 << 63:
        raise ValueError("alg_id: a non-negative integer that fits 63 bits")
    flags = (N.VEPUPD_UPDATE_EXISTING if update_existing else 0) | (N.VEPUPD_ADSP if adsp else 0)
    widen = write_name = None
    write_extra = (flags, alg_id)
    cleaned = table.cleaned_view() if table.cleaned is not None else None
    if table.freq is not None:  # K18d: the row grows by its own frequency text and <TAB> (and K18c's part)
        freq = table.freq_view()
        write_name = "avdb_vep_freq_update_write"
        write_extra = (ctypes.byref(freq), ctypes.byref(cleaned) if cleaned is not None else None, flags, alg_id)
    elif cleaned is not None:  # K18c: the row grows by <TAB> and its line's cleaned text
        write_name, write_extra = "avdb_vep_output_update_write", (ctypes.byref(cleaned), flags, alg_id)
    if write_name is not None:
        def widen(sp, row_start, out_len, row_flags, match, n, cnt):
            if n:
                rows = match[:n].long()
                add = torch.zeros(n, dtype=torch.int64, device=engine.device)
                if cleaned is not None:
                    add += 1 + table.cleaned_len[table.row_entry[rows].long()]
                if table.freq is not None:
                    add += 1 + table.freq_len[rows]
                out_len[:n] += add.to(out_len.dtype)
                cnt["out_bytes"] += int(add.sum())

    n, out, row_off, match, _, cnt = _table_update_rows(
        engine, text, table, "vep_rows_update", N.LOFUPD_COUNTS, N.LOFUPD_BAD,
        (E.existing_contig_mask(contigs), flags, alg_id), write_extra, widen=widen, write_name=write_name)
    return E.LofUpdateRows(n, out, row_off, match, cnt)


def _copy_text(column: bytes) -> str:
    """A column of ``COPY ... TO``'s text format without its backslash escapes."""
    out, i, n = bytearray(), 0, len(column)
    esc = {0x62: 8, 0x66: 12, 0x6E: 10, 0x72: 13, 0x74: 9, 0x76: 11}
    while i < n:
        c = column[i]
        if c == 0x5C and i + 1 < n:
            i += 1
            c = esc.get(column[i], column[i])
        out.append(c)
        i += 1
    return out.decode("utf-8")


def _table_update_rows(engine, text, table, name: str, count_names, bad_bit: int, size_extra, write_extra,
                       fix_host_rows=None, widen=None, write_name=None):
    """The export join K16b, K17b and K19b share: entry ``avdb_<name>_size`` / ``_write`` with ``size_extra`` and
    ``write_extra`` arguments behind the table view, one row per record of the export whose id the table holds.
    ``fix_host_rows(sp, row_start, out_len, flags, n, cnt)`` settles the rows the device left to the host between
    the passes and returns how many of them it dropped (their ``out_len`` zeroed, ``cnt`` brought up to date).
    ``widen(sp, row_start, out_len, flags, match, n, cnt)`` (K18c) adds to the rows' lengths what ``write_name``, the
    write entry in place of ``avdb_<name>_write``, puts into them beyond the size entry's row; it shares the size
    entry's workspace.
    Returns ``(rows kept, text, row_off, match, flags, cnt)``."""
    view = table.view()
    vp = ctypes.byref(view)
    sp = SlabPass(engine, text, name, f"avdb_{name}_workspace_size")
    row_start, pk_len, match, out_len, flags = sp.cols(torch.int64, torch.int32, torch.int32, torch.int32, torch.uint8)
    counts = engine.empty(len(count_names), torch.int64)
    sp.call(f"avdb_{name}_size", sp.tp, sp.nb, sp.n_lines, vp, *size_extra, row_start, pk_len, match, out_len, flags,
            counts)
    cnt = sp.counts(counts, count_names)
    if cnt["lone_cr"]:
        sp.raise_lone_cr(cnt["lone_cr"], "pass does not")
    n = cnt["rows"]
    if cnt["bad"]:
        sp.raise_bad_metaseq(row_start, flags, bad_bit, n, cnt["bad"])
    dropped = fix_host_rows(sp, row_start, out_len, flags, n, cnt) if fix_host_rows and cnt["host_rows"] else 0
    if widen is not None:
        widen(sp, row_start, out_len, flags, match, n, cnt)
    write_name = write_name or f"avdb_{name}_write"
    out_bytes = cnt["out_bytes"]
    out_text = engine.empty(max(1, out_bytes), torch.uint8)
    row_off = engine.empty(n + 1, torch.int64)
    totals = engine.empty(2, torch.int64)
    sp.call(write_name, sp.tp, sp.nb, sp.n_lines, n, vp, *write_extra, row_start, pk_len, match, out_len, flags,
            out_text, out_bytes, row_off, totals)
    sp.check_totals(write_name, totals.cpu().tolist(), out_bytes, "rows")
    return n - dropped, out_text[:out_bytes], row_off, match[:n], flags[:n], cnt


def qc_update_rows(engine, text, table, update_existing: bool = False, contigs=None):
    import json
    if table.text.device != engine.device:
        raise ValueError("QC table lives on another device than this engine")

    def fix_host_rows(sp, row_start, out_len, flags, n, cnt):
        # the columns the device does not scan: json.loads and Python's `in`, as load():49 has it
        host_rows = torch.nonzero(flags[:n] & N.QCUPD_ROW_HOST).flatten()
        release = table.release.decode("ascii")
        drop = []
        for r, at, b in zip(host_rows.tolist(), row_start[host_rows].tolist(),
                            sp.rows_bytes(row_start[host_rows], _lines_to_next(sp, host_rows, row_start, n))):
            line = b.split(b"\n", 1)[0]
            column = (line[:-1] if line.endswith(b"\r") and len(line) < len(b) else line).split(b"\t")[2]
            try:
                value = json.loads(_copy_text(column))
            except ValueError as err:
                bad = ValueError(f"line {_line_number(sp, at)} of the export: the adsp_qc column is not JSON ({err})")
                bad.line = _line_number(sp, at)
                raise bad from err
            if value is not None and release in value:
                drop.append(r)
        if drop:
            drop_t = torch.tensor(drop, dtype=torch.int64, device=engine.device)
            cnt["out_bytes"] -= int(out_len[drop_t].sum())
            out_len[drop_t] = 0
            cnt["skipped"] += len(drop)
        return len(drop)

    return E.QcUpdateRows(*_table_update_rows(
        engine, text, table, "qc_update", N.QCUPD_COUNTS, N.QCUPD_BAD,
        (E.existing_contig_mask(contigs), N.QCUPD_UPDATE_EXISTING if update_existing else 0), (), fix_host_rows))


def lof_update_rows(engine, text, table, update_existing: bool = False, contigs=None):
    if table.text.device != engine.device:
        raise ValueError("LOF table lives on another device than this engine")
    n, out, row_off, match, _, cnt = _table_update_rows(
        engine, text, table, "lof_update", N.LOFUPD_COUNTS, N.LOFUPD_BAD,
        (E.existing_contig_mask(contigs), N.LOFUPD_UPDATE_EXISTING if update_existing else 0), ())
    return E.LofUpdateRows(n, out, row_off, match, cnt)


def _txt_header(engine, text, variant_id_type: str):
    """The slab as a tensor and its header, read by ``csv`` from the first bytes (one small copy)."""
    from .text_update import HEADER_WINDOW, read_header
    text = engine._as_text(text)
    return text, read_header(text[:HEADER_WINDOW].cpu().numpy().tobytes(), variant_id_type, text.numel())


def txt_table_build(engine, text, variant_id_type: str = "METASEQ"):
    from .text_update import host_line as render
    text, header = _txt_header(engine, text, variant_id_type)

    def host_line(line, cnt):
        key, label, tail = render(line, header)
        return [key], (label or b"") + b"\t" + tail, 0 if label is not None else N.TXT_ROW_PK_CHROM

    parts = _alt_table_build(engine, text, "txt_table", N.TXT_COUNTS, header.extra(), host_line, what="file")
    return E.TxtTable(*parts, header)


def txt_update_rows(engine, text, table, id_type: str = "METASEQ", adsp: bool = False, contigs=None):
    if id_type not in ("METASEQ", "REFSNP"):
        raise ValueError("id_type must be 'METASEQ' or 'REFSNP' (a file of primary keys needs no export: "
                         "txt_direct_rows)")
    if table.text.device != engine.device:
        raise ValueError("the table lives on another device than this engine")
    key_col, flags_arg = (1 if id_type == "METASEQ" else 2), (N.TXT_ADSP if adsp else 0)
    n, out, row_off, match, _, cnt = _table_update_rows(
        engine, text, table, "txt_update", N.TXTUPD_COUNTS, N.TXTUPD_BAD,
        (E.existing_contig_mask(contigs), key_col, flags_arg), (flags_arg,))
    return E.TxtUpdateRows(n, out, row_off, match, cnt)


def txt_direct_rows(engine, text, adsp: bool = False):
    from .text_update import host_line as render
    text, header = _txt_header(engine, text, "PRIMARY_KEY")
    shape = (header.skip_lines, len(header.fields), header.id_col, N.TXT_ADSP if adsp else 0)
    sp = SlabPass(engine, text, "txt_direct", "avdb_txt_direct_workspace_size")
    row_start, out_len, flags = sp.cols(torch.int64, torch.int32, torch.uint8)
    counts = engine.empty(N.TXTDIR_N_COUNTS, torch.int64)
    sp.call("avdb_txt_direct_size", sp.tp, sp.nb, sp.n_lines, *shape, row_start, out_len, flags, counts)
    cnt = sp.counts(counts, N.TXTDIR_COUNTS)
    if cnt["lone_cr"]:
        raise ValueError(f"{cnt['lone_cr']} carriage return(s) inside lines of the file: Python's text mode ends a "
                         "line there and the device pass does not")
    n, out_bytes = cnt["rows"], cnt["out_bytes"]
    host_rows = rendered = None
    if cnt["host_rows"]:
        host_rows = torch.nonzero(flags[:n] & N.TXT_LINE_HOST).flatten()
        rendered = []
        for at, b in zip(row_start[host_rows].tolist(),
                         sp.rows_bytes(row_start[host_rows], _lines_to_next(sp, host_rows, row_start, n))):
            try:
                pk, label, tail = render(b.split(b"\n", 1)[0], header)
            except Exception as err:
                err.line = _line_number(sp, at)
                if hasattr(err, "add_note"):
                    err.add_note(f"line {err.line} of the file")
                raise
            chrom = label if label is not None else pk.split(b":")[0]
            rendered.append(pk + b"\tchr" + chrom + b"\t" + tail + (b"\ttrue" if adsp else b"") + b"\n")
        out_bytes += sum(map(len, rendered))
        out_len[host_rows] = sp.lengths(rendered).to(torch.int32)
    cnt["out_bytes"] = out_bytes
    out_text = engine.empty(max(1, out_bytes), torch.uint8)
    row_off = engine.empty(n + 1, torch.int64)
    totals = engine.empty(2, torch.int64)
    sp.call("avdb_txt_direct_write", sp.tp, sp.nb, sp.n_lines, n, *shape, row_start, out_len, flags, out_text,
            out_bytes, row_off, totals)
    if rendered is not None:
        sp.splice(out_text, row_off[host_rows], rendered)
    sp.check_totals("avdb_txt_direct_write", totals.cpu().tolist(), out_bytes, "rows")
    return E.TxtUpdateRows(n, out_text[:out_bytes], row_off, None, cnt)

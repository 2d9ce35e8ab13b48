"""K18a: the consequences of VEP's JSON output, ranked and sorted as
``VepJsonParser.adsp_rank_and_sort_consequences`` leaves them (``vep_parser.py:103-110,145-175``),
and the most severe one per allele (``get_most_severe_consequence``, ``:326-340``).

:class:`ConsequenceRanking` is the ranking file as ``ConsequenceParser.__parse_ranking_file`` reads
it, :func:`vep_line` the reference's pass over one line in Python (the host path), and
:class:`VepConsequences` what :meth:`Engine.vep_consequences
<annotatedvdb_amd.engine.Engine.vep_consequences>` returns for a slab.

    python -m annotatedvdb_amd.vep_consequences --fileName x.json[.gz] --rankingFile r.txt --out summary.tsv
"""

from __future__ import annotations

import argparse
import csv
import ctypes
import json
import os
import sys
from collections import OrderedDict
from operator import itemgetter
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native as N

CONSEQUENCE_TYPES = ("transcript", "regulatory_feature", "motif_feature", "intergenic")
TYPE_KEYS = tuple(t + "_consequences" for t in CONSEQUENCE_TYPES)
CODING_CONSEQUENCES = ("synonymous_variant", "missense_variant", "inframe_insertion", "inframe_deletion", "stop_gained",
                       "stop_lost", "stop_retained_variant", "start_lost", "frameshift_variant",
                       "coding_sequence_variant")
MAX_TERMS = 64


class UnrankedCombination(LookupError):
    """A combination of terms the ranking lacks: the reference would re-rank here."""

    def __init__(self, terms):
        self.terms = list(terms)
        self.combination = ",".join(str(t) for t in self.terms)
        super().__init__(f"consequence combination {self.combination!r} is not in the ranking "
                         "(the reference re-ranks here; this package does not)")


def _to_numeric(value):
    try:
        return int(value)
    except (ValueError, TypeError):
        return float(value)


class ConsequenceRanking:
    """The ADSP consequence ranking, read as ``__parse_ranking_file`` reads it
    (``adsp_consequence_parser.py:105-126``): a tab-delimited file with a header, through
    ``csv.DictReader``; every ``consequence`` alphabetised (its terms sorted, which is what
    ``alphabetize_string_list`` is taken to do); its rank the ``rank`` column where the file has
    one (``save_ranking_file`` writes it; ints and floats, as ``to_numeric`` keeps them), else the
    load order from 1.  A combination the file repeats keeps its first place and its last rank, as
    the reference's dict does.  ``path_or_rows``: a path, or ``(consequence, rank or None)`` pairs.

    No re-ranking: ``__update_rankings`` (``rankOnLoad=True``, a combination the file lacks) rests
    on functions of ``GenomicsDBData.Util`` that are not part of this package's reference and cannot
    be pinned; :meth:`rank_of` raises :class:`UnrankedCombination` where the reference would re-rank.

    ``ValueError``: a rank that is no number, a combination that repeats a term (the device compares
    combinations as sets of terms), more than 64 distinct terms."""

    def __init__(self, path_or_rows):
        if isinstance(path_or_rows, (str, os.PathLike)):
            with open(path_or_rows, "r", newline="") as fh:
                rows = [(row["consequence"], row["rank"] if "rank" in row else None)
                        for row in csv.DictReader(fh, delimiter="\t")]
        else:
            rows = [(c, r) for c, r in path_or_rows]
        self._rankings: "OrderedDict[str, object]" = OrderedDict()
        load_rank = 1
        for conseq, rank in rows:
            key = ",".join(sorted(conseq.split(",")))
            if rank is None:
                self._rankings[key] = load_rank
                load_rank += 1
            else:
                try:
                    self._rankings[key] = rank if isinstance(rank, (int, float)) else _to_numeric(rank)
                except ValueError:
                    raise ValueError(f"ranking: the rank {rank!r} of {conseq!r} is no number") from None
        self.terms: List[str] = []
        seen = {}
        self._entry_terms = []
        for key in self._rankings:
            parts = key.split(",")
            if len(set(parts)) != len(parts):
                raise ValueError(f"ranking: the combination {key!r} repeats a term")
            for t in parts:
                if t not in seen:
                    seen[t] = len(self.terms)
                    self.terms.append(t)
            self._entry_terms.append(sorted(parts))
        if len(self.terms) > MAX_TERMS:
            raise ValueError(f"ranking: {len(self.terms)} distinct terms (at most {MAX_TERMS})")
        self._term_id = seen
        self.ranks = list(self._rankings.values())  # by entry
        self._tables: Dict[str, "_DeviceTable"] = {}

    def rankings(self) -> "OrderedDict[str, object]":
        """``get_rankings()``: combination -> rank, in file order."""
        return self._rankings

    def rank_of(self, terms):
        """``find_matching_consequence(terms)`` without the re-rank: one term is looked up as it
        is (``None`` when the ranking lacks it); several take the first entry whose terms are
        the same multiset, and raise :class:`UnrankedCombination` when there is none."""
        if len(terms) == 1:
            return self._rankings.get(terms[0])
        want = sorted(terms)
        for parts, rank in zip(self._entry_terms, self.ranks):
            if parts == want:
                return rank
        raise UnrankedCombination(terms)

    def masks(self) -> np.ndarray:
        """Per entry, the mask of its terms' numbers (``uint64``)."""
        return np.array([sum(1 << self._term_id[t] for t in parts) for parts in self._entry_terms], dtype=np.uint64)

    def table(self, engine) -> "_DeviceTable":
        """The ranking as the library reads it (``avdb_vep_table``), on ``engine``'s device."""
        key = str(engine.device)
        tab = self._tables.get(key)
        if tab is None:
            tab = self._tables[key] = _DeviceTable(self, engine)
        return tab


class _DeviceTable:
    def __init__(self, ranking: ConsequenceRanking, engine):
        # terms the device can meet in a line it answers: plain ASCII without '"' and '\\' (any
        # other is never equal to the bytes of a string the device compares)
        words, off, length = [], [], []
        for t in ranking.terms:
            b = t.encode("utf-8")
            off.append(len(words))
            length.append(len(b))
            padded = b + b"\0" * (-len(b) % 8) or b"\0" * 8
            words += list(np.frombuffer(padded, dtype="<u8"))
        masks = ranking.masks()
        n_entries = len(masks)
        n_slots = 1
        while n_slots < max(2, 2 * n_entries):
            n_slots *= 2
        slot_mask = np.zeros(n_slots, dtype=np.uint64)
        slot_entry = np.zeros(n_slots, dtype=np.int32)
        engine._call("avdb_vep_table_build", len(ranking.terms), masks if n_entries else None, n_entries, slot_mask,
                     slot_entry, n_slots)
        _, order = np.unique(np.array([float(r) for r in ranking.ranks], dtype=np.float64), return_inverse=True)
        coding = sum(1 << i for i, t in enumerate(ranking.terms) if t in CODING_CONSEQUENCES)

        def dev(a, dt):  # (unsigned arrays travel as the signed type of their width)
            a = np.ascontiguousarray(np.asarray(a, dtype=dt).reshape(-1))
            return torch.from_numpy(a.view(np.int64 if a.itemsize == 8 else np.int32)).to(engine.device)

        self.arrays = [dev(words if words else [0], np.uint64), dev(off or [0], np.uint32),
                       dev(length or [0], np.uint32), dev(slot_mask, np.uint64), dev(slot_entry, np.int32),
                       dev(order if n_entries else [0], np.uint32)]
        a = self.arrays
        self.view = N.VepTableView(len(ranking.terms), a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(),
                                   a[4].data_ptr(), n_slots, n_entries, a[5].data_ptr(), coding)
        self.ref = ctypes.byref(self.view)


def is_coding_consequence(terms) -> bool:
    terms = terms.split(",") if isinstance(terms, str) else terms
    return any(t in CODING_CONSEQUENCES for t in terms)


def rank_annotation(annotation, ranking: ConsequenceRanking):
    """``adsp_rank_and_sort_consequences`` over a parsed line, in place; returns those of the four
    keys the line has, as they are left."""
    for key in TYPE_KEYS:
        consequences = annotation[key] if key in annotation else None
        if consequences is None:
            continue
        result = {}
        for index, conseq in enumerate(consequences):
            va = conseq["variant_allele"]
            conseq["vep_consequence_order_num"] = index
            terms = conseq["consequence_terms"]
            ",".join(terms)  # (the reference's memo key: what is no list of strings raises here)
            conseq.update({"rank": ranking.rank_of(terms), "consequence_is_coding": is_coding_consequence(terms)})
            result.setdefault(va, []).append(conseq)
        for va in result:
            result[va] = sorted(result[va], key=itemgetter("rank", "vep_consequence_order_num"))
        annotation[key] = result
    return {key: annotation[key] for key in TYPE_KEYS if key in annotation}


def vep_line(line, ranking: ConsequenceRanking):
    """The host path of one line (``bytes`` or ``str``): what the reference leaves in
    ``_annotation`` for the ``<type>_consequences`` keys the line has, ``{key: {allele: [consequence,
    ...]}}``.  Raises what the reference raises for the line (``json.JSONDecodeError``, ``KeyError``,
    ``TypeError`` for an unknown single term beside a ranked one in an allele's list), and
    :class:`UnrankedCombination` where it would re-rank."""
    return rank_annotation(json.loads(line), ranking)


def most_severe_of(ranked, allele):
    """``get_most_severe_consequence(allele)`` over :func:`vep_line`'s result."""
    for key in TYPE_KEYS:
        conseqs = ranked.get(key)
        if conseqs is not None and allele in conseqs:
            return conseqs[allele][0]
    return None


def alleles_of(ranked) -> List[str]:
    """The alleles of a ranked line, in first-appearance order over the types."""
    out = []
    for key in TYPE_KEYS:
        for va in ranked.get(key) or ():
            if va not in out:
                out.append(va)
    return out


_CSQ_ARRAYS = ("type", "order", "el_start", "el_len", "al_start", "al_len", "mask", "entry", "coding", "sorted", "head")
_LINE_ARRAYS = ("n_csq", "flags", "types", "input_start", "input_len", "id_start", "id_len", "csq_off")


class VepConsequences:
    """A slab's consequences.  Per line (``n_lines`` entries): ``n_csq``, ``flags`` (0: the device
    answered the line; else 1 + the number of the reason it is the host's, ``N.VEP_REASONS``),
    ``types`` (bit t: the line has the key of type t), the spans ``input_start/_len`` and
    ``id_start/_len`` of the top-level strings (length -1: none) and ``csq_off``.  Per consequence,
    at ``csq_off[line] + k`` in text order: ``type`` (0..3), ``order`` (vep_consequence_order_num),
    the element's span ``el_start/el_len``, its allele's ``al_start/al_len``, its term ``mask``, its
    ranking ``entry`` and ``coding``; ``sorted[csq_off[line] + p]`` is the k of the consequence at
    place p of the reference's order and ``head[csq_off[line] + p]`` is 1 where a (type, allele)
    list begins.  ``counts``: ``N.VEP_COUNTS``."""

    def __init__(self, engine, text, ranking, n_lines, counts, line_arrays, csq_arrays):
        self.engine, self.text, self.ranking, self.n_lines, self.counts = engine, text, ranking, n_lines, counts
        for name, a in zip(_LINE_ARRAYS, line_arrays):
            setattr(self, name, a[:n_lines])
        n = counts["consequences"]
        for name, a in zip(_CSQ_ARRAYS, csq_arrays):
            setattr(self, name, a[:n])
        self._np = None

    def _host(self):
        if self._np is None:
            self._np = {name: getattr(self, name).cpu().numpy() for name in _LINE_ARRAYS + _CSQ_ARRAYS}
            self._np["text"] = self.text.cpu().numpy()
            nl = np.flatnonzero(self._np["text"] == 10)
            self._np["line_start"] = np.concatenate([[0], nl + 1])[:max(self.n_lines, 1)]
            self._np["line_end"] = np.concatenate([nl, [self.text.numel()]])[:max(self.n_lines, 1)]
        return self._np

    def _span(self, start, length) -> bytes:
        return self._host()["text"][int(start):int(start) + int(length)].tobytes()

    def line(self, i: int) -> bytes:
        h = self._host()
        return self._span(h["line_start"][i], h["line_end"][i] - h["line_start"][i])

    def line_id(self, i: int) -> Optional[str]:
        """The line's top-level ``id`` (a host line's through ``json``)."""
        h = self._host()
        if h["flags"][i]:
            try:
                v = json.loads(self.line(i)).get("id")
            except (ValueError, AttributeError):
                return None
            return v if isinstance(v, str) else None
        if h["id_len"][i] < 0:
            return None
        return json.loads(b'"' + self._span(h["id_start"][i], h["id_len"][i]) + b'"')

    def ranked(self, i: int):
        """Line i as the reference leaves its four keys: ``{"<type>_consequences": {allele:
        [consequence, ...]}}``, each consequence ``json.loads`` of its element plus
        ``vep_consequence_order_num``, ``rank`` and ``consequence_is_coding``.  A line the device
        left to the host goes through :func:`vep_line` (and raises what it raises)."""
        h = self._host()
        if h["flags"][i]:
            return vep_line(self.line(i), self.ranking)
        out = {TYPE_KEYS[t]: {} for t in range(4) if (h["types"][i] >> t) & 1}
        off, lst = int(h["csq_off"][i]), None
        for p in range(int(h["n_csq"][i])):
            r = off + int(h["sorted"][off + p])
            conseq = json.loads(self._span(h["el_start"][r], h["el_len"][r]))
            conseq["vep_consequence_order_num"] = int(h["order"][r])
            conseq["rank"] = self.ranking.ranks[int(h["entry"][r])]
            conseq["consequence_is_coding"] = bool(h["coding"][r])
            if h["head"][off + p]:
                lst = out[TYPE_KEYS[int(h["type"][r])]][self._span(h["al_start"][r], h["al_len"][r]).decode("ascii")] = []
            lst.append(conseq)
        return out

    def most_severe(self, i: int, allele: str):
        """``get_most_severe_consequence(allele)`` for line i, or ``None``."""
        return most_severe_of(self.ranked(i), allele)

    def summary(self):
        """``(rows, unranked)``: per line and allele ``(id, allele, type, rank, coding, terms)`` of
        its most severe consequence; per line that needs a re-rank ``(line number, id, combination)``."""
        h = self._host()
        rows, unranked = [], []
        for i in range(self.n_lines):
            vid = self.line_id(i) or ""
            if h["flags"][i]:
                try:
                    ranked = vep_line(self.line(i), self.ranking)
                except UnrankedCombination as err:
                    unranked.append((i + 1, vid, err.combination))
                    continue
                except Exception as err:
                    err.line = i + 1
                    if hasattr(err, "add_note"):
                        err.add_note(f"line {i + 1} of the VEP output")
                    raise
                for va in alleles_of(ranked):
                    c = most_severe_of(ranked, va)
                    key = next(k for k in TYPE_KEYS if va in (ranked.get(k) or ()))
                    rows.append((vid, va, key[:-len("_consequences")], c["rank"], c["consequence_is_coding"],
                                 ",".join(c["consequence_terms"])))
                continue
            off, done = int(h["csq_off"][i]), set()
            for p in np.flatnonzero(h["head"][off:off + int(h["n_csq"][i])]):
                r = off + int(h["sorted"][off + p])
                va = self._span(h["al_start"][r], h["al_len"][r]).decode("ascii")
                if va in done:
                    continue
                done.add(va)
                terms = json.loads(self._span(h["el_start"][r], h["el_len"][r]))["consequence_terms"]
                rows.append((vid, va, CONSEQUENCE_TYPES[int(h["type"][r])], self.ranking.ranks[int(h["entry"][r])],
                             bool(h["coding"][r]), ",".join(terms)))
        return rows, unranked

    def summary_text(self) -> str:
        """``id<TAB>allele<TAB>type<TAB>rank<TAB>true|false<TAB>terms`` per line and allele."""
        rows, _ = self.summary()
        return "".join("\t".join((vid, va, t, "" if rank is None else str(rank), "true" if coding else "false", terms))
                       + "\n" for vid, va, t, rank, coding, terms in rows)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="the most severe ADSP-ranked consequence per line and allele of VEP JSON")
    ap.add_argument("--fileName", required=True, help="VEP --json output (plain, gzip or bgzip)")
    ap.add_argument("--rankingFile", required=True, help="consequence<TAB>rank, or consequences in rank order")
    ap.add_argument("--out", required=True, help="summary TSV; lines that need a re-rank go to <out>.unranked")
    ap.add_argument("--device", default=None, help="GPU index, or 'host'")
    args = ap.parse_args(argv)
    from .engine import Engine
    eng = Engine(args.device if args.device in (None, "host") else int(args.device))
    res = eng.vep_consequences(args.fileName, args.rankingFile)  # (the path: run as __main__, this module is not the package's)
    rows, unranked = res.summary()
    with open(args.out, "w") as fh:
        for vid, va, t, rank, coding, terms in rows:
            print(vid, va, t, "" if rank is None else rank, "true" if coding else "false", terms, sep="\t", file=fh)
    with open(args.out + ".unranked", "w") as fh:
        for line, vid, comb in unranked:
            print(line, vid, comb, sep="\t", file=fh)
    print(f"{res.n_lines} lines, {res.counts['host_lines']} on the host, {len(rows)} rows, {len(unranked)} unranked",
          file=sys.stderr)
    return 2 if unranked else 0


if __name__ == "__main__":
    sys.exit(main())

"""Split a whole-genome VCF by chromosome — the counterpart of ``Util/bin/split_vcf_by_chr.py``.

The reference reads one ``.vcf.gz`` (dbSNP ships such a file, with RefSeq accessions as
CHROM) line by line on one host thread and prints every data line to one of 25 open files,
``chr1.vcf`` ... ``chrM.vcf`` (``run``, ``:29-52``).  Here the file is streamed in slabs cut
at newlines and each slab's lines are partitioned on the GPU (K15, ``Engine.split_vcf``);
the slab's 25 streams are appended to the files.

    python -m annotatedvdb_amd.split_vcf_by_chr -f GCF_000001405.40.gz -c chrmap.tsv -o out

``-f/--fileName``, ``-o/--outputDir`` and ``-c/--chromosomeMap`` are the reference's.
``--batchBytes`` bounds a slab.  A bgzip file is inflated on the GPU (K11,
``BgzfFile.iter_text``); a plain or gzip file is read through ``bgzf.open_text``.  A line
no file takes ends the run with the reference's ``KeyError`` before its slab is written;
with ``--unplaced FILE`` such lines (the NT_/NW_ scaffolds of a dbSNP file) are appended
to FILE instead and the run goes on.

Not reproduced: the reference's "New Sequence Found" and "Processed N lines" warnings are
not written.
"""

from __future__ import annotations

import argparse
import os
from typing import Dict, Iterator, Optional, Sequence

from .chromosomes import CHROM_NAMES

BATCH_BYTES = 256 << 20  # load_vcf_file's default


def parse_args(argv: Optional[Sequence[str]] = None):
    ap = argparse.ArgumentParser(allow_abbrev=False, description="split a VCF file by chromosome, on one GPU")
    ap.add_argument("-f", "--fileName", required=True, help="full path to input file (plain, gzip or bgzip)")
    ap.add_argument("-o", "--outputDir", required=True, help="output directory, will create if doesn't exist")
    ap.add_argument("-c", "--chromosomeMap", help="full path to chromosome map file")
    ap.add_argument("--batchBytes", type=int, default=BATCH_BYTES, help="text bytes per slab")
    ap.add_argument("--unplaced", metavar="FILE", help="append the lines no chromosome file takes to FILE "
                    "instead of raising KeyError")
    args = ap.parse_args(argv)
    if args.batchBytes < 1:
        ap.error("--batchBytes must be at least 1")
    return args


def iter_slabs(path: str, batch_bytes: int, engine) -> Iterator:
    """The file's text in slabs cut after a newline (the last may lack it): device tensors
    for a bgzip file, ``bytes`` otherwise (about ``batch_bytes`` each, the remainder after
    the last newline carried into the next)."""
    from . import bgzf
    if bgzf.is_bgzf(path):
        pieces = bgzf.BgzfFile(path, engine).iter_text(max(1, batch_bytes // 4))
        try:
            first = next(pieces, None)
        except bgzf.NotBgzf:
            pieces = None
        if pieces is not None:
            if first is not None:
                yield first
            yield from pieces
            return
    with bgzf.open_text(path) as fh:
        carry = b""
        while True:
            block = fh.read(batch_bytes)
            if not block:
                break
            buf = carry + block
            k = buf.rfind(b"\n")
            if k < 0:
                carry = buf
                continue
            carry = buf[k + 1:]
            yield buf[:k + 1]
        if carry:
            yield carry


def main(argv: Optional[Sequence[str]] = None, engine=None) -> Dict[str, int]:
    """Runs the split; returns ``{label: lines}`` for the 25 files."""
    args = parse_args(argv)
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    chrom_map = None
    if args.chromosomeMap:
        from .parsers import ChromosomeMap
        chrom_map = engine.split_chrom_map(ChromosomeMap(args.chromosomeMap).chromosome_map())
    os.makedirs(args.outputDir, exist_ok=True)
    from .engine import SplitVcf
    # the 25 files with their header line, before any line is read (create_fh_dict)
    SplitVcf(engine._as_text(b""), [0] * 27, {}, None).append_files(args.outputDir, True)
    lines = {label: 0 for label in CHROM_NAMES}
    seen = 0  # the file's lines before this slab
    if args.unplaced:
        open(args.unplaced, "wb").close()
    for slab in iter_slabs(args.fileName, args.batchBytes, engine):
        try:
            out = engine.split_vcf(slab, chrom_map, unknown="keep" if args.unplaced else "raise")
        except KeyError as err:
            if getattr(err, "line", None) is not None:
                err.line += seen
            raise
        out.append_files(args.outputDir, False)
        if args.unplaced:
            with open(args.unplaced, "ab") as fh:
                fh.write(out.other_text.cpu().numpy().tobytes())
        for c, label in enumerate(CHROM_NAMES):
            lines[label] += out.counts["lines"][c]
        seen += sum(out.counts["lines"]) + out.counts["comments"]
    return lines


if __name__ == "__main__":
    main()

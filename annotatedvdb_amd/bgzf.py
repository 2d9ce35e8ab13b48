"""BGZF (bgzip) input through K11: the files the reference loads (dbSNP and ADSP
``.vcf.gz``, CADD's ``whole_genome_SNVs.tsv.gz``) are chains of independent gzip
members of at most 64 KiB of text each (SAM specification §4.1).  The host walks
the member headers (``avdb_bgzf_index_host``), the compressed bytes go to the
device, and ``k_bgzf_inflate`` inflates one member per wave, so the text first
exists in HBM — where K0 (``Engine.vcf_tokenize``) and K10a
(``Engine.cadd_table_build``) read it.

A plain single-member gzip file is not BGZF: :func:`is_bgzf` tells them apart from
the first 18 bytes, and the callers keep such a file on Python's ``gzip``.  Tabix
indexes and virtual offsets are not read; BGZF is not written.
"""

from __future__ import annotations

import gzip
from dataclasses import dataclass
from typing import Iterator, Optional

import numpy as np
import torch

from . import _native as N


class BgzfError(OSError):
    """A BGZF member K11 refuses (``gzip.open`` raises ``OSError`` for the same files)."""

    block: Optional[int] = None
    offset: Optional[int] = None
    status: Optional[int] = None

    @classmethod
    def for_block(cls, block: int, offset: int, status: int, failed: int = 1) -> "BgzfError":
        name = N.BGZF_STATUS[status] if 0 <= status < len(N.BGZF_STATUS) else "status %d" % status
        err = cls("BGZF block %d (file offset %d): %s (AVDB_BGZF status %d; %d block(s) failed)"
                  % (block, offset, name, status, failed))
        err.block, err.offset, err.status = block, offset, status
        return err


class NotBgzf(BgzfError):
    """The first member is gzip, but not BGZF (``AVDB_ENOTBGZF``): read it with ``gzip``."""


@dataclass
class BgzfIndex:
    """The members at the head of a buffer: ``in_off[k]`` the offset of member k,
    ``out_off`` (``n_blocks + 1`` entries) the exclusive sum of their ISIZE,
    ``consumed`` the offset after the last complete member, ``out_bytes`` their text."""
    in_off: np.ndarray
    out_off: np.ndarray
    consumed: int
    out_bytes: int

    @property
    def n_blocks(self) -> int:
        return int(self.in_off.size)


def is_bgzf(path: str) -> bool:
    """The file starts like a BGZF member (its first 18 bytes: gzip magic, CM 8, FLG 4,
    and 'BC' with length 2 as the first extra subfield, as bgzip writes it)."""
    with open(path, "rb") as fh:
        h = fh.read(18)
    return len(h) == 18 and h[:4] == b"\x1f\x8b\x08\x04" and h[12:16] == b"BC\x02\x00" and \
        int.from_bytes(h[10:12], "little") >= 6


def open_text(path: str):
    """``path`` opened for reading bytes: through ``gzip`` when it starts with the gzip magic, else as it is."""
    with open(path, "rb") as fh:
        magic = fh.read(2)
    return (gzip.open if magic == b"\x1f\x8b" else open)(path, "rb")


def read_whole(path: str, engine):
    """A plain, gzip or bgzip file's text: a ``uint8`` tensor on ``engine``'s device for
    bgzip (K11 inflates it there, the text never visits the host), else ``bytes``."""
    if is_bgzf(path):
        try:
            return BgzfFile(path, engine).read()
        except NotBgzf:
            pass
    with open_text(path) as fh:
        return fh.read()


def _last_newline(t: torch.Tensor) -> int:
    """Index of the last '\\n' of a ``uint8`` tensor, or -1 (looked for from the end, 1 MiB at a time)."""
    hi = t.numel()
    while hi > 0:
        lo = max(0, hi - (1 << 20))
        hit = torch.nonzero(t[lo:hi] == 10)
        if hit.numel():
            return lo + int(hit[-1])
        hi = lo
    return -1


class BgzfFile(object):
    """A BGZF file read through K11 on ``engine`` (default: the process-wide engine)."""

    def __init__(self, path: str, engine=None):
        if engine is None:
            from .engine import default_engine
            engine = default_engine()
        self.path, self._engine = path, engine

    def read(self) -> torch.Tensor:
        """The whole file's text as a ``uint8`` tensor on the engine's device."""
        data = np.fromfile(self.path, dtype=np.uint8)
        return self._engine.bgzf_inflate(data)

    def iter_text(self, batch_bytes: int) -> Iterator[torch.Tensor]:
        """The text in pieces cut after a newline (the last one may lack it), as
        ``uint8`` tensors on the engine's device.  The compressed file is read
        ``batch_bytes`` at a time, so host memory is bounded by the batch and device
        memory by its text; a member cut by the read and the line cut by the last
        member are carried into the next piece."""
        eng = self._engine
        tail = b""
        carry: Optional[torch.Tensor] = None
        at = 0  # file offset of tail[0]
        with open(self.path, "rb") as fh:
            while True:
                block = fh.read(max(1, int(batch_bytes)))
                if not block:
                    break
                buf = np.frombuffer(tail + block, dtype=np.uint8)
                try:
                    index = eng.bgzf_index(buf)
                except NotBgzf as err:
                    if at == 0:
                        raise
                    raise BgzfError("no BGZF member at file offset %d" % at) from err
                except BgzfError as err:
                    raise BgzfError("%s; that chain starts at file offset %d" % (err, at)) from err
                tail = buf[index.consumed:].tobytes()
                if index.n_blocks == 0:
                    continue
                try:
                    text = eng.bgzf_inflate(buf[:index.consumed], index)
                except BgzfError as err:
                    if err.block is None:
                        raise
                    raise BgzfError("%s; offsets count from file offset %d" % (err, at)) from err
                at += index.consumed
                if carry is not None:
                    text = torch.cat([carry, text])
                    carry = None
                k = _last_newline(text)
                if k < 0:
                    carry = text
                    continue
                if k + 1 < text.numel():
                    carry = text[k + 1:].clone()
                yield text[:k + 1]
        if tail:
            raise BgzfError("truncated BGZF file: %d bytes after the last complete member (file offset %d)"
                            % (len(tail), at))
        if carry is not None and carry.numel():
            yield carry

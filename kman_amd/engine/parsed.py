"""FASTA / FASTQ text to device codes and the record table (``Parsed``)."""

from __future__ import annotations

import ctypes
import logging
import os
from collections.abc import Sequence as _SequenceABC
from ctypes import byref, c_void_p
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from .. import _native as N
from .. import phases
from . import device
from .device import Device, DeviceBuffer, Scratch


def _title_name(text: bytes, hdr: int) -> bytes:
    """``title = line[1:].rstrip()``; ``name = title.split(" ")[0]``.

    parsers.py:85 and batcher.py:551.  Decoded like the reference's text-mode
    file (UTF-8), so Python's own rstrip/split semantics apply verbatim."""
    i = hdr + 1
    n = len(text)
    j = i
    # universal newlines: the header line ends at \n or \r
    while j < n and text[j] != 0x0A and text[j] != 0x0D:
        j += 1
    title = text[i:j].decode("utf-8", errors="surrogateescape").rstrip()
    return title.split(" ")[0].encode("utf-8", errors="surrogateescape")


@dataclass
class Parsed:
    dev: Device
    codes: DeviceBuffer  # n_bases codes + 64 pad (see include/kman.h)
    n_bases: int
    n_records: int
    rec_hdr: np.ndarray  # u64 byte offset of each '>'
    rec_seq: np.ndarray  # u64 first base index of each record
    names: List[bytes]
    names_blob: bytes
    name_off: np.ndarray  # u64, len n_records + 1
    n_masked: int = 0  # FASTQ with a quality threshold: the kept bytes below it (their codes read as N)
    text: Optional[DeviceBuffer] = None  # the input text on the device (text_bytes + 64), only with keep_text=True
    text_bytes: int = 0
    mates: Optional[tuple] = None  # zip_pairs' result only: the two sources (codes freed, text kept), freed with it
    # hpc(keep_map=True)'s result only: the original index of every kept base (u64, on the device) and the
    # record table and base count of the codes before the compression
    hpc_orig: Optional[DeviceBuffer] = None
    hpc_rec_seq: Optional[np.ndarray] = None
    hpc_n_bases: int = 0

    def record_of(self, base: int) -> int:
        return int(np.searchsorted(self.rec_seq, base, side="right")) - 1

    def free(self) -> None:
        self.codes.free()
        if self.text is not None:
            self.text.free()
            self.text = None
        if self.mates is not None:
            for m in self.mates:
                m.free()
        if self.hpc_orig is not None:
            self.hpc_orig.free()
            self.hpc_orig = None


FORMATS = ("auto", "fasta", "fastq")
MAX_MIN_QUAL = 93  # '~' at offset 33
PHRED_OFFSETS = (33, 64)


def _qual_byte(min_qual: int, phred_offset: int) -> int:
    """The threshold byte of kman_parse_fastq_q, `phred_offset` + `min_qual`
    (0 for ``min_qual == 0``: no threshold), both checked."""
    if isinstance(min_qual, bool) or not isinstance(min_qual, (int, np.integer)) or not 0 <= min_qual <= MAX_MIN_QUAL:
        raise AssertionError("min_qual must be an integer in 0..%d, got %r" % (MAX_MIN_QUAL, min_qual))
    if isinstance(phred_offset, bool) or phred_offset not in PHRED_OFFSETS:
        raise AssertionError("phred_offset must be 33 or 64, got %r" % (phred_offset,))
    return int(phred_offset) + int(min_qual) if min_qual else 0


def _check_qual_format(qbyte: int, fmt: str) -> None:
    if qbyte and fmt != "fastq":
        raise AssertionError("--min-qual needs fastq input")


def sniff_format(head: bytes) -> str:
    """``"fastq"`` if and only if the first byte of the first non-empty line
    of `head` (the beginning of an input) is ``@``; everything else is
    ``"fasta"``, so every input that parses as FASTA keeps doing so."""
    s = bytes(head).lstrip(b"\r\n")
    return "fastq" if s[:1] == b"@" else "fasta"


def _resolve_format(fmt: str, head) -> str:
    """`fmt` checked; ``auto`` decided from the input's head (`head`: bytes,
    or a callable ``offset -> bytes`` that reads the input piecewise)."""
    if fmt not in FORMATS:
        raise AssertionError("format must be one of %s, got %r" % (", ".join(FORMATS), fmt))
    if fmt != "auto":
        return fmt
    if not callable(head):
        return sniff_format(head)
    at = 0
    while True:  # (more than one piece only when the input starts with 64 KiB of blank lines)
        piece = head(at)
        if not piece or piece.strip(b"\r\n"):
            return sniff_format(piece)
        at += len(piece)


def sniff_file(path: str) -> str:
    """sniff_format of a file's head (a ``.gz`` is inflated only that far)."""
    if path.endswith(".gz"):
        import gzip

        with gzip.open(path, "rb") as fh:
            return _resolve_format("auto", lambda at: fh.read(1 << 16))
    with open(path, "rb") as fh:
        return _resolve_format("auto", lambda at: fh.read(1 << 16))


class BlobNames(_SequenceABC):
    """The record names as a read-only sequence over ``names_blob`` /
    ``name_off`` (no per-record objects until one is asked for)."""

    def __init__(self, blob: bytes, off: np.ndarray):
        self._blob, self._off = blob, off

    def __len__(self) -> int:
        return len(self._off) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        return self._blob[int(self._off[i]):int(self._off[i + 1])]

    def __iter__(self):
        b, o = self._blob, self._off.tolist()
        return (b[o[i]:o[i + 1]] for i in range(len(o) - 1))

    def __eq__(self, other):
        try:
            return len(self) == len(other) and all(a == b for a, b in zip(self, other))
        except TypeError:
            return NotImplemented

    __hash__ = None

    def __repr__(self) -> str:
        return "BlobNames(%d names)" % len(self)


_NAME_ROWS = 1 << 16  # header lines gathered per numpy block


def fastq_names(text, rec_hdr: np.ndarray) -> Tuple[bytes, np.ndarray]:
    """``(names_blob, name_off)`` of the records whose ``@`` sit at `rec_hdr`
    in `text`: ``_title_name`` of every header line, computed with numpy over
    blocks of header lines.  A line of plain ASCII without the whitespace that
    ``str.rstrip`` treats unlike ``" "`` (``\\t \\v \\f \\x1c-\\x1f``) has its
    name end at its first space or at its end; only the other lines go through
    ``_title_name`` itself."""
    R = len(rec_hdr)
    n = len(text)
    t = np.frombuffer(text, dtype=np.uint8)
    lens = np.zeros(R, dtype=np.int64)
    pieces: List[bytes] = []
    try:
        for r0 in range(0, R, _NAME_ROWS):
            start = rec_hdr[r0:r0 + _NAME_ROWS].astype(np.int64) + 1
            m = len(start)
            nlen = np.zeros(m, dtype=np.int64)
            odd = np.zeros(m, dtype=bool)
            todo = np.arange(m)
            base, W = np.zeros(m, dtype=np.int64), 64
            # the window [base, base + W) of every unfinished line, W doubling
            # for the lines that did not end in it
            while len(todo):
                idx = (start[todo] + base[todo])[:, None] + np.arange(W)[None, :]
                past = idx >= n
                c = t[np.minimum(idx, n - 1)]
                stop = (c == 0x0A) | (c == 0x0D) | past
                bad = ((c >= 0x80) | (c == 9) | (c == 11) | (c == 12) | ((c >= 0x1C) & (c <= 0x1F))) & ~stop
                has_stop = stop.any(axis=1)
                first_stop = np.where(has_stop, stop.argmax(axis=1), W)
                inline = np.arange(W)[None, :] < first_stop[:, None]
                odd[todo] |= (bad & inline).any(axis=1)
                space = (c == 0x20) & inline
                has_sp = space.any(axis=1)
                first_sp = np.where(has_sp, space.argmax(axis=1), W)
                # name bytes in this window: up to the first space / the line's end
                grow = nlen[todo] == base[todo]  # (no space met in the earlier windows)
                take = np.where(grow, np.minimum(first_sp, first_stop), 0)
                nlen[todo] += take
                base[todo] += W
                todo = todo[~has_stop]
                W *= 2
            nlen[odd] = 0
            sel = np.repeat(start, nlen) + (np.arange(int(nlen.sum())) - np.repeat(np.cumsum(nlen) - nlen, nlen))
            blob = t[sel].tobytes()
            if odd.any():
                offs = np.concatenate([[0], np.cumsum(nlen)])
                prev = 0
                for j in np.nonzero(odd)[0].tolist():
                    nm = _title_name(text, int(start[j]) - 1)
                    pieces.append(blob[prev:int(offs[j])])
                    pieces.append(nm)
                    prev = int(offs[j])
                    nlen[j] = len(nm)
                pieces.append(blob[prev:])
            else:
                pieces.append(blob)
            lens[r0:r0 + m] = nlen
    finally:
        del t  # (releases an mmap's buffer)
    name_off = np.zeros(R + 1, dtype=np.uint64)
    if R:
        name_off[1:] = np.cumsum(lens, dtype=np.uint64)
    return b"".join(pieces), name_off


def _parsed_fastq(dev: Device, codes: DeviceBuffer, info, rec_hdr, rec_seq, text, n_masked: int = 0,
                  min_qual: int = 0) -> Parsed:
    blob, name_off = fastq_names(text, rec_hdr)
    if min_qual:
        logging.info("masked %d of %d bases below Q%d" % (n_masked, int(info.n_bases), min_qual))
    return Parsed(dev, codes, int(info.n_bases), int(info.n_records), rec_hdr, rec_seq, BlobNames(blob, name_off),
                  blob, name_off, n_masked)


def _call_parse_fastq(dev: Device, d_text, n: int, codes, d_hdr, d_seq, cap: int, info, qbyte: int) -> int:
    """kman_parse_fastq, or kman_parse_fastq_q under a threshold byte; returns n_masked."""
    L = N.lib()
    if not qbyte:
        N.check(dev.ctx, L.kman_parse_fastq(dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr),
                                            c_void_p(d_seq.ptr), cap, byref(info)), "kman_parse_fastq")
        return 0
    masked = ctypes.c_uint64(0)
    N.check(dev.ctx, L.kman_parse_fastq_q(dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr),
                                          c_void_p(d_seq.ptr), cap, byref(info), qbyte, byref(masked)),
            "kman_parse_fastq_q")
    return int(masked.value)


def parse_fastq(dev: Device, text: bytes, min_qual: int = 0, phred_offset: int = 33, *,
                keep_text: bool = False) -> Parsed:
    """Four-line FASTQ bytes -> device codes + record table (kman_parse_fastq):
    the same ``Parsed`` as ``parse`` gives for the FASTA of the same records;
    the names follow the record name rule applied to the ``@`` line.  With
    `min_qual` > 0 (0..93) every base whose quality byte is below
    `phred_offset` (33 or 64) + `min_qual` reads as ``N`` (kman_parse_fastq_q);
    ``Parsed.n_masked`` counts them.  `keep_text`: the device copy of the text
    is not freed but kept as ``Parsed.text`` (n + 64 more bytes of device
    memory until ``Parsed.free``), for cut_records."""
    qbyte = _qual_byte(min_qual, phred_offset)
    n = len(text)
    if n == 0:
        raise AssertionError("premature end of file or empty file")
    with dev.scratch() as s:
        d_text = s.alloc(n + 64)
        codes = s.alloc(n + 64)
        dev.upload(d_text, text)
        phases.mark("h2d")
        # record capacity: four lines of at least one byte each, but for the last record
        cap = n // 4 + 1
        d_hdr = s.alloc(8 * cap)
        d_seq = s.alloc(8 * cap)
        info = N.ParseInfo()
        n_masked = _call_parse_fastq(dev, d_text, n, codes, d_hdr, d_seq, cap, info, qbyte)
        R = int(info.n_records)
        rec_hdr = dev.download(d_hdr, R, np.uint64)
        rec_seq = dev.download(d_seq, R, np.uint64)
        s.keep(codes)
        if keep_text:
            s.keep(d_text)
    p = _parsed_fastq(dev, codes, info, rec_hdr, rec_seq, text, n_masked, min_qual)
    if keep_text:
        p.text, p.text_bytes = d_text, n
    phases.mark("parse")
    return p


def parse(dev: Device, text: bytes, fmt: str = "auto", min_qual: int = 0, phred_offset: int = 33, *,
          keep_text: bool = False) -> Parsed:
    """FASTA bytes -> device codes + record table (kman_parse_fasta); FASTQ
    bytes (`fmt`, ``auto``: sniff_format) go to parse_fastq, with its quality
    threshold (`min_qual` > 0 needs FASTQ input).  `keep_text`: the device copy
    of the text is not freed but kept as ``Parsed.text`` (n + 64 more bytes of
    device memory until ``Parsed.free``), for cut_records."""
    qbyte = _qual_byte(min_qual, phred_offset)
    fmt = _resolve_format(fmt, lambda at: bytes(text[at:at + (1 << 16)]))
    _check_qual_format(qbyte, fmt)
    if fmt == "fastq":
        return parse_fastq(dev, text, min_qual, phred_offset, keep_text=keep_text)
    n = len(text)
    if n == 0:
        raise AssertionError("premature end of file or empty file")
    L = N.lib()
    with dev.scratch() as s:
        d_text = s.alloc(n + 64)
        codes = s.alloc(n + 64)
        dev.upload(d_text, text)
        phases.mark("h2d")
        # record capacity: one record per 2 bytes at most ('>' + terminator)
        cap = n // 2 + 1
        d_hdr = s.alloc(8 * cap)
        d_seq = s.alloc(8 * cap)
        info = N.ParseInfo()
        rc = L.kman_parse_fasta(dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr),
                                c_void_p(d_seq.ptr), cap, byref(info))
        N.check(dev.ctx, rc, "kman_parse_fasta")
        R = int(info.n_records)
        rec_hdr = dev.download(d_hdr, R, np.uint64)
        rec_seq = dev.download(d_seq, R, np.uint64)
        s.keep(codes)
        if keep_text:
            s.keep(d_text)
    names = [_title_name(text, int(h)) for h in rec_hdr]
    name_off = np.zeros(R + 1, dtype=np.uint64)
    if R:
        name_off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    phases.mark("parse")
    p = Parsed(dev, codes, int(info.n_bases), R, rec_hdr, rec_seq, names, b"".join(names), name_off)
    if keep_text:
        p.text, p.text_bytes = d_text, n
    return p


def parse_file(dev: Device, path: str, fmt: str = "auto", min_qual: int = 0, phred_offset: int = 33, *,
               keep_text: bool = False) -> Parsed:
    """kman_parse_fasta of a FASTA file (batcher.py:480 reads it whole), or
    kman_parse_fastq of a FASTQ file (`fmt`, ``auto``: sniff_format).  A
    plain file is read in _FMT_SLICE chunks straight into two pinned stages,
    each chunk's H2D (on the copy stream) running while the next chunk is
    read, so the text crosses host memory once and no pageable copy is made;
    the record names come from the file's header lines (mmap).  Gzip input
    is inflated into memory and parsed from there (read_input + parse).
    `min_qual`, `phred_offset`: parse_fastq's quality threshold.  `keep_text`:
    the device copy of the (inflated) text is not freed but kept as
    ``Parsed.text`` (n + 64 more bytes of device memory until ``Parsed.free``),
    for cut_records."""
    qbyte = _qual_byte(min_qual, phred_offset)
    if path.endswith(".gz"):
        if qbyte and fmt != "fastq":  # (decided from the head, before the whole file is inflated)
            _check_qual_format(qbyte, sniff_file(path) if fmt == "auto" else _resolve_format(fmt, b""))
        return parse(dev, read_input(path), fmt, min_qual, phred_offset, keep_text=keep_text)
    import mmap

    L = N.lib()
    with open(path, "rb", buffering=0) as fh:
        n = os.fstat(fh.fileno()).st_size
        if n == 0:
            raise AssertionError("premature end of file or empty file")
        fq = _resolve_format(fmt, lambda at: os.pread(fh.fileno(), 1 << 16, at)) == "fastq"
        _check_qual_format(qbyte, "fastq" if fq else "fasta")
        with dev.scratch() as s:
            d_text = s.alloc(n + 64)
            codes = s.alloc(n + 64)
            stages = dev.pinned_stages(device._FMT_SLICE + 16, 2)
            at, i = 0, 0
            while at < n:
                b, m = i % 2, min(device._FMT_SLICE, n - at)
                mv = memoryview((ctypes.c_char * m).from_address(stages[b].value)).cast("B")
                got = 0
                while got < m:
                    r = fh.readinto(mv[got:])
                    if not r:
                        raise OSError("%s: short read at byte %d of %d" % (path, at + got, n))
                    got += r
                # the chunk before this one is out of its stage (and stage b's
                # previous chunk long since): then this chunk's copy is queued
                N.check(dev.ctx, L.kman_copy_sync(dev.ctx), "kman_copy_sync")
                N.check(dev.ctx, L.kman_copy_h2d_async(dev.ctx, c_void_p(d_text.ptr + at), stages[b], m, b),
                        "kman_copy_h2d_async")
                at += m
                i += 1
            N.check(dev.ctx, L.kman_copy_sync(dev.ctx), "kman_copy_sync")
            phases.mark("file_read+h2d")
            cap = n // 4 + 1 if fq else n // 2 + 1
            d_hdr = s.alloc(8 * cap)
            d_seq = s.alloc(8 * cap)
            info = N.ParseInfo()
            n_masked = 0
            if fq:
                n_masked = _call_parse_fastq(dev, d_text, n, codes, d_hdr, d_seq, cap, info, qbyte)
            else:
                N.check(dev.ctx, L.kman_parse_fasta(dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr),
                                                    c_void_p(d_hdr.ptr), c_void_p(d_seq.ptr), cap, byref(info)),
                        "kman_parse_fasta")
            R = int(info.n_records)
            rec_hdr = dev.download(d_hdr, R, np.uint64)
            rec_seq = dev.download(d_seq, R, np.uint64)
            s.keep(codes)
            if keep_text:
                s.keep(d_text)
        mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            if fq:
                with dev.scratch() as s:  # (the names fail on a header that is not UTF-8: nothing is left behind)
                    s.own(codes)
                    if keep_text:
                        s.own(d_text)
                    p = _parsed_fastq(dev, codes, info, rec_hdr, rec_seq, mm, n_masked, min_qual)
                    s.keep(codes), s.keep(d_text)
                if keep_text:
                    p.text, p.text_bytes = d_text, n
                phases.mark("parse")
                return p
            names = [_title_name(mm, int(h)) for h in rec_hdr]
        finally:
            mm.close()
    name_off = np.zeros(R + 1, dtype=np.uint64)
    if R:
        name_off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    phases.mark("parse")
    p = Parsed(dev, codes, int(info.n_bases), R, rec_hdr, rec_seq, names, b"".join(names), name_off)
    if keep_text:
        p.text, p.text_bytes = d_text, n
    return p


def _rec_seq(scope: Scratch, p: Parsed) -> Tuple[DeviceBuffer, np.ndarray]:
    """p's record table (first base of each record, u64) uploaded into a
    buffer of `scope`: (the device buffer, the host array)."""
    rec_seq = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    d_rec = scope.alloc(8 * int(p.n_records))
    scope.dev.upload(d_rec, rec_seq)
    return d_rec, rec_seq


def check_empty_names(p: Parsed, k: int) -> None:
    """The reference re-reads every k-mer header through
    ``SequenceCoords.from_str`` (seq.py:106-127, via batch.py:170-186) whose
    regex needs a non-empty record name: a record with an empty name that
    yields any k-mer raises AssertionError before any output is written."""
    for r in np.nonzero(np.diff(p.name_off) == 0)[0].tolist():  # (the records with an empty name)
        b = int(p.rec_seq[r])
        e = int(p.rec_seq[r + 1]) if r + 1 < p.n_records else p.n_bases
        if e - b < k:
            continue
        st = first_window(p.dev.download(p.codes, e - b, np.uint8, offset=b), k)
        if st >= 0:
            raise AssertionError("incompatible string: :%d-%d:+" % (st, st + k))


def first_window(codes: np.ndarray, k: int) -> int:
    """Start of the first run of k ACGT codes (code & 7 < 4) in one record's
    codes, or -1 (vectorised: run starts and ends of the valid positions)."""
    ok = (np.asarray(codes) & 7) < 4
    if len(ok) < k or not ok.any():
        return -1
    d = np.diff(np.concatenate([[0], ok.view(np.int8), [0]]))
    starts = np.nonzero(d == 1)[0]
    ends = np.nonzero(d == -1)[0]
    long = np.nonzero(ends - starts >= k)[0]
    return int(starts[long[0]]) if len(long) else -1


def read_input(path: str) -> bytes:
    """Bytes of a FASTA file; ``.gz`` is decompressed (batcher.py:480)."""
    if path.endswith(".gz"):
        import gzip

        with gzip.open(path, "rb") as fh:
            text = fh.read()
    else:
        with open(path, "rb") as fh:
            text = fh.read()
    phases.mark("file_read")
    return text

"""Device-side engine: FASTA bytes -> parse -> extract -> sort -> count/uniq.

Thin Python orchestration over the C ABI (``_native``).  All per-base and
per-k-mer arithmetic runs in the gfx950 kernels of libkman.so; Python only
moves handles, sizes and the (small) record-name table.

The mapping to the reference (kmermaid 1.0.0):

=====================  ==========================================  ============================
engine function        reference                                   kernel(s)
=====================  ==========================================  ============================
``parse``              SmartFastaParser.parse, parsers.py:86-128   parse_reduce/scan/emit
``parse_fastq``        (four-line FASTQ; not in the reference)     fq_reduce/scan/emit/validate
``  min_qual > 0``     (quality threshold: low bases read as N)    + fq_qmask
``record names``       record[0].split(" ")[0], batcher.py:551     host (names only)
``extract``            Sequence.yield_kmers, seq.py:285-328        extract_kernel
``sort``               Batch.sorted, batch.py:156-168              onesweep_pass x P
``count``              Crawler.do_batch + join_sequence_count      rle_count_kernel
``uniq``               Crawler.do_batch + join_unique              rle_uniq_kernel
``zip_pairs``          (read pairs; not in the reference)          zip_offsets/zip_copy
``format_*``           join.py:262,284 / seq.py:489-495            host threads (C++)
=====================  ==========================================  ============================
"""

from __future__ import annotations

import ctypes
import logging
import math
import os
from collections.abc import Sequence as _SequenceABC
from ctypes import byref, c_int, c_size_t, c_uint32, c_uint64, c_void_p
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from . import _native as N
from . import phases

MAX_K = 32       # 2-bit keys in one u64 (the region / prefix-split paths)
MAX_K_WIDE = 64  # k <= 64: kman_extract_wide rolls the two words of a key; beyond, kman_extract_words


def host_threads() -> int:
    n = os.cpu_count() or 1
    return max(1, min(n, int(os.environ.get("KMAN_HOST_THREADS", "16"))))


class DeviceBuffer:
    """A device allocation owned by a :class:`Device`."""

    __slots__ = ("dev", "ptr", "nbytes")

    def __init__(self, dev: "Device", nbytes: int):
        self.dev = dev
        p = c_void_p()
        N.check(dev.ctx, N.lib().kman_malloc(dev.ctx, byref(p), max(1, int(nbytes))), "kman_malloc(%d)" % nbytes)
        self.ptr = p.value
        self.nbytes = int(nbytes)

    def free(self) -> None:
        if self.ptr and self.dev is not None and self.dev.ctx:
            N.lib().kman_free(self.dev.ctx, c_void_p(self.ptr))
        self.ptr = None

    def __del__(self):  # pragma: no cover - best effort at teardown
        try:
            self.free()
        except Exception:
            pass

    def offset(self, nbytes: int) -> int:
        return self.ptr + int(nbytes)


class Device:
    """One HIP context (stream, look-back scratch) on one GPU."""

    def __init__(self, device: int = 0):
        L = N.lib()
        ctx = c_void_p()
        rc = L.kman_create(int(device), byref(ctx))
        if rc != N.KMAN_OK:
            raise RuntimeError(
                "kman_create(device=%d) failed (%d): no usable MI355X/HIP device (%d visible)"
                % (device, rc, N.device_count())
            )
        self.ctx = ctx.value
        self.index = device
        self._fmt = None  # (cap, pinned stages) of the pipelined writer and the file loader
        phases.mark("device_init")

    def pinned_stages(self, cap: int, nb: int):
        """nb pinned host stages of >= cap bytes, kept across calls (a pinned
        allocation of a few hundred MB costs tens of ms: per call it was a
        large part of a bounded write): the pipelined writer's D2H stages and
        the chunked file loader's H2D stages.  Device memory is not held."""
        if self._fmt is not None and self._fmt[0] >= cap and len(self._fmt[1]) >= nb:
            return self._fmt[1]
        self._free_fmt()
        L = N.lib()
        stages = []
        try:
            for _ in range(nb):
                hp = c_void_p()
                N.check(self.ctx, L.kman_host_alloc(self.ctx, byref(hp), cap), "kman_host_alloc")
                stages.append(hp)
        except Exception:
            for hp in stages:
                L.kman_host_free(self.ctx, hp)
            raise
        self._fmt = (cap, stages)
        return stages

    def _free_fmt(self) -> None:
        if self._fmt is not None and self.ctx:
            L = N.lib()
            L.kman_copy_sync(self.ctx)
            for hp in self._fmt[1]:
                L.kman_host_free(self.ctx, hp)
        self._fmt = None

    def close(self) -> None:
        if self.ctx:
            self._free_fmt()
            N.lib().kman_destroy(c_void_p(self.ctx))
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- memory
    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def upload(self, buf: DeviceBuffer, data, offset: int = 0) -> None:
        mv = memoryview(data).cast("B")
        if offset + mv.nbytes > buf.nbytes:
            raise ValueError("upload overflows the device buffer")
        src = (ctypes.c_char * mv.nbytes).from_buffer_copy(mv) if mv.readonly else (ctypes.c_char * mv.nbytes).from_buffer(mv)
        N.check(self.ctx, N.lib().kman_memcpy_h2d(self.ctx, c_void_p(buf.ptr + offset), src, mv.nbytes), "h2d")

    def download(self, buf: DeviceBuffer, count: int, dtype, offset: int = 0) -> np.ndarray:
        out = np.empty(int(count), dtype=dtype)
        if out.nbytes:
            N.check(
                self.ctx,
                N.lib().kman_memcpy_d2h(self.ctx, out.ctypes.data_as(c_void_p), c_void_p(buf.ptr + offset), out.nbytes),
                "d2h",
            )
        return out

    def memset(self, buf: DeviceBuffer, value: int, nbytes: int, offset: int = 0) -> None:
        N.check(self.ctx, N.lib().kman_memset(self.ctx, c_void_p(buf.ptr + offset), value, nbytes), "memset")

    def sync(self) -> None:
        N.check(self.ctx, N.lib().kman_sync(self.ctx), "sync")


_DEFAULT: Optional[Device] = None


def default_device() -> Device:
    """Process-wide device (LOCAL_RANK when launched one process per GPU)."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = Device(int(os.environ.get("KMAN_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    return _DEFAULT


# --------------------------------------------------------------------- parse


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
    L = N.lib()
    d_text = dev.alloc(n + 64)
    codes = dev.alloc(n + 64)
    try:
        dev.upload(d_text, text)
        phases.mark("h2d")
        # record capacity: four lines of at least one byte each, but for the last record
        cap = n // 4 + 1
        d_hdr = dev.alloc(8 * cap)
        d_seq = dev.alloc(8 * cap)
        try:
            info = N.ParseInfo()
            n_masked = _call_parse_fastq(dev, d_text, n, codes, d_hdr, d_seq, cap, info, qbyte)
            R = int(info.n_records)
            rec_hdr = dev.download(d_hdr, R, np.uint64)
            rec_seq = dev.download(d_seq, R, np.uint64)
        finally:
            d_hdr.free()
            d_seq.free()
    except BaseException:
        codes.free()
        if keep_text:
            d_text.free()
        raise
    finally:
        if not keep_text:
            d_text.free()
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
    d_text = dev.alloc(n + 64)
    codes = dev.alloc(n + 64)
    try:
        dev.upload(d_text, text)
        phases.mark("h2d")
        # record capacity: one record per 2 bytes at most ('>' + terminator)
        cap = n // 2 + 1
        d_hdr = dev.alloc(8 * cap)
        d_seq = dev.alloc(8 * cap)
        info = N.ParseInfo()
        rc = L.kman_parse_fasta(dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr),
                                c_void_p(d_seq.ptr), cap, byref(info))
        N.check(dev.ctx, rc, "kman_parse_fasta")
        R = int(info.n_records)
        rec_hdr = dev.download(d_hdr, R, np.uint64)
        rec_seq = dev.download(d_seq, R, np.uint64)
        d_hdr.free()
        d_seq.free()
    except BaseException:
        if keep_text:
            d_text.free()
        raise
    finally:
        if not keep_text:
            d_text.free()
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
        d_text = dev.alloc(n + 64)
        codes = dev.alloc(n + 64)
        try:
            stages = dev.pinned_stages(_FMT_SLICE + 16, 2)
            at, i = 0, 0
            while at < n:
                b, m = i % 2, min(_FMT_SLICE, n - at)
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
            d_hdr = dev.alloc(8 * cap)
            d_seq = dev.alloc(8 * cap)
            try:
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
            finally:
                d_hdr.free()
                d_seq.free()
        except BaseException:
            codes.free()
            if keep_text:
                d_text.free()
            raise
        finally:
            if not keep_text:
                d_text.free()
        mm = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        try:
            if fq:
                try:
                    p = _parsed_fastq(dev, codes, info, rec_hdr, rec_seq, mm, n_masked, min_qual)
                except BaseException:
                    codes.free()
                    if keep_text:
                        d_text.free()
                    raise
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


# ------------------------------------------------------------------- extract


@dataclass
class Kmers:
    """k-mer keys (+ pos payload) in the reference's stream order."""

    keys: DeviceBuffer
    alt: DeviceBuffer
    pos: Optional[DeviceBuffer]
    pos_alt: Optional[DeviceBuffer]
    pos_bytes: int
    n: int
    k: int
    hist: DeviceBuffer
    sorted: bool = False
    # histogram plan of kman_extract: bits [lo_bit, 2k) (kman_split_bits);
    # hist_valid False = no usable histogram (sort computes its own)
    lo_bit: int = 0
    hist_valid: bool = False
    prefix_sorted: bool = False  # keys stably sorted by bits [lo_bit, 2k) (kman_extract_sorted)

    def free(self) -> None:
        for b in (self.keys, self.alt, self.pos, self.pos_alt, self.hist):
            if b is not None:
                b.free()


def flags_for(rc: bool, want_pos: bool, canonical: bool = False, mixed: bool = False) -> int:
    """kman_extract flags; mixed (with canonical): the keys through the
    bijection of KMAN_MIXED -- spectra only, the keys are not printed."""
    return ((N.KMAN_RC if rc else 0) | (N.KMAN_WANT_POS if want_pos else 0) | (N.KMAN_CANONICAL if canonical else 0)
            | (N.KMAN_MIXED if canonical and mixed else 0))


def count_kmers(p: Parsed, k: int, rc: bool, canonical: bool = False) -> int:
    _check_k(k, wide=True)
    out = c_uint64(0)
    if k > MAX_K_WIDE:
        N.check(p.dev.ctx, N.lib().kman_extract_words(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                      flags_for(rc, False, canonical), None, 0, None, 0, 0,
                                                      byref(out)), "kman_extract_words")
        return int(out.value)
    if k > MAX_K:
        N.check(p.dev.ctx, N.lib().kman_extract_wide(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                     flags_for(rc, False, canonical), None, None, None, 0, 0,
                                                     byref(out)), "kman_extract_wide")
        return int(out.value)
    N.check(p.dev.ctx, N.lib().kman_count_kmers(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                 flags_for(rc, False, canonical), byref(out)), "kman_count_kmers")
    return int(out.value)


def _check_k(k: int, wide: bool = False) -> None:
    """batcher.py:477-478 (k <= 1 raises AssertionError); a path that packs a
    k-mer in one 64-bit key (region / prefix-split / multi-GPU) takes
    k <= 32, the word-key path (wide) every k."""
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    if not wide and k > MAX_K:
        raise NotImplementedError("k=%d: this path packs k-mers in one 64-bit key (k <= %d); the word-key path "
                                  "takes larger k" % (k, MAX_K))


def extract(p: Parsed, k: int, rc: bool, want_pos: bool, canonical: bool = False) -> Kmers:
    """kman_extract: keys (+ pos) in stream order, plus the radix histograms."""
    _check_k(k)
    dev = p.dev
    L = N.lib()
    bound = p.n_bases * (2 if rc and not canonical else 1)
    n = max(bound, 1)
    pos_bytes = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
    keys = dev.alloc(8 * n)
    alt = dev.alloc(8 * n)
    pos = dev.alloc(pos_bytes * n) if want_pos else None
    pos_alt = dev.alloc(pos_bytes * n) if want_pos else None
    hist = dev.alloc(8 * 256 * 8)
    dev.memset(hist, 0, 8 * 256 * 8)
    out = c_uint64(0)
    lo = split_bits(bound, 2 * k)
    rc_ = L.kman_extract(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                         flags_for(rc, want_pos, canonical) | N.KMAN_HIST_LO(lo),
                         c_void_p(keys.ptr), c_void_p(pos.ptr if pos else None), pos_bytes, bound,
                         c_void_p(hist.ptr), byref(out))
    N.check(dev.ctx, rc_, "kman_extract")
    return Kmers(keys, alt, pos, pos_alt, pos_bytes if want_pos else 0, int(out.value), k, hist, lo_bit=lo,
                 hist_valid=True)


def extract_sorted(p: Parsed, k: int, rc: bool, want_pos: bool, canonical: bool = False) -> Kmers:
    """kman_extract_sorted: the k-mers already stably sorted by their prefix
    bits [lo, 2k) (first prefix pass fused into the extraction)."""
    _check_k(k)
    dev = p.dev
    L = N.lib()
    bound = p.n_bases * (2 if rc and not canonical else 1)
    n = max(bound, 1)
    pos_bytes = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
    keys, alt = dev.alloc(8 * n), dev.alloc(8 * n)
    pos = dev.alloc(pos_bytes * n) if want_pos else None
    pos_alt = dev.alloc(pos_bytes * n) if want_pos else None
    lo = split_bits(bound, 2 * k)
    out, res = c_uint64(0), c_int(0)
    N.check(dev.ctx, L.kman_extract_sorted(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                           flags_for(rc, want_pos, canonical), lo,
                                           c_void_p(keys.ptr), c_void_p(alt.ptr),
                                           c_void_p(pos.ptr if pos else None), c_void_p(pos_alt.ptr if pos else None),
                                           pos_bytes, bound, byref(out), byref(res)), "kman_extract_sorted")
    if res.value:
        keys, alt = alt, keys
        pos, pos_alt = pos_alt, pos
    return Kmers(keys, alt, pos, pos_alt, pos_bytes if want_pos else 0, int(out.value), k, dev.alloc(8), lo_bit=lo,
                 prefix_sorted=True)


def split_bits(n: int, key_bits: int) -> int:
    """kman_split_bits: low bit of the prefix the global passes sort by."""
    lo = ctypes.c_uint32(0)
    if N.lib().kman_split_bits(max(int(n), 0), key_bits, byref(lo)) != N.KMAN_OK:
        raise ValueError("bad key_bits %d" % key_bits)
    return int(lo.value)


def _sort_prefix(km: Kmers, dev: Device, key_bits: int) -> None:
    """kman_sort_range over bits [km.lo_bit, key_bits): a stable sort by the
    prefix; km.keys / km.pos then hold the prefix-sorted data."""
    if km.prefix_sorted:
        return
    res = c_int(0)
    hist = c_void_p(km.hist.ptr) if km.hist_valid and km.hist is not None else c_void_p(None)
    rc = N.lib().kman_sort_range(dev.ctx, c_void_p(km.keys.ptr), c_void_p(km.alt.ptr),
                                 c_void_p(km.pos.ptr if km.pos else None),
                                 c_void_p(km.pos_alt.ptr if km.pos_alt else None), km.pos_bytes, km.n, km.lo_bit,
                                 key_bits, hist, byref(res))
    N.check(dev.ctx, rc, "kman_sort_range")
    if res.value:
        km.keys, km.alt = km.alt, km.keys
        km.pos, km.pos_alt = km.pos_alt, km.pos
    km.prefix_sorted = True


def _finish(km: Kmers, dev: Device, key_bits: int, mode: int, okeys=None, ovals=None, ob: int = 0) -> int:
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_finish(dev.ctx, c_void_p(km.keys.ptr), c_void_p(km.alt.ptr),
                                         c_void_p(km.pos.ptr if km.pos else None),
                                         c_void_p(km.pos_alt.ptr if km.pos_alt else None), km.pos_bytes, km.n,
                                         key_bits, km.lo_bit, mode, c_void_p(okeys.ptr if okeys else None),
                                         c_void_p(ovals.ptr if ovals else None), ob, byref(out)), "kman_finish")
    return int(out.value)


def sort(km: Kmers, dev: Device) -> None:
    """Stable sort of km.keys (+ km.pos) by key, Batch.sorted (batch.py:156-168):
    kman_sort_range over the prefix bits, then kman_finish(SORT) in LDS."""
    if km.sorted:
        return
    if km.n > 1:
        _sort_prefix(km, dev, 2 * km.k)
        _finish(km, dev, 2 * km.k, N.KMAN_FINISH_SORT)
    km.sorted = True


@dataclass
class CountResult:
    ukeys: DeviceBuffer
    counts: DeviceBuffer
    count_bytes: int
    n: int
    k: int


def rle_count(km: Kmers, dev: Device) -> CountResult:
    """(key, group size) per distinct key.  Sorted input: kman_rle_count;
    unsorted: the prefix sort + kman_finish(COUNT) (km is consumed)."""
    cb = 4 if km.n <= 0xFFFFFFFF else 8
    ukeys = dev.alloc(8 * max(km.n, 1))
    counts = dev.alloc(cb * max(km.n, 1))
    if not km.sorted:
        _sort_prefix(km, dev, 2 * km.k)
        n = _finish(km, dev, 2 * km.k, N.KMAN_FINISH_COUNT, ukeys, counts, cb)
        return CountResult(ukeys, counts, cb, n, km.k)
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_rle_count(dev.ctx, c_void_p(km.keys.ptr), km.n, c_void_p(ukeys.ptr),
                                             c_void_p(counts.ptr), cb, byref(out)), "kman_rle_count")
    return CountResult(ukeys, counts, cb, int(out.value), km.k)


@dataclass
class UniqResult:
    keys: DeviceBuffer
    pos: DeviceBuffer
    pos_bytes: int
    n: int
    k: int


def rle_uniq(km: Kmers, dev: Device) -> UniqResult:
    if km.pos is None:
        raise ValueError("uniq needs the pos payload (extract with want_pos=True)")
    okeys = dev.alloc(8 * max(km.n, 1))
    opos = dev.alloc(km.pos_bytes * max(km.n, 1))
    if not km.sorted:
        _sort_prefix(km, dev, 2 * km.k)
        n = _finish(km, dev, 2 * km.k, N.KMAN_FINISH_UNIQ, okeys, opos, km.pos_bytes)
        return UniqResult(okeys, opos, km.pos_bytes, n, km.k)
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_rle_uniq(dev.ctx, c_void_p(km.keys.ptr), c_void_p(km.pos.ptr), km.pos_bytes,
                                            km.n, c_void_p(okeys.ptr), c_void_p(opos.ptr), byref(out)),
            "kman_rle_uniq")
    return UniqResult(okeys, opos, km.pos_bytes, int(out.value), km.k)


def groups(p: Parsed, k: int, rc: bool, mode: str, canonical: bool = False, mixed: bool = False):
    """kman_groups: count / uniq of the whole stream straight from the codes
    (region.h).  Returns a CountResult / UniqResult, or None when the input
    is outside the region path (kman_groups_plan / a region overflow said
    KMAN_EFALLBACK): the caller then runs extract_sorted + rle_*."""
    L, dev = N.lib(), p.dev
    m = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
    flags = flags_for(rc, mode == "uniq", canonical, mixed)
    wb = c_uint64(0)
    rc_ = L.kman_groups_plan(p.n_bases, k, flags, m, byref(wb))
    if rc_ == N.KMAN_EFALLBACK:
        return None
    N.check(dev.ctx, rc_, "kman_groups_plan")
    cap = max(1, p.n_bases * (2 if rc and not canonical else 1))
    vb = (4 if 2 * p.n_bases <= 0xFFFFFFFF else 8) if mode == "uniq" else (4 if cap <= 0xFFFFFFFF else 8)
    work = dev.alloc(int(wb.value))
    okeys = dev.alloc(8 * cap)
    ovals = dev.alloc(vb * cap)
    phases.mark("groups_alloc")
    nk, no = c_uint64(0), c_uint64(0)
    try:
        rc_ = L.kman_groups(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, flags, m, c_void_p(work.ptr), wb.value,
                            c_void_p(okeys.ptr), c_void_p(ovals.ptr), vb, byref(nk), byref(no))
    finally:
        work.free()
    phases.mark("groups_kernels")
    if rc_ == N.KMAN_EFALLBACK:
        okeys.free()
        ovals.free()
        return None
    N.check(dev.ctx, rc_, "kman_groups")
    if mode == "uniq":
        return UniqResult(okeys, ovals, vb, int(no.value), k)
    return CountResult(okeys, ovals, vb, int(no.value), k)


def mem_info(dev: Device) -> Tuple[int, int]:
    """(free, total) HBM bytes of the device (kman_mem_info)."""
    f, t = c_size_t(0), c_size_t(0)
    N.check(dev.ctx, N.lib().kman_mem_info(dev.ctx, byref(f), byref(t)), "kman_mem_info")
    return int(f.value), int(t.value)


def _prefix_hist_into(p: Parsed, k: int, rc: bool, h: DeviceBuffer) -> Tuple[np.ndarray, int]:
    n = c_uint64(0)
    N.check(p.dev.ctx, N.lib().kman_kmer_prefix_hist(p.dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                      N.KMAN_RC if rc else 0, c_void_p(h.ptr), byref(n)),
            "kman_kmer_prefix_hist")
    bins = 256 if 2 * k >= 8 else 1 << (2 * k)
    return p.dev.download(h, bins, np.uint64), int(n.value)


def prefix_hist(p: Parsed, k: int, rc: bool) -> Tuple[np.ndarray, int]:
    """Histogram of the top 8 key bits of the stream (kman_kmer_prefix_hist):
    4^k bins when 2k < 8.  Returns (hist, n_kmers)."""
    _check_k(k)
    h = p.dev.alloc(8 * 256)
    try:
        return _prefix_hist_into(p, k, rc, h)
    finally:
        h.free()


def key_ranges(hist: np.ndarray, k: int, max_keys: int, count=None) -> List[Tuple[int, int, int]]:
    """Consecutive top-8-bit prefixes grouped into key ranges of at most
    max_keys k-mers: [(key_lo, key_hi, n)] in key order, empty ranges dropped.
    The batches of a multi-batch join (join.py:63-130) cut by key instead of
    by stream position: their n-way merge is then their concatenation.  A
    prefix holding more than max_keys k-mers (repeats, poly-A) is bisected
    by key with count(lo, hi) -> k-mers in [lo, hi] until its pieces fit;
    only one key value repeated more than max_keys times cannot be cut."""
    shift = max(0, 2 * k - 8)
    out, lo, acc = [], 0, 0

    def split(a, b, c):
        if c <= max_keys:
            return [(a, b, c)] if c else []
        if a == b or count is None:
            raise MemoryError("%d k-mers in key range [%x, %x]: more than a batch of %d" % (c, a, b, max_keys))
        m = (a + b) // 2
        c0 = count(a, m)
        return split(a, m, c0) + split(m + 1, b, c - c0)

    for b, c in enumerate(hist.tolist()):
        if c > max_keys:
            if acc:
                out.append((lo << shift, (b << shift) - 1, acc))
            out.extend(split(b << shift, ((b + 1) << shift) - 1, c))
            lo, acc = b + 1, 0
            continue
        if acc and acc + c > max_keys:
            out.append((lo << shift, (b << shift) - 1, acc))
            lo, acc = b, 0
        acc += c
    if acc:
        out.append((lo << shift, (len(hist) << shift) - 1, acc))
    return out


class _At:
    """A device pointer inside a buffer (an output slice) for _finish."""

    def __init__(self, buf: DeviceBuffer, offset: int):
        self.ptr = buf.ptr + int(offset)


class RangedJoin:
    """Multi-batch device join (BASELINE config 3): count / uniq of a stream
    whose k-mers do not fit the device at once.  The stream is cut into key
    ranges of at most max_keys k-mers (prefix_hist + key_ranges); each range
    is extracted from the resident codes (kman_extract_range, stream order),
    prefix-sorted (kman_sort_range) and finished in LDS (kman_finish), its
    output appended to the global output, which is therefore in key order.
    Same results as groups() / extract_sorted + rle_* (join.py:95-130,
    244-285 over batch.py:156-168).  Every buffer is allocated here, once:
    ``step()`` re-plans (prefix histogram) and runs the batches."""

    def __init__(self, p: Parsed, k: int, rc: bool, mode: str, max_keys: Optional[int] = None):
        _check_k(k)
        self.p, self.k, self.rc, self.mode = p, k, rc, mode
        dev = self.dev = p.dev
        self.want_pos = mode == "uniq"
        self._bufs = []
        self.phist = self._alloc(8 * 256)
        hist, n = _prefix_hist_into(p, k, rc, self.phist)
        self.n_kmers = n
        self.pos_bytes = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
        self.vb = self.pos_bytes if self.want_pos else (4 if n <= 0xFFFFFFFF else 8)
        per_key = 16 + (2 * self.pos_bytes if self.want_pos else 0)
        if max_keys is None:
            free, _ = mem_info(dev)
            max_keys = max(1 << 20, (int(free * 0.85) - (8 + self.vb) * n) // per_key)
        self.max_keys = int(max_keys)
        self.ranges = key_ranges(hist, k, self.max_keys, self._count_range)
        self.cap = max([r[2] for r in self.ranges] + [1])
        self.okeys = self._alloc(8 * max(n, 1))
        self.ovals = self._alloc(self.vb * max(n, 1))
        self.keys, self.alt = self._alloc(8 * self.cap), self._alloc(8 * self.cap)
        self.pos = self._alloc(self.pos_bytes * self.cap) if self.want_pos else None
        self.pos_alt = self._alloc(self.pos_bytes * self.cap) if self.want_pos else None
        self.hbuf = self._alloc(8 * 256 * 8)
        self.n_out = 0

    def _count_range(self, lo: int, hi: int) -> int:
        """k-mers with keys in [lo, hi] (kman_extract_range with no capacity:
        counted, nothing written)."""
        got = c_uint64(0)
        rc = N.lib().kman_extract_range(self.dev.ctx, c_void_p(self.p.codes.ptr), self.p.n_bases, self.k,
                                        flags_for(self.rc, False), lo, hi, None, None, 4, 0, None, byref(got))
        if rc not in (N.KMAN_OK, N.KMAN_ECAP):
            N.check(self.dev.ctx, rc, "kman_extract_range")
        return int(got.value)

    def _alloc(self, nbytes: int) -> DeviceBuffer:
        try:
            b = self.dev.alloc(nbytes)
        except BaseException:
            self.free()
            raise
        self._bufs.append(b)
        return b

    def step(self) -> int:
        """One whole join: plan the key ranges, then extract + sort + finish
        each range into the output.  Returns the number of k-mers joined."""
        dev, L, k, p = self.dev, N.lib(), self.k, self.p
        hist, n = _prefix_hist_into(p, k, self.rc, self.phist)
        ranges = self.ranges
        if n != self.n_kmers:
            raise RuntimeError("the stream changed under a planned RangedJoin")
        flags = flags_for(self.rc, self.want_pos)
        fmode = N.KMAN_FINISH_UNIQ if self.want_pos else N.KMAN_FINISH_COUNT
        shift = max(0, 2 * k - 8)
        vb, pb = self.vb, self.pos_bytes
        total = 0
        for lo_key, hi_key, nr in ranges:
            # the range's keys fill (hi - lo + 1) of the len(hist) prefixes:
            # segment bits as for a stream that dense over the whole key space
            lo = split_bits(nr * (1 << (2 * k)) // (hi_key - lo_key + 1), 2 * k)
            dev.memset(self.hbuf, 0, 8 * 256 * 8)
            got = c_uint64(0)
            N.check(dev.ctx, L.kman_extract_range(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                  flags | N.KMAN_HIST_LO(lo), lo_key, hi_key,
                                                  c_void_p(self.keys.ptr),
                                                  c_void_p(self.pos.ptr if self.pos else None), pb, self.cap,
                                                  c_void_p(self.hbuf.ptr), byref(got)), "kman_extract_range")
            if int(got.value) != nr:
                raise RuntimeError("key range [%x, %x]: %d k-mers extracted, histogram said %d"
                                   % (lo_key, hi_key, got.value, nr))
            km = Kmers(self.keys, self.alt, self.pos, self.pos_alt, pb if self.want_pos else 0, nr, k, self.hbuf,
                       lo_bit=lo, hist_valid=True)
            _sort_prefix(km, dev, 2 * k)
            total += _finish(km, dev, 2 * k, fmode, _At(self.okeys, 8 * total), _At(self.ovals, vb * total), vb)
            self.keys, self.alt, self.pos, self.pos_alt = km.keys, km.alt, km.pos, km.pos_alt
        self.n_out = total
        return n

    def result(self):
        """The output (CountResult / UniqResult); its buffers now belong to
        the caller."""
        r = (UniqResult if self.want_pos else CountResult)(self.okeys, self.ovals, self.vb, self.n_out, self.k)
        self._bufs = [b for b in self._bufs if b is not self.okeys and b is not self.ovals]
        return r

    def free(self) -> None:
        for b in self._bufs:
            b.free()
        self._bufs = []


def ranged_groups(p: Parsed, k: int, rc: bool, mode: str, max_keys: Optional[int] = None):
    """RangedJoin in one call: the CountResult / UniqResult of the stream."""
    j = RangedJoin(p, k, rc, mode, max_keys)
    try:
        j.step()
        return j.result()
    finally:
        j.free()


# ------------------------------------------------------------------ formatting


def _format(fn, *args) -> bytes:
    used = c_size_t(0)
    rc = fn(*args, None, 0, byref(used), host_threads())
    if rc not in (N.KMAN_OK, N.KMAN_ECAP):
        raise RuntimeError("formatter failed (%d)" % rc)
    buf = ctypes.create_string_buffer(max(1, used.value))
    rc = fn(*args, buf, used.value, byref(used), host_threads())
    if rc != N.KMAN_OK:
        raise RuntimeError("formatter failed (%d)" % rc)
    return buf.raw[: used.value]


def format_fasta_words(rows: np.ndarray, pos: np.ndarray, k: int, p: Parsed) -> bytes:
    """The batch-file FASTA (KMer.as_fasta, seq.py:489-495) of word-key rows
    ((n, W) host array) with headers from the record table (host writer
    kman_format_uniq_words)."""
    planes = np.ascontiguousarray(np.asarray(rows, dtype=np.uint64).T)
    n = planes.shape[1] if planes.ndim == 2 else 0
    pos = np.ascontiguousarray(pos, dtype=np.uint64)
    names = ctypes.create_string_buffer(p.names_blob, max(1, len(p.names_blob)))
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    rs = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    return _format(N.lib().kman_format_uniq_words, planes.ctypes.data_as(c_void_p), max(n, 1),
                   pos.ctypes.data_as(c_void_p), 8, n, k, names, off.ctypes.data_as(c_void_p),
                   rs.ctypes.data_as(c_void_p), max(p.n_records, 1))


def format_count(ukeys: np.ndarray, counts: np.ndarray, k: int) -> bytes:
    """``"%s\\t%d\\n" % (seq, count)`` per group (join.py:283-284)."""
    ukeys = np.ascontiguousarray(ukeys, dtype=np.uint64)
    cb = counts.dtype.itemsize
    return _format(N.lib().kman_format_count, ukeys.ctypes.data_as(c_void_p),
                   np.ascontiguousarray(counts).ctypes.data_as(c_void_p), cb, len(ukeys), k)


def format_fasta(keys: np.ndarray, pos: np.ndarray, k: int, p: Parsed) -> bytes:
    """``">%s\\n%s\\n" % (header, seq)`` (join.py:262 / seq.py:495)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    pos = np.ascontiguousarray(pos)
    names = ctypes.create_string_buffer(p.names_blob, max(1, len(p.names_blob)))
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    rs = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    return _format(N.lib().kman_format_uniq, keys.ctypes.data_as(c_void_p), pos.ctypes.data_as(c_void_p),
                   pos.dtype.itemsize, len(keys), k, names, off.ctypes.data_as(c_void_p),
                   rs.ctypes.data_as(c_void_p), p.n_records)


# device-side formatting: the text is built in HBM and only
# the text crosses PCIe; slices of at most _FMT_CHUNK text bytes per launch
_FMT_CHUNK = 1 << 31
_FMT_SLICE = 256 << 20  # text bytes per pipelined slice (_format_dev)
_FMT_THREADS = int(os.environ.get("KMAN_FMT_THREADS", "8"))  # host copy threads
# the format kernels write the pinned stages directly (zero-copy over PCIe)
# instead of a device slice + a copy-engine D2H: the copy engine ran a fresh
# process's first ~2 s at ~31 GB/s (8.2 ms per 256 MiB slice, then 4.2 once
# warm), the kernels' own writes reach ~54 GB/s from the first slice
# (tools/fmtcold.py: 49 GB of uniq text 1.02 s cold vs 1.76; warm 0.92 vs
# 0.88).  KMAN_FMT_ZC=0: the copy-engine pipeline.
_FMT_ZC = os.environ.get("KMAN_FMT_ZC", "1") != "0"


def _pwrite_target(sink):
    """(fd, offset) when the pipelined writer may put slices at computed
    offsets with os.pwrite -- a regular file not opened for appending (pwrite
    on an O_APPEND descriptor ignores the offset on Linux, and a pipe or a
    terminal has no offsets) -- else (None, 0): the slices are then written
    in order by the calling thread through sink.write."""
    import fcntl
    import stat

    try:
        sink.flush()
        fd = sink.fileno()
        if not stat.S_ISREG(os.fstat(fd).st_mode) or fcntl.fcntl(fd, fcntl.F_GETFL) & os.O_APPEND:
            return None, 0
        return fd, sink.tell()
    except (AttributeError, OSError, ValueError):
        return None, 0


def _format_dev(dev: Device, n: int, row_bytes: int, call, sink=None, *, slices=None):
    """Run a kman_format_*_dev call over row slices.  call(i0, rows, d_out,
    cap, used) formats rows [i0, i0 + rows); row_bytes bounds one row.
    Returns the text (a bytearray), or, with a sink (a binary file), writes
    it there and returns None.

    Pipelined over slices of <= _FMT_SLICE text bytes through two pinned
    stages: the format kernel writes slice i straight into stage i % 2 over
    PCIe (_FMT_ZC, the default) while a pool of host threads copies slice
    i - 1 out of the other stage -- pwrite at its file offset, or memmove
    into the result.  (KMAN_FMT_ZC=0: slice i formatted into a device slice
    while slice i - 1 crosses PCIe on the copy stream, kman_copy_d2h_async,
    and slice i - 2 leaves its stage.)

    `slices`: the caller's own (i0, rows, text bound) per slice, in order, for
    rows of very different sizes (cut_records); row_bytes is not used then."""
    if n == 0:
        return None if sink is not None else bytearray()
    import concurrent.futures as cf

    L = N.lib()
    used = c_size_t(0)
    if slices is None:
        rows = max(1, min(n, _FMT_SLICE // max(1, row_bytes)))
        cap = rows * row_bytes + 16
        slices = [(i0, min(rows, n - i0)) for i0 in range(0, n, rows)]
        sizing = [(0, n)]  # one sizing pass over every row
    else:
        cap = max(b for _, _, b in slices) + 16
        slices = sizing = [(i0, m) for i0, m, _ in slices]
    out, fd, base = None, None, 0
    if sink is None:
        size = 0
        for i0, m in sizing:
            rc_ = call(i0, m, None, 0, used)
            if rc_ not in (N.KMAN_OK, N.KMAN_ECAP):
                N.check(dev.ctx, rc_, "kman_format_*_dev")
            size += int(used.value)
        out = bytearray(size)
        dst0 = ctypes.addressof((ctypes.c_char * max(1, len(out))).from_buffer(out)) if len(out) else 0
    else:
        fd, base = _pwrite_target(sink)
    NB = 2
    stages = dev.pinned_stages(max(cap, _FMT_SLICE + 16), NB)
    # (the device text slices live for this call only: held across calls
    # they would hide 2 x 256 MiB from later mem_info-based plans)
    dbufs = [] if _FMT_ZC else [dev.alloc(cap) for _ in range(NB)]
    phases.mark("fmt_buffers")
    pool = cf.ThreadPoolExecutor(max_workers=_FMT_THREADS)
    wpool = cf.ThreadPoolExecutor(max_workers=1)
    try:
        pending = [[] for _ in range(NB)]
        piece = max(1 << 20, cap // _FMT_THREADS + 1)

        def copy_piece(src, at, u):
            if out is not None:
                ctypes.memmove(dst0 + at, src, u)
            else:
                mv = memoryview((ctypes.c_char * u).from_address(src)).cast("B")
                done = 0
                while done < u:
                    done += os.pwrite(fd, mv[done:], base + at + done)

        def drain(b, at, u):
            """slice in stage b (u bytes at text offset `at`) out to the host"""
            N.check(dev.ctx, L.kman_copy_d2h_wait(dev.ctx, b), "kman_copy_d2h_wait")
            if out is None and fd is None:
                sink.write(memoryview((ctypes.c_char * u).from_address(stages[b].value)).cast("B"))
                return
            pending[b] = [pool.submit(copy_piece, stages[b].value + o, at + o, min(piece, u - o))
                          for o in range(0, u, piece)]

        at, last = 0, None
        if _FMT_ZC:
            # zero-copy: the format kernel writes slice i straight into pinned
            # stage b over PCIe (no copy engine); the host drains stage b while
            # slice i + 1 is formatted into the other stage
            for i, (i0, m) in enumerate(slices):
                b = i % NB
                for f in pending[b]:
                    f.result()
                pending[b] = []
                N.check(dev.ctx, call(i0, m, stages[b], cap, used), "kman_format_*_dev")
                u = int(used.value)
                if out is None and fd is None:  # a stream: one writer thread keeps the slices in order
                    mv = memoryview((ctypes.c_char * u).from_address(stages[b].value)).cast("B")
                    pending[b] = [wpool.submit(sink.write, mv)]
                else:
                    pending[b] = [pool.submit(copy_piece, stages[b].value + o, at + o, min(piece, u - o))
                                  for o in range(0, u, piece)]
                if i == 0:
                    phases.mark("fmt_first_slice")
                at += u
            for pb in pending:
                for f in pb:
                    f.result()
        else:
            for i, (i0, m) in enumerate(slices):
                b = i % NB
                for f in pending[b]:  # slice i - 2 out of stage b (its D2H finished before)
                    f.result()
                pending[b] = []
                N.check(dev.ctx, call(i0, m, c_void_p(dbufs[b].ptr), cap, used), "kman_format_*_dev")
                u = int(used.value)
                N.check(dev.ctx, L.kman_copy_d2h_async(dev.ctx, stages[b], c_void_p(dbufs[b].ptr), u, b),
                        "kman_copy_d2h_async")
                if last is not None:
                    drain(*last)
                    if i == 1:
                        phases.mark("fmt_first_slice")
                last = (b, at, u)
                at += u
            if last is not None:
                drain(*last)
            for pb in pending:
                for f in pb:
                    f.result()
    finally:
        pool.shutdown(wait=True)
        wpool.shutdown(wait=True)
        N.check(dev.ctx, L.kman_copy_sync(dev.ctx), "kman_copy_sync")
        for b_ in dbufs:
            b_.free()
    if out is not None:
        assert at == len(out)
        return out
    if fd is not None:
        sink.seek(base + at)
    return None


def format_count_dev(dev: Device, r: CountResult, sink=None):
    """``"%s\t%d\n" % (seq, count)`` per group (join.py:283-284), built on
    the device from the device-resident result (kman_format_count_dev)."""
    L, cb = N.lib(), r.count_bytes

    def call(i0, m, d_out, cap, used):
        return L.kman_format_count_dev(dev.ctx, c_void_p(r.ukeys.ptr + 8 * i0), c_void_p(r.counts.ptr + cb * i0), cb,
                                       m, r.k, d_out, cap, byref(used))

    return _format_dev(dev, r.n, r.k + 2 + (10 if cb == 4 else 20), call, sink)


class DeviceNames:
    """The record table of a Parsed input on the device (names blob, name
    offsets, first base of each record) for kman_format_uniq_dev."""

    def __init__(self, p: Parsed):
        dev = p.dev
        self.names = dev.alloc(max(16, len(p.names_blob)))
        self.off = dev.alloc(8 * (p.n_records + 1))
        self.rec = dev.alloc(8 * max(1, p.n_records))
        if p.names_blob:
            dev.upload(self.names, p.names_blob)
        dev.upload(self.off, np.ascontiguousarray(p.name_off, dtype=np.uint64))
        if p.n_records:
            dev.upload(self.rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        self.n_records = p.n_records
        self.max_name = int(np.diff(p.name_off).max()) if p.n_records else 0
        self.n_bases = p.n_bases

    def free(self) -> None:
        for b in (self.names, self.off, self.rec):
            b.free()


def format_uniq_dev(p: Parsed, r: UniqResult, sink=None):
    """``">%s\n%s\n" % (header, seq)`` (join.py:262 / seq.py:495), built on
    the device (kman_format_uniq_dev)."""
    dev, L, pb = p.dev, N.lib(), r.pos_bytes
    nm = DeviceNames(p)
    try:
        D = len(str(p.n_bases + r.k))

        def call(i0, m, d_out, cap, used):
            return L.kman_format_uniq_dev(dev.ctx, c_void_p(r.keys.ptr + 8 * i0), c_void_p(r.pos.ptr + pb * i0), pb,
                                          m, r.k, c_void_p(nm.names.ptr), c_void_p(nm.off.ptr), c_void_p(nm.rec.ptr),
                                          nm.n_records, d_out, cap, byref(used))

        return _format_dev(dev, r.n, 1 + nm.max_name + 1 + D + 1 + D + 3 + r.k + 1, call, sink)
    finally:
        nm.free()


def host_format() -> bool:
    """KMAN_HOST_FORMAT=1: format on host threads (kman_format_*) from
    downloaded results instead of on the device."""
    return os.environ.get("KMAN_HOST_FORMAT", "0") not in ("", "0")


def _to(sink, data):
    if sink is None:
        return data
    sink.write(data)
    return None


def emit_count(dev: Device, r: CountResult, sink=None):
    """The count output text of a device-resident result: returned, or
    written to the binary file `sink`."""
    if host_format():
        ukeys, counts = download_count(dev, r)
        return _to(sink, format_count(ukeys, counts, r.k))
    return format_count_dev(dev, r, sink)


def emit_uniq(p: Parsed, r: UniqResult, sink=None):
    """The uniq output text of a device-resident result over one input."""
    if host_format():
        keys, pos = download_uniq(p.dev, r)
        return _to(sink, format_fasta(keys, pos, r.k, p))
    return format_uniq_dev(p, r, sink)


def download_count(dev: Device, r: CountResult):
    ukeys = dev.download(r.ukeys, r.n, np.uint64)
    counts = dev.download(r.counts, r.n, np.uint32 if r.count_bytes == 4 else np.uint64)
    return ukeys, counts


def download_uniq(dev: Device, r: UniqResult):
    keys = dev.download(r.keys, r.n, np.uint64)
    pos = dev.download(r.pos, r.n, np.uint32 if r.pos_bytes == 4 else np.uint64)
    return keys, pos


# ------------------------------------------------------------------ pipelines


_CODE_TABLE = np.full(128, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE_TABLE[ord(_c)] = _i
    _CODE_TABLE[ord(_c.lower())] = _i


def decode_key(key: int, k: int) -> str:
    """2-bit MSB-first key -> upper-case sequence."""
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - j))) & 3] for j in range(k))


def kmers_of_sequence(seq: str, k: int, rc: bool, dev: Optional[Device] = None):
    """Keys + pos payloads of every valid window of one sequence string
    (Sequence.yield_kmers, seq.py:285-328), enumerated by kman_extract."""
    _check_k(k)
    dev = dev or default_device()
    cp = np.frombuffer(seq.encode("utf-32-le"), dtype=np.uint32)
    codes = np.where(cp < 128, _CODE_TABLE[np.minimum(cp, 127)], 4).astype(np.uint8)
    n = len(codes)
    if n < k:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    codes[0] |= 8
    buf = dev.alloc(n + 64)
    try:
        dev.upload(buf, np.concatenate([codes, np.full(64, 4, np.uint8)]))
        p = Parsed(dev, buf, n, 1, np.zeros(1, np.uint64), np.zeros(1, np.uint64), [b""], b"",
                   np.zeros(2, np.uint64))
        km = extract(p, k, rc, want_pos=True)
        try:
            keys = dev.download(km.keys, km.n, np.uint64)
            pos = dev.download(km.pos, km.n, np.uint32 if km.pos_bytes == 4 else np.uint64).astype(np.uint64)
        finally:
            km.free()
    finally:
        buf.free()
    return keys, pos


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


def count_groups(p: Parsed, k: int, rc: bool = False, canonical: bool = False, ordered: bool = True) -> CountResult:
    """(key, count) per distinct k-mer on the device: the region path, else
    the prefix-split path (None only when there are no k-mers).
    ordered=False: the rows may come in any order (a spectrum needs only
    the multiset; the key rounds then skip merging a redone key range).
    k > 32: a WordsResult (word keys, its counts in .vals)."""
    if k > MAX_K:
        return words_groups(p, k, rc, "count", canonical)
    # a spectrum (ordered=False) of canonical keys counts mixed keys
    # (KMAN_MIXED): the same counts, uniform buckets for the region passes
    mixed = canonical and not ordered
    r = groups(p, k, rc, "count", canonical, mixed)
    if r is not None:
        return r
    if p.n_bases:
        from . import dist

        r = dist.local_groups(p, k, rc, "count", canonical, ordered=ordered)
        if r is not None:
            return r
    km = extract_sorted(p, k, rc, want_pos=False, canonical=canonical)
    try:
        if km.n == 0:
            return None
        return rle_count(km, p.dev)
    finally:
        km.free()


def abundance_hist(text: bytes, k: int, canonical: bool = True, nbins: int = 10001,
                   dev: Optional[Device] = None, fmt: str = "auto", min_qual: int = 0,
                   phred_offset: int = 33, hpc: bool = False) -> np.ndarray:
    """k-mer abundance spectrum (BASELINE config 5; SURVEY §8f-1, not in the
    reference): h[c] = distinct (canonical) k-mers seen c times, h[-1] every
    count >= nbins - 1 (kman_count_hist over the count output).  `min_qual`,
    `phred_offset`: parse_fastq's quality threshold; `hpc`: homopolymer-compressed
    k-mers (hpc() right after the parse)."""
    _check_k(k, wide=True)
    _check_qual_format(_qual_byte(min_qual, phred_offset),
                       _resolve_format(fmt, lambda at: bytes(text[at:at + (1 << 16)])))
    dev = dev or default_device()
    p = parse(dev, text, fmt, min_qual, phred_offset)
    if hpc:
        p = _hpc_parsed(p)
    try:
        r = count_groups(p, k, False, canonical, ordered=False)
        d_h = dev.alloc(8 * nbins)
        try:
            if r is None:
                return np.zeros(nbins, np.uint64)
            try:
                cnt, cb = (r.vals, r.val_bytes) if isinstance(r, WordsResult) else (r.counts, r.count_bytes)
                N.check(dev.ctx, N.lib().kman_count_hist(dev.ctx, c_void_p(cnt.ptr), cb, r.n,
                                                         c_void_p(d_h.ptr), nbins), "kman_count_hist")
                return dev.download(d_h, nbins, np.uint64)
            finally:
                free_result(r)
        finally:
            d_h.free()
    finally:
        p.free()


def format_hist(h: np.ndarray) -> bytes:
    """``"%d\t%d\n" % (count, n_kmers)`` for every non-empty bin; the last bin
    reads ``">=N"``."""
    out = []
    last = len(h) - 1
    for c in np.nonzero(h)[0].tolist():
        out.append("%s\t%d\n" % ((">=%d" % c) if c == last else str(c), int(h[c])))
    return "".join(out).encode()


def _fits(p: Parsed, k: int, rc: bool, mode: str) -> bool:
    """Does the single-batch general path (extract_sorted + rle_*) fit the
    free HBM?  If not, the multi-batch join (ranged_groups) takes the input."""
    n = p.n_bases * (2 if rc else 1)
    pb = 4 if 2 * p.n_bases <= 0xFFFFFFFF else 8
    need = n * (16 + 8 + (3 * pb if mode == "uniq" else (4 if n <= 0xFFFFFFFF else 8)))
    return need <= 0.85 * mem_info(p.dev)[0]


def nwords(k: int) -> int:
    """64-bit words per k-mer of the any-k path (words.hip): ceil(k / 32)."""
    return (k + 31) // 32


@dataclass
class Words:
    """k-mer keys of any k as W word planes (words.hip layout: word 0 the
    first k - 32 (W - 1) bases, then 32 bases per word, all MSB-first; word j
    of item i at words[j * stride + i]) + an optional u64 pos payload."""

    words: DeviceBuffer
    pos: Optional[DeviceBuffer]
    n: int
    k: int
    stride: int

    @property
    def W(self) -> int:
        return nwords(self.k)

    def plane(self, j: int) -> int:
        return self.words.ptr + 8 * j * self.stride

    def free(self) -> None:
        for b in (self.words, self.pos):
            if b is not None:
                b.free()


@dataclass
class WordsResult:
    """count / uniq rows of k > 32: keys as W word planes, row j's word q at
    words[q * stride + j] (stride: max(n, 1) of the rows as they were made; a
    filter_counts lowers n and leaves the planes where they are)."""

    words: DeviceBuffer
    vals: DeviceBuffer
    val_bytes: int
    n: int
    k: int
    mode: str
    stride: Optional[int] = None

    def __post_init__(self):
        if self.stride is None:
            self.stride = max(self.n, 1)

    @property
    def W(self) -> int:
        return nwords(self.k)

    def free(self) -> None:
        self.words.free()
        self.vals.free()


def extract_words(p: Parsed, k: int, rc: bool, want_pos: bool, canonical: bool = False) -> Words:
    """Keys (+ u64 pos) of the stream as word planes, in stream order
    (Sequence.yield_kmers, seq.py:285-328): kman_extract_wide's rolled
    LDS-staged kernel for k <= 64 (its (hi, lo) are planes 0 and 1),
    kman_extract_words beyond."""
    _check_k(k, wide=True)
    dev, L = p.dev, N.lib()
    n = count_kmers(p, k, rc, canonical)
    W = nwords(k)
    words = dev.alloc(8 * W * max(n, 1))
    pos = dev.alloc(8 * max(n, 1)) if want_pos else None
    w = Words(words, pos, n, k, max(n, 1))
    if n == 0:
        return w
    got = c_uint64(0)
    try:
        if k <= MAX_K_WIDE:
            N.check(dev.ctx, L.kman_extract_wide(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                 flags_for(rc, want_pos, canonical), c_void_p(w.plane(0)),
                                                 c_void_p(w.plane(1)), c_void_p(pos.ptr) if pos else None, 8, n,
                                                 byref(got)), "kman_extract_wide")
        else:
            N.check(dev.ctx, L.kman_extract_words(dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k,
                                                  flags_for(rc, want_pos, canonical), c_void_p(words.ptr), w.stride,
                                                  c_void_p(pos.ptr) if pos else None, 8, n, byref(got)),
                    "kman_extract_words")
    except BaseException:
        w.free()
        raise
    assert int(got.value) == n
    return w


def sort_words(w: Words, start: int = 0, per_batch: Optional[int] = None, dev: Optional[Device] = None) -> Words:
    """A stably sorted copy of word keys (+ pos): LSD over the planes, last
    word first, each a stable kman_sort of the gathered plane carrying the
    permutation (ties keep stream order, as the reference's Timsort,
    batch.py:156-168); per_batch: items in consecutive chunks of that many
    from stream index `start` sorted chunk by chunk (one Batch each) -- a
    final stable sort by the chunk tag (kman_batch_tags)."""
    dev, L = dev or w.words.dev, N.lib()
    n, W, k = w.n, w.W, w.k
    out = Words(dev.alloc(8 * W * max(n, 1)), dev.alloc(8 * max(n, 1)) if w.pos is not None else None, n, k,
                max(n, 1))
    if n == 0:
        return out
    bufs = [dev.alloc(8 * n) for _ in range(4)]
    try:
        perm, key, alt_k, alt_p = bufs
        N.check(dev.ctx, L.kman_iota_u64(dev.ctx, c_void_p(perm.ptr), n), "iota")
        res = c_int(0)

        def stable(keys_, bits):
            nonlocal perm, alt_k, alt_p
            N.check(dev.ctx, L.kman_sort(dev.ctx, c_void_p(keys_.ptr), c_void_p(alt_k.ptr), c_void_p(perm.ptr),
                                         c_void_p(alt_p.ptr), 8, n, bits, None, byref(res)), "kman_sort")
            if res.value:  # (the sorted copy is in the alternates)
                perm, alt_p = alt_p, perm
                return alt_k, keys_
            return keys_, alt_k

        h = k - 32 * (W - 1)
        for j in reversed(range(W)):
            N.check(dev.ctx, L.kman_gather(dev.ctx, c_void_p(w.plane(j)), c_void_p(perm.ptr), n, c_void_p(key.ptr), 8),
                    "gather")
            key, alt_k = stable(key, 64 if j else 2 * h)
        if per_batch is not None:
            last = (start + n - 1) // per_batch
            N.check(dev.ctx, L.kman_batch_tags(dev.ctx, c_void_p(perm.ptr), n, start, per_batch, c_void_p(key.ptr)),
                    "kman_batch_tags")
            key, alt_k = stable(key, max(1, int(last).bit_length()))
        for j in range(W):
            N.check(dev.ctx, L.kman_gather(dev.ctx, c_void_p(w.plane(j)), c_void_p(perm.ptr), n,
                                           c_void_p(out.plane(j)), 8), "gather")
        if w.pos is not None:
            N.check(dev.ctx, L.kman_gather(dev.ctx, c_void_p(w.pos.ptr), c_void_p(perm.ptr), n, c_void_p(out.pos.ptr),
                                           8), "gather")
    except BaseException:
        out.free()
        raise
    finally:
        for b in bufs:
            b.free()
    return out


def rle_words(w: Words, mode: str) -> WordsResult:
    """Run-length rows of sorted word keys (Crawler.do_batch + the count /
    uniq writers, join.py:95-130, 244-285)."""
    dev, L = w.words.dev, N.lib()
    n, W = w.n, w.W
    uniq = mode == "uniq"
    vb = 8 if uniq else (4 if n <= 0xFFFFFFFF else 8)
    ow = dev.alloc(8 * W * max(n, 1))
    ov = dev.alloc(vb * max(n, 1))
    out = c_uint64(0)
    try:
        N.check(dev.ctx, L.kman_rle_words(dev.ctx, N.KMAN_FINISH_UNIQ if uniq else N.KMAN_FINISH_COUNT,
                                          c_void_p(w.words.ptr), W, w.stride, c_void_p(w.pos.ptr) if uniq else None,
                                          8, n, c_void_p(ow.ptr), max(n, 1), c_void_p(ov.ptr), vb, byref(out)),
                "kman_rle_words")
    except BaseException:
        ow.free()
        ov.free()
        raise
    # (planes keep the input's stride n: row j's word q at ow[q * n + j])
    return WordsResult(ow, ov, vb, int(out.value), w.k, mode, stride=max(n, 1))


def words_groups(p: Parsed, k: int, rc: bool, mode: str, canonical: bool = False) -> Optional[WordsResult]:
    """k > 32 (seq.py:285-328 has no k limit): the keys as word planes
    (extract_words), an LSD sort over the planes (sort_words,
    batch.py:156-168), kman_rle_words (join.py:95-130, 244-285).  None when
    the stream has no k-mers."""
    w = extract_words(p, k, rc, mode == "uniq", canonical)
    try:
        if w.n == 0:
            return None
        sw = sort_words(w)
    finally:
        w.free()
    try:
        return rle_words(sw, mode)
    finally:
        sw.free()


wide_groups = words_groups  # (the word-pair name of round 2: k in 33..64 is W = 2)


def download_words(dev: Device, words: DeviceBuffer, n: int, k: int, stride: Optional[int] = None) -> np.ndarray:
    """Word planes to a host (n, W) uint64 array."""
    W = nwords(k)
    stride = n if stride is None else stride
    flat = dev.download(words, W * stride, np.uint64) if n else np.zeros(0, np.uint64)
    return np.ascontiguousarray(flat.reshape(W, stride)[:, :n].T) if n else np.zeros((0, W), np.uint64)


def decode_words(row, k: int) -> str:
    """The k-mer text of one (W,) word row."""
    W = nwords(k)
    h = k - 32 * (W - 1)
    return "".join(decode_key(int(x), h if j == 0 else 32) for j, x in enumerate(row))


def check_count_range(min_count=1, max_count=None) -> Tuple[int, Optional[int]]:
    """The abundance range of filter_counts, checked: integers >= 1,
    `max_count` None (no upper bound) or >= `min_count`."""
    for name, v in (("min_count", min_count), ("max_count", max_count)):
        if v is None and name == "max_count":
            continue
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise AssertionError("%s must be an integer >= 1, got %r" % (name, v))
    if max_count is not None and min_count > max_count:
        raise AssertionError("min_count %d is greater than max_count %d" % (min_count, max_count))
    return int(min_count), None if max_count is None else int(max_count)


def _count_rows(r):
    """(key planes ptr, W, stride, counts ptr, count bytes) of a count result."""
    if isinstance(r, WordsResult):
        if r.mode != "count":
            raise ValueError("filter_counts takes count rows, not uniq rows")
        return r.words.ptr, r.W, r.stride, r.vals.ptr, r.val_bytes
    if not isinstance(r, CountResult):
        raise ValueError("filter_counts takes a CountResult or a count-mode WordsResult")
    return r.ukeys.ptr, 1, max(r.n, 1), r.counts.ptr, r.count_bytes


def _filter_call(dev: Device, r, lo: int, hi: int, okeys, ocounts) -> int:
    kp, W, stride, cp, cb = _count_rows(r)
    out = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_filter_counts(dev.ctx, c_void_p(kp), W, stride, c_void_p(cp), cb, r.n, lo, hi,
                                                c_void_p(okeys), c_void_p(ocounts), byref(out)), "kman_filter_counts")
    return int(out.value)


_U64_MAX = (1 << 64) - 1


def filter_counts(dev: Device, r, min_count: int = 1, max_count: Optional[int] = None):
    """Keep the rows of a count result (CountResult, or a count-mode
    WordsResult) whose count is in [min_count, max_count], in their order, in
    place on the device (kman_filter_counts): r.n becomes the rows kept, the
    buffers (and a WordsResult's stride) stay.  Returns r.  The identity
    range (min_count <= 1, no max_count) launches nothing."""
    if r is None or (min_count <= 1 and max_count is None):
        return r
    lo, hi = check_count_range(max(1, min_count), max_count)
    kp, _, _, cp, _ = _count_rows(r)
    r.n = _filter_call(dev, r, lo, _U64_MAX if hi is None else hi, kp, cp)
    return r


def filtered_copy(dev: Device, r: CountResult, min_count: int = 1, max_count: Optional[int] = None) -> CountResult:
    """filter_counts out of place: the kept rows of a CountResult in fresh
    buffers sized by a counting call first; r and its buffers are left as
    they are (rows that are read again, such as a pipeline's)."""
    lo, hi = check_count_range(min_count, max_count)
    hi = _U64_MAX if hi is None else hi
    n = _filter_call(dev, r, lo, hi, None, None)
    ok_ = dev.alloc(8 * max(n, 1))
    oc_ = dev.alloc(r.count_bytes * max(n, 1))
    try:
        if n:
            got = _filter_call(dev, r, lo, hi, ok_.ptr, oc_.ptr)
            assert got == n
    except BaseException:
        ok_.free()
        oc_.free()
        raise
    return CountResult(ok_, oc_, r.count_bytes, n, r.k)


# ------------------------------------------------- two count tables (set ops)

MATCH_OPS = {
    "right": N.KMAN_MATCH_RIGHT, "left": N.KMAN_MATCH_LEFT, "min": N.KMAN_MATCH_MIN, "max": N.KMAN_MATCH_MAX,
    "sum": N.KMAN_MATCH_SUM, "absent": N.KMAN_MATCH_ABSENT, "any_sum": N.KMAN_MATCH_ANY_SUM,
    "any_max": N.KMAN_MATCH_ANY_MAX,
}
SET_OPS = {  # op -> the `counts` choices it takes, the default first
    "intersect": ("left", "right", "min", "max", "sum"),
    "subtract": ("left",),
    "union": ("sum", "max"),
}


def check_set_op(op: str, counts: Optional[str] = None) -> str:
    """The `counts` choice of set_op(op), checked (AssertionError); None: the
    op's default."""
    if op not in SET_OPS:
        raise AssertionError("op must be one of %s, got %r" % (", ".join(SET_OPS), op))
    if counts is None:
        return SET_OPS[op][0]
    if counts not in SET_OPS[op]:
        raise AssertionError("--counts %s: --op %s takes %s" % (counts, op, " | ".join(SET_OPS[op])))
    return counts


def empty_count(dev: Device, k: int) -> CountResult:
    """The count table of an input without k-mers: the empty set."""
    return CountResult(dev.alloc(8), dev.alloc(4), 4, 0, k)


def _match_bytes(a: CountResult, b: CountResult) -> int:
    return 8 if 8 in (a.count_bytes, b.count_bytes) else 4


def match_counts(dev: Device, a: CountResult, b: CountResult, op: str = "right") -> DeviceBuffer:
    """kman_match_counts: one value per row of `a` from the row of `b` with
    the same key (MATCH_OPS; include/kman.h), as a fresh device vector of
    a.n values, 4 bytes wide unless either table's counts are 8.  `a` and `b`
    are key-sorted distinct count rows of one k (join_groups(.., "count"))."""
    if op not in MATCH_OPS:
        raise AssertionError("match op must be one of %s, got %r" % (", ".join(MATCH_OPS), op))
    if a.k != b.k:
        raise AssertionError("the two tables hold k-mers of different k: %d and %d" % (a.k, b.k))
    ob = _match_bytes(a, b)
    out = dev.alloc(ob * max(a.n, 1))
    try:
        N.check(dev.ctx, N.lib().kman_match_counts(
            dev.ctx, c_void_p(a.ukeys.ptr), c_void_p(a.counts.ptr), a.count_bytes, a.n, c_void_p(b.ukeys.ptr),
            c_void_p(b.counts.ptr), b.count_bytes, b.n, MATCH_OPS[op], c_void_p(out.ptr), ob), "kman_match_counts")
    except BaseException:
        out.free()
        raise
    return out


def _matched_rows(dev: Device, a: CountResult, b: CountResult, op: str, lo: int = 1,
                  hi: Optional[int] = None) -> CountResult:
    """The rows (key of a, match_counts(a, b, op)) whose value is in [lo, hi],
    in fresh buffers: the match vector, then one out-of-place filter over a's
    keys and that vector (rows whose value is 0 are dropped: lo >= 1)."""
    v = match_counts(dev, a, b, op)
    try:
        return filtered_copy(dev, CountResult(a.ukeys, v, _match_bytes(a, b), a.n, a.k), lo, hi)
    finally:
        v.free()


def set_op(dev: Device, a: CountResult, b: CountResult, op: str, counts: Optional[str] = None, min_count: int = 1,
           max_count: Optional[int] = None) -> CountResult:
    """Set operations on two count tables of one k, on the device; a fresh
    CountResult (key-sorted, distinct), `a` and `b` left as they are.
      intersect  the rows of a whose key is in b; counts: left (default, a's) |
                 right (b's) | min | max | sum
      subtract   the rows of a whose key is not in b, with a's counts
      union      every key of either; counts: sum (default) | max
    Only rows whose resulting count is in [max(1, min_count), max_count] are
    kept.  intersect / subtract: kman_match_counts + one out-of-place
    kman_filter_counts (the range costs no pass of its own); union: a's rows
    with ANY_SUM / ANY_MAX, b's rows absent from a, one 2-run kman_merge_runs,
    then the range.  No row is downloaded."""
    counts = check_set_op(op, counts)
    if a.k != b.k:
        raise AssertionError("the two tables hold k-mers of different k: %d and %d" % (a.k, b.k))
    lo, hi = check_count_range(max(1, min_count) if isinstance(min_count, (int, np.integer)) else min_count,
                               max_count)
    if op == "intersect":
        return _matched_rows(dev, a, b, counts, lo, hi)
    if op == "subtract":
        return _matched_rows(dev, a, b, "absent", lo, hi)
    vb = _match_bytes(a, b)
    va = only_b = ok_ = oc_ = None
    try:
        va = match_counts(dev, a, b, "any_" + counts)
        only_b = _matched_rows(dev, b, a, "absent")
        n = a.n + only_b.n
        ok_ = dev.alloc(8 * max(n, 1))
        oc_ = dev.alloc(vb * max(n, 1))
        runs = (N.Run * 2)(N.Run(a.ukeys.ptr, va.ptr, a.n), N.Run(only_b.ukeys.ptr, only_b.counts.ptr, only_b.n))
        N.check(dev.ctx, N.lib().kman_merge_runs(dev.ctx, runs, 2, vb, c_void_p(ok_.ptr), c_void_p(oc_.ptr), None,
                                                 None), "kman_merge_runs")
        r = CountResult(ok_, oc_, vb, n, a.k)
        filter_counts(dev, r, lo, hi)
        ok_ = oc_ = None  # (the result's now)
        return r
    finally:
        for buf in (va, ok_, oc_):
            if buf is not None:
                buf.free()
        free_result(only_b)


# ------------------------------------------------- reads against a table (screen)


def default_index_bits(n: int, k: int) -> int:
    """table_index's default width: about 8 rows per bucket on spread keys."""
    return min(2 * k, N.KMAN_SCREEN_MAX_INDEX_BITS, max(1, (max(int(n), 2) - 1).bit_length() - 3))


def _check_index_bits(index_bits: int, k: int) -> int:
    top = min(2 * k, N.KMAN_SCREEN_MAX_INDEX_BITS)
    if isinstance(index_bits, bool) or not isinstance(index_bits, (int, np.integer)) or not 1 <= index_bits <= top:
        raise AssertionError("index_bits must be an integer in [1, %d] for k = %d, got %r" % (top, k, index_bits))
    return int(index_bits)


def table_index(dev: Device, table: CountResult, index_bits: Optional[int] = None) -> DeviceBuffer:
    """kman_table_index: the prefix index of a key-sorted distinct count table
    (join_groups(.., "count")), 2^index_bits + 1 u64 words in a fresh device
    buffer: word p = the rows whose top index_bits key bits are < p.
    index_bits None: min(2k, 24, max(1, ceil(log2(max(n, 2))) - 3)), about 8
    rows per bucket on spread keys -- a choice nobody has measured against
    wider or narrower indexes."""
    if table.k > MAX_K:
        raise AssertionError("a table index takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    bits = default_index_bits(table.n, table.k) if index_bits is None else _check_index_bits(index_bits, table.k)
    idx = dev.alloc(8 * ((1 << bits) + 1))
    try:
        N.check(dev.ctx, N.lib().kman_table_index(dev.ctx, c_void_p(table.ukeys.ptr), table.n, table.k, bits,
                                                  c_void_p(idx.ptr)), "kman_table_index")
    except BaseException:
        idx.free()
        raise
    return idx


def screen(p: Parsed, table: CountResult, canonical: bool = False, index: Optional[DeviceBuffer] = None,
           index_bits: Optional[int] = None) -> np.ndarray:
    """kman_screen_records: for every record of p, (valid k-mer windows, those
    whose key is a row of `table`, the sum of those rows' counts), k =
    table.k, as an (n_records, 3) u64 array.  canonical: the windows' keys are
    min(k-mer, reverse complement), for a table counted that way.  `index`: a
    table_index(dev, table, index_bits) kept by the caller (index_bits is then
    the width it was built with; None: the default width); None: built and
    freed here."""
    if table.k > MAX_K:
        raise AssertionError("screen takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    dev, k, R = p.dev, table.k, int(p.n_records)
    bits = default_index_bits(table.n, k) if index_bits is None else _check_index_bits(index_bits, k)
    if R == 0:
        return np.zeros((0, 3), np.uint64)
    own = d_rec = d_out = None
    try:
        if index is None:
            index = own = table_index(dev, table, bits)
        d_rec = dev.alloc(8 * R)
        dev.upload(d_rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        d_out = dev.alloc(24 * R)
        N.check(dev.ctx, N.lib().kman_screen_records(
            dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, N.KMAN_CANONICAL if canonical else 0, c_void_p(d_rec.ptr), R,
            c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n, c_void_p(index.ptr),
            bits, c_void_p(d_out.ptr)), "kman_screen_records")
        planes = dev.download(d_out, 3 * R, np.uint64)
    finally:
        for b in (own, d_rec, d_out):
            if b is not None:
                b.free()
    return np.ascontiguousarray(planes.reshape(3, R).T)


def window_counts(p: Parsed, table: CountResult, canonical: bool = False, index: Optional[DeviceBuffer] = None,
                  index_bits: Optional[int] = None) -> DeviceBuffer:
    """kman_window_counts: one u32 per base of p in a fresh device buffer (the
    caller frees it): the count in `table` of the k-mer window that starts at
    that base (0: not a row; counts above 0xFFFFFFFE saturate there),
    N.KMAN_WC_NONE where no valid window starts.  canonical, index, index_bits
    as for screen()."""
    if table.k > MAX_K:
        raise AssertionError("window_counts takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    dev, k = p.dev, table.k
    bits = default_index_bits(table.n, k) if index_bits is None else _check_index_bits(index_bits, k)
    own = d_wc = None
    try:
        if index is None:
            index = own = table_index(dev, table, bits)
        d_wc = dev.alloc(max(16, 4 * int(p.n_bases)))
        N.check(dev.ctx, N.lib().kman_window_counts(
            dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, N.KMAN_CANONICAL if canonical else 0,
            c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n, c_void_p(index.ptr),
            bits, c_void_p(d_wc.ptr)), "kman_window_counts")
        res, d_wc = d_wc, None
        return res
    finally:
        for b in (own, d_wc):
            if b is not None:
                b.free()


def quantile_plan(rec_seq, n_bases: int):
    """(records longer than KMAN_QUANTILE_REC_CAP bases, the bases they hold
    together) of a record table, as kman_record_quantile clamps and cuts it:
    the arguments of kman_record_quantile_plan."""
    rs = np.minimum(np.asarray(rec_seq, dtype=np.uint64), np.uint64(n_bases))
    if rs.size == 0:
        return 0, 0
    ends = np.concatenate([rs[1:], np.asarray([n_bases], dtype=np.uint64)])
    lens = np.where(ends > rs, ends - rs, np.uint64(0))
    long_ = lens > np.uint64(N.KMAN_QUANTILE_REC_CAP)
    return int(long_.sum()), int(lens[long_].sum())


def record_quantile(p: Parsed, d_wc: DeviceBuffer, num: int = 1, den: int = 2) -> np.ndarray:
    """kman_record_quantile over window_counts()'s words: per record of p, the
    word of rank floor((w - 1) * num / den) among its w words that are not
    KMAN_WC_NONE, ascending (1/2: the lower median, 0/1: the minimum, 1/1: the
    maximum), 0 for a record without windows; u32, n_records.  d_wc is
    scratch afterwards (still the caller's to free)."""
    for v in (num, den):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise AssertionError("quantile %r / %r: integers" % (num, den))
    if not (1 <= den <= 65535 and 0 <= num <= den):
        raise AssertionError("quantile %r / %r: 1 <= den <= 65535 and 0 <= num <= den" % (num, den))
    dev, R = p.dev, int(p.n_records)
    if R == 0:
        return np.zeros(0, np.uint32)
    rec_seq = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    n_long, n_values = quantile_plan(rec_seq, int(p.n_bases))
    need = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_record_quantile_plan(n_long, n_values, byref(need)), "kman_record_quantile_plan")
    d_rec = d_work = d_q = None
    try:
        d_rec = dev.alloc(8 * R)
        dev.upload(d_rec, rec_seq)
        d_work = dev.alloc(need.value)
        d_q = dev.alloc(max(16, 4 * R))
        N.check(dev.ctx, N.lib().kman_record_quantile(
            dev.ctx, c_void_p(d_wc.ptr), p.n_bases, c_void_p(d_rec.ptr), R, int(num), int(den), c_void_p(d_work.ptr),
            need.value, c_void_p(d_q.ptr)), "kman_record_quantile")
        return dev.download(d_q, R, np.uint32)
    finally:
        for b in (d_rec, d_work, d_q):
            if b is not None:
                b.free()


def screen_median(p: Parsed, table: CountResult, canonical: bool = False, index: Optional[DeviceBuffer] = None,
                  index_bits: Optional[int] = None, num: int = 1, den: int = 2):
    """(stats, median): screen()'s rows, from kman_screen_records exactly as
    screen() gets them, and record_quantile(num, den) of the records' window
    counts (u32, n_records).  The table's index is built once (or taken from
    the caller) and used by both kernels."""
    if table.k > MAX_K:
        raise AssertionError("screen takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    bits = default_index_bits(table.n, table.k) if index_bits is None else _check_index_bits(index_bits, table.k)
    own = d_wc = None
    try:
        if index is None:
            index = own = table_index(p.dev, table, bits)
        stats = screen(p, table, canonical, index=index, index_bits=bits)
        d_wc = window_counts(p, table, canonical, index=index, index_bits=bits)
        return stats, record_quantile(p, d_wc, num, den)
    finally:
        for b in (own, d_wc):
            if b is not None:
                b.free()


def _check_min_count(min_count) -> int:
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or \
            not 1 <= min_count <= N.KMAN_WC_NONE - 1:
        raise AssertionError("min_count must be an integer in [1, %d], got %r" % (N.KMAN_WC_NONE - 1, min_count))
    return int(min_count)


def record_runs(p: Parsed, d_wc: DeviceBuffer, min_count: int) -> np.ndarray:
    """kman_record_runs over window_counts()'s words: per record of p, (start,
    len) of its longest run of solid bases (word != KMAN_WC_NONE and >=
    min_count): len in windows, start the offset from the record's first base
    of the leftmost run of that length, both 0 for a record without a solid
    base; an (n_records, 2) u64 array.  d_wc is not modified."""
    min_count = _check_min_count(min_count)
    dev, R = p.dev, int(p.n_records)
    if R == 0:
        return np.zeros((0, 2), np.uint64)
    need = c_uint64(0)
    N.check(dev.ctx, N.lib().kman_record_runs_plan(int(p.n_bases), R, byref(need)), "kman_record_runs_plan")
    d_rec = d_work = d_out = None
    try:
        d_rec = dev.alloc(8 * R)
        dev.upload(d_rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        d_work = dev.alloc(need.value)
        d_out = dev.alloc(16 * R)
        N.check(dev.ctx, N.lib().kman_record_runs(
            dev.ctx, c_void_p(d_wc.ptr), p.n_bases, c_void_p(d_rec.ptr), R, min_count, c_void_p(d_work.ptr),
            need.value, c_void_p(d_out.ptr)), "kman_record_runs")
        planes = dev.download(d_out, 2 * R, np.uint64)
    finally:
        for b in (d_rec, d_work, d_out):
            if b is not None:
                b.free()
    return np.ascontiguousarray(planes.reshape(2, R).T)


def solid_spans(runs, k: int):
    """(START, END) of record_runs()'s rows in bases within the record, as
    `codes` holds them (every sequence character counts, N included; line
    breaks do not): START = start, END = start + len + k - 1 where len > 0 (a
    run of len windows covers len + k - 1 bases), both 0 otherwise."""
    runs = np.asarray(runs, dtype=np.uint64).reshape(-1, 2)
    has = runs[:, 1] > 0
    start = np.where(has, runs[:, 0], np.uint64(0)).astype(np.uint64)
    end = np.where(has, runs[:, 0] + runs[:, 1] + np.uint64(int(k) - 1), np.uint64(0)).astype(np.uint64)
    return np.ascontiguousarray(start), np.ascontiguousarray(end)


def screen_solid(p: Parsed, table: CountResult, canonical: bool, min_count: int, *, median: bool = False,
                 index: Optional[DeviceBuffer] = None, index_bits: Optional[int] = None):
    """(stats, median or None, runs): screen()'s rows, record_quantile()'s
    lower median when `median`, and record_runs(min_count) of the records'
    window counts.  The table's index is built once (or taken from the caller)
    and serves every kernel; window_counts runs once, and the runs are taken
    before the quantile, which leaves the words as scratch."""
    if table.k > MAX_K:
        raise AssertionError("screen takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    min_count = _check_min_count(min_count)
    bits = default_index_bits(table.n, table.k) if index_bits is None else _check_index_bits(index_bits, table.k)
    own = d_wc = None
    try:
        if index is None:
            index = own = table_index(p.dev, table, bits)
        stats = screen(p, table, canonical, index=index, index_bits=bits)
        d_wc = window_counts(p, table, canonical, index=index, index_bits=bits)
        runs = record_runs(p, d_wc, min_count)
        med = record_quantile(p, d_wc) if median else None
        return stats, med, runs
    finally:
        for b in (own, d_wc):
            if b is not None:
                b.free()


def correct(p: Parsed, table: CountResult, canonical: bool, min_count: int, *, index: Optional[DeviceBuffer] = None,
            index_bits: Optional[int] = None, d_wc: Optional[DeviceBuffer] = None) -> np.ndarray:
    """Isolated substitution errors of p's records put right against `table`
    (kman_correct_sites, kman_apply_fixes; the rule: include/kman.h): a run of
    at most k window counts below min_count with a count >= min_count next to
    it names one base, and the base is replaced when exactly one other base
    makes every window over it reach min_count.  ``p.codes`` is patched in
    place, and ``p.text`` (four-line FASTQ) when the parse kept it; quality
    values never change.  Returns the fixes per record, u32.  `d_wc`:
    window_counts() of p as it is, kept by the caller (not modified; stale
    afterwards where a base changed); None: computed and freed here.  One
    pass: the corrected records are not examined again.  index, index_bits as
    for screen()."""
    if table.k > MAX_K:
        raise AssertionError("correct takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    min_count = _check_min_count(min_count)
    dev, k, R, n = p.dev, table.k, int(p.n_records), int(p.n_bases)
    bits = default_index_bits(table.n, k) if index_bits is None else _check_index_bits(index_bits, k)
    if R == 0 or n == 0:
        return np.zeros(R, np.uint32)
    bufs = []
    try:
        if index is None:
            index = table_index(dev, table, bits)
            bufs.append(index)
        if d_wc is None:
            d_wc = window_counts(p, table, canonical, index=index, index_bits=bits)
            bufs.append(d_wc)
        d_rec = dev.alloc(8 * R)
        bufs.append(d_rec)
        dev.upload(d_rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        d_fix = dev.alloc(max(16, n))
        bufs.append(d_fix)
        n_fixed = c_uint64(0)
        N.check(dev.ctx, N.lib().kman_correct_sites(
            dev.ctx, c_void_p(p.codes.ptr), n, k, N.KMAN_CANONICAL if canonical else 0, c_void_p(d_wc.ptr),
            c_void_p(d_rec.ptr), R, c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n,
            c_void_p(index.ptr), bits, min_count, c_void_p(d_fix.ptr), byref(n_fixed)), "kman_correct_sites")
        d_text = d_off = None
        if p.text is not None:
            off = np.empty(R + 1, dtype=np.uint64)
            off[:R] = p.rec_hdr
            off[R] = int(p.text_bytes)
            d_off = dev.alloc(off.nbytes)
            bufs.append(d_off)
            dev.upload(d_off, off)
            d_text = p.text
        d_nfix = dev.alloc(max(16, 4 * R))
        bufs.append(d_nfix)
        N.check(dev.ctx, N.lib().kman_apply_fixes(
            dev.ctx, c_void_p(p.codes.ptr), n, c_void_p(d_fix.ptr), c_void_p(d_rec.ptr), R,
            c_void_p(d_text.ptr) if d_text is not None else None, int(p.text_bytes) if d_text is not None else 0,
            c_void_p(d_off.ptr) if d_off is not None else None, c_void_p(d_nfix.ptr)), "kman_apply_fixes")
        return dev.download(d_nfix, R, np.uint32)
    finally:
        for b in bufs:
            b.free()


def _span_arrays(span, R: int):
    start, end = (np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1)) for a in span)
    if start.shape != (R,) or end.shape != (R,):
        raise AssertionError("span arrays of %r and %r for %d records" % (start.shape, end.shape, R))
    return start, end


def screen_keep(stats: np.ndarray, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False, *, median=None,
                min_median: Optional[int] = None, max_median: Optional[int] = None, span=None,
                min_solid_len: Optional[int] = None) -> np.ndarray:
    """Which records of screen()'s rows are written, a u8 mask: those with
    hits >= min_hits and hits >= min_frac * windows (float64) and, with
    `median` (screen_median()'s second result), min_median <= median <=
    max_median (each bound only when given) and, with `span` (solid_spans()'s
    pair), END - START >= min_solid_len (when given), the others when
    `invert`."""
    stats = np.asarray(stats, dtype=np.uint64).reshape(-1, 3)
    windows, hits = stats[:, 0].astype(np.float64), stats[:, 1].astype(np.float64)
    keep = (hits >= min_hits) & (hits >= min_frac * windows)
    if min_median is not None or max_median is not None:
        if median is None:
            raise AssertionError("min_median / max_median need the median array")
        med = np.asarray(median, dtype=np.uint32).reshape(-1).astype(np.int64)
        if med.shape[0] != stats.shape[0]:
            raise AssertionError("%d medians for %d records" % (med.shape[0], stats.shape[0]))
        if min_median is not None:
            keep &= med >= min(int(min_median), 1 << 40)  # (bounds outside u32 clipped into int64)
        if max_median is not None:
            keep &= med <= max(int(max_median), -1)
    if min_solid_len is not None:
        if span is None:
            raise AssertionError("min_solid_len needs the span arrays")
        start, end = _span_arrays(span, stats.shape[0])
        keep &= (end - np.minimum(start, end)).astype(np.float64) >= float(min_solid_len)
    if invert:
        keep = ~keep
    return keep.astype(np.uint8)


def emit_screen(p: Parsed, stats: np.ndarray, keep, sink=None, median=None, *, span=None, fixes=None):
    """The `kmer screen` text of screen()'s rows: one "name<TAB>windows<TAB>
    hits<TAB>sum" line per record with keep != 0 (None: all), in input order
    (kman_format_screen); with `median` (u32 per record) a fifth column
    "<TAB>median" (kman_format_screen_median); with `span` (solid_spans()'s
    pair) two last columns "<TAB>START<TAB>END" (kman_format_screen_solid);
    with `fixes` (correct()'s array; needs `span`) one more, "<TAB>FIXES"
    (kman_format_screen_correct).  Returned, or written to the binary file
    `sink`."""
    stats = np.asarray(stats, dtype=np.uint64).reshape(-1, 3)
    R = stats.shape[0]
    if R != p.n_records:
        raise AssertionError("%d rows for %d records" % (R, p.n_records))
    planes = np.ascontiguousarray(stats.T)
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    kp = None
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.shape != (R,):
            raise AssertionError("keep mask of %r for %d records" % (keep.shape, R))
        kp = keep.ctypes.data_as(c_void_p)
    if median is not None:
        median = np.ascontiguousarray(median, dtype=np.uint32)
        if median.shape != (R,):
            raise AssertionError("median array of %r for %d records" % (median.shape, R))
    if fixes is not None:
        if span is None:
            raise AssertionError("fixes need the span arrays")
        fixes = np.ascontiguousarray(fixes, dtype=np.uint32)
        if fixes.shape != (R,):
            raise AssertionError("fixes array of %r for %d records" % (fixes.shape, R))
        start, end = _span_arrays(span, R)
        mp = median.ctypes.data_as(c_void_p) if median is not None else None
        return _to(sink, _format(N.lib().kman_format_screen_correct, planes.ctypes.data_as(c_void_p), mp,
                                 start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p),
                                 fixes.ctypes.data_as(c_void_p), R, kp, p.names_blob, off.ctypes.data_as(c_void_p)))
    if span is not None:
        start, end = _span_arrays(span, R)
        mp = median.ctypes.data_as(c_void_p) if median is not None else None
        return _to(sink, _format(N.lib().kman_format_screen_solid, planes.ctypes.data_as(c_void_p), mp,
                                 start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), R, kp, p.names_blob,
                                 off.ctypes.data_as(c_void_p)))
    if median is not None:
        return _to(sink, _format(N.lib().kman_format_screen_median, planes.ctypes.data_as(c_void_p),
                                 median.ctypes.data_as(c_void_p), R, kp, p.names_blob, off.ctypes.data_as(c_void_p)))
    return _to(sink, _format(N.lib().kman_format_screen, planes.ctypes.data_as(c_void_p), R, kp, p.names_blob,
                             off.ctypes.data_as(c_void_p)))


def emit_bed(p: Parsed, span, keep, sink=None):
    """The BED of the solid spans: one "name<TAB>START<TAB>END" line per
    record with keep != 0 (None: all) and END > START, in input order
    (kman_format_bed).  Returned, or written to the binary file `sink`."""
    R = int(p.n_records)
    start, end = _span_arrays(span, R)
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    kp = None
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        if keep.shape != (R,):
            raise AssertionError("keep mask of %r for %d records" % (keep.shape, R))
        kp = keep.ctypes.data_as(c_void_p)
    return _to(sink, _format(N.lib().kman_format_bed, start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), R,
                             kp, p.names_blob, off.ctypes.data_as(c_void_p)))


_CUT_MAX_RECORDS = 1 << 24  # records per slice of cut_records (its work memory: 16 B each, 64 B under trim)


def _keep_array(keep, R: int):
    if keep is None:
        return None
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    if keep.shape != (R,):
        raise AssertionError("keep mask of %r for %d records" % (keep.shape, R))
    return keep


def _cut_slices(bound: np.ndarray, limit: int):
    """(i0, records, text bound) per slice: as many records as fit `limit`
    bytes of text bound (at most _CUT_MAX_RECORDS), at least one, so a record
    larger than `limit` gets a slice of its own."""
    cum = np.cumsum(bound, dtype=np.uint64)
    R, i0, done, res = len(bound), 0, 0, []
    while i0 < R:
        j = int(np.searchsorted(cum, np.uint64(done + limit), side="right"))
        j = min(max(j, i0 + 1), i0 + _CUT_MAX_RECORDS, R)
        res.append((i0, j - i0, int(cum[j - 1]) - done))
        i0, done = j, int(cum[j - 1])
    return res


def cut_records(p: Parsed, keep, sink=None, *, span=None, trim=False):
    """The text of the records of p with keep != 0 (None: all), in input order
    (kman_cut_records), from the device text that parse(..., keep_text=True)
    left in ``p.text``: record r is the input's bytes from rec_hdr[r] to
    rec_hdr[r + 1] (the last one runs to the text's end), verbatim.  With
    `trim` (FASTQ records; `span`: solid_spans()'s pair) every record is cut to
    its columns [START, END): header, sequence[START:END], the ``+`` line and
    quality[START:END], each followed by ``"\\n"``; a record with END <= START
    is left out.  Returned (a bytearray), or written to the binary file `sink`,
    through _format_dev's pinned stages and writer pool, in slices of whole
    records chosen from rec_hdr (a record's text is at most its bytes + 4); a
    record larger than a slice gets a slice, and stages, sized for it."""
    if p.text is None:
        raise AssertionError("cut_records needs the input text on the device: parse with keep_text=True")
    dev, L, R, n = p.dev, N.lib(), int(p.n_records), int(p.text_bytes)
    keep = _keep_array(keep, R)
    if trim and span is None:
        raise AssertionError("trim needs the span arrays")
    if span is not None and not trim:
        raise AssertionError("span arrays are for trim=True")
    if R == 0:
        return None if sink is not None else bytearray()
    off = np.empty(R + 1, dtype=np.uint64)
    off[:R] = p.rec_hdr
    off[R] = n
    ends = np.minimum(off[1:], np.uint64(n)).astype(np.int64)
    bound = np.maximum(ends - np.minimum(off[:R], np.uint64(n)).astype(np.int64), 0) + 4
    if keep is not None:
        bound[keep == 0] = 0
    slices = _cut_slices(bound, _FMT_SLICE)
    flags = N.KMAN_CUT_TRIM if trim else 0
    need = c_uint64(0)
    N.check(dev.ctx, L.kman_cut_records_plan(max(m for _, m, _ in slices), flags, byref(need)),
            "kman_cut_records_plan")
    bufs = []
    try:
        def up(a):
            b = dev.alloc(a.nbytes)
            bufs.append(b)
            dev.upload(b, a)
            return b.ptr

        d_off = up(off)
        d_keep = up(keep) if keep is not None else None
        d_start = d_end = None
        if trim:
            start, end = _span_arrays(span, R)
            d_start, d_end = up(start), up(end)
        d_work = dev.alloc(need.value)
        bufs.append(d_work)

        def at(ptr, nbytes):
            return c_void_p(ptr + nbytes) if ptr is not None else None

        def call(i0, m, d_out, cap, used):
            return L.kman_cut_records(dev.ctx, c_void_p(p.text.ptr), n, at(d_off, 8 * i0), m, at(d_keep, i0),
                                      at(d_start, 8 * i0), at(d_end, 8 * i0), flags, c_void_p(d_work.ptr), need.value,
                                      d_out, cap, byref(used))

        return _format_dev(dev, R, 0, call, sink, slices=slices)
    finally:
        for b in bufs:
            b.free()


def _cut_host(text: bytes, off, keep, span, trim: bool) -> bytes:
    """cut_records' bytes by a plain host loop (KMAN_HOST_FORMAT)."""
    import re

    out = []
    for r in range(len(off) - 1):
        if keep is not None and not keep[r]:
            continue
        rec = text[int(off[r]):int(off[r + 1])]
        if not trim:
            out.append(rec)
            continue
        s, e = int(span[0][r]), int(span[1][r])
        lines = (re.split(rb"\r\n|\n|\r", rec) + [b""] * 4)[:4]
        body = lines[1].rstrip(b" \t\n\r\v\f\x1c\x1d\x1e\x1f")
        cols = [c for c in range(len(body)) if body[c] not in b" \r"]
        e = min(e, len(cols))
        if s >= e:
            continue
        c0, c1 = cols[s], cols[e - 1] + 1
        out.append(lines[0] + b"\n" + lines[1][c0:c1] + b"\n" + lines[2] + b"\n" + lines[3][c0:c1] + b"\n")
    return b"".join(out)


def emit_reads(p: Parsed, keep, sink, *, span=None, trim=False):
    """`kmer screen --reads-out`: cut_records of the listed records; under
    `trim` the listed records without a stretch (END == START) are left out,
    as emit_bed leaves them out.  KMAN_HOST_FORMAT=1: a host loop over the
    downloaded text instead of the device kernels."""
    R = int(p.n_records)
    keep = _keep_array(keep, R)
    if trim:
        if span is None:
            raise AssertionError("trim needs the span arrays")
        start, end = _span_arrays(span, R)
        keep = (np.ones(R, np.uint8) if keep is None else keep.copy())
        keep[end == start] = 0
        span = (start, end)
    if host_format():
        if p.text is None:
            raise AssertionError("emit_reads needs the input text on the device: parse with keep_text=True")
        text = p.dev.download(p.text, p.text_bytes, np.uint8).tobytes()
        off = list(p.rec_hdr) + [p.text_bytes]
        return _to(sink, _cut_host(text, off, keep, span, trim))
    return cut_records(p, keep, sink, span=span, trim=trim)


# ------------------------------------------------- homopolymer compression
#
# One more transformation of the parsed codes, like the -q mask and the mate
# zip: every run of one base collapses to its first base (kman_hpc_records;
# the rule: include/kman.h).  Everything downstream takes the new Parsed.


def hpc(p: Parsed, *, keep_map: bool = False) -> Parsed:
    """p with homopolymer-compressed codes (kman_hpc_records): a new Parsed
    with the kept codes (a record's first base, N and other letters and bases
    masked by -q are always kept, so the mask is applied before the
    compression), the new ``rec_seq`` and ``n_bases`` and p's names,
    ``rec_hdr``, ``text`` and ``text_bytes``, so cut_records still writes the
    original records.  `keep_map`: the result also carries ``hpc_orig`` (the
    original index of every kept base, u64 on the device), ``hpc_rec_seq`` and
    ``hpc_n_bases`` (p's own), for hpc_spans.  ``p.codes`` is freed (peak:
    twice the codes, plus 8 B per base for the map); the result owns the text
    and every buffer, and p must not be used afterwards."""
    if p.mates is not None:
        raise AssertionError("hpc takes a plain parse: compress each input before zip_pairs")
    dev, R, n = p.dev, int(p.n_records), int(p.n_bases)
    codes = d_rec = d_out = orig = None
    try:
        codes = dev.alloc(n + 64)
        d_rec, d_out = dev.alloc(max(16, 8 * R)), dev.alloc(max(16, 8 * R))
        if R:
            dev.upload(d_rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        if keep_map:
            orig = dev.alloc(max(16, 8 * n))
        n_out = c_uint64(0)
        N.check(dev.ctx, N.lib().kman_hpc_records(
            dev.ctx, c_void_p(p.codes.ptr), n, c_void_p(d_rec.ptr), R, c_void_p(codes.ptr), c_void_p(d_out.ptr),
            c_void_p(orig.ptr) if orig is not None else None, byref(n_out)), "kman_hpc_records")
        rec_seq = dev.download(d_out, R, np.uint64) if R else np.zeros(0, np.uint64)
        res, codes, omap, orig = codes, None, orig, None
    finally:
        for b in (codes, d_rec, d_out, orig):
            if b is not None:
                b.free()
    p.codes.free()
    text, p.text = p.text, None
    phases.mark("hpc")
    return Parsed(dev, res, int(n_out.value), R, p.rec_hdr, rec_seq, p.names, p.names_blob, p.name_off, p.n_masked,
                  text=text, text_bytes=p.text_bytes, hpc_orig=omap,
                  hpc_rec_seq=np.ascontiguousarray(p.rec_seq, dtype=np.uint64) if keep_map else None,
                  hpc_n_bases=n if keep_map else 0)


_hpc_parsed = hpc  # (for callers whose own `hpc` argument hides the function)


def hpc_spans(p: Parsed, span):
    """(START, END) per record of hpc(keep_map=True)'s result, from compressed
    columns to the columns of the original record: START_o = orig[rs_c +
    START] - rs_o, END_o = orig[rs_c + END] - rs_o, or, when END is the
    compressed record's length, the original record's length: the whole run of
    the stretch's last base lies inside it.  A record without a stretch (END
    <= START) gets 0 and 0.  The two look-ups per record are one kman_gather
    from the device map."""
    if p.hpc_orig is None:
        raise AssertionError("hpc_spans needs the map: hpc(p, keep_map=True)")
    dev, R = p.dev, int(p.n_records)
    start, end = _span_arrays(span, R)
    if R == 0:
        return start, end
    rs_c = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    rs_o = p.hpc_rec_seq
    end_c = np.append(rs_c[1:], np.uint64(p.n_bases))
    end_o = np.append(rs_o[1:], np.uint64(p.hpc_n_bases))
    has = (end > start) & (rs_c + end <= end_c)
    inner = has & (rs_c + end < end_c)  # END is a base of the record: its first original column ends the stretch
    idx = np.zeros(2 * R, dtype=np.uint64)
    idx[:R] = np.where(has, rs_c + start, np.uint64(0))
    idx[R:] = np.where(inner, rs_c + end, np.uint64(0))
    if not has.any():
        return np.zeros(R, np.uint64), np.zeros(R, np.uint64)
    d_idx = d_val = None
    try:
        d_idx, d_val = dev.alloc(idx.nbytes), dev.alloc(idx.nbytes)
        dev.upload(d_idx, idx)
        N.check(dev.ctx, N.lib().kman_gather(dev.ctx, c_void_p(p.hpc_orig.ptr), c_void_p(d_idx.ptr), 2 * R,
                                             c_void_p(d_val.ptr), 8), "gather")
        val = dev.download(d_val, 2 * R, np.uint64)
    finally:
        for b in (d_idx, d_val):
            if b is not None:
                b.free()
    zero = np.uint64(0)
    s_o = np.where(has, val[:R] - rs_o, zero).astype(np.uint64)
    e_o = np.where(has, np.where(inner, val[R:], end_o) - rs_o, zero).astype(np.uint64)
    return np.ascontiguousarray(s_o), np.ascontiguousarray(e_o)


# ------------------------------------------------------------------ read pairs
#
# Two views of one code buffer in which the mates of every pair are neighbours
# (kman_zip_records, or an interleaved input as it is parsed): the MATE VIEW
# has one record per mate, the PAIR VIEW one per pair, its table being every
# second entry of the mate view's.  The lookup kernels cut windows at bit 3 of
# the codes, so no window spans two mates in either view.


class BorrowedBuffer:
    """A device buffer that somebody else owns: ``ptr`` follows the owner's
    (None once the owner freed it) and ``free`` does nothing, so a view can be
    freed, or dropped, any number of times without touching the allocation."""

    __slots__ = ("_owner",)

    def __init__(self, owner: DeviceBuffer):
        self._owner = owner

    @property
    def ptr(self):
        return self._owner.ptr

    @property
    def nbytes(self) -> int:
        return self._owner.nbytes

    @property
    def dev(self):
        return self._owner.dev

    def free(self) -> None:
        pass

    def offset(self, nbytes: int) -> int:
        return self.ptr + int(nbytes)


def _pair_keys(p: Parsed):
    """(bytes, starts, lengths) of p's names by the pair name rule: a name is
    ``Parsed.names[i]`` with one trailing ``/1`` or ``/2`` removed."""
    arr = np.frombuffer(p.names_blob, dtype=np.uint8)
    off = np.asarray(p.name_off, dtype=np.int64)
    ln = off[1:] - off[:-1]
    suf = np.zeros(len(ln), dtype=bool)
    two = np.nonzero(ln >= 2)[0]
    if len(two):
        last, prev = arr[off[1:][two] - 1], arr[off[1:][two] - 2]
        suf[two] = (prev == 0x2F) & ((last == 0x31) | (last == 0x32))
    return arr, off[:-1], ln - 2 * suf


def _first_name_mismatch(k1, k2) -> int:
    """The first index at which two _pair_keys differ, -1 when none does."""
    (a1, s1, l1), (a2, s2, l2) = k1, k2
    bad = np.nonzero(l1 != l2)[0]
    first = int(bad[0]) if len(bad) else len(l1)
    ln = np.where(l1 == l2, l1, 0)
    tot = int(ln.sum())
    if tot:
        base = np.cumsum(ln) - ln
        within = np.arange(tot, dtype=np.int64) - np.repeat(base, ln)
        diff = np.nonzero(a1[np.repeat(s1, ln) + within] != a2[np.repeat(s2, ln) + within])[0]
        if len(diff):
            first = min(first, int(np.searchsorted(base + ln, diff[0], side="right")))
    return first if first < len(l1) else -1


def check_pair_names(names1: Parsed, names2: Parsed) -> None:
    """Refuses (AssertionError) the first pair whose two names differ by the
    pair name rule (_pair_keys), naming the 1-based pair and both names.  Host
    code over the parses' name blobs."""
    i = _first_name_mismatch(_pair_keys(names1), _pair_keys(names2))
    if i >= 0:
        raise AssertionError("pair %d: the mates' names differ, %r and %r (a trailing /1 or /2 is ignored): the "
                             "files are not in step" % (i + 1, bytes(names1.names[i]), bytes(names2.names[i])))


def _even_names(p: Parsed):
    """(names, blob, name_off) of the records 0, 2, 4, .. of p."""
    arr = np.frombuffer(p.names_blob, dtype=np.uint8)
    off = np.asarray(p.name_off, dtype=np.int64)
    st, ln = off[:-1][0::2], (off[1:] - off[:-1])[0::2]
    tot = int(ln.sum())
    base = np.cumsum(ln) - ln
    blob = arr[np.repeat(st, ln) + (np.arange(tot, dtype=np.int64) - np.repeat(base, ln))].tobytes() if tot else b""
    name_off = np.zeros(len(ln) + 1, dtype=np.uint64)
    if len(ln):
        name_off[1:] = np.cumsum(ln, dtype=np.uint64)
    return BlobNames(blob, name_off), blob, name_off


def zip_pairs(p1: Parsed, p2: Parsed, *, check_names: bool = True) -> Parsed:
    """The mate view of two parses whose i-th records are the two mates of pair
    i (kman_zip_records): 2R records, record 2i mate 1 and record 2i + 1 mate 2
    of pair i, their codes copied verbatim (bit 3, a ``-q`` mask) into one
    fresh buffer.  Different record counts are refused, and with `check_names`
    the first pair whose names differ (check_pair_names), both before any
    device work.
    ``p1.codes`` and ``p2.codes`` are freed once the zip is done (peak: twice
    the codes).  Names, ``rec_hdr`` and the texts are not merged: the result
    has no names, and carries the two sources as ``mates`` -- with their
    names, ``rec_hdr`` and, when they were parsed with keep_text, their device
    texts, for cut_records.  ``free()`` of the result frees them too; p1 and p2
    must not be used for lookups afterwards."""
    if p1.n_records != p2.n_records:
        raise AssertionError("READS has %d records and READS2 has %d: the files are not the two ends of the same "
                             "fragments" % (p1.n_records, p2.n_records))
    if p1.dev is not p2.dev:
        raise AssertionError("zip_pairs: the two parses are on different devices")
    if check_names:
        check_pair_names(p1, p2)
    dev, R = p1.dev, int(p1.n_records)
    n = int(p1.n_bases) + int(p2.n_bases) if R else 0
    codes = d1 = d2 = d_out = None
    try:
        codes = dev.alloc(int(p1.n_bases) + int(p2.n_bases) + 64)
        d1, d2, d_out = dev.alloc(max(16, 8 * R)), dev.alloc(max(16, 8 * R)), dev.alloc(max(16, 16 * R))
        if R:
            dev.upload(d1, np.ascontiguousarray(p1.rec_seq, dtype=np.uint64))
            dev.upload(d2, np.ascontiguousarray(p2.rec_seq, dtype=np.uint64))
        N.check(dev.ctx, N.lib().kman_zip_records(
            dev.ctx, c_void_p(p1.codes.ptr), int(p1.n_bases), c_void_p(d1.ptr), c_void_p(p2.codes.ptr),
            int(p2.n_bases), c_void_p(d2.ptr), R, c_void_p(codes.ptr), c_void_p(d_out.ptr)), "kman_zip_records")
        rec_seq = dev.download(d_out, 2 * R, np.uint64)
        res, codes = codes, None
    finally:
        for b in (codes, d1, d2, d_out):
            if b is not None:
                b.free()
    p1.codes.free()
    p2.codes.free()
    phases.mark("zip_pairs")
    return Parsed(dev, res, n, 2 * R, np.zeros(0, np.uint64), rec_seq, [], b"", np.zeros(1, np.uint64),
                  int(p1.n_masked) + int(p2.n_masked), mates=(p1, p2))


def pair_view(pz: Parsed) -> Parsed:
    """The pair view of zip_pairs' result: the same codes with every second
    entry of its record table, so R records, each a pair; names and
    ``rec_hdr`` are mate 1's as READS has them.  The view borrows the codes
    (BorrowedBuffer): freeing it frees nothing, and it is valid only while
    `pz` is."""
    if pz.mates is None:
        raise AssertionError("pair_view takes zip_pairs' result; an interleaved parse goes to pairs_of")
    p1 = pz.mates[0]
    return Parsed(pz.dev, BorrowedBuffer(pz.codes), pz.n_bases, pz.n_records // 2, p1.rec_hdr,
                  np.ascontiguousarray(pz.rec_seq[0::2]), p1.names, p1.names_blob, p1.name_off, pz.n_masked)


def pairs_of(p: Parsed, *, check_names: bool = True) -> Parsed:
    """The pair view of an ordinary parse of an interleaved input (records 2i
    and 2i + 1 are the mates of pair i); `p` itself is the mate view.  No
    kernel runs.  An odd record count is refused, and with `check_names` the
    first pair whose two names differ (check_pair_names' rule).  Names and
    ``rec_hdr`` are mate 1's.  The view borrows p's codes: freeing it frees
    nothing."""
    R2 = int(p.n_records)
    if R2 % 2:
        raise AssertionError("%d records: an interleaved input holds the two mates of every pair, an even number"
                             % R2)
    if check_names:
        a, s, ln = _pair_keys(p)
        i = _first_name_mismatch((a, s[0::2], ln[0::2]), (a, s[1::2], ln[1::2]))
        if i >= 0:
            raise AssertionError("pair %d: the mates' names differ, %r and %r (a trailing /1 or /2 is ignored): the "
                                 "input is not interleaved" % (i + 1, bytes(p.names[2 * i]), bytes(p.names[2 * i + 1])))
    names, blob, name_off = _even_names(p)
    return Parsed(p.dev, BorrowedBuffer(p.codes), p.n_bases, R2 // 2, np.ascontiguousarray(p.rec_hdr[0::2]),
                  np.ascontiguousarray(p.rec_seq[0::2]), names, blob, name_off, p.n_masked)


def screen_pairs(pm: Parsed, pv: Parsed, table: CountResult, canonical: bool = False, *, median: bool = False,
                 min_count: Optional[int] = None, index: Optional[DeviceBuffer] = None,
                 index_bits: Optional[int] = None):
    """(stats, median or None, runs or None) of read pairs: `pm` the mate view
    and `pv` the pair view of the same codes.  stats: screen()'s rows per pair,
    joint over both mates' windows; median (`median`): record_quantile's lower
    median of the union of both mates' window counts, per pair; runs
    (`min_count`): record_runs' rows per MATE, 2R of them.  kman_window_counts
    runs once and serves both; the runs are taken first because the quantile
    leaves the words as scratch.  Each k-mer is looked up once per kernel."""
    if table.k > MAX_K:
        raise AssertionError("screen takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, table.k))
    if pm.codes.ptr != pv.codes.ptr or pm.n_records != 2 * pv.n_records:
        raise AssertionError("screen_pairs: the two views are not of the same codes")
    if min_count is not None:
        min_count = _check_min_count(min_count)
    bits = default_index_bits(table.n, table.k) if index_bits is None else _check_index_bits(index_bits, table.k)
    own = d_wc = None
    try:
        if index is None:
            index = own = table_index(pm.dev, table, bits)
        stats = screen(pv, table, canonical, index=index, index_bits=bits)
        med = runs = None
        if median or min_count is not None:
            d_wc = window_counts(pm, table, canonical, index=index, index_bits=bits)
            if min_count is not None:
                runs = record_runs(pm, d_wc, min_count)
            if median:
                med = record_quantile(pv, d_wc)
        return stats, med, runs
    finally:
        for b in (own, d_wc):
            if b is not None:
                b.free()


def pair_min_span(span):
    """The mates' spans (2R rows, solid_spans of the mate view) as one span
    per pair for screen_keep's ``min_solid_len``: (0, the shorter of the two
    stretches), so a pair passes when both stretches do."""
    start, end = (np.asarray(a, dtype=np.uint64).reshape(-1) for a in span)
    ln = end - np.minimum(start, end)
    m = np.minimum(ln[0::2], ln[1::2])
    return np.zeros(len(m), np.uint64), np.ascontiguousarray(m)


def emit_screen_pairs(pv: Parsed, stats: np.ndarray, keep, sink=None, median=None, *, span=None):
    """The `kmer screen` text of read pairs: emit_screen's lines with one line
    per pair of the pair view `pv` (the name is mate 1's); with `span` (the
    mates' solid_spans, 2R rows) four last columns "<TAB>START<TAB>END<TAB>
    START2<TAB>END2", mate 1's stretch and mate 2's (kman_format_screen_pair).
    Returned, or written to the binary file `sink`."""
    if span is None:
        return emit_screen(pv, stats, keep, sink, median=median)
    stats = np.asarray(stats, dtype=np.uint64).reshape(-1, 3)
    R = stats.shape[0]
    if R != pv.n_records:
        raise AssertionError("%d rows for %d pairs" % (R, pv.n_records))
    planes = np.ascontiguousarray(stats.T)
    off = np.ascontiguousarray(pv.name_off, dtype=np.uint64)
    keep = _keep_array(keep, R)
    kp = keep.ctypes.data_as(c_void_p) if keep is not None else None
    mp = None
    if median is not None:
        median = np.ascontiguousarray(median, dtype=np.uint32)
        if median.shape != (R,):
            raise AssertionError("median array of %r for %d pairs" % (median.shape, R))
        mp = median.ctypes.data_as(c_void_p)
    start, end = _span_arrays(span, 2 * R)
    return _to(sink, _format(N.lib().kman_format_screen_pair, planes.ctypes.data_as(c_void_p), mp,
                             start.ctypes.data_as(c_void_p), end.ctypes.data_as(c_void_p), R, kp, pv.names_blob,
                             off.ctypes.data_as(c_void_p)))


def emit_pair_reads(pm: Parsed, keep, sink1, sink2=None, *, span=None, trim=False):
    """`--reads-out` for read pairs: the listed pairs' records, both mates of a
    pair or neither.  `pm` is the mate view: zip_pairs' result (the mates'
    texts are cut into `sink1` and `sink2`, both calls of cut_records with the
    same keep array, so record i of one file and record i of the other are
    mates), or an interleaved parse (one interleaved text into `sink1`, the
    pair's flag applied to both of its records).  Under `trim` (`span`: the
    mates' solid_spans, 2R rows) each mate is cut to its own stretch and a pair
    with a mate that has no stretch is left out whole."""
    R = int(pm.n_records) // 2
    keep = _keep_array(keep, R)
    keep = np.ones(R, np.uint8) if keep is None else keep.copy()
    if trim:
        if span is None:
            raise AssertionError("trim needs the span arrays")
        start, end = _span_arrays(span, 2 * R)
        has = end > start
        keep[~(has[0::2] & has[1::2])] = 0
    if pm.mates is None:
        if sink2 is not None:
            raise AssertionError("an interleaved input is written to one file")
        return emit_reads(pm, np.repeat(keep, 2), sink1, span=(start, end) if trim else None, trim=trim)
    if sink2 is None:
        raise AssertionError("two inputs are written to two files")
    for m, sink, sl in ((pm.mates[0], sink1, slice(0, None, 2)), (pm.mates[1], sink2, slice(1, None, 2))):
        sp = (np.ascontiguousarray(start[sl]), np.ascontiguousarray(end[sl])) if trim else None
        emit_reads(m, keep, sink, span=sp, trim=trim)


# ------------------------------------------------- reads among references (classify)

MAX_COLORS = N.KMAN_CLASSIFY_MAX_COLORS
UNASSIGNED, AMBIGUOUS = -1, -2  # classify_assign's values below the colours


def color_table(dev: Device, tables) -> CountResult:
    """The coloured table of 1..64 key-sorted distinct count tables of one k
    (join_groups(.., "count")): the union of their keys with count_bytes == 8,
    the "count" of a row being the mask of the tables that hold its key, bit c
    for tables[c].  The tables are CONSUMED: each one's buffers are freed as
    soon as it is folded in, so the peak is the union so far plus one table
    (free_result on them afterwards is harmless).  An empty table is legal:
    its colour is never hit.
    Table c's counts become 8-byte words all equal to 1 << c (kman_memset,
    kman_or_u64) and the table is folded into the running union with
    set_op(.., "union", "sum"): the bits are disjoint, so the sum is the OR,
    it never carries (KMAN_MATCH_ANY_SUM saturates only on a carry) and a mask
    with bit 63 set is inside filter_counts' unsigned range [1, 2^64 - 1]."""
    tables = list(tables)
    if not 1 <= len(tables) <= MAX_COLORS:
        raise AssertionError("a coloured table takes 1 to %d tables, got %d" % (MAX_COLORS, len(tables)))
    k = tables[0].k
    if k > MAX_K:
        raise AssertionError("a coloured table takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, k))
    for t in tables:
        if t.k != k:
            raise AssertionError("the tables hold k-mers of different k: %d and %d" % (k, t.k))
    acc = None
    try:
        for c, t in enumerate(tables):
            m = dev.alloc(8 * max(t.n, 1))
            try:
                if t.n:
                    dev.memset(m, 0, 8 * t.n)
                    N.check(dev.ctx, N.lib().kman_or_u64(dev.ctx, c_void_p(m.ptr), t.n, 1 << c), "kman_or_u64")
            except BaseException:
                m.free()
                raise
            t.counts.free()
            # the table's keys move to the coloured rows: a new handle owns the allocation, the table's is emptied
            ukeys = object.__new__(DeviceBuffer)
            ukeys.dev, ukeys.ptr, ukeys.nbytes = t.ukeys.dev, t.ukeys.ptr, t.ukeys.nbytes
            t.ukeys.ptr = None
            col = CountResult(ukeys, m, 8, t.n, k)
            t.n = 0
            if acc is None:
                acc = col
                continue
            try:
                u = set_op(dev, acc, col, "union", "sum")
            finally:
                free_result(col)
            free_result(acc)
            acc = u
        res, acc = acc, None
        return res
    finally:
        free_result(acc)


def classify(p: Parsed, ctable: CountResult, n_colors: int, canonical: bool = False, specific: bool = False,
             index: Optional[DeviceBuffer] = None, index_bits: Optional[int] = None, planes: bool = False):
    """kman_classify_records + kman_classify_pick: for every record of p,
    (windows, best, hits, second), four u32 arrays of n_records: its valid
    k-mer windows, the lowest-indexed reference with the most hits
    (N.KMAN_CLASSIFY_NONE when nothing hit), those hits, and the most hits
    among the other references.  `ctable`: color_table()'s result for
    n_colors references, k = ctable.k.  specific: a window counts only for the
    one reference that holds its k-mer.  canonical, index, index_bits as for
    screen().  planes: a fifth result, the (n_records, n_colors) u32 hits of
    every reference; without it only the windows plane and the three picked
    planes leave the device."""
    if ctable.k > MAX_K:
        raise AssertionError("classify takes k <= %d (one 64-bit key per k-mer), got %d" % (MAX_K, ctable.k))
    if isinstance(n_colors, bool) or not isinstance(n_colors, (int, np.integer)) or not 1 <= n_colors <= MAX_COLORS:
        raise AssertionError("n_colors must be an integer in [1, %d], got %r" % (MAX_COLORS, n_colors))
    if ctable.count_bytes != 8:
        raise AssertionError("classify takes a coloured table (8-byte masks: color_table), got %d-byte counts"
                             % ctable.count_bytes)
    dev, k, R, nc = p.dev, ctable.k, int(p.n_records), int(n_colors)
    bits = default_index_bits(ctable.n, k) if index_bits is None else _check_index_bits(index_bits, k)
    rec_seq = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    if R:
        ends = np.concatenate([rec_seq[1:], np.asarray([p.n_bases], dtype=np.uint64)])
        if int((ends - np.minimum(rec_seq, ends)).max()) >= 1 << 32:
            raise AssertionError("classify counts in 32 bits: a record of 2^32 or more bases is refused")
    if R == 0:
        z = np.zeros(0, np.uint32)
        return (z, z.copy(), z.copy(), z.copy()) + ((np.zeros((0, nc), np.uint32),) if planes else ())
    flags = (N.KMAN_CANONICAL if canonical else 0) | (N.KMAN_CLASSIFY_SPECIFIC if specific else 0)
    own = d_rec = d_out = d_pick = None
    try:
        if index is None:
            index = own = table_index(dev, ctable, bits)
        d_rec = dev.alloc(8 * R)
        dev.upload(d_rec, rec_seq)
        d_out = dev.alloc(4 * (1 + nc) * R)
        d_pick = dev.alloc(12 * R)
        N.check(dev.ctx, N.lib().kman_classify_records(
            dev.ctx, c_void_p(p.codes.ptr), p.n_bases, k, flags, c_void_p(d_rec.ptr), R, c_void_p(ctable.ukeys.ptr),
            c_void_p(ctable.counts.ptr), ctable.n, c_void_p(index.ptr), bits, nc, c_void_p(d_out.ptr)),
            "kman_classify_records")
        N.check(dev.ctx, N.lib().kman_classify_pick(dev.ctx, c_void_p(d_out.ptr), R, nc, c_void_p(d_pick.ptr)),
                "kman_classify_pick")
        windows = dev.download(d_out, R, np.uint32)
        pick = dev.download(d_pick, 3 * R, np.uint32).reshape(3, R)
        res = (windows, pick[0].copy(), pick[1].copy(), pick[2].copy())
        if planes:
            res += (np.ascontiguousarray(dev.download(d_out, nc * R, np.uint32, 4 * R).reshape(nc, R).T),)
        return res
    finally:
        for b in (own, d_rec, d_out, d_pick):
            if b is not None:
                b.free()


def classify_assign(windows, best, hits, second, min_hits: int = 1, min_frac: float = 0.0,
                    min_margin: int = 1) -> np.ndarray:
    """The reference each record of classify()'s arrays is assigned to, an
    int32 array: UNASSIGNED (-1) when hits < max(min_hits, 1) or hits <
    min_frac * windows (float64), else AMBIGUOUS (-2) when hits - second <
    min_margin, else `best`.  min_margin >= 1: a tie is never decided by the
    order of the references."""
    for name, v in (("min_hits", min_hits), ("min_margin", min_margin)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise AssertionError("%s must be an integer, got %r" % (name, v))
    if min_hits < 0:
        raise AssertionError("min_hits must be >= 0, got %d" % min_hits)
    if min_margin < 1:
        raise AssertionError("min_margin must be >= 1, got %d" % min_margin)
    if isinstance(min_frac, bool) or not isinstance(min_frac, (int, float, np.integer, np.floating)) or \
            not 0.0 <= min_frac <= 1.0:  # (a NaN is refused too)
        raise AssertionError("min_frac must be in [0, 1], got %r" % (min_frac,))
    w, b, h, s = (np.asarray(a, dtype=np.uint32).reshape(-1) for a in (windows, best, hits, second))
    if not (w.shape == b.shape == h.shape == s.shape):
        raise AssertionError("classify_assign: arrays of %r, %r, %r and %r" % (w.shape, b.shape, h.shape, s.shape))
    hf, h64 = h.astype(np.float64), h.astype(np.int64)
    un = (h64 < max(int(min_hits), 1)) | (hf < float(min_frac) * w.astype(np.float64)) | \
        (b == np.uint32(N.KMAN_CLASSIFY_NONE))
    amb = (h64 - s.astype(np.int64)) < int(min_margin)
    out = np.where(un, UNASSIGNED, np.where(amb, AMBIGUOUS, b.astype(np.int64)))
    return out.astype(np.int32)


def _label_blob(labels):
    labels = [x if isinstance(x, bytes) else str(x).encode("utf-8", errors="surrogateescape") for x in labels]
    if not 1 <= len(labels) <= MAX_COLORS:
        raise AssertionError("1 to %d labels, got %d" % (MAX_COLORS, len(labels)))
    off = np.zeros(len(labels) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in labels])
    return b"".join(labels), off


def emit_classify(p: Parsed, labels, windows, assign, hits, second, sink=None, *, planes=None, keep=None):
    """The `kmer classify` text: one "name<TAB>windows<TAB>LABEL<TAB>hits<TAB>
    second" line per record with keep != 0 (None: all), in input order
    (kman_format_classify); LABEL is labels[assign], "?" for AMBIGUOUS, "-" for
    UNASSIGNED.  `planes` (classify(.., planes=True)'s (n_records, n_colors)
    array) appends one column per reference.  Returned, or written to the
    binary file `sink`."""
    R = int(p.n_records)
    blob, loff = _label_blob(labels)
    nc = len(loff) - 1
    w, h, s = (np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in (windows, hits, second))
    a = np.ascontiguousarray(assign, dtype=np.int32).reshape(-1)
    for x in (w, h, s, a):
        if x.shape != (R,):
            raise AssertionError("array of %r for %d records" % (x.shape, R))
    if R and int(a.max()) >= nc:
        raise AssertionError("assignment %d with %d labels" % (int(a.max()), nc))
    pp = None
    if planes is not None:
        planes = np.asarray(planes, dtype=np.uint32)
        if planes.shape != (R, nc):
            raise AssertionError("hit planes of %r for %d records and %d labels" % (planes.shape, R, nc))
        planes = np.ascontiguousarray(planes.T)
        pp = planes.ctypes.data_as(c_void_p)
    keep = _keep_array(keep, R)
    kp = keep.ctypes.data_as(c_void_p) if keep is not None else None
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    return _to(sink, _format(N.lib().kman_format_classify, w.ctypes.data_as(c_void_p), a.ctypes.data_as(c_void_p),
                             h.ctypes.data_as(c_void_p), s.ctypes.data_as(c_void_p), pp, nc, R, kp, blob,
                             loff.ctypes.data_as(c_void_p), p.names_blob, off.ctypes.data_as(c_void_p)))


# ------------------------------------------------- all pairs of a coloured table (compare)

COMPARE_METRICS = ("jaccard", "dist", "shared", "containment")


def mask_gram(dev: Device, ctable: CountResult, n_colors: int):
    """kman_mask_gram on a coloured table (color_table): (gram, occ, private),
    numpy u64 arrays of shapes (n_colors, n_colors), (n_colors + 1,) and
    (n_colors,).  gram[i][j]: the rows held by references i and j (the
    diagonal: each reference's rows); occ[p]: the rows held by exactly p
    references; private[c]: the rows held by reference c alone.  An empty
    table gives zeros."""
    if isinstance(n_colors, bool) or not isinstance(n_colors, (int, np.integer)) or not 1 <= n_colors <= MAX_COLORS:
        raise AssertionError("n_colors must be an integer in [1, %d], got %r" % (MAX_COLORS, n_colors))
    if ctable.count_bytes != 8:
        raise AssertionError("mask_gram takes a coloured table (8-byte masks: color_table), got %d-byte counts"
                             % ctable.count_bytes)
    nc, n = int(n_colors), int(ctable.n)
    words = nc * nc + (nc + 1) + nc
    d_out = dev.alloc(8 * words)
    try:
        N.check(dev.ctx, N.lib().kman_mask_gram(
            dev.ctx, c_void_p(ctable.counts.ptr if n else None), n, nc, c_void_p(d_out.ptr),
            c_void_p(d_out.ptr + 8 * nc * nc), c_void_p(d_out.ptr + 8 * (nc * nc + nc + 1))), "kman_mask_gram")
        out = dev.download(d_out, words, np.uint64)
    finally:
        d_out.free()
    return out[:nc * nc].reshape(nc, nc).copy(), out[nc * nc:nc * nc + nc + 1].copy(), out[nc * nc + nc + 1:].copy()


def compare_rows(gram, k: int):
    """The per-pair metrics of mask_gram's matrix, computed in float64 from
    the exact integers: a list of (i, j, a, b, s, jaccard, cont_i, cont_j,
    dist) for every pair i < j, a = gram[i][i], b = gram[j][j], s =
    gram[i][j] as Python ints.  See compare_metrics."""
    g = np.asarray(gram, dtype=np.uint64)
    if g.ndim != 2 or g.shape[0] != g.shape[1]:
        raise AssertionError("compare_rows takes a square matrix, got %r" % (g.shape,))
    rows = []
    for i in range(g.shape[0]):
        for j in range(i + 1, g.shape[0]):
            a, b, s = int(g[i, i]), int(g[j, j]), int(g[i, j])
            rows.append((i, j, a, b, s) + compare_metrics(a, b, s, k))
    return rows


def compare_metrics(a: int, b: int, s: int, k: int):
    """(jaccard, containment of the first, containment of the second, Mash
    distance) of two k-mer sets of a and b k-mers that share s, with u = a +
    b - s: J = s / u (0 when u == 0); s / a and s / b (0 for an empty set);
    D = -ln(2 J / (1 + J)) / k, 1 when J == 0, exactly 0 when J == 1, clamped
    to [0, 1]."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise AssertionError("k must be a positive integer, got %r" % (k,))
    a, b, s = int(a), int(b), int(s)
    u = a + b - s
    jac = float(s) / float(u) if u else 0.0
    ca = float(s) / float(a) if a else 0.0
    cb = float(s) / float(b) if b else 0.0
    if jac <= 0.0:
        dist = 1.0
    elif jac >= 1.0:
        dist = 0.0
    else:
        dist = min(1.0, max(0.0, -math.log(2.0 * jac / (1.0 + jac)) / float(k)))
    return jac, ca, cb, dist


def _compare_labels(labels, n: int):
    labels = [x.decode("utf-8", errors="surrogateescape") if isinstance(x, bytes) else str(x) for x in labels]
    if len(labels) != n:
        raise AssertionError("%d labels for %d inputs" % (len(labels), n))
    return labels


def emit_compare(labels, gram, k: int, sink=None):
    """The `kmer compare` text: one "LABEL_I<TAB>LABEL_J<TAB>KMERS_I<TAB>
    KMERS_J<TAB>SHARED<TAB>JACCARD<TAB>CONT_I<TAB>CONT_J<TAB>DIST" line per
    pair i < j in input order, the reals as %.6f.  Plain host formatting.
    Returned, or written to the binary file `sink`."""
    g = np.asarray(gram, dtype=np.uint64)
    labels = _compare_labels(labels, g.shape[0])
    out = ["%s\t%s\t%d\t%d\t%d\t%.6f\t%.6f\t%.6f\t%.6f\n" % ((labels[i], labels[j]) + tuple(r))
           for (i, j, *r) in compare_rows(g, k)]
    return _to(sink, "".join(out).encode("utf-8", errors="surrogateescape"))


def emit_compare_matrix(labels, gram, k: int, metric: str = "dist", sink=None):
    """The `kmer compare --matrix` text: a first line with the number of
    inputs, then "LABEL<TAB>v_0<TAB>...<TAB>v_{n-1}" per input.  metric:
    "dist", "jaccard", "containment" (row in column, gram[r][c] / gram[r][r]:
    not symmetric) as %.6f, or "shared" as integers.  The diagonal is the
    input's k-mers (shared), 1 (jaccard, containment; 0 for an empty input)
    and 0 (dist)."""
    if metric not in COMPARE_METRICS:
        raise AssertionError("metric must be one of %s, got %r" % (", ".join(COMPARE_METRICS), metric))
    g = np.asarray(gram, dtype=np.uint64)
    n = g.shape[0]
    labels = _compare_labels(labels, n)
    out = ["%d\n" % n]
    for r in range(n):
        cells = []
        for c in range(n):
            a, b, s = int(g[r, r]), int(g[c, c]), int(g[r, c])
            if metric == "shared":
                cells.append("%d" % s)
                continue
            jac, ca, _, dist = compare_metrics(a, b, s, k)
            if r == c:
                jac, ca, dist = (1.0 if a else 0.0), (1.0 if a else 0.0), 0.0
            cells.append("%.6f" % {"jaccard": jac, "containment": ca, "dist": dist}[metric])
        out.append("\t".join([labels[r]] + cells) + "\n")
    return _to(sink, "".join(out).encode("utf-8", errors="surrogateescape"))


def emit_occupancy(occ, sink=None):
    """The `kmer compare --occupancy` text, the pan-genome spectrum: "P<TAB>
    KMERS" for P = 1 .. n, the k-mers held by exactly P inputs (P = n: the
    core).  `occ`: mask_gram's second array (occ[0] is not written)."""
    o = np.asarray(occ, dtype=np.uint64).reshape(-1)
    return _to(sink, "".join("%d\t%d\n" % (p, int(o[p])) for p in range(1, len(o))).encode())


def emit_compare_summary(labels, gram, private, sink=None):
    """The `kmer compare --summary` text: "LABEL<TAB>KMERS<TAB>PRIVATE" per
    input (its k-mers, and those of them no other input holds)."""
    g = np.asarray(gram, dtype=np.uint64)
    pr = np.asarray(private, dtype=np.uint64).reshape(-1)
    labels = _compare_labels(labels, g.shape[0])
    if len(pr) != len(labels):
        raise AssertionError("%d private counts for %d inputs" % (len(pr), len(labels)))
    out = ["%s\t%d\t%d\n" % (lab, int(g[c, c]), int(pr[c])) for c, lab in enumerate(labels)]
    return _to(sink, "".join(out).encode("utf-8", errors="surrogateescape"))


# ------------------------------------------------- unitigs of a count table (unitigs)

UNITIG_MIN_K, UNITIG_MAX_K = 3, 31


def check_unitig_k(k: int) -> int:
    """The K of the unitig graph, checked: odd (no k-mer is then its own
    reverse complement) and in [3, 31] (one 64-bit key, and a spare base)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise AssertionError("K must be an integer, got %r" % (k,))
    if k > UNITIG_MAX_K:
        raise AssertionError("unitigs take K <= %d, got %d: larger K is a stated limit of this command"
                             % (UNITIG_MAX_K, k))
    if k < UNITIG_MIN_K:
        raise AssertionError("unitigs take K >= %d, got %d" % (UNITIG_MIN_K, k))
    if k % 2 == 0:
        raise AssertionError("unitigs take an odd K (a k-mer of even length can be its own reverse complement), "
                             "got %d" % k)
    return int(k)


@dataclass
class UnitigResult:
    """The unitigs of a table, on the host, in file order: unitig u is
    seqs[off[u]:off[u + 1]] (ASCII), made of nodes[u] rows whose counts sum to
    kc[u] (modulo 2^64).  rounds / cycles: what kman_graph_rank reports."""
    seqs: np.ndarray
    off: np.ndarray
    nodes: np.ndarray
    kc: np.ndarray
    k: int
    rounds: int = 0
    cycles: int = 0

    @property
    def n(self) -> int:
        return len(self.nodes)

    def seq(self, u: int) -> str:
        return self.seqs[int(self.off[u]):int(self.off[u + 1])].tobytes().decode()


def graph_links(dev: Device, table: CountResult, index: Optional[DeviceBuffer] = None,
                index_bits: Optional[int] = None) -> DeviceBuffer:
    """kman_graph_links: the 2 n link words of a canonical count table in a
    fresh device buffer.  `index` / `index_bits` as for screen."""
    k = check_unitig_k(table.k)
    bits = default_index_bits(table.n, k) if index_bits is None else _check_index_bits(index_bits, k)
    own = None
    link = dev.alloc(8 * max(table.n, 1))
    try:
        if index is None:
            index = own = table_index(dev, table, bits)
        N.check(dev.ctx, N.lib().kman_graph_links(dev.ctx, c_void_p(table.ukeys.ptr), table.n, k, c_void_p(index.ptr),
                                                  bits, c_void_p(link.ptr)), "kman_graph_links")
    except BaseException:
        link.free()
        raise
    finally:
        if own is not None:
            own.free()
    return link


def unitigs(dev: Device, table: CountResult, index: Optional[DeviceBuffer] = None,
            index_bits: Optional[int] = None) -> UnitigResult:
    """The maximal unitigs of a CANONICAL count table (join_groups(..,
    "count", canonical=True), K odd and in [3, 31]) as include/kman.h defines
    them: kman_graph_links, kman_graph_rank, kman_unitig_spell (a sizing call,
    then the filling one), and one download.  `index`: a table_index(dev,
    table, index_bits) kept by the caller; None: built and freed here.  An
    empty table gives zero unitigs."""
    k = check_unitig_k(table.k)
    n = int(table.n)
    if n >= N.KMAN_GRAPH_MAX_ROWS:
        raise AssertionError("unitigs take tables of fewer than 2^31 rows, got %d" % n)
    if n == 0:
        if index_bits is not None:
            _check_index_bits(index_bits, k)
        return UnitigResult(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32),
                            np.zeros(0, np.uint64), k)
    L = N.lib()
    bufs = []

    def alloc(nbytes):
        bufs.append(dev.alloc(max(16, nbytes)))
        return bufs[-1]

    try:
        link = graph_links(dev, table, index, index_bits)
        bufs.append(link)
        rank = alloc(12 * n)
        start, pos, nodes = (c_void_p(rank.ptr + 4 * n * j) for j in range(3))
        rounds, cycles = c_uint32(0), c_uint64(0)
        N.check(dev.ctx, L.kman_graph_rank(dev.ctx, c_void_p(link.ptr), n, start, pos, nodes, byref(rounds),
                                           byref(cycles)), "kman_graph_rank")
        link.free()
        bufs.remove(link)
        nu, nb = c_uint64(0), c_uint64(0)
        keys, counts = c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr)
        N.check(dev.ctx, L.kman_unitig_spell(dev.ctx, keys, counts, table.count_bytes, n, k, start, pos, nodes, None,
                                             None, None, 0, None, 0, byref(nu), byref(nb)), "kman_unitig_spell")
        U, B = int(nu.value), int(nb.value)
        d_off, d_un, d_kc, d_seq = alloc(8 * (U + 1)), alloc(4 * U), alloc(8 * U), alloc(B)
        N.check(dev.ctx, L.kman_unitig_spell(dev.ctx, keys, counts, table.count_bytes, n, k, start, pos, nodes,
                                             c_void_p(d_off.ptr), c_void_p(d_un.ptr), c_void_p(d_kc.ptr), U,
                                             c_void_p(d_seq.ptr), B, byref(nu), byref(nb)), "kman_unitig_spell")
        assert int(nu.value) == U and int(nb.value) == B
        return UnitigResult(dev.download(d_seq, B, np.uint8), dev.download(d_off, U + 1, np.uint64),
                            dev.download(d_un, U, np.uint32), dev.download(d_kc, U, np.uint64), k,
                            int(rounds.value), int(cycles.value))
    finally:
        for b in bufs:
            b.free()


_UNITIG_SLICE = 64 << 20  # bases formatted per call of the host writer


def emit_unitigs(r: UnitigResult, sink=None):
    """The `kmer unitigs` text, ">ID LN:i:BASES KC:i:SUM" and the sequence on
    one line per unitig in file order (kman_format_unitigs on host threads, a
    slice of unitigs at a time).  Returned, or written to the binary file
    `sink`."""
    seqs = np.ascontiguousarray(r.seqs, dtype=np.uint8)
    off = np.ascontiguousarray(r.off, dtype=np.uint64)
    kc = np.ascontiguousarray(r.kc, dtype=np.uint64)
    n = len(kc)
    if len(off) != n + 1 or (n and int(off[n]) > len(seqs)):
        raise AssertionError("emit_unitigs: %d offsets and %d sequence bytes for %d unitigs" % (len(off), len(seqs), n))
    out, u0 = [], 0
    while u0 < n:
        u1 = int(np.searchsorted(off, int(off[u0]) + _UNITIG_SLICE, side="right")) - 1
        u1 = min(n, max(u1, u0 + 1))
        text = _format(N.lib().kman_format_unitigs, seqs.ctypes.data_as(c_void_p),
                       c_void_p(off.ctypes.data + 8 * u0), c_void_p(kc.ctypes.data + 8 * u0), u1 - u0, u0)
        if sink is None:
            out.append(text)
        else:
            sink.write(text)
        u0 = u1
    return b"".join(out) if sink is None else None


def join_groups(p: Parsed, k: int, rc: bool, mode: str, max_keys: Optional[int] = None, canonical: bool = False):
    """The count / uniq result of the whole stream of p on the device, by the
    fastest path that takes it: the region path (kman_groups); the multi-batch
    join (RangedJoin) when the single-batch general path does not fit the
    free HBM or max_keys asks for it; else the general path (extract_sorted +
    rle_*); k > 32: the word-pair path (wide_groups).  None when the stream
    has no k-mers.  canonical: the rows of min(k-mer, reverse complement)
    (count only; `rc` is then moot, both strands fold into one key); a
    sub-path that cannot take canonical keys raises NotImplementedError."""
    if canonical and mode == "uniq":
        raise ValueError("canonical k-mers are counted (config 5), not uniq'd")
    if k > MAX_K:
        return words_groups(p, k, rc, mode, canonical)
    r = groups(p, k, rc, mode, canonical) if max_keys is None else None
    if r is None and max_keys is None and p.n_bases:
        # outside kman_groups (too many k-mers for its regions, -r on large
        # inputs, skewed keys): the key rounds of the multi-GPU path on one GPU
        from . import dist

        r = dist.local_groups(p, k, rc, mode, canonical)
    if r is None and (max_keys is not None or not _fits(p, k, rc and not canonical, mode)):
        if canonical:
            # (RangedJoin cuts the stream by forward-key ranges: kman_extract_range has no canonical keys)
            raise NotImplementedError("canonical k-mers through the multi-batch join (RangedJoin)")
        r = ranged_groups(p, k, rc, mode, max_keys)
    if r is None:
        km = extract_sorted(p, k, rc, want_pos=mode == "uniq", canonical=canonical)
        try:
            if km.n == 0:
                return None
            r = rle_count(km, p.dev) if mode == "count" else rle_uniq(km, p.dev)
        finally:
            km.free()
    return r


def free_result(r) -> None:
    if r is None:
        return
    if isinstance(r, WordsResult):
        bs = (r.words, r.vals)
    else:
        bs = (r.ukeys, r.counts) if isinstance(r, CountResult) else (r.keys, r.pos)
    for b in bs:
        b.free()


def _emit_words(p: Parsed, r: WordsResult, sink=None):
    """Word-key rows as the reference's text: built on the device
    (kman_format_*_words_dev), or by the host writers (kman_format_*_words)
    with KMAN_HOST_FORMAT=1."""
    dev, L = p.dev, N.lib()
    vb = r.val_bytes
    # (row j's word q at words[q * stride + j]: a slice of rows is the same planes offset by i0)
    if not host_format():
        if r.mode == "count":
            def call(i0, m, d_out, cap, used):
                return L.kman_format_count_words_dev(dev.ctx, c_void_p(r.words.ptr + 8 * i0), r.stride,
                                                     c_void_p(r.vals.ptr + vb * i0), vb, m, r.k, d_out, cap,
                                                     byref(used))

            return _format_dev(dev, r.n, r.k + 2 + 20, call, sink)
        nm = DeviceNames(p)
        try:
            D = len(str(p.n_bases + r.k))

            def call(i0, m, d_out, cap, used):
                return L.kman_format_uniq_words_dev(dev.ctx, c_void_p(r.words.ptr + 8 * i0), r.stride,
                                                    c_void_p(r.vals.ptr + vb * i0), vb, m, r.k,
                                                    c_void_p(nm.names.ptr), c_void_p(nm.off.ptr), c_void_p(nm.rec.ptr),
                                                    nm.n_records, d_out, cap, byref(used))

            return _format_dev(dev, r.n, 1 + nm.max_name + 1 + D + 1 + D + 3 + r.k + 1, call, sink)
        finally:
            nm.free()
    words = dev.download(r.words, r.W * r.stride, np.uint64)
    vals = dev.download(r.vals, r.n, np.uint32 if vb == 4 else np.uint64)
    if r.mode == "count":
        return _to(sink, _format(L.kman_format_count_words, words.ctypes.data_as(c_void_p), r.stride,
                                 vals.ctypes.data_as(c_void_p), vb, r.n, r.k))
    names = ctypes.create_string_buffer(p.names_blob, max(1, len(p.names_blob)))
    off = np.ascontiguousarray(p.name_off, dtype=np.uint64)
    rs = np.ascontiguousarray(p.rec_seq, dtype=np.uint64)
    return _to(sink, _format(L.kman_format_uniq_words, words.ctypes.data_as(c_void_p), r.stride,
                             vals.ctypes.data_as(c_void_p), vb, r.n, r.k, names, off.ctypes.data_as(c_void_p),
                             rs.ctypes.data_as(c_void_p), p.n_records))


_emit_wide = _emit_words  # (round-2 name)


def count_text(text: bytes, k: int, rc: bool = False, dev: Optional[Device] = None,
               max_keys: Optional[int] = None) -> bytes:
    """``kmer count`` output bytes for a FASTA text (SEQ_COUNT mode).
    max_keys: run the multi-batch join with key ranges of at most that many
    k-mers (by default only when the single batch does not fit the HBM)."""
    dev = dev or default_device()
    _check_k(k, wide=True)
    p = parse(dev, text)
    try:
        check_empty_names(p, k)
        r = join_groups(p, k, rc, "count", max_keys)
        if r is None:
            return b""
        try:
            if isinstance(r, WordsResult):
                return _emit_words(p, r)
            return emit_count(dev, r)
        finally:
            free_result(r)
    finally:
        p.free()


def uniq_text(text: bytes, k: int, rc: bool = False, dev: Optional[Device] = None,
              max_keys: Optional[int] = None) -> bytes:
    """``kmer uniq`` output bytes for a FASTA text (UNIQUE mode); max_keys as
    in count_text."""
    dev = dev or default_device()
    _check_k(k, wide=True)
    p = parse(dev, text)
    try:
        check_empty_names(p, k)
        r = join_groups(p, k, rc, "uniq", max_keys)
        if r is None:
            return b""
        try:
            if isinstance(r, WordsResult):
                return _emit_words(p, r)
            return emit_uniq(p, r)
        finally:
            free_result(r)
    finally:
        p.free()


# ------------------------------------------------------- resident pipeline


class ResidentPipeline:
    """One FASTA text resident in HBM, every buffer preallocated: ``step()``
    runs parse -> extract -> sort -> count|uniq with no allocation, leaving
    the result device-resident (what bench.py times)."""

    def __init__(self, dev: Device, text: bytes, k: int, mode: str = "uniq", rc: bool = False,
                 pos_bytes: Optional[int] = None, path: str = "region"):
        _check_k(k)
        if mode not in ("count", "uniq"):
            raise ValueError(mode)
        if path not in ("region", "split", "full"):
            raise ValueError(path)
        # region: kman_groups (default; falls back to split when the input is
        # outside the region path); split: prefix passes + kman_finish; full:
        # every bit in global passes + kman_rle_* (kept for A/B runs)
        self.path = path
        self.work = None
        self.dev, self.k, self.mode, self.rc = dev, k, mode, rc
        n = len(text)
        self.n_bytes = n
        self.text = dev.alloc(n + 64)
        dev.upload(self.text, text)
        self.codes = dev.alloc(n + 64)
        self.rec_cap = n // 2 + 1
        self.rec_hdr = dev.alloc(8 * self.rec_cap)
        self.rec_seq = dev.alloc(8 * self.rec_cap)
        self.bound = max(1, n * (2 if rc else 1))
        self.pos_bytes = pos_bytes or (4 if 2 * n <= 0xFFFFFFFF else 8)
        want_pos = mode == "uniq"
        self.keys = dev.alloc(8 * self.bound)
        self.alt = dev.alloc(8 * self.bound)
        self.pos = dev.alloc(self.pos_bytes * self.bound) if want_pos else None
        self.pos_alt = dev.alloc(self.pos_bytes * self.bound) if want_pos else None
        self.hist = dev.alloc(8 * 256 * 8)
        self.out_keys = dev.alloc(8 * self.bound)
        self.count_bytes = 4 if self.bound <= 0xFFFFFFFF else 8
        self.out_vals = dev.alloc((self.pos_bytes if want_pos else self.count_bytes) * self.bound)
        self.lo_bit = split_bits(self.bound, 2 * k) if path == "split" else 0
        self.flags = flags_for(rc, want_pos) | N.KMAN_HIST_LO(self.lo_bit)
        self.n_kmers = 0
        self.n_out = 0
        self.n_bases = 0
        self.sorted_in_alt = False
        if self.path == "region":
            self._parse()
            wb = c_uint64(0)
            m = N.KMAN_FINISH_UNIQ if mode == "uniq" else N.KMAN_FINISH_COUNT
            r = N.lib().kman_groups_plan(self.n_bases, k, flags_for(rc, want_pos), m, byref(wb))
            if r == N.KMAN_EFALLBACK:
                self._to_split()
            else:
                N.check(dev.ctx, r, "kman_groups_plan")
                self.work = dev.alloc(int(wb.value))
                self.work_bytes = int(wb.value)

    def _to_split(self) -> None:
        """Switch to the prefix-split path with its own digit plan (the region
        path plans no prefix passes: lo_bit 0 would run every key bit through
        the global passes)."""
        self.path = "split"
        if self.work is not None:
            self.work.free()
            self.work = None
        self.lo_bit = split_bits(self.bound, 2 * self.k)
        self.flags = flags_for(self.rc, self.mode == "uniq") | N.KMAN_HIST_LO(self.lo_bit)

    def _parse(self) -> None:
        info = N.ParseInfo()
        N.check(self.dev.ctx, N.lib().kman_parse_fasta(self.dev.ctx, c_void_p(self.text.ptr), self.n_bytes,
                                                        c_void_p(self.codes.ptr), c_void_p(self.rec_hdr.ptr),
                                                        c_void_p(self.rec_seq.ptr), self.rec_cap, byref(info)),
                "kman_parse_fasta")
        self.n_bases = int(info.n_bases)

    def extract_only(self) -> int:
        """parse + extract (stream-order keys / pos in self.keys / self.pos)."""
        L, ctx = N.lib(), self.dev.ctx
        info = N.ParseInfo()
        N.check(ctx, L.kman_parse_fasta(ctx, c_void_p(self.text.ptr), self.n_bytes, c_void_p(self.codes.ptr),
                                        c_void_p(self.rec_hdr.ptr), c_void_p(self.rec_seq.ptr), self.rec_cap,
                                        byref(info)), "kman_parse_fasta")
        self.n_bases = int(info.n_bases)
        n = c_uint64(0)
        pos = c_void_p(self.pos.ptr) if self.pos else c_void_p(None)
        N.check(ctx, L.kman_extract(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k, self.flags,
                                    c_void_p(self.keys.ptr), pos, self.pos_bytes, self.bound, None, byref(n)),
                "kman_extract")
        self.n_kmers = int(n.value)
        return self.n_kmers

    def step(self) -> int:
        L, ctx = N.lib(), self.dev.ctx
        self._parse()
        if self.path == "region":
            m = N.KMAN_FINISH_UNIQ if self.mode == "uniq" else N.KMAN_FINISH_COUNT
            ob = self.count_bytes if self.mode == "count" else self.pos_bytes
            nk, no = c_uint64(0), c_uint64(0)
            r = L.kman_groups(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k, self.flags & 0xff, m,
                              c_void_p(self.work.ptr), self.work_bytes, c_void_p(self.out_keys.ptr),
                              c_void_p(self.out_vals.ptr), ob, byref(nk), byref(no))
            if r != N.KMAN_EFALLBACK:
                N.check(ctx, r, "kman_groups")
                self.n_kmers, self.n_out = int(nk.value), int(no.value)
                return self.n_kmers
            # a region overflowed (skewed input): the general path from here on
            self._to_split()
        n = c_uint64(0)
        res = c_int(0)
        pos = c_void_p(self.pos.ptr) if self.pos else c_void_p(None)
        vb = self.pos_bytes if self.pos else 0
        pos_alt = c_void_p(self.pos_alt.ptr if self.pos_alt else None)
        if self.path == "split":
            # extraction fused with the first prefix pass, then the other prefix passes
            N.check(ctx, L.kman_extract_sorted(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k,
                                               self.flags & 0xff, self.lo_bit, c_void_p(self.keys.ptr),
                                               c_void_p(self.alt.ptr), pos, pos_alt, self.pos_bytes, self.bound,
                                               byref(n), byref(res)), "kman_extract_sorted")
            self.n_kmers = int(n.value)
        else:
            N.check(ctx, L.kman_memset(ctx, c_void_p(self.hist.ptr), 0, 8 * 256 * 8), "memset")
            N.check(ctx, L.kman_extract(ctx, c_void_p(self.codes.ptr), self.n_bases, self.k, self.flags,
                                        c_void_p(self.keys.ptr), pos, self.pos_bytes, self.bound,
                                        c_void_p(self.hist.ptr), byref(n)), "kman_extract")
            self.n_kmers = int(n.value)
            N.check(ctx, L.kman_sort(ctx, c_void_p(self.keys.ptr), c_void_p(self.alt.ptr), pos, pos_alt, vb,
                                     self.n_kmers, 2 * self.k, c_void_p(self.hist.ptr), byref(res)), "kman_sort")
        self.sorted_in_alt = bool(res.value)
        skeys = self.alt if res.value else self.keys
        out = c_uint64(0)
        if self.path == "split":
            spos = self.pos_alt if res.value else self.pos
            other = self.keys if res.value else self.alt
            opos = self.pos if res.value else self.pos_alt
            mode = N.KMAN_FINISH_COUNT if self.mode == "count" else N.KMAN_FINISH_UNIQ
            ob = self.count_bytes if self.mode == "count" else self.pos_bytes
            N.check(ctx, L.kman_finish(ctx, c_void_p(skeys.ptr), c_void_p(other.ptr),
                                       c_void_p(spos.ptr if spos else None), c_void_p(opos.ptr if opos else None), vb,
                                       self.n_kmers, 2 * self.k, self.lo_bit, mode, c_void_p(self.out_keys.ptr),
                                       c_void_p(self.out_vals.ptr), ob, byref(out)), "kman_finish")
        elif self.mode == "count":
            N.check(ctx, L.kman_rle_count(ctx, c_void_p(skeys.ptr), self.n_kmers, c_void_p(self.out_keys.ptr),
                                          c_void_p(self.out_vals.ptr), self.count_bytes, byref(out)),
                    "kman_rle_count")
        else:
            spos = self.pos_alt if res.value else self.pos
            N.check(ctx, L.kman_rle_uniq(ctx, c_void_p(skeys.ptr), c_void_p(spos.ptr), self.pos_bytes,
                                         self.n_kmers, c_void_p(self.out_keys.ptr), c_void_p(self.out_vals.ptr),
                                         byref(out)), "kman_rle_uniq")
        self.n_out = int(out.value)
        return self.n_kmers

    @property
    def n_sorted(self) -> int:
        return self.n_kmers

    def timing(self, enable: bool) -> None:
        N.check(self.dev.ctx, N.lib().kman_timing_enable(self.dev.ctx, 1 if enable else 0), "timing")

    def timed(self, tag: str):
        n, ms = c_uint64(0), ctypes.c_double(0)
        N.check(self.dev.ctx, N.lib().kman_timing_query(self.dev.ctx, tag.encode(), byref(n), byref(ms)), "timing")
        return int(n.value), float(ms.value)

    def free(self) -> None:
        for b in (self.text, self.codes, self.rec_hdr, self.rec_seq, self.keys, self.alt, self.pos, self.pos_alt,
                  self.hist, self.out_keys, self.out_vals, self.work):
            if b is not None:
                b.free()

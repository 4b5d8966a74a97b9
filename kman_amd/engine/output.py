"""The output text: host formatters, the pipelined device writer, downloads and decoders."""

from __future__ import annotations

import ctypes
import os
from ctypes import byref, c_size_t, c_void_p
from typing import Optional

import numpy as np

from .. import _native as N
from .. import phases
from . import device
from .device import Device, DeviceBuffer, host_threads
from .parsed import Parsed
from .kmers import CountResult, UniqResult
from .words import WordsResult, nwords


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
        rows = max(1, min(n, device._FMT_SLICE // max(1, row_bytes)))
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
    stages = dev.pinned_stages(max(cap, device._FMT_SLICE + 16), NB)
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


def decode_key(key: int, k: int) -> str:
    """2-bit MSB-first key -> upper-case sequence."""
    return "".join("ACGT"[(int(key) >> (2 * (k - 1 - j))) & 3] for j in range(k))


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

#!/usr/bin/env python3
"""Time kman_cut_records, the kernels behind `kmer screen --reads-out` (HIP
events of kman_timing around the launches, tag "cut_records": 3 warm-up + 10
timed calls, pass 1, the scan and pass 2 together), beside a device-to-device
copy of as many bytes as the call writes on the same machine in the same run
(HIP events around kman_memcpy_d2d's stream are not kept by the library, so 10
copies are timed by the wall clock, one synchronisation at the end).

Three inputs of about --bytes of FASTQ text (default 256 MiB) each, every
second record listed:

  short   tests/fastq_cases.short_reads (25- to 150-base reads), whole records
  trim    the same reads, each cut to the middle half of its bases
  long    tests/fastq_cases.long_reads (10 000- to 30 000-base reads), whole

The text is tiled from a 2 MB (short) or 8 MB (long) piece of the builders'
output.  The output is checked against the plain-Python statement of
tests/reads_cases.py on the first piece, and its size on the whole."""
import argparse
import ctypes
import os
import sys
import time
from ctypes import byref, c_size_t, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import fastq_cases as fq  # noqa: E402
import reads_cases as rcs  # noqa: E402
from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

WARM, TIMED = 3, 10


def timed(dev, L, tag: bytes, call, per_call: int) -> float:
    """ms per call of the launches tagged `tag` over TIMED calls after WARM."""
    for _ in range(WARM):
        call()
    L.kman_timing_enable(dev.ctx, 1)
    for _ in range(TIMED):
        call()
    cnt, ms = c_uint64(), ctypes.c_double()
    L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(ms))
    L.kman_timing_enable(dev.ctx, 0)
    assert cnt.value == per_call * TIMED, (tag, cnt.value)
    return ms.value / TIMED


def copy_ms(dev, L, dst, src, nbytes: int) -> float:
    for _ in range(WARM):
        N.check(dev.ctx, L.kman_memcpy_d2d(dev.ctx, c_void_p(dst.ptr), c_void_p(src.ptr), nbytes), "d2d")
    N.check(dev.ctx, L.kman_sync(dev.ctx), "sync")
    t0 = time.perf_counter()
    for _ in range(TIMED):
        N.check(dev.ctx, L.kman_memcpy_d2d(dev.ctx, c_void_p(dst.ptr), c_void_p(src.ptr), nbytes), "d2d")
    N.check(dev.ctx, L.kman_sync(dev.ctx), "sync")
    return (time.perf_counter() - t0) * 1e3 / TIMED


def run_case(dev, L, label: str, piece: bytes, copies: int, trim: bool) -> str:
    off1 = np.array(rcs.fastq_offsets(piece), np.uint64)
    R1, n1 = len(off1) - 1, len(piece)
    keep1 = (np.arange(R1) % 2 == 0).astype(np.uint8)
    start1 = end1 = None
    if trim:
        bases = np.array([len(rcs.record_lines(rec)[1]) for rec in rcs.records_of(piece, off1)], np.uint64)
        start1, end1 = bases // np.uint64(4), bases - bases // np.uint64(4)
    want1 = rcs.cut_trimmed(piece, off1, start1, end1, keep1) if trim else rcs.cut_whole(piece, off1, keep1)

    n, R = n1 * copies, R1 * copies
    off = np.empty(R + 1, np.uint64)
    for c in range(copies):
        off[c * R1:(c + 1) * R1] = off1[:-1] + np.uint64(c * n1)
    off[R] = n
    flags = N.KMAN_CUT_TRIM if trim else 0
    need = c_uint64()
    assert L.kman_cut_records_plan(R, flags, byref(need)) == N.KMAN_OK
    size = len(want1) * copies
    bufs = [dev.alloc(n + 64), dev.alloc(8 * (R + 1)), dev.alloc(R), dev.alloc(need.value), dev.alloc(size + 16),
            dev.alloc(size + 16)]
    d_text, d_off, d_keep, d_work, d_out, d_out2 = bufs
    for c in range(copies):
        dev.upload(d_text, piece, c * n1)
    dev.upload(d_off, off)
    dev.upload(d_keep, np.tile(keep1, copies))
    d_start = d_end = None
    if trim:
        d_start, d_end = dev.alloc(8 * R), dev.alloc(8 * R)
        bufs += [d_start, d_end]
        dev.upload(d_start, np.tile(start1, copies))
        dev.upload(d_end, np.tile(end1, copies))
    used = c_size_t()

    def call():
        N.check(dev.ctx, L.kman_cut_records(
            dev.ctx, c_void_p(d_text.ptr), n, c_void_p(d_off.ptr), R, c_void_p(d_keep.ptr),
            c_void_p(d_start.ptr) if trim else None, c_void_p(d_end.ptr) if trim else None, flags,
            c_void_p(d_work.ptr), need.value, c_void_p(d_out.ptr), size, byref(used)), "kman_cut_records")

    k_ms = timed(dev, L, b"cut_records", call, 2)
    assert used.value == size, (used.value, size)
    c_ms = copy_ms(dev, L, d_out2, d_out, size)
    got = dev.download(d_out, len(want1), np.uint8).tobytes()
    assert got == want1, "the first piece differs from the statement"
    last = dev.download(d_out, len(want1), np.uint8, size - len(want1)).tobytes()
    assert last == want1, "the last piece differs from the statement"
    for b in bufs:
        b.free()
    return ("%-5s %4d MB of text, %8d records, %4d MB written, work buffer %5.1f MB | cut_records %8.3f ms "
            "(%6.1f GB/s written), copy of the same bytes %7.3f ms (%6.1f GB/s written), cut_records / copy %.2f" % (
                label, n >> 20, R, size >> 20, need.value / 2 ** 20, k_ms, size / k_ms / 1e6, c_ms,
                size / c_ms / 1e6, k_ms / c_ms))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bytes", type=int, default=1 << 28)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    lines = ["tile %d output bytes, %d segments staged, %d + %d timed calls, every second record listed" % (
        N.KMAN_CUT_TILE, N.KMAN_CUT_SEG_CAP, WARM, TIMED)]
    short = fq.short_reads()
    long_ = fq.long_reads(8_000_000)
    for label, piece, trim in (("short", short, False), ("trim", short, True), ("long", long_, False)):
        lines.append(run_case(dev, L, label, piece, max(1, a.bytes // len(piece)), trim))
        print(lines[-1], flush=True)
    dev.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time kman_record_runs, the kernels behind `kmer screen --solid` (HIP
events of kman_timing around the launches, tag "record_runs": 3 warm-up + 10
timed calls), beside a device-to-device copy of the same 4 * n_bases bytes on
the same machine in the same run (HIP events around kman_memcpy_d2d's stream
are not kept by the library, so 10 copies are timed by the wall clock, one
synchronisation at the end).

Two inputs of --bases words (default 2^28) each:

  reads   records of 150 bases: the last 20 words of a record are
          KMAN_WC_NONE (k = 21), one read in ten has 21 weak words (one wrong
          base) somewhere, every other word is solid
  one     one record of --bases words, every word solid but one in the
          middle: pass 1 finds no break in most tiles and reads them whole,
          the two runs reach over half the tiles each

The results are checked: every read against numpy on a sample, the one
record's two runs exactly.  The work buffer is kman_record_runs_plan's."""
import argparse
import ctypes
import os
import sys
import time
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

WARM, TIMED = 3, 10
READ, K = 150, 21


def timed(dev, L, tag: bytes, call) -> float:
    """ms per call of the launches tagged `tag` over TIMED calls after WARM."""
    for _ in range(WARM):
        call()
    L.kman_timing_enable(dev.ctx, 1)
    for _ in range(TIMED):
        call()
    cnt, ms = c_uint64(), ctypes.c_double()
    L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(ms))
    L.kman_timing_enable(dev.ctx, 0)
    assert cnt.value == TIMED, (tag, cnt.value)
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


def read_words(n_reads: int, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    w = np.full((n_reads, READ), 5, np.uint32)
    w[:, READ - K + 1:] = N.KMAN_WC_NONE
    bad = np.flatnonzero(rng.random(n_reads) < 0.1)
    at = rng.integers(0, READ - K + 1, len(bad))
    for d in range(K):  # the K windows over one wrong base (those before the read's first base do not exist)
        col = at - d
        ok = col >= 0
        w[bad[ok], col[ok]] = 1
    return w


def run_case(dev, L, label: str, words: np.ndarray, rec_seq: np.ndarray, min_count: int, check) -> str:
    n, R = int(words.size), int(rec_seq.size)
    need = c_uint64()
    assert L.kman_record_runs_plan(n, R, byref(need)) == N.KMAN_OK
    wc, wc2 = dev.alloc(4 * n), dev.alloc(4 * n)
    step = 1 << 24
    flat = words.reshape(-1)
    for i in range(0, n, step):
        dev.upload(wc, np.ascontiguousarray(flat[i:i + step]), 4 * i)
    rec, work, out = dev.alloc(8 * R), dev.alloc(need.value), dev.alloc(16 * R)
    dev.upload(rec, rec_seq)

    def call():
        N.check(dev.ctx, L.kman_record_runs(dev.ctx, c_void_p(wc.ptr), n, c_void_p(rec.ptr), R, min_count,
                                            c_void_p(work.ptr), need.value, c_void_p(out.ptr)), "kman_record_runs")

    r_ms = timed(dev, L, b"record_runs", call)
    c_ms = copy_ms(dev, L, wc2, wc, 4 * n)
    got = dev.download(out, 2 * R, np.uint64).reshape(2, R)
    check(got)
    for b in (wc, wc2, rec, work, out):
        b.free()
    return ("%-5s %10d words in %8d records, work buffer %5.1f MB | record_runs %8.3f ms (%6.1f GB/s of words), "
            "copy of %d MB %7.3f ms (%6.1f GB/s read + written), record_runs / copy %.2f" % (
                label, n, R, need.value / 2 ** 20, r_ms, 4 * n / r_ms / 1e6, 4 * n >> 20, c_ms, 8 * n / c_ms / 1e6,
                r_ms / c_ms))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=1 << 28)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    lines = ["tile %d bases, %d + %d timed calls, min_count 3" % (N.KMAN_RUNS_TILE, WARM, TIMED)]

    n_reads = a.bases // READ
    words = read_words(n_reads)
    rec_seq = np.arange(n_reads, dtype=np.uint64) * np.uint64(READ)

    def check_reads(got):
        solid = (words != N.KMAN_WC_NONE) & (words >= 3)
        for r in range(0, n_reads, max(1, n_reads // 2000)):
            best_s = best_l = 0
            i = 0
            row = solid[r]
            while i < READ:
                if not row[i]:
                    i += 1
                    continue
                j = i
                while j < READ and row[j]:
                    j += 1
                if j - i > best_l:
                    best_s, best_l = i, j - i
                i = j
            assert (int(got[0, r]), int(got[1, r])) == (best_s, best_l), r
        assert int(got[1].max()) == READ - K + 1

    lines.append(run_case(dev, L, "reads", words, rec_seq, 3, check_reads))
    print(lines[-1], flush=True)
    del words

    n = a.bases
    one = np.full(n, 5, np.uint32)
    mid = n // 2 + 1234
    one[mid] = N.KMAN_WC_NONE

    def check_one(got):
        assert (int(got[0, 0]), int(got[1, 0])) == (0, mid), got[:, 0]  # (the left run is the longer one)

    lines.append(run_case(dev, L, "one", one, np.zeros(1, np.uint64), 3, check_one))
    print(lines[-1], flush=True)
    dev.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

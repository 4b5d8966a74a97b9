#!/usr/bin/env python3
"""Time kman_match_counts (HIP events of kman_timing around the split and the
tile kernel, 5 warm-up + 20 timed calls) against a device-to-device copy that
moves the same number of bytes, and `kmer sets --op subtract` file to file
against the two `kmer count` runs that the same question cost before.

Tables (u32 counts, u32 out): A[i] = 4 ra i, B[j] = 4 rb j + 2 bit(j) with
bit(j) the top bit of a hash of j, ra = max(1, nb / na), rb = max(1, na / nb):
both strictly ascending, and half the rows of the smaller table (of both, at
na = nb) have their partner in the other.  Shapes: na = nb = --rows / 10 and
--rows, na : nb = 1 : 100 and 100 : 1 with the larger table of --rows rows.

The yardstick: the match reads 8 (+ 4: A's counts, not read by RIGHT) bytes
per A row and 8 + 4 per B row and writes 4 per A row; a copy of X bytes reads
X and writes X, so it is timed at X = half the bytes the match moves.
kman_memcpy_d2d has no event pair of its own: 20 copies are queued and timed
by the wall clock around them and one kman_sync."""
import argparse
import ctypes
import os
import subprocess
import sys
import time
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import numpy as np  # noqa: E402

from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

WARM, TIMED = 5, 20
CHUNK = 1 << 26


def fill_keys(dev, buf, n: int, step: int, hashed: bool) -> None:
    """keys[i] = step * i (+ 2 * top bit of a hash of i when hashed), uploaded in chunks."""
    for at in range(0, n, CHUNK):
        i = np.arange(at, min(at + CHUNK, n), dtype=np.uint64)
        k = i * np.uint64(step)
        if hashed:
            k += ((i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63)) << np.uint64(1)
        dev.upload(buf, k, 8 * at)


def fill_counts(dev, buf, n: int) -> None:
    c = (np.arange(CHUNK, dtype=np.uint32) % np.uint32(7)) + np.uint32(1)
    for at in range(0, n, CHUNK):
        dev.upload(buf, c[:min(CHUNK, n - at)], 4 * at)


def rows_bench(rows: int) -> None:
    dev = engine.Device(0)
    L = N.lib()
    small = max(1, rows // 100)
    big_a, big_b = (dev.alloc(8 * rows), dev.alloc(4 * rows)), (dev.alloc(8 * rows), dev.alloc(4 * rows))
    few_a, few_b = (dev.alloc(8 * small), dev.alloc(4 * small)), (dev.alloc(8 * small), dev.alloc(4 * small))
    out, dst = dev.alloc(4 * rows), dev.alloc(8 * rows)
    fill_keys(dev, big_a[0], rows, 4, False)
    fill_keys(dev, big_b[0], rows, 4, True)
    fill_keys(dev, few_a[0], small, 4 * (rows // small), False)
    fill_keys(dev, few_b[0], small, 4 * (rows // small), True)
    for t, n in ((big_a, rows), (big_b, rows), (few_a, small), (few_b, small)):
        fill_counts(dev, t[1], n)
    print("kman_match_counts, tile %d merged rows, u32 counts, u32 out; %d + %d timed calls" % (
        N.KMAN_MATCH_TILE, WARM, TIMED), flush=True)

    def timed_match(a, na, b, nb, op):
        args = (dev.ctx, c_void_p(a[0].ptr), c_void_p(a[1].ptr), 4, na, c_void_p(b[0].ptr), c_void_p(b[1].ptr), 4, nb,
                op, c_void_p(out.ptr), 4)
        for _ in range(WARM):
            N.check(dev.ctx, L.kman_match_counts(*args), "kman_match_counts")
        L.kman_timing_enable(dev.ctx, 1)
        for _ in range(TIMED):
            N.check(dev.ctx, L.kman_match_counts(*args), "kman_match_counts")
        cnt, ms = c_uint64(), ctypes.c_double()
        L.kman_timing_query(dev.ctx, b"match_counts", byref(cnt), byref(ms))
        L.kman_timing_enable(dev.ctx, 0)
        assert cnt.value == TIMED
        return ms.value / TIMED

    def timed_copy(nbytes):
        nbytes = min(nbytes, 8 * rows)
        for _ in range(WARM):
            L.kman_memcpy_d2d(dev.ctx, c_void_p(dst.ptr), c_void_p(big_a[0].ptr), nbytes)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(TIMED):
            L.kman_memcpy_d2d(dev.ctx, c_void_p(dst.ptr), c_void_p(big_a[0].ptr), nbytes)
        dev.sync()
        return nbytes, (time.perf_counter() - t0) * 1e3 / TIMED

    shapes = (
        ("na = nb, half shared", big_a, rows // 10, big_b, rows // 10),
        ("na = nb, half shared", big_a, rows, big_b, rows),
        ("na : nb = 1 : 100", few_a, small, big_b, rows),
        ("na : nb = 100 : 1", big_a, rows, few_b, small),
    )
    for name, a, na, b, nb in shapes:
        for op, opname in ((N.KMAN_MATCH_RIGHT, "RIGHT"), (N.KMAN_MATCH_SUM, "SUM")):
            ms = timed_match(a, na, b, nb, op)
            hits = int((dev.download(out, min(na, 1 << 20), np.uint32) != 0).sum())
            moved = na * (8 + (0 if op == N.KMAN_MATCH_RIGHT else 4)) + nb * 12 + na * 4
            cb, cms = timed_copy(moved // 2)
            mrate, crate = moved / ms / 1e6, 2 * cb / cms / 1e6
            print("%-22s na %10d nb %10d %-5s %8.3f ms %7.1f GB/s (%.2f GB; matched %d of the first %d rows) | "
                  "d2d copy of %5.2f GB %7.3f ms %7.1f GB/s | match / copy rate %.2f" % (
                      name, na, nb, opname, ms, mrate, moved / 1e9, hits, min(na, 1 << 20), cb / 1e9, cms, crate,
                      mrate / crate), flush=True)
    for t in (big_a, big_b, few_a, few_b):
        t[0].free()
        t[1].free()
    out.free()
    dst.free()
    dev.close()


def e2e(bases: int, k: int, tmp: str) -> None:
    import inputs

    a = os.path.join(tmp, "match_bench_a_%d.fa" % bases)
    b = os.path.join(tmp, "match_bench_b_%d.fa" % bases)
    text = inputs.syn_numpy(bases, 1)
    with open(a, "wb") as fh:
        fh.write(text)
    with open(b, "wb") as fh:  # the first half of A's lines, then as many bases of its own
        fh.write(text[:text.rindex(b"\n", 0, len(text) // 2) + 1])
        fh.write(inputs.syn_numpy(bases // 2, 2))
    del text
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = os.path.join(tmp, "match_bench_out.txt")

    def run(*argv):
        t0 = time.perf_counter()
        subprocess.run([sys.executable, "-m", "kman_amd"] + [str(x) for x in argv], check=True, env=env, cwd=ROOT,
                       stdout=subprocess.DEVNULL)
        dt = time.perf_counter() - t0
        size = os.path.getsize(out)
        os.remove(out)
        return dt, size

    for rep in range(2):
        ta, sa = run("count", a, out, k)
        tb, sb = run("count", b, out, k)
        print("count A %.2f s (%d bytes) + count B %.2f s (%d bytes) = %.2f s, before any host join; %d bases k=%d" % (
            ta, sa, tb, sb, ta + tb, bases, k), flush=True)
        ts, ss = run("sets", a, b, out, k, "--op", "subtract")
        print("sets --op subtract A B, file to file %.2f s, output %d bytes" % (ts, ss), flush=True)
    os.remove(a)
    os.remove(b)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000_000, help="rows of the larger shapes")
    ap.add_argument("--e2e-bases", type=int, default=100_000_000, help="0: skip the file-to-file runs")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    if a.rows:
        rows_bench(a.rows)
    if a.e2e_bases:
        e2e(a.e2e_bases, a.k, a.tmp)

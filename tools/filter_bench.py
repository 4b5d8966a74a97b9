#!/usr/bin/env python3
"""Time kman_filter_counts (HIP events of kman_timing, 5 warm-up + 20 timed
launches) at three keep rates against a device-to-device copy that moves the
same number of bytes, and `kmer count` file to file with and without -L 2.

The count rows of the bench's 1 GB k=21 input are all singletons (4^21 keys,
10^9 k-mers), so the rows are synthetic: --rows (default 10^9) rows of
(iota key, u32 count in {1, 2} by a hash of the row), filtered out of place.

The yardstick: the filter reads 12 B per row and writes 12 B per kept row; a
copy of X bytes reads X and writes X, so X = 6 (rows + kept).  kman_memcpy_d2d
has no event pair of its own: 20 copies are queued and timed by the wall
clock around them and one kman_sync (a copy takes milliseconds, a launch
microseconds)."""
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
U64 = (1 << 64) - 1


def rows_bench(n: int) -> None:
    dev = engine.Device(0)
    L = N.lib()
    keys, counts = dev.alloc(8 * n), dev.alloc(4 * n)
    okeys, ocounts = dev.alloc(8 * n), dev.alloc(4 * n)
    N.check(dev.ctx, L.kman_iota_u64(dev.ctx, c_void_p(keys.ptr), n), "iota")
    chunk = 1 << 26
    i = np.arange(chunk, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(63)
    c = (h + np.uint64(1)).astype(np.uint32)  # 1 or 2, about half each
    for at in range(0, n, chunk):
        m = min(chunk, n - at)
        dev.upload(counts, c[:m], 4 * at)
    print("rows %d (tile %d, %d tiles), u32 counts in {1, 2}, out of place unless said" % (
        n, N.KMAN_FILTER_TILE, -(-n // N.KMAN_FILTER_TILE)), flush=True)

    def timed_filter(lo, hi, ok_, oc_):
        out = c_uint64(0)
        args = (dev.ctx, c_void_p(keys.ptr), 1, n, c_void_p(counts.ptr), 4, n, lo, hi, c_void_p(ok_), c_void_p(oc_),
                byref(out))
        for _ in range(WARM):
            N.check(dev.ctx, L.kman_filter_counts(*args), "kman_filter_counts")
        L.kman_timing_enable(dev.ctx, 1)
        for _ in range(TIMED):
            N.check(dev.ctx, L.kman_filter_counts(*args), "kman_filter_counts")
        cnt, ms = c_uint64(), ctypes.c_double()
        L.kman_timing_query(dev.ctx, b"filter_counts", byref(cnt), byref(ms))
        L.kman_timing_enable(dev.ctx, 0)
        assert cnt.value == TIMED
        return int(out.value), ms.value / TIMED

    def timed_copy(nbytes):
        nbytes = min(nbytes, 8 * n)
        for _ in range(WARM):
            L.kman_memcpy_d2d(dev.ctx, c_void_p(okeys.ptr), c_void_p(keys.ptr), nbytes)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(TIMED):
            L.kman_memcpy_d2d(dev.ctx, c_void_p(okeys.ptr), c_void_p(keys.ptr), nbytes)
        dev.sync()
        return nbytes, (time.perf_counter() - t0) * 1e3 / TIMED

    for name, lo, hi, ok_, oc_ in (
        ("keep ~0 %", 3, U64, okeys.ptr, ocounts.ptr),
        ("keep ~50 %", 2, U64, okeys.ptr, ocounts.ptr),
        ("keep 100 % (hi just above the largest count)", 1, 3, okeys.ptr, ocounts.ptr),
        ("count only (NULL outputs), ~50 %", 2, U64, None, None),
        ("in place, keep ~0 %", 3, U64, keys.ptr, counts.ptr),
        ("in place, keep 100 %", 1, 3, keys.ptr, counts.ptr),
    ):
        kept, ms = timed_filter(lo, hi, ok_, oc_)
        moved = (4 * n) if ok_ is None else 12 * (n + kept)
        cb, cms = timed_copy(moved // 2)
        # (a copy larger than the key array is cut to it: the rate is what is compared)
        frate, crate = moved / ms / 1e6, 2 * cb / cms / 1e6
        print("%-46s kept %10d  filter %7.3f ms  %7.1f GB/s | d2d copy of %5.2f GB %7.3f ms %7.1f GB/s | "
              "filter/copy time at equal bytes %.2f" % (name, kept, ms, frate, cb / 1e9, cms, crate, crate / frate),
              flush=True)
    for b in (keys, counts, okeys, ocounts):
        b.free()
    dev.close()


def e2e(bases: int, k: int, tmp: str) -> None:
    import inputs

    src = os.path.join(tmp, "filter_bench_%d.fa" % bases)
    with open(src, "wb") as fh:
        fh.write(inputs.syn_numpy(bases, 1))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for flags in ([], ["-L", "2"], [], ["-L", "2"]):
        out = os.path.join(tmp, "filter_bench_out.txt")
        t0 = time.perf_counter()
        subprocess.run([sys.executable, "-m", "kman_amd", "count", src, out, str(k)] + flags, check=True, env=env,
                       cwd=ROOT, stdout=subprocess.DEVNULL)
        dt = time.perf_counter() - t0
        print("count %d bases k=%d %-6s file to file %.2f s, output %d bytes" % (
            bases, k, " ".join(flags) or "(all)", dt, os.path.getsize(out)), flush=True)
        os.remove(out)
    os.remove(src)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--e2e-bases", type=int, default=100_000_000, help="0: skip the file-to-file runs")
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--tmp", default="/tmp")
    a = ap.parse_args()
    rows_bench(a.rows)
    if a.e2e_bases:
        e2e(a.e2e_bases, a.k, a.tmp)

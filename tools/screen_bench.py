#!/usr/bin/env python3
"""Time kman_screen_records (HIP events of kman_timing around the kernel, tag
"screen", 5 warm-up + 20 timed calls) on synthetic 150-base reads against
tables of about 10^6, 10^8 and 10^9 rows at hit rates of about 1, 0.5 and 0,
beside kman_count_kmers over the same codes: the same read and roll with no
lookup, the floor for this kernel.

Reads: --reads records of 150 random ACGT bases.  Tables (u32 counts), for a
target of R rows with kt = round(log4 R):
  hit ~1    every kt-mer: 4^kt rows, keys 0, 1, 2, ..          looked up at k = kt
  hit ~0.5  every second kt-mer: 4^kt / 2 rows, keys 0, 2, ..   looked up at k = kt
  hit ~0    4^kt rows spread evenly over the 21-mers            looked up at k = 21
so the row counts are 4^10, 4^13 and 4^15 (halved at 0.5), not the round
figures.  The hit rate that is printed is the measured one (hits / windows).

kman_count_kmers has no event pair of its own: 20 calls are timed by the wall
clock (each call synchronises and brings 8 bytes back)."""
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

WARM, TIMED = 5, 20
CHUNK = 1 << 26
READ = 150


def fill_keys(dev, buf, n: int, step: int) -> None:
    """keys[i] = step * i, uploaded in chunks."""
    for at in range(0, n, CHUNK):
        i = np.arange(at, min(at + CHUNK, n), dtype=np.uint64)
        dev.upload(buf, i * np.uint64(step), 8 * at)


def fill_counts(dev, buf, n: int) -> None:
    c = (np.arange(min(CHUNK, n), dtype=np.uint32) % np.uint32(7)) + np.uint32(1)
    for at in range(0, n, CHUNK):
        dev.upload(buf, c[:min(CHUNK, n - at)], 4 * at)


def make_reads(dev, n_reads: int, seed: int = 1):
    """(codes buffer, rec_seq buffer, n_bases): the parsers' layout."""
    rng = np.random.default_rng(seed)
    n = n_reads * READ
    codes = dev.alloc(n + 64)
    per = max(1, CHUNK // READ)
    for r0 in range(0, n_reads, per):
        m = min(per, n_reads - r0)
        c = rng.integers(0, 4, (m, READ), dtype=np.uint8)
        c[:, 0] |= 8  # a record's first base
        dev.upload(codes, c.reshape(-1), r0 * READ)
    dev.upload(codes, np.full(64, 4, np.uint8), n)
    rec = dev.alloc(8 * n_reads)
    dev.upload(rec, np.arange(n_reads, dtype=np.uint64) * np.uint64(READ))
    return codes, rec, n


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=2_000_000, help="150-base reads")
    ap.add_argument("--rows", type=float, nargs="+", default=[1e6, 1e8, 1e9], help="target table rows")
    ap.add_argument("--index-bits", type=int, default=None, help="default: engine.default_index_bits")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    codes, rec, n_bases = make_reads(dev, a.reads)
    out = dev.alloc(24 * a.reads)
    print("kman_screen_records, tile %d windows, %d reads of %d bases (%d bases), u32 counts; %d + %d timed calls" % (
        N.KMAN_SCREEN_TILE, a.reads, READ, n_bases, WARM, TIMED), flush=True)

    def floor_ms(k: int) -> float:
        nk = c_uint64()
        for _ in range(WARM):
            N.check(dev.ctx, L.kman_count_kmers(dev.ctx, c_void_p(codes.ptr), n_bases, k, 0, byref(nk)), "count")
        t0 = time.perf_counter()
        for _ in range(TIMED):
            N.check(dev.ctx, L.kman_count_kmers(dev.ctx, c_void_p(codes.ptr), n_bases, k, 0, byref(nk)), "count")
        dt = (time.perf_counter() - t0) * 1e3 / TIMED
        assert nk.value == a.reads * (READ - k + 1)
        return dt

    floors = {}
    for target in a.rows:
        kt = int(round(np.log(target) / np.log(4)))
        full = 4 ** kt
        for label, k, nt, step in (("hit ~1", kt, full, 1), ("hit ~0.5", kt, full // 2, 2),
                                   ("hit ~0", 21, full, 4 ** 21 // full)):
            keys, counts = dev.alloc(8 * nt), dev.alloc(4 * nt)
            fill_keys(dev, keys, nt, step)
            fill_counts(dev, counts, nt)
            bits = a.index_bits or engine.default_index_bits(nt, k)
            bits = min(bits, 2 * k)
            index = dev.alloc(8 * ((1 << bits) + 1))
            N.check(dev.ctx, L.kman_table_index(dev.ctx, c_void_p(keys.ptr), nt, k, bits, c_void_p(index.ptr)),
                    "kman_table_index")
            args = (dev.ctx, c_void_p(codes.ptr), n_bases, k, 0, c_void_p(rec.ptr), a.reads, c_void_p(keys.ptr),
                    c_void_p(counts.ptr), 4, nt, c_void_p(index.ptr), bits, c_void_p(out.ptr))
            for _ in range(WARM):
                N.check(dev.ctx, L.kman_screen_records(*args), "kman_screen_records")
            L.kman_timing_enable(dev.ctx, 1)
            for _ in range(TIMED):
                N.check(dev.ctx, L.kman_screen_records(*args), "kman_screen_records")
            cnt, ms = c_uint64(), ctypes.c_double()
            L.kman_timing_query(dev.ctx, b"screen", byref(cnt), byref(ms))
            L.kman_timing_enable(dev.ctx, 0)
            assert cnt.value == TIMED
            ms = ms.value / TIMED
            st = dev.download(out, 3 * a.reads, np.uint64).reshape(3, a.reads)
            windows, hits = int(st[0].sum()), int(st[1].sum())
            assert windows == a.reads * (READ - k + 1)
            if k not in floors:
                floors[k] = floor_ms(k)
            print("%-9s k %2d rows %11d index bits %2d (%.1f rows / bucket) | %9.3f ms %8.1f M windows/s, measured "
                  "hit rate %.4f | count_kmers %8.3f ms %9.1f M windows/s | screen / floor time %.1f" % (
                      label, k, nt, bits, nt / (1 << bits), ms, windows / ms / 1e3, hits / windows, floors[k],
                      windows / floors[k] / 1e3, ms / floors[k]), flush=True)
            for b in (keys, counts, index):
                b.free()
    for b in (codes, rec, out):
        b.free()
    dev.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the two kernels behind `kmer screen --median` (HIP events of
kman_timing around the launches, 5 warm-up + 20 timed calls):

  kman_window_counts (tag "window_counts") beside kman_screen_records (tag
  "screen") on the same reads, table and index in the same run: the lookups
  are the same, the per-record reduction is replaced by a 4 B store per window.

  kman_record_quantile (tag "record_quantile") on those words beside a
  kman_memcpy_d2d of the same 4 * n_bases bytes, its floor: every word is read
  once and almost nothing is written.  The copy has no event pair of its own:
  20 copies are timed by the wall clock, one synchronisation at the end.

Reads: --reads records of 150 random ACGT bases (tools/screen_bench.py's).
Tables (u32 counts): 4^10 = 1.05 x 10^6 and 4^13 = 6.7 x 10^7 rows, each looked
up at k = kt with every kt-mer a row (hit ~1) and at k = 21 with the rows
spread evenly over the 21-mers (hit ~0).

The long path: --long-records records of --long-bases words each (random
words, a fifth KMAN_WC_NONE), timed by the wall clock per call (list, gather,
kman_sort, pick) with the event times of "record_quantile" and
"record_quantile_long" beside it."""
import argparse
import ctypes
import os
import sys
import time
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402
from screen_bench import READ, fill_counts, fill_keys, make_reads  # noqa: E402

WARM, TIMED = 5, 20


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


def plan_bytes(L, n_long: int, n_values: int) -> int:
    out = c_uint64()
    assert L.kman_record_quantile_plan(n_long, n_values, byref(out)) == N.KMAN_OK
    return out.value


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=2_000_000, help="150-base reads")
    ap.add_argument("--kt", type=int, nargs="+", default=[10, 13], help="tables of 4^kt rows")
    ap.add_argument("--long-records", type=int, default=64)
    ap.add_argument("--long-bases", type=int, default=4_000_000)
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    codes, rec, n_bases = make_reads(dev, a.reads)
    out = dev.alloc(24 * a.reads)
    wc, wc2 = dev.alloc(4 * n_bases), dev.alloc(4 * n_bases)
    q = dev.alloc(4 * a.reads)
    work_bytes = plan_bytes(L, 0, 0)
    work = dev.alloc(work_bytes)
    print("tile %d windows, chunk %d bases, %d reads of %d bases (%d bases), u32 counts; %d + %d timed calls" % (
        N.KMAN_SCREEN_TILE, N.KMAN_QUANTILE_TILE, a.reads, READ, n_bases, WARM, TIMED), flush=True)
    for kt in a.kt:
        full = 4 ** kt
        for label, k, nt, step in (("hit ~1", kt, full, 1), ("hit ~0", 21, full, 4 ** 21 // full)):
            keys, counts = dev.alloc(8 * nt), dev.alloc(4 * nt)
            fill_keys(dev, keys, nt, step)
            fill_counts(dev, counts, nt)
            bits = min(engine.default_index_bits(nt, k), 2 * k)
            index = dev.alloc(8 * ((1 << bits) + 1))
            N.check(dev.ctx, L.kman_table_index(dev.ctx, c_void_p(keys.ptr), nt, k, bits, c_void_p(index.ptr)),
                    "kman_table_index")
            table = (c_void_p(keys.ptr), c_void_p(counts.ptr), 4, nt, c_void_p(index.ptr), bits)
            s_ms = timed(dev, L, b"screen", lambda: N.check(dev.ctx, L.kman_screen_records(
                dev.ctx, c_void_p(codes.ptr), n_bases, k, 0, c_void_p(rec.ptr), a.reads, *table, c_void_p(out.ptr)),
                "kman_screen_records"))
            w_ms = timed(dev, L, b"window_counts", lambda: N.check(dev.ctx, L.kman_window_counts(
                dev.ctx, c_void_p(codes.ptr), n_bases, k, 0, *table, c_void_p(wc.ptr)), "kman_window_counts"))
            st = dev.download(out, 3 * a.reads, np.uint64).reshape(3, a.reads)
            windows, hits = int(st[0].sum()), int(st[1].sum())
            words = dev.download(wc, n_bases, np.uint32)
            valid = words != N.KMAN_WC_NONE
            assert int(valid.sum()) == windows and int(np.count_nonzero(words[valid])) == hits

            def quantile():
                # (d_wc is scratch after a call: each one runs on a fresh copy)
                N.check(dev.ctx, L.kman_memcpy_d2d(dev.ctx, c_void_p(wc2.ptr), c_void_p(wc.ptr), 4 * n_bases), "d2d")
                N.check(dev.ctx, L.kman_record_quantile(dev.ctx, c_void_p(wc2.ptr), n_bases, c_void_p(rec.ptr),
                                                        a.reads, 1, 2, c_void_p(work.ptr), work_bytes,
                                                        c_void_p(q.ptr)), "kman_record_quantile")

            q_ms = timed(dev, L, b"record_quantile", quantile)
            c_ms = copy_ms(dev, L, wc2, wc, 4 * n_bases)
            med = dev.download(q, a.reads, np.uint32)
            some = np.arange(0, a.reads, max(1, a.reads // 1000))
            for r in some:  # a thousand records against numpy
                v = np.sort(words[r * READ:(r + 1) * READ][valid[r * READ:(r + 1) * READ]])
                assert med[r] == v[(len(v) - 1) // 2], r
            print("%-7s k %2d rows %9d index bits %2d hit rate %.4f | screen %8.3f ms, window_counts %8.3f ms "
                  "(%8.1f M windows/s), window_counts / screen %.2f | record_quantile %8.3f ms (%6.1f GB/s of words), "
                  "copy of %d MB %7.3f ms, record_quantile / copy %.1f" % (
                      label, k, nt, bits, hits / windows, s_ms, w_ms, windows / w_ms / 1e3, w_ms / s_ms, q_ms,
                      4 * n_bases / q_ms / 1e6, 4 * n_bases >> 20, c_ms, q_ms / c_ms), flush=True)
            for b in (keys, counts, index):
                b.free()
    for b in (codes, rec, out, wc, wc2, q, work):
        b.free()

    # ---- the long path
    R, B = a.long_records, a.long_bases
    n = R * B
    rng = np.random.default_rng(2)
    one = rng.integers(0, 1000, B, dtype=np.uint64).astype(np.uint32)
    one[rng.random(B) < 0.2] = N.KMAN_WC_NONE
    src, dst = dev.alloc(4 * n), dev.alloc(4 * n)
    for r in range(R):
        dev.upload(src, one, 4 * r * B)
    rec = dev.alloc(8 * R)
    dev.upload(rec, np.arange(R, dtype=np.uint64) * np.uint64(B))
    q = dev.alloc(max(16, 4 * R))
    work_bytes = plan_bytes(L, R, n)
    work = dev.alloc(work_bytes)

    def long_call():
        N.check(dev.ctx, L.kman_memcpy_d2d(dev.ctx, c_void_p(dst.ptr), c_void_p(src.ptr), 4 * n), "d2d")
        N.check(dev.ctx, L.kman_sync(dev.ctx), "sync")
        t0 = time.perf_counter()
        N.check(dev.ctx, L.kman_record_quantile(dev.ctx, c_void_p(dst.ptr), n, c_void_p(rec.ptr), R, 1, 2,
                                                c_void_p(work.ptr), work_bytes, c_void_p(q.ptr)),
                "kman_record_quantile")
        return (time.perf_counter() - t0) * 1e3

    for _ in range(WARM):
        long_call()
    L.kman_timing_enable(dev.ctx, 1)
    wall = sum(long_call() for _ in range(TIMED)) / TIMED
    tags = {}
    for tag in (b"record_quantile", b"record_quantile_long"):
        cnt, ms = c_uint64(), ctypes.c_double()
        L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(ms))
        tags[tag] = ms.value / TIMED
    L.kman_timing_enable(dev.ctx, 0)
    c_ms = copy_ms(dev, L, dst, src, 4 * n)
    v = np.sort(one[one != N.KMAN_WC_NONE])
    assert np.all(dev.download(q, R, np.uint32) == v[(len(v) - 1) // 2])
    print("long path: %d records of %d words (%d MB), work buffer %d MB | %9.3f ms per call by the wall clock "
          "(%.2f GB/s of words); events: list kernel %.3f ms, gather + pick %.3f ms, the rest kman_sort and the host "
          "| copy %.3f ms, call / copy %.1f" % (R, B, 4 * n >> 20, work_bytes >> 20, wall, 4 * n / wall / 1e6,
                                                tags[b"record_quantile"], tags[b"record_quantile_long"], c_ms,
                                                wall / c_ms), flush=True)
    for b in (src, dst, rec, q, work):
        b.free()
    dev.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time kman_classify_records (HIP events of kman_timing around the kernel, tag
"classify", 5 warm-up + 20 timed calls) at 1, 2, 8 and 64 colours, with and
without KMAN_CLASSIFY_SPECIFIC, beside kman_screen_records (tag "screen") on
the same reads and the same rows: what one reference costs today.  N colours
cost a user N screens today, so each classify time is printed beside N times
the screen time.

Reads and table keys are tools/screen_bench.py's: --reads records of 150
random ACGT bases; for a target of R rows with kt = round(log4 R), every
kt-mer (hit ~1), every second kt-mer (hit ~0.5), and 4^kt rows spread evenly
over the 21-mers (hit ~0).  screen reads u32 counts; classify reads u64 masks:
row i holds colour i mod N and, every fourth row, colour (i / 4) mod N too, so
at N >= 2 a quarter of the rows (less where the two coincide) are shared by two
references and vote for neither under SPECIFIC.  At N = 1 every row has mask 1:
the same hits as screen."""
import argparse
import ctypes
import os
import sys
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402
from screen_bench import READ, TIMED, WARM, fill_counts, fill_keys, make_reads  # noqa: E402

MCHUNK = 1 << 22  # mask rows per upload; a multiple of every pattern's period 4 N
COLOURS = (1, 2, 8, 64)


def fill_masks(dev, buf, n: int, nc: int) -> None:
    i = np.arange(MCHUNK, dtype=np.uint64)
    m = np.uint64(1) << (i % np.uint64(nc))
    m |= np.where(i % np.uint64(4) == 0, np.uint64(1) << ((i // np.uint64(4)) % np.uint64(nc)), np.uint64(0))
    for at in range(0, n, MCHUNK):
        dev.upload(buf, m[:min(MCHUNK, n - at)], 8 * at)


def timed(dev, L, tag: bytes, fn, args) -> float:
    for _ in range(WARM):
        N.check(dev.ctx, fn(*args), tag.decode())
    L.kman_timing_enable(dev.ctx, 1)
    for _ in range(TIMED):
        N.check(dev.ctx, fn(*args), tag.decode())
    cnt, ms = c_uint64(), ctypes.c_double()
    L.kman_timing_query(dev.ctx, tag, byref(cnt), byref(ms))
    L.kman_timing_enable(dev.ctx, 0)
    assert cnt.value == TIMED
    return ms.value / TIMED


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=2_000_000, help="150-base reads")
    ap.add_argument("--rows", type=float, nargs="+", default=[1e6, 1e8, 1e9], help="target table rows")
    ap.add_argument("--index-bits", type=int, default=None, help="default: engine.default_index_bits")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    codes, rec, n_bases = make_reads(dev, a.reads)
    out = dev.alloc(max(24, 4 * (1 + max(COLOURS))) * a.reads)
    print("kman_classify_records beside kman_screen_records, tile %d windows, %d reads of %d bases (%d bases); "
          "%d + %d timed calls each" % (N.KMAN_SCREEN_TILE, a.reads, READ, n_bases, WARM, TIMED), flush=True)
    for target in a.rows:
        kt = int(round(np.log(target) / np.log(4)))
        full = 4 ** kt
        for label, k, nt, step in (("hit ~1", kt, full, 1), ("hit ~0.5", kt, full // 2, 2),
                                   ("hit ~0", 21, full, 4 ** 21 // full)):
            keys, counts, masks = dev.alloc(8 * nt), dev.alloc(4 * nt), dev.alloc(8 * nt)
            fill_keys(dev, keys, nt, step)
            fill_counts(dev, counts, nt)
            bits = min(a.index_bits or engine.default_index_bits(nt, k), 2 * k)
            index = dev.alloc(8 * ((1 << bits) + 1))
            N.check(dev.ctx, L.kman_table_index(dev.ctx, c_void_p(keys.ptr), nt, k, bits, c_void_p(index.ptr)),
                    "kman_table_index")
            windows = a.reads * (READ - k + 1)
            s_ms = timed(dev, L, b"screen", L.kman_screen_records,
                         (dev.ctx, c_void_p(codes.ptr), n_bases, k, 0, c_void_p(rec.ptr), a.reads, c_void_p(keys.ptr),
                          c_void_p(counts.ptr), 4, nt, c_void_p(index.ptr), bits, c_void_p(out.ptr)))
            st = dev.download(out, 3 * a.reads, np.uint64).reshape(3, a.reads)
            assert int(st[0].sum()) == windows
            s_hits = int(st[1].sum())
            print("%-9s k %2d rows %11d index bits %2d | screen %9.3f ms, hit rate %.4f" % (
                label, k, nt, bits, s_ms, s_hits / windows), flush=True)
            for nc in COLOURS:
                fill_masks(dev, masks, nt, nc)
                for spec in (0, N.KMAN_CLASSIFY_SPECIFIC):
                    c_ms = timed(dev, L, b"classify", L.kman_classify_records,
                                 (dev.ctx, c_void_p(codes.ptr), n_bases, k, spec, c_void_p(rec.ptr), a.reads,
                                  c_void_p(keys.ptr), c_void_p(masks.ptr), nt, c_void_p(index.ptr), bits, nc,
                                  c_void_p(out.ptr)))
                    pl = dev.download(out, (1 + nc) * a.reads, np.uint32).reshape(1 + nc, a.reads)
                    assert int(pl[0].sum(dtype=np.uint64)) == windows
                    votes = int(pl[1:].sum(dtype=np.uint64))
                    if nc == 1:
                        assert votes == s_hits  # (one colour on every row: screen's hits)
                    print("    colours %2d %-8s | classify %9.3f ms = %5.2f x screen, %6.3f x %2d screens (%9.3f ms); "
                          "votes / windows %.4f" % (nc, "specific" if spec else "", c_ms, c_ms / s_ms,
                                                    c_ms / (nc * s_ms), nc, nc * s_ms, votes / windows), flush=True)
            for b in (keys, counts, masks, index):
                b.free()
    for b in (codes, rec, out):
        b.free()
    dev.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time kman_zip_records, the kernel behind `kmer screen --mate` and `kmer
classify --mate` (HIP events of kman_timing around its launches, tag "zip": the
offsets kernel and the copy pass together, 3 warm-up + 10 timed calls), beside

  a device-to-device copy of the same n_bases1 + n_bases2 bytes (HIP events
  around kman_memcpy_d2d's stream are not kept by the library, so 10 copies
  are timed by the wall clock, one synchronisation at the end), and

  kman_window_counts (tag "window_counts") on the zipped reads against a table
  of tools/screen_bench.py's shape: 4^13 rows spread evenly over the 21-mers,
  k = 21 -- the lookup that the zip enables.

Two inputs of about --bases bases in all (default 512 Mi), random ACGT codes
with bit 3 on every mate's first base:

  short   mates of 150 bases (2 x 150 per pair)
  long    mates of 10 000 bases (2 x 10 kb per pair)

The codes are tiled on the device from a 16 MiB host piece per source; the
zipped codes of the first and the last pairs and the whole table are checked
against the plain statement of tests/pair_cases.py."""
import argparse
import ctypes
import os
import sys
import time
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import pair_cases as pc  # noqa: E402
from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402
from screen_bench import fill_counts, fill_keys  # noqa: E402

WARM, TIMED = 3, 10
PIECE = 1 << 24  # bases of the host piece that is tiled into a source
K, KT = 21, 13


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


def source(dev, mate: int, copies: int, seed: int):
    """(device codes + pad, device table, host piece, records, bases): `copies`
    tiles of a piece of PIECE // mate mates of `mate` bases."""
    per = PIECE // mate
    piece, _, n1 = pc.mate_codes([mate] * per, seed, masked=False)
    R, n = per * copies, n1 * copies
    codes = dev.alloc(n + 64)
    for c in range(copies):
        dev.upload(codes, piece, c * n1)
    dev.upload(codes, np.full(64, 4, np.uint8), n)
    rec = dev.alloc(8 * R)
    dev.upload(rec, np.arange(R, dtype=np.uint64) * np.uint64(mate))
    return codes, rec, piece, R, n


def run_case(dev, L, label: str, mate: int, bases: int, table) -> str:
    copies = max(1, bases // 2 // (PIECE // mate * mate))
    c1, r1, piece1, R, n1 = source(dev, mate, copies, 1)
    c2, r2, piece2, _, n2 = source(dev, mate, copies, 2)
    n = n1 + n2
    out, out2, rec = dev.alloc(n + 64), dev.alloc(n + 64), dev.alloc(16 * R)

    def call():
        N.check(dev.ctx, L.kman_zip_records(dev.ctx, c_void_p(c1.ptr), n1, c_void_p(r1.ptr), c_void_p(c2.ptr), n2,
                                            c_void_p(r2.ptr), R, c_void_p(out.ptr), c_void_p(rec.ptr)),
                "kman_zip_records")

    z_ms = timed(dev, L, b"zip", call, 1)  # (one event pair around both launches)
    c_ms = copy_ms(dev, L, out2, out, n)
    out2.free()
    # the statement on the first and the last 1000 pairs, the table on the whole
    m = min(R, 1000)
    want, _ = pc.zip_codes(piece1, np.arange(m) * mate, m * mate, piece2, np.arange(m) * mate, m * mate)
    assert (dev.download(out, 2 * m * mate, np.uint8) == want[:-64]).all(), "the first pairs differ"
    per = len(piece1) // mate
    tail1, tail2 = piece1[(per - m) * mate:], piece2[(per - m) * mate:]
    want, _ = pc.zip_codes(tail1, np.arange(m) * mate, m * mate, tail2, np.arange(m) * mate, m * mate)
    assert (dev.download(out, 2 * m * mate + 64, np.uint8, n - 2 * m * mate) == want).all(), "the last pairs differ"
    assert (dev.download(rec, 2 * R, np.uint64) == np.arange(2 * R, dtype=np.uint64) * np.uint64(mate)).all()
    for b in (c1, c2, r1, r2):
        b.free()
    wc = dev.alloc(4 * n)
    w_ms = timed(dev, L, b"window_counts", lambda: N.check(dev.ctx, L.kman_window_counts(
        dev.ctx, c_void_p(out.ptr), n, K, 0, *table, c_void_p(wc.ptr)), "kman_window_counts"), 1)
    for b in (out, rec, wc):
        b.free()
    return ("%-5s %8d pairs of 2 x %5d bases, %4d MB of codes | zip %7.3f ms (%6.1f GB/s read + written), copy of "
            "the same bytes %7.3f ms (%6.1f GB/s), zip / copy %.2f | window_counts k=%d on the zipped codes %8.3f ms, "
            "zip / window_counts %.3f" % (label, R, mate, n >> 20, z_ms, 2 * n / z_ms / 1e6, c_ms, 2 * n / c_ms / 1e6,
                                          z_ms / c_ms, K, w_ms, z_ms / w_ms))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=1 << 29, help="bases of both sources together")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    nt = 4 ** KT
    keys, counts = dev.alloc(8 * nt), dev.alloc(4 * nt)
    fill_keys(dev, keys, nt, 4 ** K // nt)
    fill_counts(dev, counts, nt)
    bits = min(engine.default_index_bits(nt, K), 2 * K)
    index = dev.alloc(8 * ((1 << bits) + 1))
    N.check(dev.ctx, L.kman_table_index(dev.ctx, c_void_p(keys.ptr), nt, K, bits, c_void_p(index.ptr)),
            "kman_table_index")
    table = (c_void_p(keys.ptr), c_void_p(counts.ptr), 4, nt, c_void_p(index.ptr), bits)
    lines = ["tile %d output bytes, %d segments staged, table of 4^%d rows at k = %d (%d index bits), %d + %d timed "
             "calls" % (N.KMAN_ZIP_TILE, N.KMAN_ZIP_SEG_CAP, KT, K, bits, WARM, TIMED)]
    print(lines[0], flush=True)
    for label, mate in (("short", 150), ("long", 10_000)):
        lines.append(run_case(dev, L, label, mate, a.bases, table))
        print(lines[-1], flush=True)
    dev.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

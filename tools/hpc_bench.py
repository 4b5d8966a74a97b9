#!/usr/bin/env python3
"""Time kman_hpc_records, the kernel behind `--hpc` (HIP events of kman_timing
around its launches, tag "hpc": the compaction and the record table together,
3 warm-up + 10 timed calls), without and with the map to original indices,
against its algorithmic bytes (n read, the kept bytes written, 8 B per kept
base for the map), beside

  kman_zip_records (tag "zip") on the same bytes, the first half of the codes
  zipped with the second: the nearest existing kernel that only moves bytes.

About --bases bases (default 1 G) of synthetic codes: records of 10 000 bases,
bit 3 on every first base, base probabilities skewed so that runs are common
(the kept fraction is printed).  The codes are tiled on the device from one
host piece; the compressed codes and the map of the first bytes and the whole
record table are checked against the plain statement of tests/hpc_cases.py."""
import argparse
import ctypes
import os
import sys
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import hpc_cases as hc  # noqa: E402
from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

WARM, TIMED = 3, 10
REC = 10_000          # bases per record
PIECE_RECS = 1600     # records of the host piece that is tiled into the codes
P = (0.55, 0.15, 0.15, 0.15)
CHECK = 200_000       # bytes of the statement check


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


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=10 ** 9)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    n1 = PIECE_RECS * REC
    piece = hc.skewed_codes(n1, 1, p=P, n_frac=0.001, starts=range(0, n1, REC))
    copies = max(2, -(-a.bases // n1))
    copies += copies % 2  # (two equal halves for the zip)
    n, R = n1 * copies, PIECE_RECS * copies
    codes = dev.alloc(n + 64)
    dev.upload(codes, piece)
    for c in range(1, copies):
        N.check(dev.ctx, L.kman_memcpy_d2d(dev.ctx, c_void_p(codes.ptr + c * n1), c_void_p(codes.ptr), n1), "d2d")
    dev.upload(codes, np.full(64, 4, np.uint8), n)
    rec_host = np.arange(R, dtype=np.uint64) * np.uint64(REC)
    rec, out_rec = dev.alloc(8 * R), dev.alloc(8 * R)
    dev.upload(rec, rec_host)
    out, orig = dev.alloc(n + 64), dev.alloc(8 * n)
    n_out = c_uint64(0)

    def call(with_map):
        N.check(dev.ctx, L.kman_hpc_records(dev.ctx, c_void_p(codes.ptr), n, c_void_p(rec.ptr), R, c_void_p(out.ptr),
                                            c_void_p(out_rec.ptr), c_void_p(orig.ptr) if with_map else None,
                                            byref(n_out)), "kman_hpc_records")

    plain_ms = timed(dev, L, b"hpc", lambda: call(False), 2)  # (two event pairs: the compaction, the table)
    map_ms = timed(dev, L, b"hpc", lambda: call(True), 2)
    m = n_out.value
    # the statement: the first bytes, their map, and the whole table (every piece compresses alike)
    want, want_rec, want_orig = hc.hpc_codes(piece[:CHECK], rec_host[:CHECK // REC])
    got = dev.download(out, len(want) - 1, np.uint8)  # (the last run may go on past the checked bytes)
    assert (got == want[:-1]).all(), "the first kept bytes differ"
    assert (dev.download(orig, len(want) - 1, np.uint64) == want_orig[:-1]).all(), "the map differs"
    table = dev.download(out_rec, R, np.uint64)
    assert (table[:CHECK // REC] == want_rec).all() and m % copies == 0, "the table differs"
    per = m // copies
    assert (table.reshape(copies, PIECE_RECS) ==
            table[:PIECE_RECS][None, :] + (np.arange(copies, dtype=np.uint64) * np.uint64(per))[:, None]).all()
    orig.free()
    # the zip of the two halves of the same codes
    h, hr = n // 2, R // 2
    zout, zrec = dev.alloc(n + 64), dev.alloc(16 * hr)
    zip_ms = timed(dev, L, b"zip", lambda: N.check(dev.ctx, L.kman_zip_records(
        dev.ctx, c_void_p(codes.ptr), h, c_void_p(rec.ptr), c_void_p(codes.ptr + h), h, c_void_p(rec.ptr), hr,
        c_void_p(zout.ptr), c_void_p(zrec.ptr)), "kman_zip_records"), 1)
    for b in (codes, rec, out_rec, out, zout, zrec):
        b.free()
    dev.close()
    by_plain, by_map = n + m, n + 9 * m
    lines = [
        "tile %d input bytes, %d records of %d bases, %d MB of codes, %.1f %% kept, %d + %d timed calls"
        % (N.KMAN_HPC_TILE, R, REC, n // 10 ** 6, 100.0 * m / n, WARM, TIMED),
        "hpc without the map %8.3f ms, %6.1f GB/s of its %d algorithmic MB (n read + kept written)"
        % (plain_ms, by_plain / plain_ms / 1e6, by_plain // 10 ** 6),
        "hpc with the map    %8.3f ms, %6.1f GB/s of its %d algorithmic MB (+ 8 B per kept base)"
        % (map_ms, by_map / map_ms / 1e6, by_map // 10 ** 6),
        "zip of the same bytes %6.3f ms, %6.1f GB/s of its %d MB (n read + n written); hpc / zip %.2f, with the map %.2f"
        % (zip_ms, 2 * n / zip_ms / 1e6, 2 * n // 10 ** 6, plain_ms / zip_ms, map_ms / zip_ms),
    ]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

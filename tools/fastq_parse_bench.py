"""Device time of kman_parse_fastq on a synthetic FASTQ of 150-base reads against
kman_parse_fasta on a FASTA of the same byte size with 150-column lines: input
GB/s of both and their ratio (HIP events, kman_timing_query).

    python tools/fastq_parse_bench.py [--mb 256] [--warmup 5] [--steps 20] [--out FILE]
"""

from __future__ import annotations

import argparse
import os
import sys
from ctypes import byref, c_double, c_uint64, c_void_p

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402


def synth_fastq(n_bytes: int, seed: int = 1) -> bytes:
    """Records "@read<9 digits>\\n<150 bases>\\n+\\n<150 quality bytes>\\n" (319 bytes each)."""
    rng = np.random.default_rng(seed)
    R = n_bytes // 319
    a = np.empty((R, 319), dtype=np.uint8)
    a[:, 0:5] = np.frombuffer(b"@read", np.uint8)
    idx = np.arange(R)
    for d in range(9):
        a[:, 5 + d] = ord("0") + (idx // 10 ** (8 - d)) % 10
    a[:, 14] = 10
    a[:, 15:165] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (R, 150))]
    a[:, 165:168] = np.frombuffer(b"\n+\n", np.uint8)
    a[:, 168:318] = rng.integers(33, 127, (R, 150), dtype=np.uint8)
    a[:, 318] = 10
    return a.tobytes()


def synth_fasta(n_bytes: int, seed: int = 2) -> bytes:
    rng = np.random.default_rng(seed)
    L = (n_bytes - 5) // 151
    a = np.empty((L, 151), dtype=np.uint8)
    a[:, :150] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (L, 150))]
    a[:, 150] = 10
    return b">syn\n" + a.tobytes()


def time_parse(dev, text: bytes, fn, tag: str, cap: int, warmup: int, steps: int):
    L = N.lib()
    n = len(text)
    d_text, codes = dev.alloc(n + 64), dev.alloc(n + 64)
    d_hdr, d_seq = dev.alloc(8 * cap), dev.alloc(8 * cap)
    try:
        dev.upload(d_text, text)
        info = N.ParseInfo()

        def run():
            N.check(dev.ctx, fn(dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr),
                                c_void_p(d_seq.ptr), cap, byref(info)), tag)

        for _ in range(warmup):
            run()
        N.check(dev.ctx, L.kman_timing_enable(dev.ctx, 1), "timing")
        for _ in range(steps):
            run()
        launches, ms = c_uint64(0), c_double(0)
        N.check(dev.ctx, L.kman_timing_query(dev.ctx, tag.encode(), byref(launches), byref(ms)), "timing")
        N.check(dev.ctx, L.kman_timing_enable(dev.ctx, 0), "timing")
        return ms.value / steps, int(info.n_bases), int(info.n_records)
    finally:
        for b in (d_text, codes, d_hdr, d_seq):
            b.free()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    nb = a.mb << 20
    fq, fa = synth_fastq(nb), synth_fasta(nb)
    ms_q, bases_q, rec_q = time_parse(dev, fq, L.kman_parse_fastq, "parse_fastq", len(fq) // 4 + 1, a.warmup, a.steps)
    ms_a, bases_a, rec_a = time_parse(dev, fa, L.kman_parse_fasta, "parse", len(fa) // 2 + 1, a.warmup, a.steps)
    gq, ga = len(fq) / ms_q / 1e6, len(fa) / ms_a / 1e6
    lines = [
        "kman_parse_fastq vs kman_parse_fasta, device time (HIP events), %d warm-up + %d timed launches" % (a.warmup,
                                                                                                         a.steps),
        "fastq  %11d bytes  %9d records  %11d bases  %8.3f ms  %8.1f GB/s input" % (len(fq), rec_q, bases_q, ms_q, gq),
        "fasta  %11d bytes  %9d records  %11d bases  %8.3f ms  %8.1f GB/s input" % (len(fa), rec_a, bases_a, ms_a, ga),
        "ratio fastq / fasta (input bytes per second): %.3f" % (gq / ga),
    ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    dev.close()


if __name__ == "__main__":
    main()

"""Device time of kman_parse_fastq on a synthetic FASTQ of 150-base reads against
kman_parse_fasta on a FASTA of the same byte size with 150-column lines: input
GB/s of both and their ratio (HIP events, kman_timing_query).

    python tools/fastq_parse_bench.py [--mb 256] [--warmup 5] [--steps 20] [--out FILE]

With ``--min-qual Q`` it times the quality threshold instead: the plain parse
(kman_parse_fastq) and the masked parse (kman_parse_fastq_q, fq_qmask) of the
same FASTQ, alternating, in ``--pairs`` interleaved pairs of warm-up + timed
launches each, with the pair-to-pair spread of both and the bytes the mask
pass moves, derived from the input's shape.

    python tools/fastq_parse_bench.py --min-qual 20 [--phred-offset 33] [--pairs 5] ...
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


def mask_bytes_per_input_byte(read_len: int = 150, rec_bytes: int = 319, min_qual: int = 20):
    """What fq_qmask moves per input byte on synth_fastq's records, from the
    kernel's code: (text re-read, quality read as issued, quality read unique,
    codes read, codes written).  A run of `read_len` sequence bytes at a random
    phase touches (read_len + 63) / 64 chunks of 64 bytes, each of which loads
    17 dwords of quality bytes; a 16-byte vector of codes is read and written
    unless none of its codes is masked (qualities uniform over 94 values)."""
    chunks = (read_len + 63) / 64.0
    touched = 1.0 - (1.0 - min(min_qual, 94) / 94.0) ** 16
    codes = read_len * touched / rec_bytes
    return 1.0, chunks * 68 / rec_bytes, read_len / rec_bytes, codes, codes


def time_pairs(dev, text: bytes, qbyte: int, warmup: int, steps: int, pairs: int):
    """[(ms plain, ms masked)] per pair and (n_bases, n_masked); one upload."""
    L = N.lib()
    n = len(text)
    cap = n // 4 + 1
    d_text, codes = dev.alloc(n + 64), dev.alloc(n + 64)
    d_hdr, d_seq = dev.alloc(8 * cap), dev.alloc(8 * cap)
    try:
        dev.upload(d_text, text)
        info, masked = N.ParseInfo(), c_uint64(0)
        args = (dev.ctx, c_void_p(d_text.ptr), n, c_void_p(codes.ptr), c_void_p(d_hdr.ptr), c_void_p(d_seq.ptr), cap)

        def plain():
            N.check(dev.ctx, L.kman_parse_fastq(*args, byref(info)), "parse_fastq")

        def with_mask():
            N.check(dev.ctx, L.kman_parse_fastq_q(*args, byref(info), qbyte, byref(masked)), "parse_fastq_q")

        def timed(run):
            for _ in range(warmup):
                run()
            N.check(dev.ctx, L.kman_timing_enable(dev.ctx, 1), "timing")
            for _ in range(steps):
                run()
            launches, ms = c_uint64(0), c_double(0)
            N.check(dev.ctx, L.kman_timing_query(dev.ctx, b"parse_fastq", byref(launches), byref(ms)), "timing")
            N.check(dev.ctx, L.kman_timing_enable(dev.ctx, 0), "timing")
            return ms.value / steps

        out = [(timed(plain), timed(with_mask)) for _ in range(pairs)]
        return out, int(info.n_bases), int(masked.value)
    finally:
        for b in (d_text, codes, d_hdr, d_seq):
            b.free()


def report_min_qual(a, dev) -> str:
    qbyte = engine._qual_byte(a.min_qual, a.phred_offset)
    fq = synth_fastq(a.mb << 20)
    pairs, n_bases, n_masked = time_pairs(dev, fq, qbyte, a.warmup, a.steps, a.pairs)
    p_ms, m_ms = [p for p, _ in pairs], [m for _, m in pairs]
    med = lambda v: float(np.median(v))  # noqa: E731
    extra = med([m - p for p, m in pairs])
    b = mask_bytes_per_input_byte(min_qual=a.min_qual)
    issued, unique = b[0] + b[1] + b[3] + b[4], b[0] + b[2] + b[3] + b[4]
    lines = [
        "kman_parse_fastq_q (min_qual %d, offset %d: threshold byte %d) vs kman_parse_fastq, device time (HIP events),"
        % (a.min_qual, a.phred_offset, qbyte),
        "%d interleaved pairs of %d warm-up + %d timed launches each; %d bytes, %d bases, %d masked"
        % (a.pairs, a.warmup, a.steps, len(fq), n_bases, n_masked),
    ]
    for i, (p, m) in enumerate(pairs):
        lines.append("pair %d  plain %8.4f ms  masked %8.4f ms  extra %8.4f ms" % (i, p, m, m - p))
    lines += [
        "plain   median %8.4f ms  min %8.4f  max %8.4f  (pair-to-pair spread %.4f ms)  %8.1f GB/s input"
        % (med(p_ms), min(p_ms), max(p_ms), max(p_ms) - min(p_ms), len(fq) / med(p_ms) / 1e6),
        "masked  median %8.4f ms  min %8.4f  max %8.4f  (pair-to-pair spread %.4f ms)  %8.1f GB/s input"
        % (med(m_ms), min(m_ms), max(m_ms), max(m_ms) - min(m_ms), len(fq) / med(m_ms) / 1e6),
        "extra   median %8.4f ms per parse for the mask pass (fq_qmask, its memset and 8-byte copy back)" % extra,
        "bytes the mask pass moves per input byte (150-base reads, 319-byte records): text re-read %.2f, quality "
        "read %.2f issued / %.2f unique," % (b[0], b[1], b[2]),
        "  codes read %.2f, codes written %.2f: %.2f issued / %.2f unique B per input byte = %.0f / %.0f MB"
        % (b[3], b[4], issued, unique, issued * len(fq) / 1e6, unique * len(fq) / 1e6),
        "extra bytes / extra time: %.0f GB/s issued, %.0f GB/s unique"
        % (issued * len(fq) / extra / 1e6, unique * len(fq) / extra / 1e6),
    ]
    return "\n".join(lines) + "\n"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--min-qual", type=int, default=0, help="time the masked parse against the plain one")
    ap.add_argument("--phred-offset", type=int, default=33, choices=[33, 64])
    ap.add_argument("--pairs", type=int, default=5, help="interleaved (plain, masked) pairs with --min-qual")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    if a.min_qual:
        text = report_min_qual(a, dev)
        sys.stdout.write(text)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write(text)
        dev.close()
        return
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

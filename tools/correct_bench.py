#!/usr/bin/env python3
"""Time kman_correct_sites and kman_apply_fixes, the kernels behind `kmer
screen --solid C --correct`, beside kman_window_counts on the same reads and
table: the step that every --solid run already pays (HIP events of
kman_timing around the launches, tags "window_counts", "correct_sites" and
"apply_fixes": 3 warm-up + 10 timed calls each).

The reads: --bases bases (default 2^25) as 150-base four-line FASTQ records
cut at random places from one random genome of --genome bases (default 2^22),
every base substituted with probability 0, 0.005 and 0.02.  The table: the
genome's canonical 21-mers, counted on the GPU; min_count 1, so a window is
weak when its k-mer is not in the genome.  kman_apply_fixes patches the codes
and the FASTQ text; it is timed on the unchanged d_fix ten times (the patch is
idempotent), after kman_correct_sites was timed on the unpatched codes.

Checked: *n_fixed equals the sum of d_nfix, and at the rate 0 both are 0."""
import argparse
import ctypes
import os
import sys
from ctypes import byref, c_uint64, c_void_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from kman_amd import _native as N  # noqa: E402
from kman_amd import engine  # noqa: E402

WARM, TIMED = 3, 10
READ, K, C = 150, 21, 1


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


def fastq_of(genome: np.ndarray, n_reads: int, rate: float, seed: int):
    """(text, substituted bases): n_reads records "@r\\n" + 150 bases + "\\n+\\n" + 150 x "I" + "\\n"."""
    rng = np.random.default_rng(seed)
    at = rng.integers(0, len(genome) - READ + 1, n_reads)
    seq = genome[at[:, None] + np.arange(READ)[None, :]]
    hit = rng.random(seq.shape) < rate
    seq = np.where(hit, (seq + rng.integers(1, 4, seq.shape)) & 3, seq)
    rows = np.empty((n_reads, 3 + READ + 3 + READ + 1), np.uint8)
    rows[:, :3] = np.frombuffer(b"@r\n", np.uint8)
    rows[:, 3:3 + READ] = np.frombuffer(b"ACGT", np.uint8)[seq]
    rows[:, 3 + READ:6 + READ] = np.frombuffer(b"\n+\n", np.uint8)
    rows[:, 6 + READ:6 + 2 * READ] = ord("I")
    rows[:, -1] = ord("\n")
    return rows.tobytes(), int(hit.sum())


def run_case(dev, L, table, idx, bits: int, genome: np.ndarray, n_reads: int, rate: float) -> str:
    text, n_sub = fastq_of(genome, n_reads, rate, 7)
    p = engine.parse(dev, text, "fastq", keep_text=True)
    n, R = int(p.n_bases), int(p.n_records)
    bufs = []
    try:
        def alloc(nbytes):
            bufs.append(dev.alloc(max(16, nbytes)))
            return bufs[-1]

        wc, rec, fix, nfix, off = alloc(4 * n), alloc(8 * R), alloc(n), alloc(4 * R), alloc(8 * (R + 1))
        dev.upload(rec, np.ascontiguousarray(p.rec_seq, dtype=np.uint64))
        dev.upload(off, np.concatenate([p.rec_hdr, [p.text_bytes]]).astype(np.uint64))
        tab = (c_void_p(table.ukeys.ptr), c_void_p(table.counts.ptr), table.count_bytes, table.n)
        n_fixed = c_uint64(0)

        def counts():
            N.check(dev.ctx, L.kman_window_counts(dev.ctx, c_void_p(p.codes.ptr), n, K, N.KMAN_CANONICAL, *tab,
                                                  c_void_p(idx.ptr), bits, c_void_p(wc.ptr)), "kman_window_counts")

        def sites():
            N.check(dev.ctx, L.kman_correct_sites(dev.ctx, c_void_p(p.codes.ptr), n, K, N.KMAN_CANONICAL,
                                                  c_void_p(wc.ptr), c_void_p(rec.ptr), R, *tab, c_void_p(idx.ptr), bits,
                                                  C, c_void_p(fix.ptr), byref(n_fixed)), "kman_correct_sites")

        def apply():
            N.check(dev.ctx, L.kman_apply_fixes(dev.ctx, c_void_p(p.codes.ptr), n, c_void_p(fix.ptr),
                                                c_void_p(rec.ptr), R, c_void_p(p.text.ptr), int(p.text_bytes),
                                                c_void_p(off.ptr), c_void_p(nfix.ptr)), "kman_apply_fixes")

        w_ms = timed(dev, L, b"window_counts", counts)
        s_ms = timed(dev, L, b"correct_sites", sites)
        a_ms = timed(dev, L, b"apply_fixes", apply)
        total = int(dev.download(nfix, R, np.uint32).astype(np.uint64).sum())
        assert total == n_fixed.value, (total, n_fixed.value)
        assert rate > 0 or total == 0
        return ("rate %5.3f  %9d bases in %7d reads, %7d substituted, %7d corrected | window_counts %7.3f ms, "
                "correct_sites %7.3f ms (%.2f x), apply_fixes %7.3f ms (%.2f x), both %.2f x" % (
                    rate, n, R, n_sub, total, w_ms, s_ms, s_ms / w_ms, a_ms, a_ms / w_ms, (s_ms + a_ms) / w_ms))
    finally:
        for b in bufs:
            b.free()
        p.free()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--bases", type=int, default=1 << 25)
    ap.add_argument("--genome", type=int, default=1 << 22)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    dev = engine.Device(0)
    L = N.lib()
    genome = np.random.default_rng(1).integers(0, 4, a.genome)
    g = engine.parse(dev, b">g\n" + np.frombuffer(b"ACGT", np.uint8)[genome].tobytes() + b"\n")
    try:
        table = engine.join_groups(g, K, False, "count", canonical=True)
    finally:
        g.free()
    bits = engine.default_index_bits(table.n, K)
    idx = engine.table_index(dev, table, bits)
    lines = ["tile %d bases, k %d canonical, min_count %d, table of %d rows (index of %d bits), %d + %d timed calls" % (
        N.KMAN_CORRECT_TILE, K, C, table.n, bits, WARM, TIMED)]
    print(lines[0], flush=True)
    try:
        for rate in (0.0, 0.005, 0.02):
            lines.append(run_case(dev, L, table, idx, bits, genome, a.bases // READ, rate))
            print(lines[-1], flush=True)
    finally:
        idx.free()
        engine.free_result(table)
    dev.close()
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""FASTQ quality-threshold test helper (not a conftest): a pure-Python
restatement of kman_parse_fastq_q's masking rule (include/kman.h), built on
fastq_cases.fastq_lines and independent of the code under test.

The expected value of every threshold test is what the FASTA oracles
(np_oracle.parse_fasta, oracle/kman_oracle) give for ``mask_fastq(...)[0]``.
"""

from __future__ import annotations

import fastq_cases as fq

_WS = b" \t\n\x0b\x0c\r\x1c\x1d\x1e\x1f"  # what the sequence-line cleaning strips when trailing


def mask_fastq(text: bytes, min_qual: int, phred_offset: int = 33):
    """``(fasta_bytes, n_masked)``: the FASTA of fastq_cases.fastq_to_fasta
    with byte j of every sequence line replaced by ``N`` when it is a kept byte
    (not ``' '``, not trailing whitespace) and byte j of the record's quality
    line is below ``phred_offset + min_qual`` (``min_qual == 0``: no byte is).
    n_masked counts those bytes.  Errors are fastq_to_fasta's."""
    fq.fastq_to_fasta(text)  # (raises for an input that breaks a rule)
    t = phred_offset + min_qual if min_qual else 0
    lines = fq.fastq_lines(text)
    out, n_masked = [], 0
    for r in range(0, len(lines), 4):
        l0, l1, _, l3 = lines[r:r + 4]
        kept_end = len(l1.rstrip(_WS))
        seq = bytearray(l1)
        for j in range(kept_end):
            if seq[j] != 0x20 and l3[j] < t:
                seq[j] = ord("N")
                n_masked += 1
        out.append(b">" + l0[1:] + b"\n" + bytes(seq) + b"\n")
    return b"".join(out), n_masked

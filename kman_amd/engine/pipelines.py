"""One-call pipelines from a text or a sequence string to its result."""

from __future__ import annotations

from ctypes import c_void_p
from typing import Optional

import numpy as np

from .. import _native as N
from .device import Device, default_device
from .parsed import Parsed, _check_qual_format, _qual_byte, _resolve_format, check_empty_names, parse
from .kmers import _check_k, extract
from .words import WordsResult
from .join import count_groups, free_result, join_groups
from .output import _emit_words, emit_count, emit_uniq
from .reads import _hpc_parsed


_CODE_TABLE = np.full(128, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE_TABLE[ord(_c)] = _i
    _CODE_TABLE[ord(_c.lower())] = _i


def kmers_of_sequence(seq: str, k: int, rc: bool, dev: Optional[Device] = None):
    """Keys + pos payloads of every valid window of one sequence string
    (Sequence.yield_kmers, seq.py:285-328), enumerated by kman_extract."""
    _check_k(k)
    dev = dev or default_device()
    cp = np.frombuffer(seq.encode("utf-32-le"), dtype=np.uint32)
    codes = np.where(cp < 128, _CODE_TABLE[np.minimum(cp, 127)], 4).astype(np.uint8)
    n = len(codes)
    if n < k:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    codes[0] |= 8
    with dev.scratch() as s:
        buf = s.alloc(n + 64)
        dev.upload(buf, np.concatenate([codes, np.full(64, 4, np.uint8)]))
        p = Parsed(dev, buf, n, 1, np.zeros(1, np.uint64), np.zeros(1, np.uint64), [b""], b"",
                   np.zeros(2, np.uint64))
        km = extract(p, k, rc, want_pos=True)
        try:
            keys = dev.download(km.keys, km.n, np.uint64)
            pos = dev.download(km.pos, km.n, np.uint32 if km.pos_bytes == 4 else np.uint64).astype(np.uint64)
        finally:
            km.free()
    return keys, pos


def abundance_hist(text: bytes, k: int, canonical: bool = True, nbins: int = 10001,
                   dev: Optional[Device] = None, fmt: str = "auto", min_qual: int = 0,
                   phred_offset: int = 33, hpc: bool = False) -> np.ndarray:
    """k-mer abundance spectrum (BASELINE config 5; SURVEY §8f-1, not in the
    reference): h[c] = distinct (canonical) k-mers seen c times, h[-1] every
    count >= nbins - 1 (kman_count_hist over the count output).  `min_qual`,
    `phred_offset`: parse_fastq's quality threshold; `hpc`: homopolymer-compressed
    k-mers (hpc() right after the parse)."""
    _check_k(k, wide=True)
    _check_qual_format(_qual_byte(min_qual, phred_offset),
                       _resolve_format(fmt, lambda at: bytes(text[at:at + (1 << 16)])))
    dev = dev or default_device()
    p = parse(dev, text, fmt, min_qual, phred_offset)
    if hpc:
        p = _hpc_parsed(p)
    try:
        r = count_groups(p, k, False, canonical, ordered=False)
        with dev.scratch() as s:
            d_h = s.alloc(8 * nbins)
            if r is None:
                return np.zeros(nbins, np.uint64)
            try:
                cnt, cb = (r.vals, r.val_bytes) if isinstance(r, WordsResult) else (r.counts, r.count_bytes)
                N.check(dev.ctx, N.lib().kman_count_hist(dev.ctx, c_void_p(cnt.ptr), cb, r.n,
                                                         c_void_p(d_h.ptr), nbins), "kman_count_hist")
                return dev.download(d_h, nbins, np.uint64)
            finally:
                free_result(r)
    finally:
        p.free()


def format_hist(h: np.ndarray) -> bytes:
    """``"%d\t%d\n" % (count, n_kmers)`` for every non-empty bin; the last bin
    reads ``">=N"``."""
    out = []
    last = len(h) - 1
    for c in np.nonzero(h)[0].tolist():
        out.append("%s\t%d\n" % ((">=%d" % c) if c == last else str(c), int(h[c])))
    return "".join(out).encode()


def _text(text: bytes, k: int, rc: bool, dev: Optional[Device], max_keys: Optional[int], mode: str) -> bytes:
    dev = dev or default_device()
    _check_k(k, wide=True)
    p = parse(dev, text)
    try:
        check_empty_names(p, k)
        r = join_groups(p, k, rc, mode, max_keys)
        if r is None:
            return b""
        try:
            if isinstance(r, WordsResult):
                return _emit_words(p, r)
            return emit_count(dev, r) if mode == "count" else emit_uniq(p, r)
        finally:
            free_result(r)
    finally:
        p.free()


def count_text(text: bytes, k: int, rc: bool = False, dev: Optional[Device] = None,
               max_keys: Optional[int] = None) -> bytes:
    """``kmer count`` output bytes for a FASTA text (SEQ_COUNT mode).
    max_keys: run the multi-batch join with key ranges of at most that many
    k-mers (by default only when the single batch does not fit the HBM)."""
    return _text(text, k, rc, dev, max_keys, "count")


def uniq_text(text: bytes, k: int, rc: bool = False, dev: Optional[Device] = None,
              max_keys: Optional[int] = None) -> bytes:
    """``kmer uniq`` output bytes for a FASTA text (UNIQUE mode); max_keys as
    in count_text."""
    return _text(text, k, rc, dev, max_keys, "uniq")

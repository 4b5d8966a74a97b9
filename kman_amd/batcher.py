"""Batchers: FASTA file -> collection of k-mer batches (kmermaid/batcher.py).

``FastaBatcher.do(fasta, k)`` reads the file once, parses it on the GPU
(kman_parse_fasta), and cuts the reference's k-mer stream — records in file
order, windows in position order, + then - strand with ``-r`` — into
consecutive batches of ``size`` k-mers (BatcherBase.new_batch/add_record,
batcher.py:118-131; one FastaRecordBatcher spans all records in KMERS mode,
batcher.py:386).  The batches are views of the device-resident stream; each
is sorted on the GPU when its contents are asked for, which is what the
reference's forced ``write_all(doSort=True)`` re-sort guarantees
(batcher.py:392, §A-1).

Divergences (documented in DESIGN.md):
* RECORDS scan mode batches every record separately and keeps every batch
  sorted — the reference leaves full batches unsorted there (§A-2), which
  only corrupts its own join.
* ``threads`` is accepted and ignored: the GPU is the parallelism.
* ``load_batches`` implements the evident intent (the reference raises when
  the folder is NOT empty, batcher.py:631, §A-5).
"""

from __future__ import annotations

import logging
import os
import tempfile
from enum import Enum
from typing import List, Optional, Type

from . import engine, phases
from .batch import Batch
from .seq import NATYPES, KMer


class BatcherBase:
    DEFAULT_BATCH_SIZE = int(1e6)
    DEFAULT_NATYPE = NATYPES.DNA
    _type: Type = KMer

    def __init__(self, size: int, natype: Optional[NATYPES] = None, tmp: Optional[str] = None):
        self.__size = self.DEFAULT_BATCH_SIZE
        self.__natype = self.DEFAULT_NATYPE
        self.size = size
        self.natype = natype
        if isinstance(tmp, tempfile.TemporaryDirectory):
            self._tmpH = tmp
            self._tmp = tmp.name
        elif isinstance(tmp, str):
            self._tmp = tmp
        else:
            self._tmp = tempfile.gettempdir()
        self._batches: List[Batch] = [Batch.from_batcher(self.type, self.size, self.tmp)]

    @property
    def size(self) -> int:
        return self.__size

    @size.setter
    def size(self, size: Optional[int]) -> None:
        if size is not None:
            if size < 1:
                raise AssertionError
            self.__size = int(size)

    @property
    def type(self):
        return self._type

    @property
    def natype(self):
        return self.__natype

    @natype.setter
    def natype(self, natype: Optional[NATYPES]) -> None:
        if natype is not None:
            if not isinstance(natype, NATYPES):
                raise AssertionError
            self.__natype = natype

    @property
    def collection(self) -> List[Batch]:
        return self._batches

    @property
    def tmp(self) -> str:
        if self._tmp is None:
            self._tmpH = tempfile.TemporaryDirectory(prefix="kmermaidBatch")
            self._tmp = self._tmpH.name
        return self._tmp

    def new_batch(self) -> None:
        if self.collection[-1].is_full():
            self.collection[-1].write()
            self._batches.append(Batch.from_batcher(self.type, self.size, self.tmp))

    def add_record(self, record) -> None:
        self.new_batch()
        self.collection[-1].add(record)

    def write_all(self, f: str = "as_fasta", doSort: bool = False, verbose: bool = False) -> None:
        """Write every non-empty batch, sorted (the reference's effective
        behaviour, §A-1: its positional-argument bug makes every call sort)."""
        for b in self.collection:
            if b.current_size != 0:
                b.write(doSort=True, force=bool(doSort))


class BatcherThreading(BatcherBase):
    class FEED_MODE(Enum):
        REPLACE = 1
        FLOW = 2
        APPEND = 3

    def __init__(self, size: int, threads: int = 1, natype: Optional[NATYPES] = None, tmp: Optional[str] = None):
        super().__init__(size, natype, tmp)
        self.threads = threads

    @property
    def threads(self) -> int:
        return self.__threads

    @threads.setter
    def threads(self, t: int) -> None:
        self.__threads = max(1, min(int(t), os.cpu_count() or 1))

    def feed_collection(self, new_collection: List[Batch], mode: "BatcherThreading.FEED_MODE" = FEED_MODE.FLOW):
        if any(b.type != self.type for b in new_collection):
            raise AssertionError
        if mode == self.FEED_MODE.REPLACE:
            self._batches = list(new_collection)
        else:
            # FLOW re-batches the same records into this batcher's batches of
            # the same size: the k-mer stream and its chunking are identical.
            self._batches.extend(new_collection)

    @staticmethod
    def from_files(dirPath: str, threads: int = 1, t: Type = KMer, isFasta: bool = True,
                   reSort: bool = False) -> List[Batch]:
        if not os.path.isdir(dirPath):
            raise AssertionError
        return [Batch.from_file(os.path.join(dirPath, f), t, isFasta, reSort=reSort)
                for f in sorted(os.listdir(dirPath))]


class FastaBatcher(BatcherThreading):
    class MODE(Enum):
        KMERS = 1
        RECORDS = 2

    def __init__(self, scan_mode: "FastaBatcher.MODE" = MODE.KMERS, reverse: bool = False, threads: int = 1,
                 size: int = BatcherThreading.DEFAULT_BATCH_SIZE, natype: NATYPES = BatcherThreading.DEFAULT_NATYPE,
                 tmp: Optional[str] = None, device: Optional[engine.Device] = None,
                 distributed: Optional[bool] = None, fmt: str = "auto", min_qual: int = 0,
                 phred_offset: int = 33, hpc: bool = False):
        super().__init__(size, threads, natype, tmp if tmp is not None else tempfile.gettempdir())
        self.hpc = bool(hpc)  # homopolymer-compressed k-mers (engine.hpc): one GPU, the whole input
        if fmt not in engine.FORMATS:
            raise AssertionError("format must be one of %s, got %r" % (", ".join(engine.FORMATS), fmt))
        self.fmt = fmt  # input format: "auto" (engine.sniff_format), "fasta" or "fastq"
        # FASTQ quality threshold (engine.parse_fastq): bases below it read as N; 0 = none
        self._qbyte = engine._qual_byte(min_qual, phred_offset)
        self.min_qual, self.phred_offset = min_qual, phred_offset
        self.mode = scan_mode
        self.doReverseComplement = reverse
        self._device = device
        # one process per GPU (kman_amd/launch.py): None = from the launcher's
        # environment (WORLD_SIZE > 1, or KMAN_DIST=1)
        self._distributed = distributed
        self.source = None

    @property
    def mode(self):
        return self._mode

    @mode.setter
    def mode(self, m) -> None:
        if not isinstance(m, self.MODE):
            raise AssertionError
        self._mode = m

    @property
    def doReverseComplement(self) -> bool:
        return self._doReverseComplement

    @doReverseComplement.setter
    def doReverseComplement(self, rc) -> None:
        if type(rc) is not bool:
            raise AssertionError
        self._doReverseComplement = rc

    def do(self, fasta: str, k: int, feedMode: BatcherThreading.FEED_MODE = BatcherThreading.FEED_MODE.APPEND
           ) -> "FastaBatcher":
        """Batch the k-mers of a FASTA file (batcher.py:454-487)."""
        if not os.path.isfile(fasta):
            raise AssertionError(f"input file not found: {fasta}")
        if k <= 1:
            raise AssertionError(f"k must be >= 1, got {k} instead.")
        if self.natype != NATYPES.DNA:
            raise NotImplementedError("the k-mer path is DNA-only, as the reference CLI")
        from . import launch
        from .source import FastaSource

        fmt = engine.sniff_file(fasta) if self.fmt == "auto" else self.fmt
        engine._check_qual_format(self._qbyte, fmt)  # (before any device work)
        dev = self._device or engine.default_device()
        dist = launch.distributed() if self._distributed is None else self._distributed
        if dist and self.hpc:
            raise AssertionError("homopolymer compression runs on one GPU (rank 0 alone under a launch)")
        if dist and k <= engine.MAX_K and fmt != "fastq":  # (the byte-range shards cut FASTA only)
            # this rank's byte range only; ONE batch of its windows, joined
            # across the ranks by KJoiner.join (the batch cut does not change
            # count / uniq output)
            src = launch.ShardedSource(dev, fasta, k, self.doReverseComplement)
            self.source = src
            n = src.n_kmers
            self.feed_collection([Batch.from_source(src, 0, n, max(1, n), self.tmp)], feedMode)
            return self
        kw = {"hpc": True} if self.hpc else {}
        src = FastaSource(dev, None, k, self.doReverseComplement, path=fasta, fmt=fmt, min_qual=self.min_qual,
                          phred_offset=self.phred_offset, **kw)
        self.source = src
        if fmt == "fastq":  # (reads: millions of records, one line for all)
            logging.info("Batching %d reads..." % src.parsed.n_records)
        else:
            for name in src.parsed.names:
                logging.info("Batching record '%s'..." % name.decode("utf-8", "surrogateescape"))
        batches = []
        if self.mode == self.MODE.KMERS:
            n = src.n_kmers
            starts = list(range(0, n, self.size)) or [0]
            for s in starts:
                batches.append(Batch.from_source(src, s, min(n, s + self.size), self.size, self.tmp))
        else:
            batches = self._record_batches(src)
        self.feed_collection(batches, feedMode)
        phases.mark("batches")
        return self

    def _record_batches(self, src) -> List[Batch]:
        """RECORDS mode: every record batched on its own (evident intent of
        batcher.py:394-452)."""
        import numpy as np

        from . import _native as N

        out = []
        p = src.parsed
        # k-mers per record from the stream's pos payloads (one device pass)
        km = src.kmers(True)
        pos = p.dev.download(km.pos, km.n, np.uint32 if km.pos_bytes == 4 else np.uint64).astype(np.uint64)
        rec = np.searchsorted(p.rec_seq, pos >> np.uint64(1), side="right") - 1
        bounds = np.searchsorted(rec, np.arange(p.n_records + 1))
        del N
        for r in range(p.n_records):
            b, e = int(bounds[r]), int(bounds[r + 1])
            for s in range(b, e, self.size):
                out.append(Batch.from_source(src, s, min(e, s + self.size), self.size, self.tmp))
        return out or [Batch.from_source(src, 0, 0, self.size, self.tmp)]


class FastaRecordBatcher(BatcherThreading):
    """Batcher of one FASTA record (batcher.py:490-613)."""

    _doReverseComplement = False

    def __init__(self, size: int, threads: int = 1, natype: NATYPES = NATYPES.DNA, tmp: Optional[str] = None):
        super().__init__(size=size, threads=threads, natype=natype, tmp=tmp or tempfile.gettempdir())

    @property
    def doReverseComplement(self) -> bool:
        return self._doReverseComplement

    @doReverseComplement.setter
    def doReverseComplement(self, rc) -> None:
        if type(rc) is not bool:
            raise AssertionError
        self._doReverseComplement = rc

    def do(self, record, k: int, verbose: bool = True) -> "FastaRecordBatcher":
        """k-mers of one (title, sequence) record, batched, on the GPU."""
        import tempfile as _t

        title, seq = record
        with _t.NamedTemporaryFile("wb", suffix=".fa", delete=False) as fh:
            fh.write((">%s\n%s\n" % (title, seq)).encode("utf-8", "surrogateescape"))
            path = fh.name
        try:
            fb = FastaBatcher(FastaBatcher.MODE.KMERS, self.doReverseComplement, self.threads, self.size,
                              self.natype, self.tmp)
            fb.do(path, k, self.FEED_MODE.REPLACE)
        finally:
            os.remove(path)
        self._batches = [b for b in fb.collection]
        return self

    @staticmethod
    def from_parent(parent: "FastaBatcher") -> "FastaRecordBatcher":
        b = FastaRecordBatcher(parent.size, parent.threads, parent.natype, parent.tmp)
        b._doReverseComplement = parent.doReverseComplement
        return b


def load_batches(previous_batches: str, threads: int = 1, re_sort: bool = False) -> List[Batch]:
    """Load batch files written by ``kmer batch`` onto the GPU (-B).

    The reference rejects every non-empty folder (batcher.py:631, §A-5);
    this implements the evident intent: the folder must exist and hold files."""
    if not os.path.isdir(previous_batches) or len(os.listdir(previous_batches)) == 0:
        raise AssertionError(f"folder with previous batches empty or not found: {previous_batches}")
    from .source import BatchFileSource

    logging.info(f"Loading previous batches from '{previous_batches}'...")
    files = sorted(os.path.join(previous_batches, f) for f in os.listdir(previous_batches))
    src = BatchFileSource(engine.default_device(), files)
    out, at = [], 0
    for n in src.file_sizes:
        n = int(n)
        out.append(Batch.from_source(src, at, at + n, max(n, 1), previous_batches))
        at += n
    return out

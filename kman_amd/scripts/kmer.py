"""``kmer`` command group: batch / count / uniq (kmermaid/scripts/*.py).

Same arguments, flags, defaults, outputs and errors as the reference CLI; the
work runs on the GPU through kman_amd (FastaBatcher.do + KJoiner.join).
``hist``, ``sets``, ``screen``, ``classify``, ``compare`` and ``unitigs`` are
this engine's own commands.
"""

from __future__ import annotations

import logging
import os
import resource
import tempfile
import warnings
from typing import Optional

import click

from .. import __version__, engine, launch
from ..batcher import BatcherThreading, FastaBatcher, load_batches
from ..io import copy_batches, input_file_exists, set_tempdir
from ..join import KJoiner, KJoinerThreading
from . import arguments as args

CONTEXT_SETTINGS = dict(help_option_names=["-h", "--help"])

# `kmer count` declares -m twice (batch mode and count mode), exactly like the
# reference (arguments.py:104-115 and 134-149); the later one wins in both.
warnings.filterwarnings("ignore", message="The parameter -m is used more than once")


@click.group(name="kmer", context_settings=CONTEXT_SETTINGS,
             help="K-mer management tools, MI355X engine (kman_amd %s)." % __version__)
@click.version_option(__version__)
def main():
    """Entry point."""


def _batches(input_path, k, reverse, scan_mode, batch_size, batch_mode, threads, tmp, dist=False, fmt="auto",
             min_qual=0, phred_offset=33, hpc=False):
    kw = {"hpc": True} if hpc else {}  # (absent: today's call)
    return (
        FastaBatcher(scan_mode=FastaBatcher.MODE[scan_mode], reverse=reverse, size=batch_size, threads=threads,
                     tmp=tmp, distributed=dist, fmt=fmt, min_qual=min_qual, phred_offset=phred_offset, **kw)
        .do(input_path, k, BatcherThreading.FEED_MODE[batch_mode])
        .collection
    )


@main.command(name="count", context_settings=CONTEXT_SETTINGS, help="""
Count occurrences of all k-mers from INPUT.

\b
Counting modes:
       SEQ_COUNT a tabulation-separated table with sequence and count
       VEC_COUNT / VEC_COUNT_MASKED: abundance vectors; like the reference,
                 they raise NotImplementedError, unless KMAN_VEC_COUNT=1
                 selects this engine's vector writer (INTEGRATION.md §4)
INPUT fasta or fastq file, plain or gzipped.  Launched one process per GPU
(WORLD_SIZE > 1), the join runs across the GPUs into one OUTPUT (a fastq
INPUT runs on rank 0 alone).
""")
@args.input_path()
@args.output_path(file_okay=True)
@args.k()
@args.reverse()
@args.scan_mode()
@args.batch_size()
@args.batch_mode()
@args.previous_batches()
@args.count_mode()
@args.memory_mode()
@args.threads()
@args.tmp()
@args.re_sort()
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.min_count()
@args.max_count()
@args.canonical()
@args.hpc()
def count(input_path: str, output_path: str, k: int, reverse: bool = False, scan_mode: str = "KMERS",
          batch_size: int = 1000000, batch_mode: str = "APPEND", previous_batches: Optional[str] = None,
          count_mode: str = "SEQ_COUNT", memory_mode: str = "NORMAL", threads: int = 1,
          tmp: str = tempfile.gettempdir(), re_sort: bool = False, input_format: str = "auto",
          min_qual: int = 0, phred_offset: str = "33", min_count: int = 1, max_count: Optional[int] = None,
          canonical: bool = False, hpc: bool = False) -> None:
    input_file_exists(input_path)
    _check_min_qual(min_qual, input_path, input_format, previous_batches)
    _check_count_options(min_count, max_count, canonical, count_mode, reverse, previous_batches, hpc=hpc)
    set_tempdir(tmp)
    dist = _multi_gpu(k, previous_batches, count_mode, input_path, input_format, canonical=canonical, hpc=hpc)
    if dist is None:
        return  # (a rank other than 0, for work outside the multi-GPU domain)
    if previous_batches is not None:
        batches = load_batches(previous_batches, threads, re_sort)
    else:
        batches = _batches(input_path, k, reverse, scan_mode, batch_size, batch_mode, threads, tmp, dist,
                           input_format, min_qual, int(phred_offset), hpc)
    joiner = prep_joiner(KJoinerThreading(KJoiner.MODE[count_mode], KJoiner.MEMORY[memory_mode]), len(batches),
                         threads)
    joiner.min_count, joiner.max_count, joiner.canonical = min_count, max_count, canonical
    joiner.join(batches, output_path)
    logging.info("That's all!")


def _check_count_options(min_count: int, max_count: Optional[int], canonical: bool, count_mode: str, reverse: bool,
                         previous_batches: Optional[str], *, hpc: bool = False) -> None:
    """The abundance range, --canonical and --hpc of `kmer count`: what they
    cannot be combined with is refused before any device work or output.
    --hpc follows --canonical's restrictions."""
    filtered = min_count > 1 or max_count is not None
    if max_count is not None and min_count > max_count:
        raise AssertionError("--min-count %d is greater than --max-count %d" % (min_count, max_count))
    if (filtered or canonical) and count_mode != "SEQ_COUNT":
        raise AssertionError("--min-count / --max-count / --canonical need -m SEQ_COUNT, not %s" % count_mode)
    if canonical and reverse:
        raise AssertionError("--canonical with -r: the strands are already folded into one k-mer")
    if canonical and previous_batches is not None:
        raise AssertionError("--canonical with -B: canonical k-mers come from the INPUT, not from reloaded batches")
    if hpc and count_mode != "SEQ_COUNT":
        raise AssertionError("--hpc needs -m SEQ_COUNT, not %s" % count_mode)
    if hpc and reverse:
        raise AssertionError("--hpc with -r: as --canonical, it counts one strand's stream of the INPUT")
    if hpc and previous_batches is not None:
        raise AssertionError("--hpc with -B: the compressed k-mers come from the INPUT, not from reloaded batches")


def _parse_input(dev, path: str, input_format: str, min_qual: int, phred_offset: int, hpc: bool = False, *,
                 keep_text: bool = False, keep_map: bool = False):
    """engine.parse_file, and under --hpc the compression right after it."""
    if keep_text:
        p = engine.parse_file(dev, path, input_format, min_qual, phred_offset, keep_text=True)
    else:  # (not one allocation or call differs from a run without the options)
        p = engine.parse_file(dev, path, input_format, min_qual, phred_offset)
    if not hpc:
        return p
    try:
        return engine.hpc(p, keep_map=keep_map)
    except BaseException:
        p.free()
        raise


def _check_min_qual(min_qual: int, input_path: str, input_format: str,
                    previous_batches: Optional[str] = None) -> None:
    """--min-qual masks bases by the quality line of a fastq INPUT: refused for
    fasta input and for -B reloads, before any device work or output."""
    if min_qual > 0 and (previous_batches is not None or not _is_fastq(input_path, input_format)):
        raise AssertionError("--min-qual needs fastq input")


def _is_fastq(input_path: Optional[str], input_format: str) -> bool:
    """The input's format as every rank decides it alone, from the file's head."""
    if input_format != "auto":
        return input_format == "fastq"
    return input_path is not None and engine.sniff_file(input_path) == "fastq"


def _multi_gpu(k: int, previous_batches: Optional[str], count_mode: str = "SEQ_COUNT",
               input_path: Optional[str] = None, input_format: str = "auto", *,
               canonical: bool = False, hpc: bool = False) -> Optional[bool]:
    """Under a one-process-per-GPU launch (kman_amd/launch.py): True = this
    rank joins across the GPUs; False = the single-GPU path (no launch, or
    rank 0 alone for work outside the multi-GPU domain: k > 32, -B reloads,
    VEC_* modes, fastq input, count --canonical or --hpc); None = a rank that leaves
    that work to rank 0."""
    if not launch.distributed():
        return False
    if canonical and k > 1:
        launch.log_solo("count --canonical")  # (ordered canonical rows across ranks: DESIGN §8)
        return False if launch.solo_rank() else None
    if hpc and k > 1:
        launch.log_solo("count --hpc")  # (a run may cross a shard's cut: DESIGN §8)
        return False if launch.solo_rank() else None
    if k > 1 and previous_batches is None and _is_fastq(input_path, input_format):
        launch.log_solo("fastq input")  # (the byte-range shards cut FASTA only)
        return False if launch.solo_rank() else None
    if k <= 1 or (k <= engine.MAX_K and previous_batches is None and count_mode in ("SEQ_COUNT", "UNIQUE")):
        return True  # (k <= 1 raises in FastaBatcher.do on every rank, as the reference)
    launch.log_solo("k=%d%s%s" % (k, " -B" if previous_batches else "", "" if count_mode == "SEQ_COUNT"
                                  else " " + count_mode))
    return False if launch.solo_rank() else None


def prep_joiner(joiner: KJoinerThreading, n_batches: int, threads: int = 1) -> KJoinerThreading:
    """kmer_count.py:123-144 (the file-descriptor limit is irrelevant on the
    GPU path, but the joiner settings are kept)."""
    joiner.threads = threads
    joiner.batch_size = max(2, int(n_batches / max(1, threads)))
    try:
        lo, hi = resource.getrlimit(resource.RLIMIT_NOFILE)
        joiner.batch_size = min(joiner.batch_size, hi if hi > 0 else joiner.batch_size)
    except (ValueError, OSError):
        pass
    return joiner


@main.command(name="uniq", context_settings=CONTEXT_SETTINGS,
              help="Extract all k-mers that appear only once in the INPUT fasta or fastq file, plain or gzipped.")
@args.input_path()
@args.output_path(file_okay=True)
@args.k()
@args.reverse()
@args.scan_mode()
@args.batch_size()
@args.batch_mode()
@args.previous_batches()
@args.threads()
@args.tmp()
@args.re_sort()
@args.input_format()
@args.min_qual()
@args.phred_offset()
def uniq(input_path: str, output_path: str, k: int, reverse: bool = False, scan_mode: str = "KMERS",
         batch_size: int = 1000000, batch_mode: str = "APPEND", previous_batches: Optional[str] = None,
         threads: int = 1, tmp: str = tempfile.gettempdir(), re_sort: bool = False,
         input_format: str = "auto", min_qual: int = 0, phred_offset: str = "33") -> None:
    input_file_exists(input_path)
    _check_min_qual(min_qual, input_path, input_format, previous_batches)
    set_tempdir(tmp)
    dist = _multi_gpu(k, previous_batches, "UNIQUE", input_path, input_format)
    if dist is None:
        return
    if previous_batches is not None:
        batches = load_batches(previous_batches, threads, re_sort)
    else:
        batches = _batches(input_path, k, reverse, scan_mode, batch_size, batch_mode, threads, tmp, dist,
                           input_format, min_qual, int(phred_offset))
    joiner = KJoinerThreading()
    joiner.threads = threads
    joiner.batch_size = max(2, int(len(batches) / max(1, threads)))
    joiner.join(batches, output_path)
    logging.info("That's all!")


@main.command(name="batch", context_settings=CONTEXT_SETTINGS, help="""
Generate batches of k-mers from an INPUT fasta or fastq file, plain or gzipped.

Batches are written to an OUTPUT folder, which must be empty or non-existent.
""")
@args.input_path()
@args.output_path(dir_okay=True)
@args.k()
@args.reverse()
@args.scan_mode()
@args.batch_size()
@args.batch_mode()
@args.threads()
@args.tmp()
@args.compress()
@args.input_format()
@args.min_qual()
@args.phred_offset()
def batch(input_path: str, output_path: str, k: int, reverse: bool = False, scan_mode: str = "KMERS",
          batch_size: int = 1000000, batch_mode: str = "APPEND", threads: int = 1,
          tmp: str = tempfile.gettempdir(), compress: bool = False, input_format: str = "auto",
          min_qual: int = 0, phred_offset: str = "33") -> None:
    input_file_exists(input_path)
    _check_min_qual(min_qual, input_path, input_format)
    if launch.distributed() and not launch.solo_rank():
        launch.log_solo("kmer batch")  # (the batch files are one stream's consecutive chunks)
        return
    if os.path.isdir(output_path) and len(os.listdir(output_path)) != 0:
        raise AssertionError("output folder must be empty or non-existent.")
    set_tempdir(tmp)
    os.makedirs(output_path, exist_ok=True)
    try:
        copy_batches(_batches(input_path, k, reverse, scan_mode, batch_size, batch_mode, threads, tmp, False,
                              input_format, min_qual, int(phred_offset)), output_path, compress)
    except IOError as e:
        logging.error(f"Unable to write to output directory '{output_path}'.\n{e}")
    logging.info("That's all!")


@main.command(name="hist", context_settings=CONTEXT_SETTINGS, help="""
Abundance spectrum of the (canonical) k-mers of INPUT: one line per
abundance c, "c<TAB>number of distinct k-mers seen c times".

Not part of the reference kman CLI (SURVEY.md §8f-1, BASELINE config 5):
canonical k-mers are min(k-mer, reverse complement); for odd k their counts
are the `kmer count -r` rows whose sequence is <= its reverse complement.
INPUT fasta or fastq file, plain or gzipped.
""")
@args.input_path()
@args.output_path(file_okay=True)
@args.k()
@click.option("--forward", is_flag=True, help="Count forward k-mers instead of canonical ones.")
@click.option("--max-count", type=click.INT, default=10000, show_default=True,
              help="Abundances from this one up share the last line (>=N).")
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.hpc()
def hist(input_path: str, output_path: str, k: int, forward: bool = False, max_count: int = 10000,
         input_format: str = "auto", min_qual: int = 0, phred_offset: str = "33", hpc: bool = False) -> None:
    input_file_exists(input_path)
    _check_min_qual(min_qual, input_path, input_format)
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    fastq = launch.distributed() and _is_fastq(input_path, input_format)
    if fastq and not launch.solo_rank():
        launch.log_solo("fastq input")
        return
    if launch.distributed() and k > engine.MAX_K and not launch.solo_rank():
        launch.log_solo("kmer hist k=%d" % k)
        return
    if launch.distributed() and hpc and not launch.solo_rank():
        launch.log_solo("kmer hist --hpc")  # (a run may cross a shard's cut)
        return
    if launch.distributed() and k <= engine.MAX_K and not fastq and not hpc:
        # every rank counts its shard's (canonical) k-mers, the spectrum is
        # all-reduced, rank 0 writes it
        src = launch.ShardedSource(engine.default_device(), input_path, k, False)
        try:
            h = src.hist(max_count + 1, canonical=not forward)
        finally:
            src.free()
        if launch.solo_rank():
            with open(output_path, "wb") as fh:
                fh.write(engine.format_hist(h))
        logging.info("That's all!")
        return
    kw = {"hpc": True} if hpc else {}  # (absent: today's call)
    h = engine.abundance_hist(engine.read_input(input_path), k, canonical=not forward, nbins=max_count + 1,
                              fmt=input_format, min_qual=min_qual, phred_offset=int(phred_offset), **kw)
    with open(output_path, "wb") as fh:
        fh.write(engine.format_hist(h))
    logging.info("That's all!")


@main.command(name="sets", context_settings=CONTEXT_SETTINGS, help="""
Set operations on the k-mers of two inputs: the k-mers of INPUT_A that also
occur in INPUT_B (--op intersect), those that do not (--op subtract), or the
k-mers of either (--op union), written to OUTPUT as `count` writes them, one
"SEQ<TAB>N" line per k-mer in ascending order.

Not part of the reference kman CLI.  Both inputs are counted on the GPU and
their tables are matched there (kman_match_counts); no table goes through a
text file.  INPUT_A, INPUT_B: fasta or fastq files, plain or gzipped, each
detected on its own.  K <= 32.  -L / -U select by the count that is written.
Launched one process per GPU, the command runs on rank 0 alone.
""")
@args.input_a()
@args.input_b()
@args.output_path(file_okay=True)
@args.k()
@args.set_op()
@args.set_counts()
@args.reverse()
@args.canonical()
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.min_count()
@args.max_count()
@args.hpc()
def sets(input_a: str, input_b: str, output_path: str, k: int, op: str, counts: Optional[str] = None,
         reverse: bool = False, canonical: bool = False, input_format: str = "auto", min_qual: int = 0,
         phred_offset: str = "33", min_count: int = 1, max_count: Optional[int] = None, hpc: bool = False) -> None:
    input_file_exists(input_a)
    input_file_exists(input_b)
    fastq = [_is_fastq(p, input_format) for p in (input_a, input_b)]
    _check_sets_options(k, op, counts, reverse, canonical, min_qual, fastq, min_count, max_count)
    if launch.distributed() and not launch.solo_rank():
        launch.log_solo("kmer sets")  # (two whole tables on one GPU: DESIGN §8)
        return
    dev = engine.default_device()
    tables = []
    try:
        for path, fq in zip((input_a, input_b), fastq):
            # (A's parse buffers are freed before B is read)
            p = _parse_input(dev, path, input_format, min_qual if fq else 0, int(phred_offset), hpc)
            try:
                engine.check_empty_names(p, k)
                r = engine.join_groups(p, k, reverse, "count", canonical=canonical)
            finally:
                p.free()
            tables.append(r if r is not None else engine.empty_count(dev, k))  # (no k-mers: the empty set)
        r = engine.set_op(dev, tables[0], tables[1], op, counts, min_count, max_count)
        try:
            with open(output_path, "wb") as fh:
                engine.emit_count(dev, r, fh)
        finally:
            engine.free_result(r)
    finally:
        for t in tables:
            engine.free_result(t)
    logging.info("That's all!")


def _check_sets_options(k: int, op: str, counts: Optional[str], reverse: bool, canonical: bool, min_qual: int,
                        fastq, min_count: int, max_count: Optional[int]) -> None:
    """What `kmer sets` refuses, before any device work or output."""
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    if k > engine.MAX_K:
        raise AssertionError("kmer sets takes K <= %d (one 64-bit key per k-mer), got %d: word keys are a stated "
                             "limit of this command" % (engine.MAX_K, k))
    if canonical and reverse:
        raise AssertionError("--canonical with -r: the strands are already folded into one k-mer")
    if min_qual > 0 and not any(fastq):
        raise AssertionError("--min-qual needs fastq input: neither INPUT_A nor INPUT_B is fastq")
    engine.check_set_op(op, counts)
    if max_count is not None and min_count > max_count:
        raise AssertionError("--min-count %d is greater than --max-count %d" % (min_count, max_count))


@main.command(name="screen", context_settings=CONTEXT_SETTINGS, help="""
Per-read k-mer hits against a table: for every record of READS, how many of
its k-mers occur among the k-mers of TABLE_INPUT, written to OUTPUT as one
"NAME<TAB>K-MERS<TAB>HITS<TAB>SUM" line per record in input order (SUM: the
sum over the record's found k-mers of their counts in TABLE_INPUT).

Not part of the reference kman CLI.  TABLE_INPUT is counted on the GPU and
the reads' k-mers are looked up there (kman_screen_records); neither goes
through a text file.  READS, TABLE_INPUT: fasta or fastq files, plain or
gzipped, each detected on its own.  K <= 32.  -L / -U select the k-mers of
TABLE_INPUT that are looked up; --min-hits / --min-frac / -v the records that
are written.  --median adds a fifth column "<TAB>MEDIAN": the median over the
record's k-mers of their counts in TABLE_INPUT (0 for a k-mer that is not
there), selected on the GPU (kman_window_counts, kman_record_quantile); counts
above 4294967294 enter it as 4294967294.  --min-median / --max-median select
records by it and imply --median; a record without k-mers has median 0.
Screened against itself (READS = TABLE_INPUT, --canonical) the median is the
read's coverage estimate.  --solid C adds two last columns "<TAB>START<TAB>END"
(after MEDIAN when that is there): the longest stretch of the record whose
k-mers all have a count of at least C in TABLE_INPUT, the leftmost of equal
ones, found on the GPU (kman_record_runs); one threshold per call.  START and
END count the record's sequence characters from 0, END exclusive: N and other
non-ACGT letters count (and end a stretch, as do bases masked by -q), line
breaks of a multi-line fasta do not; a record without such a k-mer has 0 and 0.
--min-solid-len N selects records with END - START >= N; --bed FILE also writes
"NAME<TAB>START<TAB>END" for the written records that have a stretch, the
regions that e.g. `seqtk subseq` cuts out; both need --solid.  --reads-out
FILE also writes the written records themselves to FILE, byte for byte as READS
has them, cut out of the input text on the GPU (kman_cut_records); FILE is
never compressed.  --trim cuts each of them to its solid stretch: the header
line, the sequence columns [START, END), the "+" line and the same columns of
the quality line, every line ended by "\n"; reads without a stretch are left
out as --bed leaves them out; it needs --solid, --reads-out and fastq READS.
--correct (with --solid C) first repairs isolated substitution errors on the
GPU (kman_correct_sites, kman_apply_fixes): at most K k-mers in a row with a
count below C, next to a k-mer with a count of at least C, name one base, and
it is replaced when exactly one other base lifts every k-mer over it to C.
Every column, --bed and every selection then describe the corrected reads, and
one last column "<TAB>FIXES" counts the record's replaced bases; --reads-out
writes the corrected records (fastq READS only; cut after the correction under
--trim), quality values unchanged.  One pass: run the command on its output to
correct again.
--mate READS2 (-2) reads paired files, record i of READS2 the mate of record i
of READS (same record count; same names, a trailing /1 or /2 aside);
--interleaved reads the pairs from READS alone, mates as neighbours.  The
mates' bases are interleaved on the GPU (kman_zip_records) and every k-mer is
looked up once: OUTPUT has one line per pair, NAME mate 1's, and K-MERS, HITS,
SUM and MEDIAN are joint over both mates' k-mers (no k-mer spans the mates);
--min-hits, --min-frac, -v, --min-median and --max-median select pairs.
--solid C then writes "START<TAB>END<TAB>START2<TAB>END2", each mate's own
stretch, and --min-solid-len N keeps a pair when both stretches have N bases.
--reads-out FILE with --reads-out2 FILE2 (both or neither) writes the written
pairs' mates from READS and from READS2: record i of FILE and of FILE2 are
always mates, a pair is kept or dropped whole; --trim cuts each mate to its own
stretch and leaves out a pair with a mate that has none.  Under --interleaved
--reads-out writes one interleaved file.  Pairs take neither --bed nor
--correct, and READS and READS2 must both be fastq or both be fasta.
Launched one process per GPU, the command runs on rank 0 alone.
""")
@args.reads_path()
@args.table_input()
@args.output_path(file_okay=True)
@args.k()
@args.screen_canonical()
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.table_min_count()
@args.table_max_count()
@args.min_hits()
@args.min_frac()
@args.invert()
@args.median()
@args.min_median()
@args.max_median()
@args.solid()
@args.min_solid_len()
@args.bed()
@args.reads_out()
@args.trim()
@args.correct()
@args.mate()
@args.interleaved()
@args.reads_out2()
@args.index_bits()
@args.hpc()
def screen(reads_path: str, table_input: str, output_path: str, k: int, canonical: bool = False,
           input_format: str = "auto", min_qual: int = 0, phred_offset: str = "33", min_count: int = 1,
           max_count: Optional[int] = None, min_hits: int = 0, min_frac: float = 0.0, invert: bool = False,
           index_bits: Optional[int] = None, median: bool = False, min_median: Optional[int] = None,
           max_median: Optional[int] = None, solid: Optional[int] = None, min_solid_len: Optional[int] = None,
           bed_path: Optional[str] = None, reads_out: Optional[str] = None, trim: bool = False,
           correct: bool = False, mate_path: Optional[str] = None, interleaved: bool = False,
           reads_out2: Optional[str] = None, hpc: bool = False) -> None:
    input_file_exists(reads_path)
    input_file_exists(table_input)
    fastq = [_is_fastq(p, input_format) for p in (reads_path, table_input)]
    fastq_mate = None
    if mate_path is not None:
        input_file_exists(mate_path)
        fastq_mate = _is_fastq(mate_path, input_format)
    _check_screen_options(k, min_qual, fastq, min_count, max_count, min_hits, min_frac, index_bits, min_median,
                          max_median, solid, min_solid_len, bed_path, reads_out=reads_out, trim=trim,
                          output_path=output_path, correct=correct, mate_path=mate_path, interleaved=interleaved,
                          reads_out2=reads_out2, fastq_mate=fastq_mate, hpc=hpc)
    median = median or min_median is not None or max_median is not None
    if launch.distributed() and not launch.solo_rank():
        launch.log_solo("kmer screen")  # (the table and the reads on one GPU: DESIGN §8)
        return
    dev = engine.default_device()
    table = None
    try:
        # (the table input's parse buffers are freed before READS is parsed)
        p = _parse_input(dev, table_input, input_format, min_qual if fastq[1] else 0, int(phred_offset), hpc)
        try:
            engine.check_empty_names(p, k)
            table = engine.join_groups(p, k, False, "count", canonical=canonical)
        finally:
            p.free()
        if table is None:
            table = engine.empty_count(dev, k)  # (no k-mers: the empty table, every read has 0 hits)
        elif min_count > 1 or max_count is not None:
            ranged = engine.filtered_copy(dev, table, min_count, max_count)
            engine.free_result(table)
            table = ranged
        if mate_path is not None or interleaved:
            _screen_pairs(dev, table, reads_path, mate_path, output_path, canonical, input_format,
                          min_qual if fastq[0] else 0, int(phred_offset), min_hits, min_frac, invert, index_bits,
                          median, min_median, max_median, solid, min_solid_len, reads_out, reads_out2, trim, hpc)
            logging.info("That's all!")
            return
        p = _parse_input(dev, reads_path, input_format, min_qual if fastq[0] else 0, int(phred_offset), hpc,
                         keep_text=reads_out is not None, keep_map=hpc and solid is not None)
        try:
            span = fixes = None
            if correct:  # (then every step below reads the corrected codes, and --reads-out the corrected text)
                fixes = engine.correct(p, table, canonical, solid, index_bits=index_bits)
            if solid is not None:
                stats, med, runs = engine.screen_solid(p, table, canonical, solid, median=median,
                                                       index_bits=index_bits)
                span = engine.solid_spans(runs, k)
                if hpc:  # (START, END, --min-solid-len, --bed and --trim: the original record's columns)
                    span = engine.hpc_spans(p, span)
                keep = engine.screen_keep(stats, min_hits, min_frac, invert, median=med, min_median=min_median,
                                          max_median=max_median, span=span, min_solid_len=min_solid_len)
            elif median:
                stats, med = engine.screen_median(p, table, canonical, index_bits=index_bits)
                keep = engine.screen_keep(stats, min_hits, min_frac, invert, median=med, min_median=min_median,
                                          max_median=max_median)
            else:  # (no new kernel, today's bytes)
                stats, med = engine.screen(p, table, canonical, index_bits=index_bits), None
                keep = engine.screen_keep(stats, min_hits, min_frac, invert)
            with open(output_path, "wb") as fh:
                if fixes is None:  # (today's call, today's bytes)
                    engine.emit_screen(p, stats, keep, fh, median=med, span=span)
                else:
                    engine.emit_screen(p, stats, keep, fh, median=med, span=span, fixes=fixes)
            if bed_path is not None:
                with open(bed_path, "wb") as fh:
                    engine.emit_bed(p, span, keep, fh)
            if reads_out is not None:
                with open(reads_out, "wb") as fh:
                    engine.emit_reads(p, keep, fh, span=span if trim else None, trim=trim)
        finally:
            p.free()
    finally:
        engine.free_result(table)
    logging.info("That's all!")


def _parse_pairs(dev, reads_path: str, mate_path: Optional[str], input_format: str, min_qual: int,
                 phred_offset: int, keep_text: bool, hpc: bool = False):
    """(mate view, pair view) of READS and READS2 (zipped on the GPU), or of an
    interleaved READS alone (`mate_path` None).  Freeing the mate view frees
    everything; the pair view borrows its codes.  `hpc`: every input is
    compressed right after its parse, before the zip."""
    def parse(path):
        return _parse_input(dev, path, input_format, min_qual, phred_offset, hpc, keep_text=keep_text)

    p1 = parse(reads_path)
    if mate_path is None:
        try:
            return p1, engine.pairs_of(p1)
        except BaseException:
            p1.free()
            raise
    p2 = None
    try:
        p2 = parse(mate_path)
        pm = engine.zip_pairs(p1, p2)
    except BaseException:
        p1.free()
        if p2 is not None:
            p2.free()
        raise
    return pm, engine.pair_view(pm)


def _screen_pairs(dev, table, reads_path: str, mate_path: Optional[str], output_path: str, canonical: bool,
                  input_format: str, min_qual: int, phred_offset: int, min_hits: int, min_frac: float, invert: bool,
                  index_bits: Optional[int], median: bool, min_median: Optional[int], max_median: Optional[int],
                  solid: Optional[int], min_solid_len: Optional[int], reads_out: Optional[str],
                  reads_out2: Optional[str], trim: bool, hpc: bool = False) -> None:
    """`kmer screen --mate` / `--interleaved`: one line per pair, the listed
    pairs' records in step."""
    pm, pv = _parse_pairs(dev, reads_path, mate_path, input_format, min_qual, phred_offset, reads_out is not None,
                          hpc)
    try:
        stats, med, runs = engine.screen_pairs(pm, pv, table, canonical, median=median, min_count=solid,
                                               index_bits=index_bits)
        span = engine.solid_spans(runs, table.k) if runs is not None else None
        keep = engine.screen_keep(stats, min_hits, min_frac, invert, median=med, min_median=min_median,
                                  max_median=max_median, span=engine.pair_min_span(span) if span is not None else None,
                                  min_solid_len=min_solid_len)
        with open(output_path, "wb") as fh:
            engine.emit_screen_pairs(pv, stats, keep, fh, median=med, span=span)
        if reads_out is not None and reads_out2 is not None:
            with open(reads_out, "wb") as f1, open(reads_out2, "wb") as f2:
                engine.emit_pair_reads(pm, keep, f1, f2, span=span if trim else None, trim=trim)
        elif reads_out is not None:
            with open(reads_out, "wb") as fh:
                engine.emit_pair_reads(pm, keep, fh, span=span if trim else None, trim=trim)
    finally:
        pm.free()


def _check_screen_options(k: int, min_qual: int, fastq, min_count: int, max_count: Optional[int], min_hits: int,
                          min_frac: float, index_bits: Optional[int], min_median: Optional[int] = None,
                          max_median: Optional[int] = None, solid: Optional[int] = None,
                          min_solid_len: Optional[int] = None, bed_path: Optional[str] = None, *,
                          reads_out: Optional[str] = None, trim: bool = False,
                          output_path: Optional[str] = None, correct: bool = False,
                          mate_path: Optional[str] = None, interleaved: bool = False,
                          reads_out2: Optional[str] = None, fastq_mate: Optional[bool] = None,
                          hpc: bool = False) -> None:
    """What `kmer screen` refuses, before any device work or output."""
    if hpc and correct:
        raise AssertionError("--hpc with --correct: a substitution changes the runs, so the compressed reads "
                             "cannot be repaired in place")
    if hpc and solid is not None and (mate_path is not None or interleaved):
        raise AssertionError("--hpc with --solid is not offered for read pairs: the map to original columns is "
                             "not zipped")
    if mate_path is not None and interleaved:
        raise AssertionError("--mate and --interleaved exclude each other: the pairs are in two files or in one")
    if reads_out2 is not None and mate_path is None:
        raise AssertionError("--reads-out2 needs --mate: it takes the second mates from READS2%s"
                             % (" (--interleaved writes one interleaved --reads-out file)" if interleaved else ""))
    if mate_path is not None or interleaved:
        if bed_path is not None:
            raise AssertionError("--bed is not offered for read pairs: one region file for two read files is "
                                 "ambiguous")
        if correct:
            raise AssertionError("--correct is not offered for read pairs: applying the fixes to two source texts "
                                 "is a later change")
    if mate_path is not None:
        if fastq_mate is not None and bool(fastq_mate) != bool(fastq[0]):
            raise AssertionError("READS is %s and READS2 is %s: mixed formats are not offered, both must be fastq or "
                                 "both fasta" % tuple("fastq" if f else "fasta" for f in (fastq[0], fastq_mate)))
        if (reads_out is None) != (reads_out2 is None):
            raise AssertionError("with --mate, --reads-out and --reads-out2 go together (both or neither): a pair is "
                                 "written to two files that stay in step")
    if reads_out2 is not None:
        if reads_out2.endswith(".gz"):
            raise AssertionError("--reads-out2 writes plain text: %r ends in .gz" % reads_out2)
        for name, other in (("OUTPUT", output_path), ("--reads-out", reads_out)):
            if other is not None and _same_path(reads_out2, other):
                raise AssertionError("--reads-out2 and %s name the same file, %r" % (name, reads_out2))
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    if k > engine.MAX_K:
        raise AssertionError("kmer screen takes K <= %d (one 64-bit key per k-mer), got %d: word keys are a stated "
                             "limit of this command" % (engine.MAX_K, k))
    if min_qual > 0 and not any(fastq):
        raise AssertionError("--min-qual needs fastq input: neither READS nor TABLE_INPUT is fastq")
    if max_count is not None and min_count > max_count:
        raise AssertionError("--min-count %d is greater than --max-count %d" % (min_count, max_count))
    if not 0.0 <= min_frac <= 1.0:  # (a NaN is refused too)
        raise AssertionError("--min-frac must be in [0, 1], got %r" % min_frac)
    if min_hits < 0:
        raise AssertionError("--min-hits must be >= 0, got %d" % min_hits)
    if index_bits is not None and index_bits > 2 * k:
        raise AssertionError("--index-bits %d is more than the 2 K = %d bits of a k-mer" % (index_bits, 2 * k))
    for name, v in (("--min-median", min_median), ("--max-median", max_median)):
        if v is not None and v < 0:
            raise AssertionError("%s must be >= 0, got %d" % (name, v))
    if min_median is not None and max_median is not None and min_median > max_median:
        raise AssertionError("--min-median %d is greater than --max-median %d" % (min_median, max_median))
    if solid is not None and not 1 <= solid <= 4294967294:
        raise AssertionError("--solid must be in [1, 4294967294], got %d" % solid)
    if min_solid_len is not None:
        if solid is None:
            raise AssertionError("--min-solid-len needs --solid")
        if min_solid_len < 0:
            raise AssertionError("--min-solid-len must be >= 0, got %d" % min_solid_len)
    if bed_path is not None and solid is None:
        raise AssertionError("--bed needs --solid")
    if trim:
        if solid is None:
            raise AssertionError("--trim needs --solid")
        if reads_out is None:
            raise AssertionError("--trim needs --reads-out")
        if not fastq[0]:
            raise AssertionError("--trim needs fastq READS")
    if correct:
        if solid is None:
            raise AssertionError("--correct needs --solid")
        if reads_out is not None and not fastq[0]:
            raise AssertionError("--correct with --reads-out needs fastq READS")
    if reads_out is not None:
        if reads_out.endswith(".gz"):
            raise AssertionError("--reads-out writes plain text: %r ends in .gz" % reads_out)
        for name, other in (("OUTPUT", output_path), ("--bed", bed_path)):
            if other is not None and _same_path(reads_out, other):
                raise AssertionError("--reads-out and %s name the same file, %r" % (name, reads_out))


def _same_path(a: str, b: str) -> bool:
    return os.path.abspath(a) == os.path.abspath(b)


@main.command(name="classify", context_settings=CONTEXT_SETTINGS, help="""
Assign reads among references: for every record of READS, which of the --ref
files holds most of its k-mers, written to OUTPUT as one
"NAME<TAB>K-MERS<TAB>LABEL<TAB>HITS<TAB>SECOND" line per record in input
order (HITS: the record's k-mers found in the best reference, SECOND: in the
best of the others).

Not part of the reference kman CLI.  Every --ref is counted on the GPU and the
tables are united into one coloured table there: each k-mer of any reference
with the set of references that hold it.  The reads' k-mers are looked up in
it once, whatever the number of references (kman_classify_records,
kman_classify_pick); nothing goes through a text file.  READS and every
--ref: fasta or fastq files, plain or gzipped, each detected on its own.
K <= 32; 1 to 64 --ref.  LABEL is the reference's label (its file name
without a trailing .gz and then one extension), "?" for an ambiguous record
(the best reference leads by fewer than --min-margin k-mers) and "-" for an
unassigned one (fewer than --min-hits k-mers, never with 0, or less than
--min-frac of the record's k-mers).  -L / -U select the k-mers of each
reference, by their count in that reference.  --specific counts a k-mer only
when exactly one reference holds it, so k-mers shared between references
(human and mouse, host and vector) vote for none.  --hits appends one column
per reference.  --summary FILE writes "LABEL<TAB>TABLE_KMERS<TAB>READS" per
reference (its k-mers after -L / -U, the records assigned to it), then
"?<TAB>0<TAB>N" and "-<TAB>0<TAB>N".  --reads-out-prefix P writes the
records themselves to P.LABEL.fq (.fa for fasta READS) per reference,
P.ambiguous.* and P.unassigned.*, byte for byte as READS has them, cut out on
the GPU (kman_cut_records) and never compressed.
--mate READS2 (-2) reads paired files, record i of READS2 the mate of record i
of READS (same record count; same names, a trailing /1 or /2 aside; both fastq
or both fasta); --interleaved reads the pairs from READS alone, mates as
neighbours.  The mates' bases are interleaved on the GPU (kman_zip_records)
and a pair gets ONE label, from the k-mers of both mates: OUTPUT has one line
per pair (NAME mate 1's), --hits and --summary count pairs.
--reads-out-prefix then writes P.LABEL.1.fq from READS and P.LABEL.2.fq from
READS2 (record i of the two are always mates), under --interleaved one
interleaved P.LABEL.fq.
Launched one process per GPU, the command runs on rank 0 alone.
""")
@args.reads_path()
@args.output_path(file_okay=True)
@args.k()
@args.refs()
@args.classify_canonical()
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.ref_min_count()
@args.ref_max_count()
@args.specific()
@args.classify_min_hits()
@args.classify_min_frac()
@args.min_margin()
@args.hits()
@args.summary()
@args.reads_out_prefix()
@args.mate()
@args.interleaved()
@args.index_bits()
@args.hpc()
def classify(reads_path: str, output_path: str, k: int, refs=(), canonical: bool = False, input_format: str = "auto",
             min_qual: int = 0, phred_offset: str = "33", min_count: int = 1, max_count: Optional[int] = None,
             specific: bool = False, min_hits: int = 1, min_frac: float = 0.0, min_margin: int = 1,
             hits: bool = False, summary_path: Optional[str] = None, reads_out_prefix: Optional[str] = None,
             index_bits: Optional[int] = None, mate_path: Optional[str] = None, interleaved: bool = False,
             hpc: bool = False) -> None:
    input_file_exists(reads_path)
    refs = list(refs)
    for path in refs:
        input_file_exists(path)
    fastq = [_is_fastq(p, input_format) for p in [reads_path] + refs]
    labels = [ref_label(path) for path in refs]
    ext = "fq" if fastq[0] else "fa"
    paired = mate_path is not None or interleaved
    if paired:
        _check_pair_inputs(mate_path, interleaved, fastq[0], input_format)
    if mate_path is not None:  # (two files per class)
        pair_outs = _classify_pair_outputs(reads_out_prefix, labels, ext)
        outs = [(o[0], path) for o in pair_outs for path in o[1:]]
    else:
        outs = pair_outs = _classify_outputs(reads_out_prefix, labels, ext)
    _check_classify_options(k, labels, min_qual, fastq, min_count, max_count, min_hits, min_frac, min_margin,
                            index_bits, output_path, summary_path, outs)
    if launch.distributed() and not launch.solo_rank():
        launch.log_solo("kmer classify")  # (the coloured table and the reads on one GPU: DESIGN §8)
        return
    dev = engine.default_device()
    nc = len(refs)
    tables, ctable, table_kmers = [], None, []
    try:
        for path, fq in zip(refs, fastq[1:]):
            # (a reference's parse buffers are freed before the next one is read)
            p = _parse_input(dev, path, input_format, min_qual if fq else 0, int(phred_offset), hpc)
            try:
                engine.check_empty_names(p, k)
                t = engine.join_groups(p, k, False, "count", canonical=canonical)
            finally:
                p.free()
            if t is None:
                t = engine.empty_count(dev, k)  # (no k-mers: a colour that is never hit)
            elif min_count > 1 or max_count is not None:
                ranged = engine.filtered_copy(dev, t, min_count, max_count)
                engine.free_result(t)
                t = ranged
            tables.append(t)
            table_kmers.append(int(t.n))
        ctable = engine.color_table(dev, tables)  # (frees each table as it is folded in)
        index = engine.table_index(dev, ctable, index_bits)
        try:
            if paired:
                _classify_pairs(dev, ctable, nc, index, reads_path, mate_path, output_path, canonical, specific,
                                input_format, min_qual if fastq[0] else 0, int(phred_offset), min_hits, min_frac,
                                min_margin, hits, summary_path, labels, table_kmers, pair_outs, index_bits, hpc)
                logging.info("That's all!")
                return
            p = _parse_input(dev, reads_path, input_format, min_qual if fastq[0] else 0, int(phred_offset), hpc,
                             keep_text=reads_out_prefix is not None)
            try:
                res = engine.classify(p, ctable, nc, canonical, specific, index=index, index_bits=index_bits,
                                      planes=hits)
                windows, best, nhits, second = res[:4]
                assign = engine.classify_assign(windows, best, nhits, second, min_hits, min_frac, min_margin)
                with open(output_path, "wb") as fh:
                    engine.emit_classify(p, labels, windows, assign, nhits, second, fh,
                                         planes=res[4] if hits else None)
                if summary_path is not None:
                    with open(summary_path, "wb") as fh:
                        fh.write(classify_summary(labels, table_kmers, assign))
                for value, path in outs:
                    with open(path, "wb") as fh:
                        engine.emit_reads(p, (assign == value).astype("uint8"), fh)
            finally:
                p.free()
        finally:
            index.free()
    finally:
        for t in tables:
            engine.free_result(t)
        engine.free_result(ctable)
    logging.info("That's all!")


def _classify_pairs(dev, ctable, nc: int, index, reads_path: str, mate_path: Optional[str], output_path: str,
                    canonical: bool, specific: bool, input_format: str, min_qual: int, phred_offset: int,
                    min_hits: int, min_frac: float, min_margin: int, hits: bool, summary_path: Optional[str], labels,
                    table_kmers, pair_outs, index_bits: Optional[int], hpc: bool = False) -> None:
    """`kmer classify --mate` / `--interleaved`: one label and one line per
    pair, the classes' records in step."""
    pm, pv = _parse_pairs(dev, reads_path, mate_path, input_format, min_qual, phred_offset, bool(pair_outs), hpc)
    try:
        res = engine.classify(pv, ctable, nc, canonical, specific, index=index, index_bits=index_bits, planes=hits)
        windows, best, nhits, second = res[:4]
        assign = engine.classify_assign(windows, best, nhits, second, min_hits, min_frac, min_margin)
        with open(output_path, "wb") as fh:
            engine.emit_classify(pv, labels, windows, assign, nhits, second, fh, planes=res[4] if hits else None)
        if summary_path is not None:
            with open(summary_path, "wb") as fh:
                fh.write(classify_summary(labels, table_kmers, assign))
        for out in pair_outs:
            keep = (assign == out[0]).astype("uint8")
            if len(out) == 3:
                with open(out[1], "wb") as f1, open(out[2], "wb") as f2:
                    engine.emit_pair_reads(pm, keep, f1, f2)
            else:
                with open(out[1], "wb") as fh:
                    engine.emit_pair_reads(pm, keep, fh)
    finally:
        pm.free()


def _check_pair_inputs(mate_path: Optional[str], interleaved: bool, fastq_reads: bool, input_format: str) -> None:
    """What `kmer classify` refuses of --mate / --interleaved, before any device work."""
    if mate_path is not None and interleaved:
        raise AssertionError("--mate and --interleaved exclude each other: the pairs are in two files or in one")
    if mate_path is not None:
        input_file_exists(mate_path)
        fastq_mate = _is_fastq(mate_path, input_format)
        if bool(fastq_mate) != bool(fastq_reads):
            raise AssertionError("READS is %s and READS2 is %s: mixed formats are not offered, both must be fastq or "
                                 "both fasta" % tuple("fastq" if f else "fasta" for f in (fastq_reads, fastq_mate)))


def _classify_pair_outputs(prefix: Optional[str], labels, ext: str):
    """(assignment value, path of the first mates, path of the second mates) of
    every --reads-out-prefix class under --mate."""
    if prefix is None:
        return []
    names = [(c, lab) for c, lab in enumerate(labels)] + [(engine.AMBIGUOUS, "ambiguous"),
                                                          (engine.UNASSIGNED, "unassigned")]
    return [(c, "%s.%s.1.%s" % (prefix, lab, ext), "%s.%s.2.%s" % (prefix, lab, ext)) for c, lab in names]


RESERVED_LABELS = ("-", "?", "ambiguous", "unassigned")


def ref_label(path: str) -> str:
    """A reference's label: the file's basename minus a trailing .gz and then
    one extension (a.fa, a.fa.gz -> a; b.fastq.gz -> b; noext -> noext)."""
    name = os.path.basename(path)
    if name.endswith(".gz"):
        name = name[:-3]
    stem, dot, _ = name.rpartition(".")
    return stem if dot and stem else name


def classify_summary(labels, table_kmers, assign) -> bytes:
    """`kmer classify --summary`: LABEL<TAB>TABLE_KMERS<TAB>READS per
    reference, then the ambiguous and the unassigned records."""
    assign = [int(a) for a in assign]
    out = ["%s\t%d\t%d\n" % (lab, n, sum(1 for a in assign if a == c))
           for c, (lab, n) in enumerate(zip(labels, table_kmers))]
    out.append("?\t0\t%d\n" % sum(1 for a in assign if a == engine.AMBIGUOUS))
    out.append("-\t0\t%d\n" % sum(1 for a in assign if a == engine.UNASSIGNED))
    return "".join(out).encode("utf-8", errors="surrogateescape")


def _classify_outputs(prefix: Optional[str], labels, ext: str):
    """(assignment value, path) of every --reads-out-prefix file."""
    if prefix is None:
        return []
    outs = [(c, "%s.%s.%s" % (prefix, lab, ext)) for c, lab in enumerate(labels)]
    return outs + [(engine.AMBIGUOUS, "%s.ambiguous.%s" % (prefix, ext)),
                   (engine.UNASSIGNED, "%s.unassigned.%s" % (prefix, ext))]


def _check_classify_options(k: int, labels, min_qual: int, fastq, min_count: int, max_count: Optional[int],
                            min_hits: int, min_frac: float, min_margin: int, index_bits: Optional[int],
                            output_path: str, summary_path: Optional[str], outs) -> None:
    """What `kmer classify` refuses, before any device work or output."""
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    if k > engine.MAX_K:
        raise AssertionError("kmer classify takes K <= %d (one 64-bit key per k-mer), got %d: word keys are a stated "
                             "limit of this command" % (engine.MAX_K, k))
    if not 1 <= len(labels) <= engine.MAX_COLORS:
        raise AssertionError("kmer classify takes 1 to %d --ref, got %d" % (engine.MAX_COLORS, len(labels)))
    seen = set()
    for lab in labels:
        if lab in RESERVED_LABELS:
            raise AssertionError("--ref label %r is reserved (%s): rename the file" % (lab, ", ".join(RESERVED_LABELS)))
        if "\t" in lab:
            raise AssertionError("--ref label %r holds a tab" % lab)
        if lab in seen:
            raise AssertionError("two --ref have the label %r: labels must differ" % lab)
        seen.add(lab)
    if min_qual > 0 and not any(fastq):
        raise AssertionError("--min-qual needs fastq input: neither READS nor any --ref is fastq")
    if max_count is not None and min_count > max_count:
        raise AssertionError("--min-count %d is greater than --max-count %d" % (min_count, max_count))
    if not 0.0 <= min_frac <= 1.0:  # (a NaN is refused too)
        raise AssertionError("--min-frac must be in [0, 1], got %r" % min_frac)
    if min_hits < 0:
        raise AssertionError("--min-hits must be >= 0, got %d" % min_hits)
    if min_margin < 1:
        raise AssertionError("--min-margin must be >= 1, got %d" % min_margin)
    if index_bits is not None and index_bits > 2 * k:
        raise AssertionError("--index-bits %d is more than the 2 K = %d bits of a k-mer" % (index_bits, 2 * k))
    named = [("OUTPUT", output_path)] + ([("--summary", summary_path)] if summary_path is not None else []) + \
        [("--reads-out-prefix", path) for _, path in outs]
    for i, (na, pa) in enumerate(named):
        for nb, pb in named[:i]:
            if _same_path(pa, pb):
                raise AssertionError("%s and %s name the same file, %r" % (nb, na, pa))


@main.command(name="compare", context_settings=CONTEXT_SETTINGS, help="""
All against all: how many k-mers every two of the INPUT files share, written
to OUTPUT as one "LABEL_I<TAB>LABEL_J<TAB>KMERS_I<TAB>KMERS_J<TAB>SHARED<TAB>
JACCARD<TAB>CONT_I<TAB>CONT_J<TAB>DIST" line per pair in input order (JACCARD:
shared / union; CONT_I: shared / KMERS_I; DIST: the Mash distance
-ln(2 J / (1 + J)) / K, 1 for disjoint inputs), exact, not sketched.

Not part of the reference kman CLI.  Every INPUT is counted on the GPU and the
tables are united into one coloured table there, as `kmer classify` builds it
from its --ref files: each k-mer of any input with the set of inputs that hold
it.  One pass over that table (kman_mask_gram) gives every pair's shared
k-mers at once; nothing goes through a text file.  INPUT: fasta or fastq
files, plain or gzipped, each detected on its own; 2 to 64 of them, K <= 32.
LABEL is the input's label (its file name without a trailing .gz and then one
extension); labels must differ.  -L / -U select the k-mers of each input, by
their count in that input (-L 2 drops the k-mers a read set holds once).
--matrix FILE writes the square matrix of --metric (dist by default) for
clustering and tree building, --occupancy FILE the pan-genome spectrum (how
many k-mers exactly P inputs hold; P = n is the core), --summary FILE
"LABEL<TAB>KMERS<TAB>PRIVATE" per input.
Out of scope: abundance-weighted measures such as Bray-Curtis (the coloured
table keeps no counts), K > 32, more than 64 inputs, sketching, and inputs
whose union of k-mers does not fit one GPU.
Launched one process per GPU, the command runs on rank 0 alone.
""")
@args.output_path(file_okay=True)
@args.k()
@args.compare_inputs()
@args.compare_canonical()
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.compare_min_count()
@args.compare_max_count()
@args.matrix()
@args.metric()
@args.occupancy()
@args.compare_summary()
@args.hpc()
def compare(output_path: str, k: int, inputs=(), canonical: bool = False, input_format: str = "auto",
            min_qual: int = 0, phred_offset: str = "33", min_count: int = 1, max_count: Optional[int] = None,
            matrix_path: Optional[str] = None, metric: Optional[str] = None, occupancy_path: Optional[str] = None,
            summary_path: Optional[str] = None, hpc: bool = False) -> None:
    inputs = list(inputs)
    for path in inputs:
        input_file_exists(path)
    fastq = [_is_fastq(p, input_format) for p in inputs]
    labels = [ref_label(path) for path in inputs]
    _check_compare_options(k, inputs, labels, min_qual, fastq, min_count, max_count, output_path, matrix_path, metric,
                           occupancy_path, summary_path)
    if launch.distributed() and not launch.solo_rank():
        launch.log_solo("kmer compare")  # (the coloured table on one GPU, as kmer classify)
        return
    dev = engine.default_device()
    nc = len(inputs)
    tables, ctable = [], None
    try:
        for path, fq in zip(inputs, fastq):
            # (an input's parse buffers are freed before the next one is read)
            p = _parse_input(dev, path, input_format, min_qual if fq else 0, int(phred_offset), hpc)
            try:
                engine.check_empty_names(p, k)
                t = engine.join_groups(p, k, False, "count", canonical=canonical)
            finally:
                p.free()
            if t is None:
                t = engine.empty_count(dev, k)  # (no k-mers: an input that shares nothing)
            elif min_count > 1 or max_count is not None:
                ranged = engine.filtered_copy(dev, t, min_count, max_count)
                engine.free_result(t)
                t = ranged
            tables.append(t)
        ctable = engine.color_table(dev, tables)  # (frees each table as it is folded in)
        gram, occ, private = engine.mask_gram(dev, ctable, nc)
    finally:
        for t in tables:
            engine.free_result(t)
        engine.free_result(ctable)
    with open(output_path, "wb") as fh:
        engine.emit_compare(labels, gram, k, fh)
    if matrix_path is not None:
        with open(matrix_path, "wb") as fh:
            engine.emit_compare_matrix(labels, gram, k, metric or "dist", fh)
    if occupancy_path is not None:
        with open(occupancy_path, "wb") as fh:
            engine.emit_occupancy(occ, fh)
    if summary_path is not None:
        with open(summary_path, "wb") as fh:
            engine.emit_compare_summary(labels, gram, private, fh)
    logging.info("That's all!")


def _check_compare_options(k: int, inputs, labels, min_qual: int, fastq, min_count: int, max_count: Optional[int],
                           output_path: str, matrix_path: Optional[str], metric: Optional[str],
                           occupancy_path: Optional[str], summary_path: Optional[str]) -> None:
    """What `kmer compare` refuses, before any device work or output."""
    if k <= 1:
        raise AssertionError("k must be >= 1, got %d instead." % k)
    if k > engine.MAX_K:
        raise AssertionError("kmer compare takes K <= %d (one 64-bit key per k-mer), got %d: word keys are a stated "
                             "limit of this command" % (engine.MAX_K, k))
    if not 2 <= len(inputs) <= engine.MAX_COLORS:
        raise AssertionError("kmer compare takes 2 to %d INPUT, got %d" % (engine.MAX_COLORS, len(inputs)))
    seen = set()
    for lab in labels:
        if "\t" in lab:
            raise AssertionError("INPUT label %r holds a tab" % lab)
        if lab in seen:
            raise AssertionError("two INPUT have the label %r: labels must differ" % lab)
        seen.add(lab)
    if min_qual > 0 and not any(fastq):
        raise AssertionError("--min-qual needs fastq input: no INPUT is fastq")
    if max_count is not None and min_count > max_count:
        raise AssertionError("--min-count %d is greater than --max-count %d" % (min_count, max_count))
    if metric is not None and matrix_path is None:
        raise AssertionError("--metric needs --matrix: it chooses the matrix's values")
    named = [("OUTPUT", output_path)] + [(name, path) for name, path in (
        ("--matrix", matrix_path), ("--occupancy", occupancy_path), ("--summary", summary_path)) if path is not None]
    for i, (na, pa) in enumerate(named):
        for path in inputs:
            if _same_path(pa, path):
                raise AssertionError("%s and an INPUT name the same file, %r" % (na, pa))
        for nb, pb in named[:i]:
            if _same_path(pa, pb):
                raise AssertionError("%s and %s name the same file, %r" % (nb, na, pa))


@main.command(name="unitigs", context_settings=CONTEXT_SETTINGS, help="""
Compact the k-mers of INPUT into maximal unitigs: the compacted de Bruijn
graph's nodes, written to OUTPUT as FASTA, one
">ID LN:i:BASES KC:i:SUM" line and one unwrapped sequence line per unitig
(ID: the unitig's number from 0; SUM: the sum of its k-mers' counts).

Not part of the reference kman CLI.  INPUT is counted on the GPU into a table
of canonical k-mers, min(k-mer, reverse complement), always; each k-mer's
eight possible neighbours are looked up in that table, paths without a branch
are ranked by pointer doubling and spelled there (kman_graph_links,
kman_graph_rank, kman_unitig_spell); the table never goes through a text file.
Every k-mer of the table lies in exactly one unitig; a cycle is opened at its
smallest k-mer; unitigs are ordered by their smallest end k-mer, so the same
table gives the same bytes.  INPUT: a fasta or fastq file, plain or gzipped.
K is odd and in 3..31.  -L / -U select the k-mers that become nodes (-L 2
drops the k-mers a read set holds once, and with them the tips and bubbles of
sequencing errors).  An INPUT without k-mers writes an empty OUTPUT; OUTPUT is
never compressed.

--gfa writes GFA 1.0 instead: the unitigs as S lines and, as L lines with a
K-1 base overlap, every edge between two unitig ends: U + or - (the unitig's
text or its reverse complement) is followed by V + or - when its last K-1
bases and one more base give V's first k-mer.  The ends' extensions are looked
up in the table on the GPU (kman_unitig_edges); every edge is written from
both sides, an edge that is its own mirror once.  An INPUT without k-mers
then writes the header line alone.

Out of scope: colours, K > 31, and tables larger than one GPU.

Launched one process per GPU, the command runs on rank 0 alone.
""")
@args.input_path()
@args.output_path(file_okay=True)
@args.k()
@args.input_format()
@args.min_qual()
@args.phred_offset()
@args.unitig_min_count()
@args.unitig_max_count()
@args.index_bits()
@args.hpc()
@args.gfa()
def unitigs(input_path: str, output_path: str, k: int, input_format: str = "auto", min_qual: int = 0,
            phred_offset: str = "33", min_count: int = 1, max_count: Optional[int] = None,
            index_bits: Optional[int] = None, hpc: bool = False, gfa: bool = False) -> None:
    input_file_exists(input_path)
    fastq = _is_fastq(input_path, input_format)
    _check_unitig_options(k, output_path, input_path, min_qual, fastq, min_count, max_count, index_bits)
    if launch.distributed() and not launch.solo_rank():
        launch.log_solo("kmer unitigs")  # (the table and its graph on one GPU, as kmer screen)
        return
    dev = engine.default_device()
    table = None
    try:
        p = _parse_input(dev, input_path, input_format, min_qual if fastq else 0, int(phred_offset), hpc)
        try:
            engine.check_empty_names(p, k)
            table = engine.join_groups(p, k, False, "count", canonical=True)
        finally:
            p.free()
        if table is None:
            table = engine.empty_count(dev, k)  # (no k-mers: no unitigs, an empty file)
        elif min_count > 1 or max_count is not None:
            ranged = engine.filtered_copy(dev, table, min_count, max_count)
            engine.free_result(table)
            table = ranged
        res = engine.unitigs(dev, table, index_bits=index_bits, links=True) if gfa else \
            engine.unitigs(dev, table, index_bits=index_bits)
    finally:
        engine.free_result(table)
    with open(output_path, "wb") as fh:
        if gfa:
            engine.emit_gfa(res, fh)
        else:
            engine.emit_unitigs(res, fh)
    logging.info("That's all!")


def _check_unitig_options(k: int, output_path: str, input_path: str, min_qual: int, fastq: bool, min_count: int,
                          max_count: Optional[int], index_bits: Optional[int]) -> None:
    """What `kmer unitigs` refuses, before any device work or output."""
    engine.check_unitig_k(k)
    if output_path.endswith(".gz"):
        raise AssertionError("kmer unitigs writes plain text: OUTPUT %r ends in .gz" % output_path)
    if _same_path(output_path, input_path):
        raise AssertionError("OUTPUT and INPUT name the same file, %r" % output_path)
    if min_qual > 0 and not fastq:
        raise AssertionError("--min-qual needs fastq input")
    if max_count is not None and min_count > max_count:
        raise AssertionError("--min-count %d is greater than --max-count %d" % (min_count, max_count))
    if index_bits is not None and index_bits > 2 * k:
        raise AssertionError("--index-bits %d is more than the 2 K = %d bits of a k-mer" % (index_bits, 2 * k))


if __name__ == "__main__":
    main()

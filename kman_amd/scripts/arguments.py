"""Click arguments/options of the ``kmer`` CLI — same names, short flags and
defaults as the reference (kmermaid/scripts/arguments.py:14-221)."""

from __future__ import annotations

import tempfile

import click

from ..batcher import BatcherThreading, FastaBatcher
from ..join import KJoiner


def input_path():
    return click.argument("input_path", metavar="INPUT",
                          type=click.Path(exists=True, file_okay=True, readable=True))


def output_path(file_okay=False, dir_okay=False):
    return click.argument("output_path", metavar="OUTPUT",
                          type=click.Path(exists=False, file_okay=file_okay, dir_okay=dir_okay, writable=True))


def k():
    return click.argument("k", type=click.INT)


def reverse():
    return click.option("--reverse", "-r", is_flag=True, help="Include also reverse-complemented sequences")


def scan_mode():
    return click.option("--scan-mode", "-s", type=click.Choice([m.name for m in FastaBatcher.MODE],
                                                                case_sensitive=True),
                        default=FastaBatcher.MODE.KMERS.name,
                        help="KMERS: batch the k-mer stream; RECORDS: batch each record. Default: KMERS")


def batch_size():
    return click.option("--batch-size", "-b", type=click.INT, default=1000000,
                        help="Number of k-mers per batch. Default: 1000000")


def batch_mode():
    return click.option("--batch-mode", "-m", type=click.Choice([m.name for m in BatcherThreading.FEED_MODE],
                                                                 case_sensitive=True),
                        default=BatcherThreading.FEED_MODE.APPEND.name,
                        help="How batches are fed to the collection. Default: APPEND")


def previous_batches():
    return click.option("--previous-batches", "-B", type=click.Path(exists=True, dir_okay=True, readable=True),
                        help="Path to folder with previously generated batches.")


def count_mode():
    return click.option("--count-mode", "-m",
                        type=click.Choice([m.name for m in KJoiner.MODE if "COUNT" in m.name], case_sensitive=True),
                        default=KJoiner.MODE.SEQ_COUNT.name, help='Default: "%s"' % KJoiner.MODE.SEQ_COUNT.name)


def memory_mode():
    return click.option("--memory-mode", "-M", type=click.Choice([m.name for m in KJoiner.MEMORY],
                                                                  case_sensitive=True),
                        default=KJoiner.MEMORY.NORMAL.name, help='Default: "%s"' % KJoiner.MEMORY.NORMAL.name)


def threads():
    return click.option("--threads", "-t", type=click.INT, default=1,
                        help="Accepted for compatibility; the GPU path ignores it.")


def tmp():
    return click.option("--tmp", "-T", type=click.Path(exists=True), default=tempfile.gettempdir(),
                        help='Temporary folder path. Default: "%s"' % tempfile.gettempdir())


def compress():
    return click.option("--compress", "-C", is_flag=True, help="Compress output files.")


def input_format():
    return click.option("--format", "-f", "input_format", type=click.Choice(["auto", "fasta", "fastq"],
                                                                          case_sensitive=True),
                        default="auto", help="INPUT format; auto: fastq if the first non-empty line starts "
                                             "with '@', else fasta. Default: auto")


def min_qual():
    return click.option("--min-qual", "-q", "min_qual", type=click.IntRange(0, 93), default=0,
                        help="fastq INPUT only: bases whose quality is below this Phred score are read as N, "
                             "so no k-mer spans them. Default: 0 (off)")


def phred_offset():
    return click.option("--phred-offset", "phred_offset", type=click.Choice(["33", "64"]), default="33",
                        help="ASCII offset of the fastq quality bytes, for --min-qual. Default: 33")


def min_count():
    return click.option("--min-count", "-L", "min_count", type=click.IntRange(min=1), default=1,
                        help="SEQ_COUNT: leave out k-mers seen fewer times than this. Default: 1 (all)")


def max_count():
    return click.option("--max-count", "-U", "max_count", type=click.IntRange(min=1), default=None,
                        help="SEQ_COUNT: leave out k-mers seen more times than this. Default: no limit")


def canonical():
    return click.option("--canonical", "canonical", is_flag=True,
                        help="SEQ_COUNT: count canonical k-mers, min(k-mer, reverse complement); not with -r or -B")


def input_a():
    return click.argument("input_a", metavar="INPUT_A", type=click.Path(exists=True, file_okay=True, readable=True))


def input_b():
    return click.argument("input_b", metavar="INPUT_B", type=click.Path(exists=True, file_okay=True, readable=True))


def set_op():
    return click.option("--op", "op", type=click.Choice(["intersect", "subtract", "union"], case_sensitive=True),
                        required=True, help="intersect: k-mers of INPUT_A that occur in INPUT_B; subtract: those "
                                            "that do not; union: the k-mers of either")


def set_counts():
    return click.option("--counts", "counts", type=click.Choice(["left", "right", "min", "max", "sum"],
                                                                 case_sensitive=True),
                        default=None, help="The count written for a k-mer.  intersect: left (INPUT_A's, default) | "
                                           "right | min | max | sum; subtract: left; union: sum (default) | max")


def reads_path():
    return click.argument("reads_path", metavar="READS", type=click.Path(exists=True, file_okay=True, readable=True))


def table_input():
    return click.argument("table_input", metavar="TABLE_INPUT",
                          type=click.Path(exists=True, file_okay=True, readable=True))


def table_min_count():
    return click.option("--min-count", "-L", "min_count", type=click.IntRange(min=1), default=1,
                        help="Look up only k-mers seen at least this often in TABLE_INPUT. Default: 1 (all)")


def table_max_count():
    return click.option("--max-count", "-U", "max_count", type=click.IntRange(min=1), default=None,
                        help="Look up only k-mers seen at most this often in TABLE_INPUT. Default: no limit")


def screen_canonical():
    return click.option("--canonical", "canonical", is_flag=True,
                        help="Canonical k-mers, min(k-mer, reverse complement), in TABLE_INPUT and in the reads")


def min_hits():
    return click.option("--min-hits", "min_hits", type=click.INT, default=0,
                        help="Write only records with at least this many k-mers found. Default: 0 (all)")


def min_frac():
    return click.option("--min-frac", "min_frac", type=click.FLOAT, default=0.0,
                        help="Write only records with at least this fraction (0..1) of their k-mers found. "
                             "Default: 0.0 (all)")


def invert():
    return click.option("--invert", "-v", "invert", is_flag=True,
                        help="Write the records that --min-hits / --min-frac leave out instead")


def median():
    return click.option("--median", "median", is_flag=True,
                        help="Write a fifth column: the median count in TABLE_INPUT over the record's k-mers "
                             "(absent k-mers count 0; the lower median; 0 for a record without k-mers)")


def min_median():
    return click.option("--min-median", "min_median", type=click.INT, default=None,
                        help="Write only records whose median is at least this (>= 0). Implies --median")


def max_median():
    return click.option("--max-median", "max_median", type=click.INT, default=None,
                        help="Write only records whose median is at most this (>= 0). Implies --median")


def solid():
    return click.option("--solid", "solid", type=click.INT, default=None, metavar="C",
                        help="Write two last columns START and END: the longest stretch of the record whose k-mers "
                             "all have a count of at least C (1..4294967294) in TABLE_INPUT, the leftmost of equal "
                             "ones, in bases within the record (0-based, END exclusive; N counts, line breaks do "
                             "not); 0 and 0 for a record without such a k-mer")


def min_solid_len():
    return click.option("--min-solid-len", "min_solid_len", type=click.INT, default=None, metavar="N",
                        help="Write only records whose solid stretch has at least N bases (END - START >= N, N >= 0). "
                             "Needs --solid")


def bed():
    return click.option("--bed", "bed_path", type=click.Path(dir_okay=False, writable=True), default=None,
                        metavar="FILE",
                        help="Also write NAME<TAB>START<TAB>END for the written records that have a solid stretch, "
                             "in input order, to FILE. Needs --solid")


def reads_out():
    return click.option("--reads-out", "reads_out", type=click.Path(dir_okay=False, writable=True), default=None,
                        metavar="FILE",
                        help="Also write the written records themselves, byte for byte as READS has them (fasta or "
                             "fastq), in input order, to FILE, cut out on the GPU. Always uncompressed: a FILE "
                             "that ends in .gz is refused")


def mate():
    return click.option("--mate", "-2", "mate_path", metavar="READS2", default=None,
                        type=click.Path(exists=True, file_okay=True, readable=True),
                        help="The second ends of the reads: record i of READS2 is the mate of record i of READS "
                             "(same format, same number of records, same names but for a trailing /1 or /2). "
                             "Every line, every selection and every label is then one per pair, joint over "
                             "both mates' k-mers")


def interleaved():
    return click.option("--interleaved", "interleaved", is_flag=True, default=False,
                        help="READS holds read pairs interleaved: records 2i and 2i+1 are the two mates of pair i. "
                             "As --mate, with one input and one --reads-out file. Not with --mate")


def reads_out2():
    return click.option("--reads-out2", "reads_out2", type=click.Path(dir_okay=False, writable=True), default=None,
                        metavar="FILE",
                        help="With --mate: the written pairs' second mates, from READS2, as --reads-out writes the "
                             "first mates from READS; record i of the two files are always mates. Needs --mate "
                             "and --reads-out")


def trim():
    return click.option("--trim", "trim", is_flag=True, default=False,
                        help="Cut every read of --reads-out to its solid stretch: sequence and quality columns "
                             "[START, END), line ends written as \"\\n\"; reads without a stretch are left out. "
                             "Needs --solid, --reads-out and fastq READS")


def correct():
    return click.option("--correct", "correct", is_flag=True, default=False,
                        help="Repair isolated substitution errors on the GPU before anything else is computed: a base "
                             "covered by at most K k-mers in a row whose counts are below C, next to a k-mer with a "
                             "count of at least C, is replaced when exactly one other base lifts all of them to C. "
                             "Adds a last column FIXES; --reads-out then writes the corrected reads (fastq READS "
                             "only). Needs --solid")


def index_bits():
    return click.option("--index-bits", "index_bits", type=click.IntRange(1, 24), default=None,
                        help="Key bits of the table's prefix index (at most 2 K). Default: about 8 rows per bucket")


def refs():
    return click.option("--ref", "refs", type=click.Path(exists=True, file_okay=True, dir_okay=False, readable=True),
                        multiple=True, metavar="FILE",
                        help="A reference, fasta or fastq, plain or gzipped; 1 to 64 of them. Its label is the "
                             "file's name without a trailing .gz and then one extension")


def classify_canonical():
    return click.option("--canonical", "canonical", is_flag=True,
                        help="Canonical k-mers, min(k-mer, reverse complement), in every reference and in the reads")


def ref_min_count():
    return click.option("--min-count", "-L", "min_count", type=click.IntRange(min=1), default=1,
                        help="Look up only k-mers seen at least this often in their own reference. Default: 1 (all)")


def ref_max_count():
    return click.option("--max-count", "-U", "max_count", type=click.IntRange(min=1), default=None,
                        help="Look up only k-mers seen at most this often in their own reference. Default: no limit")


def specific():
    return click.option("--specific", "specific", is_flag=True,
                        help="Count a k-mer only for the one reference that holds it: k-mers shared by two or more "
                             "references vote for none")


def classify_min_hits():
    return click.option("--min-hits", "min_hits", type=click.INT, default=1,
                        help="Assign a record only when its best reference has at least this many k-mers found "
                             "(never with 0). Default: 1")


def classify_min_frac():
    return click.option("--min-frac", "min_frac", type=click.FLOAT, default=0.0,
                        help="Assign a record only when its best reference has at least this fraction (0..1) of the "
                             "record's k-mers. Default: 0.0")


def min_margin():
    return click.option("--min-margin", "min_margin", type=click.INT, default=1,
                        help="A record whose best reference leads the runner-up by fewer k-mers than this is "
                             "ambiguous ('?'); at least 1, so a tie is always ambiguous. Default: 1")


def hits():
    return click.option("--hits", "hits", is_flag=True,
                        help="Append one column per reference, in --ref order: the record's k-mers found there")


def summary():
    return click.option("--summary", "summary_path", type=click.Path(dir_okay=False, writable=True), default=None,
                        metavar="FILE",
                        help="Also write LABEL<TAB>TABLE_KMERS<TAB>READS per reference, then the '?' and '-' lines, "
                             "to FILE")


def reads_out_prefix():
    return click.option("--reads-out-prefix", "reads_out_prefix", type=click.Path(dir_okay=False), default=None,
                        metavar="PREFIX",
                        help="Also write the records themselves, byte for byte as READS has them, to PREFIX.LABEL.fq "
                             "(.fa for fasta READS) per reference, PREFIX.ambiguous.* and PREFIX.unassigned.*, cut "
                             "out on the GPU. Always uncompressed; empty files are still created")


def re_sort():
    return click.option("--re-sort", "-R", is_flag=True, help="Force batch re-sorting, when loaded with -B.")


def hpc():
    return click.option("--hpc", "hpc", is_flag=True,
                        help="Homopolymer-compressed k-mers: every run of one base in every input collapses to one "
                             "base on the GPU before k-mers are taken (minimap2 -H, meryl compress), so a wrong "
                             "homopolymer length in a long read costs no k-mer; N and other letters are kept, and "
                             "no run crosses a record")


def gfa():
    return click.option("--gfa", "gfa", is_flag=True,
                        help="Write the graph, not the nodes alone: GFA 1.0, a header line, one "
                             "\"S ID SEQ LN:i:BASES KC:i:SUM\" line per unitig and one \"L U +|- V +|- (K-1)M\" line per "
                             "edge between two unitig ends (tab-separated), the edges found on the GPU")


def compare_inputs():
    return click.argument("inputs", metavar="INPUT INPUT [INPUT ...]", nargs=-1,
                          type=click.Path(exists=True, file_okay=True, dir_okay=False, readable=True))


def compare_canonical():
    return click.option("--canonical", "canonical", is_flag=True,
                        help="Canonical k-mers, min(k-mer, reverse complement), in every input")


def compare_min_count():
    return click.option("--min-count", "-L", "min_count", type=click.IntRange(min=1), default=1,
                        help="Compare only k-mers seen at least this often in their own input. Default: 1 (all)")


def compare_max_count():
    return click.option("--max-count", "-U", "max_count", type=click.IntRange(min=1), default=None,
                        help="Compare only k-mers seen at most this often in their own input. Default: no limit")


def unitig_min_count():
    return click.option("--min-count", "-L", "min_count", type=click.IntRange(min=1), default=1,
                        help="Build the graph only of k-mers seen at least this often in INPUT. Default: 1 (all)")


def unitig_max_count():
    return click.option("--max-count", "-U", "max_count", type=click.IntRange(min=1), default=None,
                        help="Build the graph only of k-mers seen at most this often in INPUT. Default: no limit")


def matrix():
    return click.option("--matrix", "matrix_path", type=click.Path(dir_okay=False, writable=True), default=None,
                        metavar="FILE",
                        help="Also write a square matrix to FILE: a first line with the number of inputs, then "
                             "LABEL<TAB>v_0<TAB>...<TAB>v_{n-1} per input, the values chosen by --metric")


def metric():
    return click.option("--metric", "metric", type=click.Choice(["jaccard", "dist", "shared", "containment"],
                                                                case_sensitive=True),
                        default=None,
                        help="The values of --matrix: dist (Mash distance, the default), jaccard, shared (integers) "
                             "or containment (the row's k-mers found in the column, not symmetric). Needs --matrix")


def occupancy():
    return click.option("--occupancy", "occupancy_path", type=click.Path(dir_okay=False, writable=True),
                        default=None, metavar="FILE",
                        help="Also write P<TAB>KMERS for P = 1..n to FILE: the k-mers held by exactly P inputs "
                             "(P = n: the core; P = 1: k-mers of one input only)")


def compare_summary():
    return click.option("--summary", "summary_path", type=click.Path(dir_okay=False, writable=True), default=None,
                        metavar="FILE",
                        help="Also write LABEL<TAB>KMERS<TAB>PRIVATE per input to FILE (its k-mers, and those no "
                             "other input holds)")

"""Device-side engine: thin Python orchestration over the C ABI (``_native``).

All per-base and per-k-mer arithmetic runs in the gfx950 kernels of
libkman.so; Python only moves handles, sizes and the (small) record-name
table.  This package is a facade: every name of its modules, private ones
included, is an attribute of ``kman_amd.engine``.  A tunable constant
(``_FMT_SLICE``, ``_NAME_ROWS``, ..) is read through its home module at call
time, so that is where a test patches it.

=============  =========================================================  ==============================
module         holds (reference: kmermaid 1.0.0)                          kernel(s)
=============  =========================================================  ==============================
``device``     Device, DeviceBuffer, the scratch scope, ``_FMT_SLICE``    (runtime)
``parsed``     ``parse`` SmartFastaParser.parse, parsers.py:86-128        parse_reduce/scan/emit
               ``parse_fastq`` (four-line FASTQ; not in the reference)    fq_reduce/scan/emit/validate
               ``min_qual > 0`` (low bases read as N)                     + fq_qmask
               record names: record[0].split(" ")[0], batcher.py:551      host (names only)
``kmers``      ``extract`` Sequence.yield_kmers, seq.py:285-328           extract_kernel
               ``sort`` Batch.sorted, batch.py:156-168                    onesweep_pass x P
               ``rle_count`` Crawler.do_batch + join_sequence_count       rle_count_kernel
               ``rle_uniq`` Crawler.do_batch + join_unique                rle_uniq_kernel
               ``groups`` the region path, straight from the codes        rg_* (region_*.hip)
``words``      the same for k > 32, keys as word planes                   words.hip
``join``       RangedJoin, ``join_groups`` / ``count_groups``: the path   (the above)
               that takes an input (join.py:63-130)
``output``     ``format_*`` join.py:262,284 / seq.py:489-495              host threads (C++), devformat
``tables``     filter_counts, set operations, table_index                 filter, match, ops
``lookup``     screen, window_counts, quantile, runs, correct             screen, quantile, runs, correct
``reads``      cut_records, hpc, read pairs (``zip_pairs``)               cut, hpc, zip_offsets/zip_copy
``colors``     color_table, classify, compare                             classify, gram
``unitig``     unitigs of a canonical count table                         unitig.hip
``pipelines``  count_text, uniq_text, abundance_hist: text in, text out   (the above)
``resident``   ResidentPipeline: preallocated, what bench.py times        (the above)
=============  =========================================================  ==============================

Imports go one way, in the order of the table: no module imports one below it.
"""

from . import device, parsed, kmers, words, join, output, tables, lookup, reads, colors, unitig, pipelines, resident

for _m in (device, parsed, kmers, words, join, output, tables, lookup, reads, colors, unitig, pipelines, resident):
    globals().update((_k, _v) for _k, _v in vars(_m).items() if not _k.startswith("__"))
del _m

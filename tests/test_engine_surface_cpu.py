"""kman_amd.engine is a package behind a facade: every top-level name the
single-file engine.py defined (functions, classes and assignments, private
ones included) is still an attribute of ``kman_amd.engine``, and every module
of the package imports on its own (no import cycle)."""

from __future__ import annotations

import os
import pkgutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the top-level names of engine.py before the split, in file order
NAMES = [
    "MAX_K", "MAX_K_WIDE", "host_threads", "DeviceBuffer", "Device", "_DEFAULT", "default_device", "_title_name",
    "Parsed", "FORMATS", "MAX_MIN_QUAL", "PHRED_OFFSETS", "_qual_byte", "_check_qual_format", "sniff_format",
    "_resolve_format", "sniff_file", "BlobNames", "_NAME_ROWS", "fastq_names", "_parsed_fastq", "_call_parse_fastq",
    "parse_fastq", "parse", "parse_file", "check_empty_names", "first_window", "Kmers", "flags_for", "count_kmers",
    "_check_k", "extract", "extract_sorted", "split_bits", "_sort_prefix", "_finish", "sort", "CountResult",
    "rle_count", "UniqResult", "rle_uniq", "groups", "mem_info", "_prefix_hist_into", "prefix_hist", "key_ranges",
    "_At", "RangedJoin", "ranged_groups", "_format", "format_fasta_words", "format_count", "format_fasta",
    "_FMT_CHUNK", "_FMT_SLICE", "_FMT_THREADS", "_FMT_ZC", "_pwrite_target", "_format_dev", "format_count_dev",
    "DeviceNames", "format_uniq_dev", "host_format", "_to", "emit_count", "emit_uniq", "download_count",
    "download_uniq", "_CODE_TABLE", "decode_key", "kmers_of_sequence", "read_input", "count_groups",
    "abundance_hist", "format_hist", "_fits", "nwords", "Words", "WordsResult", "extract_words", "sort_words",
    "rle_words", "words_groups", "wide_groups", "download_words", "decode_words", "check_count_range",
    "_count_rows", "_filter_call", "_U64_MAX", "filter_counts", "filtered_copy", "MATCH_OPS", "SET_OPS",
    "check_set_op", "empty_count", "_match_bytes", "match_counts", "_matched_rows", "set_op", "default_index_bits",
    "_check_index_bits", "table_index", "screen", "window_counts", "quantile_plan", "record_quantile",
    "screen_median", "_check_min_count", "record_runs", "solid_spans", "screen_solid", "correct", "_span_arrays",
    "screen_keep", "emit_screen", "emit_bed", "_CUT_MAX_RECORDS", "_keep_array", "_cut_slices", "cut_records",
    "_cut_host", "emit_reads", "hpc", "_hpc_parsed", "hpc_spans", "BorrowedBuffer", "_pair_keys",
    "_first_name_mismatch", "check_pair_names", "_even_names", "zip_pairs", "pair_view", "pairs_of", "screen_pairs",
    "pair_min_span", "emit_screen_pairs", "emit_pair_reads", "MAX_COLORS", "UNASSIGNED", "AMBIGUOUS", "color_table",
    "classify", "classify_assign", "_label_blob", "emit_classify", "COMPARE_METRICS", "mask_gram", "compare_rows",
    "compare_metrics", "_compare_labels", "emit_compare", "emit_compare_matrix", "emit_occupancy",
    "emit_compare_summary", "UNITIG_MIN_K", "UNITIG_MAX_K", "check_unitig_k", "UnitigResult", "graph_links",
    "unitigs", "_UNITIG_SLICE", "emit_unitigs", "join_groups", "free_result", "_emit_words", "_emit_wide",
    "count_text", "uniq_text", "ResidentPipeline",
]


def test_every_former_name_is_an_attribute_of_the_facade():
    from kman_amd import engine

    assert len(NAMES) == len(set(NAMES)) == 170
    assert [n for n in NAMES if not hasattr(engine, n)] == []


def test_functions_win_over_modules_of_the_same_name():
    """``engine.parse`` and its like are the functions they always were."""
    from kman_amd import engine

    for name in ("parse", "screen", "classify", "groups", "hpc", "sort", "unitigs", "correct"):
        assert callable(getattr(engine, name)), name


def _modules():
    from kman_amd import engine

    return sorted(m.name for m in pkgutil.iter_modules(engine.__path__))


def test_the_package_has_its_modules():
    assert {"device", "parsed", "kmers", "output", "tables", "resident"} <= set(_modules())


@pytest.mark.parametrize("module", ["device", "parsed", "kmers", "words", "join", "output", "tables", "lookup",
                                    "reads", "colors", "unitig", "pipelines", "resident"])
def test_each_module_imports_on_its_own(module):
    assert module in _modules()
    code = ("import importlib, sys; importlib.import_module('kman_amd.engine.%s'); "
            "bad = [m for m in sys.modules if m == 'torch' or m == 'kman_amd.dist']; "
            "assert not bad, bad" % module)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_module_is_left_out_of_the_import_check():
    assert _modules() == sorted(["device", "parsed", "kmers", "words", "join", "output", "tables", "lookup", "reads",
                                 "colors", "unitig", "pipelines", "resident"])

/*
 * kman.h — C ABI of the MI355X (gfx950) k-mer extract / sort / join engine.
 *
 * The reference (ggirelli/kman, package kmermaid 1.0.0) is pure Python and has
 * no FFI of its own; its "operator API" is the class surface
 * FastaBatcher.do / Batch.sorted / Crawler.do_batch / KJoiner.join.  Every
 * entry point below replaces the arithmetic of one of those functions and is
 * what kman_amd/_native.py binds through ctypes:
 *
 *   kman_parse_fasta   SmartFastaParser.parse            kmermaid/parsers.py:86-128
 *                      + record name rule                 kmermaid/batcher.py:551
 *   kman_parse_fastq   the same outputs from four-line FASTQ (not in the reference)
 *   kman_extract       Sequence.yield_kmers / kmerator    kmermaid/seq.py:285-359
 *                      + alphabet check / mkrc            kmermaid/seq.py:279,318,500-509
 *   kman_sort          Batch.sorted (stable, by .seq)     kmermaid/batch.py:156-168
 *                      + BatcherBase.write_all re-sort    kmermaid/batcher.py:133-153,392
 *   kman_sort_range    the same, by a prefix of the key bits
 *   kman_finish        Batch.sorted / Crawler.do_batch + join_* over prefix-sorted keys
 *                                                         batch.py:156-168, join.py:95-130,244-285
 *   kman_groups        the whole count / uniq chain of one stream:
 *                      yield_kmers -> Batch.sorted -> Crawler -> join_*
 *                                                         seq.py:285-328, batch.py:156-168,
 *                                                         join.py:63-130,244-285
 *   kman_rle_count     Crawler.do_batch + join_sequence_count
 *                                                         kmermaid/join.py:95-130,266-285
 *   kman_rle_uniq      Crawler.do_batch + join_unique     kmermaid/join.py:95-130,244-263
 *   kman_merge_runs    Crawler.do_records heapq.merge     kmermaid/join.py:63-93
 *   kman_format_*      the output writers                 kmermaid/join.py:262,284; seq.py:489-495
 *
 * Conventions
 *   - Plain C, no exceptions cross the boundary.  Every call returns 0 on
 *     success or a negative KMAN_E* code; kman_last_error() has the message.
 *   - Device buffers are raw device pointers obtained from kman_malloc and
 *     owned by the caller (freed with kman_free).  Host buffers are borrowed
 *     for the duration of the call.
 *   - One context per GPU and host thread; a context is not re-entrant.  All
 *     device work of a context runs in order on its own HIP stream.
 *   - Keys are k-mers packed 2 bits per base MSB-first (A=0 C=1 G=2 T=3), so
 *     numeric order of keys == the reference's Python str order of the
 *     upper-case sequences (for a fixed k <= 32).
 *   - "pos" payloads are (global base index << 1) | strand, where the global
 *     base index addresses the cleaned, concatenated sequence of all records
 *     (see kman_parse_fasta) and strand 1 means the '-' (reverse-complement)
 *     record of seq.py:274-282.
 */
#ifndef KMAN_H
#define KMAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMAN_ABI_VERSION 1

/* error codes */
#define KMAN_OK 0
#define KMAN_EINVAL (-1)   /* bad argument (maps to AssertionError like the reference) */
#define KMAN_EHIP (-2)     /* HIP runtime error */
#define KMAN_ENOMEM (-3)   /* device or host allocation failed */
#define KMAN_EFORMAT (-4)  /* input is not parsable FASTA (parsers.py:105-107) */
#define KMAN_ETIMEOUT (-5) /* a device-side wait exceeded its bound (engine bug) */
#define KMAN_ECOMM (-6)    /* RCCL error */
#define KMAN_ECAP (-7)     /* output capacity too small; *needed reports the size */
#define KMAN_EFALLBACK (-8) /* kman_groups: input outside the region path; use the general path */
#define KMAN_EPARTIAL (-9)  /* kman_dround_finish: some key ranges left out (kman_dround_failed) */

/* kman_extract flags */
#define KMAN_RC 1u          /* also emit reverse complements (kmer -r, seq.py:274-282) */
#define KMAN_WANT_POS 2u    /* also emit the pos payload (uniq / batch modes) */
#define KMAN_CANONICAL 4u   /* emit min(fwd, rc) instead (not in the reference) */
#define KMAN_MIXED 8u       /* with KMAN_CANONICAL: the canonical key through a fixed bijection of the
                             * 2k-bit keys (odd multiply, xorshift, odd multiply mod 2^2k), so the top
                             * bits are uniform; the multiset of counts is unchanged -- for abundance
                             * spectra (kman_groups, kman_dshard_*, kman_extract_marked / _range) */
#define KMAN_ONCE 16u       /* kman_dshard_hist / _extract: the shard is extracted ONCE for all key rounds
                             * (every window kept; the rounds' items in one buffer, round-major), so
                             * both use the tiles of a shard that one round takes (16 windows per
                             * thread, 8 with KMAN_RC); the same flags on both calls */
#define KMAN_ROOMY 32u      /* kman_dround_plan / _finish: pass-1 sub-regions planned at twice their
                             * expected fill (a genome's repeat families then fit, so regions its
                             * finish leaves out can be redone from pass 1's output, kman_dround_left);
                             * the same flags on both calls */
/* kman_extract: accumulate d_hist for the passes over bits [b, 2k) only
 * (the prefix passes of kman_split_bits); default b = 0, every bit */
#define KMAN_HIST_LO(b) (((uint32_t)(b) & 0x7fu) << 8)
#define KMAN_HIST_LO_OF(flags) (((flags) >> 8) & 0x7fu)

/* kman_finish modes */
#define KMAN_FINISH_SORT 0  /* full stable sort, in place          (batch.py:156-168) */
#define KMAN_FINISH_COUNT 1 /* (key, group size) per distinct key  (join.py:266-285) */
#define KMAN_FINISH_UNIQ 2  /* keys occurring once + payload       (join.py:244-263) */

typedef struct kman_ctx kman_ctx;

/* parse result (host struct) */
typedef struct {
    uint64_t n_bases;   /* cleaned sequence characters over all records */
    uint64_t n_records; /* header lines ('>' at a line start) */
} kman_parse_info;

/* ------------------------------------------------------------------ context */
int kman_abi_version(void);
int kman_device_count(int *n);
int kman_create(int device, kman_ctx **out);
void kman_destroy(kman_ctx *ctx);
const char *kman_last_error(const kman_ctx *ctx);
int kman_sync(kman_ctx *ctx);

/* ------------------------------------------------------------------- memory */
int kman_malloc(kman_ctx *ctx, void **dptr, size_t bytes);
int kman_free(kman_ctx *ctx, void *dptr);
/* free / total HBM of the context's device: the sizing of the key ranges of
 * a multi-batch join (kman_extract_range) */
int kman_mem_info(kman_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
int kman_host_alloc(kman_ctx *ctx, void **hptr, size_t bytes); /* pinned */
int kman_host_free(kman_ctx *ctx, void *hptr);
int kman_memcpy_h2d(kman_ctx *ctx, void *dst, const void *src, size_t bytes);
int kman_memcpy_d2h(kman_ctx *ctx, void *dst, const void *src, size_t bytes);
int kman_memset(kman_ctx *ctx, void *dst, int value, size_t bytes);
/* Chunked uploads that overlap the context's work: kman_copy_h2d_async
 * enqueues a copy (from pinned memory for real overlap) on the context's copy
 * stream and marks event `slot` (0..3); kman_copy_wait makes the work stream
 * wait for that event; kman_copy_sync drains the copy stream.  The copy does
 * not wait for the work stream: a caller reusing a destination that queued
 * work still reads synchronises first (kman_sync). */
int kman_copy_h2d_async(kman_ctx *ctx, void *dst, const void *src, size_t bytes, int slot);
int kman_copy_wait(kman_ctx *ctx, int slot);
int kman_copy_sync(kman_ctx *ctx);
/* Downloads that overlap the context's work (formatted output text):
 * kman_copy_d2h_async queues a device -> host copy on the copy stream after
 * the work already queued (dst: pinned host memory, kman_host_alloc), marked
 * in d2h slot 0..3; kman_copy_d2h_wait blocks the calling host thread until
 * that copy is done. */
int kman_copy_d2h_async(kman_ctx *ctx, void *dst, const void *src, size_t bytes, int slot);
int kman_copy_d2h_wait(kman_ctx *ctx, int slot);

/* ------------------------------------------------------------------- timing
 * Optional per-kernel timing with HIP events recorded on the context's own
 * stream around every launch (bench.py's live roofline).  Tags: "parse",
 * "parse_fastq", "extract", "sort_hist", "sort_pass", "rle_count", "rle_uniq".
 * kman_timing_query synchronises and returns launches and summed ms. */
int kman_timing_enable(kman_ctx *ctx, int enable);
int kman_timing_query(kman_ctx *ctx, const char *tag, uint64_t *launches, double *total_ms);

/* ------------------------------------------------------------------- stages */

/* FASTA text -> cleaned base codes + record table  (parsers.py:86-128)
 *   d_text     n_bytes of FASTA text (uncompressed)
 *   d_codes    out, capacity >= n_bytes + 64: one byte per kept sequence char:
 *              bits 0-1 base (A/a=0 C/c=1 G/g=2 T/t=3), bit 2 set = not ACGT,
 *              bit 3 set = first char of a record.  64 pad bytes (value 4)
 *              follow the last code.
 *   d_rec_hdr  out, byte offset of each record's '>'
 *   d_rec_seq  out, global base index of each record's first char
 *   rec_cap    capacity of the two record arrays; KMAN_ECAP if exceeded
 * Returns KMAN_EFORMAT when no line starts with '>' (empty file included). */
int kman_parse_fasta(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_codes,
                     uint64_t *d_rec_hdr, uint64_t *d_rec_seq, uint64_t rec_cap,
                     kman_parse_info *info);
/* One chunk of a FASTA parsed into d_codes from code_off on (chunked H2D
 * streams and byte-range shards, kman_amd/shard.py).  The chunk starts at a
 * line start; flags KMAN_PARSE_IN_RECORD: the chunk continues a record (its
 * leading lines are sequence lines of the record opened before it; it may
 * hold no header, or nothing at all).  d_rec_seq entries and the 64 pad bytes
 * are at code_off + the chunk's own indices; d_rec_hdr holds byte offsets
 * within the chunk.  d_text and d_codes 16-byte aligned (code_off need not
 * be). */
#define KMAN_PARSE_IN_RECORD 1u
int kman_parse_fasta_at(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint32_t flags, uint8_t *d_codes,
                        uint64_t code_off, uint64_t *d_rec_hdr, uint64_t *d_rec_seq, uint64_t rec_cap,
                        kman_parse_info *info);

/* Strict four-line FASTQ text -> the same outputs, with the argument meanings,
 * capacities, alignment requirements and error conventions of
 * kman_parse_fasta (not in the reference, which reads FASTA only).  Lines are
 * split as for FASTA ("\n", "\r\n", a lone "\r"); trailing empty lines are
 * dropped and the rest padded with empty lines to a multiple of four.  Of
 * every four lines the first starts with '@' (d_rec_hdr[r] = its byte
 * offset), the second is the sequence, cleaned as a FASTA sequence line
 * (right-stripped, ' ' and '\r' removed; a leading '>' is an invalid base),
 * the third starts with '+', the fourth (quality, never in d_codes) has as
 * many bytes before its terminator as the second.  Wrapped FASTQ is not
 * supported.  KMAN_EFORMAT: no lines ("premature end of file or empty file"),
 * or "FASTQ record <1-based>: <rule>" for the first record that breaks one;
 * info is zeroed then.  Launches are timed under the tag "parse_fastq". */
int kman_parse_fastq(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_codes,
                     uint64_t *d_rec_hdr, uint64_t *d_rec_seq, uint64_t rec_cap, kman_parse_info *info);
/* kman_parse_fastq with a quality threshold.  min_qual_byte is the threshold
 * byte T = phred offset + minimal quality, 0..255 (KMAN_EINVAL above); 0 is
 * kman_parse_fastq itself (the same launches).  A kept sequence byte (one that
 * has a code) at column c of its raw line 4r + 1 is masked when the byte at
 * column c of line 4r + 3 is < T, compared unsigned; columns are counted on
 * the raw lines, before cleaning (blanks inside a sequence line shift code
 * indices, not columns).  A masked code becomes 4 | (code & 8): the code of an
 * 'N' at that place, bit 3 kept.  Everything else (n_bases, n_records, the
 * record table, the 64 pad bytes, every error) is as without a threshold: the
 * outputs are those of kman_parse_fasta for the FASTA of the same records with
 * every masked byte replaced by 'N'.  The mask pass runs after the validation
 * has passed, and is timed under "parse_fastq" too.  *n_masked (may be NULL):
 * the kept bytes whose quality byte is < T, already not-ACGT ones included; 0
 * on error. */
int kman_parse_fastq_q(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, uint8_t *d_codes,
                       uint64_t *d_rec_hdr, uint64_t *d_rec_seq, uint64_t rec_cap,
                       kman_parse_info *info, uint32_t min_qual_byte, uint64_t *n_masked);

/* Number of k-mers kman_extract will emit (valid windows x (RC ? 2 : 1)). */
int kman_count_kmers(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                     uint32_t flags, uint64_t *n_kmers);

/* base codes -> packed keys in stream order (seq.py:285-328), k in [2, 32].
 *   d_keys     out, capacity cap keys
 *   d_pos      out (flags & KMAN_WANT_POS), u32 if pos_bytes == 4 else u64
 *   d_hist     optional out (may be NULL): the radix-digit histograms that
 *              kman_sort would compute, for the pass plan of kman_sort_plan(2k)
 *              (npass x 256 u64, must be zeroed by the caller) */
int kman_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                 uint32_t flags, uint64_t *d_keys, void *d_pos, uint32_t pos_bytes, uint64_t cap,
                 uint64_t *d_hist, uint64_t *n_kmers);

/* kman_extract restricted to the keys in [key_lo, key_hi] (inclusive), in
 * stream order: one key range of a multi-batch join (inputs whose k-mers do
 * not fit the device at once are processed range by range; the ranges'
 * outputs concatenate to the global sorted output, join.py:63-130).  Keys of
 * the range past `cap` are counted, not written: KMAN_ECAP then.  Size the
 * ranges with kman_kmer_prefix_hist. */
int kman_extract_range(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                       uint64_t key_lo, uint64_t key_hi, uint64_t *d_keys, void *d_pos, uint32_t pos_bytes,
                       uint64_t cap, uint64_t *d_hist, uint64_t *n_kmers);
/* The same for the keys whose top map_bits bits p have d_map[p] == map_val
 * (d_map: 2^map_bits bytes): the key ranges a round left out
 * (kman_dround_failed), each destination's in one pass. */
int kman_extract_marked(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                        const uint8_t *d_map, uint32_t map_bits, uint32_t map_val, uint64_t *d_keys, void *d_pos,
                        uint32_t pos_bytes, uint64_t cap, uint64_t *n_kmers);
/* Histogram of the top 8 key bits of the stream (256 u64 into d_hist256) and
 * the k-mer count; flags: KMAN_RC (not KMAN_CANONICAL). */
int kman_kmer_prefix_hist(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                          uint64_t *d_hist256, uint64_t *n_kmers);

/* LSD radix sort plan for keys with key_bits significant bits:
 * npass digit passes of bits[i] bits each, starting at bit shift[i]. */
int kman_sort_plan(uint32_t key_bits, uint32_t *npass, uint32_t *shift, uint32_t *bits);

/* Stable LSD radix sort (onesweep, decoupled look-back) of n keys with an
 * optional payload (val_bytes 0, 4 or 8).  Ping-pongs between the two
 * buffers; *result_in_alt is set to 1 when the sorted data ended in the alt
 * buffers.  d_hist may be NULL (then computed) or the histogram filled by
 * kman_extract for the same key_bits.  Stability == the reference's Timsort
 * stability (batch.py:165). */
int kman_sort(kman_ctx *ctx, uint64_t *d_keys, uint64_t *d_keys_alt, void *d_vals, void *d_vals_alt,
              uint32_t val_bytes, uint64_t n, uint32_t key_bits, const uint64_t *d_hist,
              int *result_in_alt);

/* The same sort restricted to bits [lo_bit, hi_bit): a stable sort by those
 * bits only.  d_hist: NULL or kman_extract's with KMAN_HIST_LO(lo_bit). */
int kman_sort_plan_range(uint32_t lo_bit, uint32_t hi_bit, uint32_t *npass, uint32_t *shift,
                         uint32_t *bits);
int kman_sort_range(kman_ctx *ctx, uint64_t *d_keys, uint64_t *d_keys_alt, void *d_vals, void *d_vals_alt,
                    uint32_t val_bytes, uint64_t n, uint32_t lo_bit, uint32_t hi_bit, const uint64_t *d_hist,
                    int *result_in_alt);

/* Prefix-split sort: kman_sort_range over the top bits [lo_bit, key_bits)
 * (kman_split_bits picks lo_bit so that equal-prefix segments average <= 512
 * keys), then kman_finish completes the order of every segment in LDS and
 * emits in the same pass (Batch.sorted + Crawler.do_batch, batch.py:156-168,
 * join.py:95-130):
 *   SORT   d_keys / d_vals fully sorted in place (stable); *n_out = n
 *   COUNT  d_okeys[j], d_ovals[j] = group size (oval_bytes 4 | 8); d_vals unused
 *   UNIQ   d_okeys[j], d_ovals[j] = payload of keys that occur once
 *          (oval_bytes == val_bytes)
 * Input: keys stably sorted by bits [lo_bit, key_bits).  In COUNT / UNIQ mode
 * the input arrays are scratch afterwards (segments longer than a chunk's
 * staging area are sorted in place through d_*_alt-free temporary buffers).
 *
 * kman_finish takes every 0 <= lo_bit <= key_bits <= 64.  lo_bit == 0: the
 * input is fully sorted and every segment is one group (kman_split_bits
 * gives 0 from n >= 513 * 2^(key_bits - 1) on); lo_bit == key_bits: no prefix,
 * the whole array is one segment.  The input must be stably sorted by
 * key >> lo_bit (the payload of equal prefixes in input order); the order
 * within a prefix is free.  The array is read in chunks of 5120 keys; a chunk
 * owns the segments that start in it and stages them in LDS.  A segment is
 * re-sorted through the fallback (kman_sort on a temporary copy, then a
 * second run of the kernel) exactly when it is the last one its chunk owns
 * and ends at chunk offset 6144 or beyond, i.e. start offset + length >= 6144:
 * 1025 keys at offset 5119 is the shortest.  Outputs are written to rows
 * [0, *n_out) only; d_okeys / d_ovals hold n rows.  tests/finish_cases.py
 * plan() is the executable statement of the per-chunk rules. */
int kman_split_bits(uint64_t n, uint32_t key_bits, uint32_t *lo_bit);

/* kman_extract + kman_sort_range(lo_bit, 2k) in one call: the first prefix
 * pass is fused into the extraction (a histogram pre-pass over the codes, then
 * one kernel that rolls the windows and scatters them by digit 0), so the
 * keys are never written in stream order.  Same result as the two calls;
 * flags as kman_extract's (KMAN_CANONICAL, k > 25 or u64 pos run the two calls). */
int kman_extract_sorted(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                        uint32_t lo_bit, uint64_t *d_keys, uint64_t *d_keys_alt, void *d_pos, void *d_pos_alt,
                        uint32_t pos_bytes, uint64_t cap, uint64_t *n_kmers, int *result_in_alt);
int kman_finish(kman_ctx *ctx, uint64_t *d_keys, uint64_t *d_keys_alt, void *d_vals, void *d_vals_alt,
                uint32_t val_bytes, uint64_t n, uint32_t key_bits, uint32_t lo_bit, int mode,
                uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes, uint64_t *n_out);

/* Count / uniq of one k-mer stream straight from the base codes, through
 * padded regions of packed items (region.hip): extraction scattered by the
 * top 8 key bits, one pass per 8-bit bucket by the next bits, then one LDS
 * block per region sorts, groups and emits.  Replaces the chain
 * Sequence.yield_kmers -> Batch.sorted -> Crawler.do_records/do_batch ->
 * KJoiner.join_sequence_count | join_unique (seq.py:285-328,
 * batch.py:156-168, join.py:63-130,244-285) for one batch stream; same output
 * arrays as kman_extract_sorted + kman_finish(COUNT | UNIQ):
 *   COUNT  d_okeys[j], d_ovals[j] = group size (oval_bytes 4 | 8)
 *   UNIQ   d_okeys[j], d_ovals[j] = pos of the keys that occur once
 * in ascending key order; *n_kmers = k-mers extracted, *n_out = rows.
 * With KMAN_CANONICAL the keys are min(forward, reverse complement), one per
 * window.
 * kman_groups_plan gives the work-area size, or KMAN_EFALLBACK when the input
 * is outside the path (k > 25, too many k-mers for the region capacities).  kman_groups returns KMAN_EFALLBACK also when a region
 * overflowed (a strongly skewed prefix distribution); the outputs are then
 * undefined and the caller runs the general path.  The capacities are three,
 * each fixed by the plan: C0 items per pass-0 region (top 8 key bits, position
 * segment), C1 items per pass-1 sub-region (region, chain) and 8704 items
 * (FCAP) per finish region, its two sub-regions together.  A region filled
 * to exactly its capacity is inside the path (KMAN_OK, every row exact); one
 * more item is KMAN_EFALLBACK, nothing is written past a capacity, and the
 * next call on the ctx starts clean.  d_okeys / d_ovals hold
 * up to n_bases x (RC ? 2 : 1) entries. */
int kman_groups_plan(uint64_t n_bases, uint32_t k, uint32_t flags, int mode, uint64_t *work_bytes);
int kman_groups(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags, int mode,
                void *d_work, uint64_t work_bytes, uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes,
                uint64_t *n_kmers, uint64_t *n_out);

/* kman_groups in three calls, so that its first pass (the extraction) runs
 * while the FASTA is still arriving (the reference reads and extracts one
 * record at a time, batcher.py:454-470 -> seq.py:285-328):
 *   kman_groups_begin    plans, clears the work area and opens the pass;
 *                        *n_tiles tiles, tile t reads codes
 *                        [t * tile_bases, (t + 1) * tile_bases + 64)
 *                        (*n_tiles = 0: the pass runs whole at the end)
 *   kman_groups_extract  extracts tiles up to tile_hi (exclusive) once their
 *                        codes are final; call in increasing tile_hi
 *   kman_groups_end      extracts the rest, then as kman_groups
 * Every call takes the arguments kman_groups takes (n_bases = the final
 * total); no other call of this ctx that uses look-back status words (the
 * general extraction, sorts, other kman_groups) may come in between.  The
 * result equals kman_groups'. */
int kman_groups_begin(kman_ctx *ctx, uint64_t n_bases, uint32_t k, uint32_t flags, int mode, void *d_work,
                      uint64_t work_bytes, uint32_t *n_tiles, uint64_t *tile_bases);
int kman_groups_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                        int mode, void *d_work, uint64_t work_bytes, uint32_t tile_hi);
int kman_groups_end(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags, int mode,
                    void *d_work, uint64_t work_bytes, uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes,
                    uint64_t *n_kmers, uint64_t *n_out);

/* kman_groups across G ranks, in key rounds (one process per GPU over RCCL;
 * kman_amd/dist.py runs the collectives in between).  Rank q
 * holds one byte-range shard of ONE FASTA (its own bytes plus a (k-1)-base
 * halo, see kman_parse_fasta_at); every rank passes the same n_bases_q >=
 * every shard's n_bases (it fixes the pos bits of the packed 8-byte items).
 *   kman_dshard_plan     KMAN_OK, or KMAN_EFALLBACK outside the path (k > 25,
 *                        uniq pos bits + 2k - 8 > 64)
 *   kman_dshard_hist     exact item counts of the shard per (top-8-bit
 *                        bucket b, position segment s): hist[b * 64 + s]
 *                        (host copy of d_hist, 256 x 64 u32)
 *   (caller)             all-gather of the bucket totals; buckets cut into
 *                        G x R contiguous parts: rank q owns parts q*R ..
 *                        q*R+R-1, round r handles part q*R+r of every q
 *   kman_dshard_extract  one round's pass 0: the items of the buckets with
 *                        d_rtab[b * 64 + s] != ~0 written straight into
 *                        d_send, region (b, s) at d_rtab[b * 64 + s]
 *                        (destination-major, no padding, no gather)
 *   (caller)             one all-to-all of the items (kman_alltoallv, 8 B)
 *   kman_dround_plan     arena sizes of one round's finish on a rank
 *   kman_dround_finish   the received items of buckets [b_lo, b_lo + nb)
 *                        (source chunks in rank order, each in bucket order;
 *                        counts[src * nb + j] = items of bucket b_lo + j from
 *                        src) -> the round's count / uniq rows, ascending
 *                        (uniq pos u64 with the source rank in bits 56-63);
 *                        KMAN_EPARTIAL when regions overflowed (skewed
 *                        keys): their key ranges are left out (below).
 *                        d_a (>= a_bytes) may be the send buffer, d_b (>=
 *                        b_bytes) may be d_recv itself.
 * A rank's rounds emit its key range in order; the ranks' outputs in rank
 * order are the global output (Crawler.do_records / do_batch over all
 * batches, join.py:63-130). */
int kman_dshard_plan(uint64_t n_bases, uint64_t n_bases_q, uint32_t k, uint32_t flags, int mode);
int kman_dshard_hist(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint64_t n_bases_q, uint32_t k,
                     uint32_t flags, int mode, uint32_t *d_hist, uint32_t *hist);
int kman_dshard_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint64_t n_bases_q, uint32_t k,
                        uint32_t flags, int mode, const uint32_t *d_hist, const uint64_t *d_rtab, uint64_t *d_send);
int kman_dround_plan(uint32_t k, uint32_t flags, int mode, uint32_t world, uint64_t n_bases_q, uint32_t nb,
                     const uint64_t *counts, uint64_t *a_bytes, uint64_t *b_bytes);
int kman_dround_finish(kman_ctx *ctx, const uint64_t *d_recv, uint32_t k, uint32_t flags, int mode, uint32_t world,
                       uint64_t n_bases_q, uint32_t b_lo, uint32_t nb, const uint64_t *counts, void *d_a,
                       uint64_t a_bytes, void *d_b, uint64_t b_bytes, uint64_t *d_okeys, void *d_ovals,
                       uint32_t oval_bytes, uint64_t *n_out);
/* After kman_dround_finish returned KMAN_EPARTIAL: regions that overflowed a
 * capacity (a key repeated far beyond its region's share) emitted nothing,
 * the other *n_out rows are in place in key order.  kman_dround_failed gives
 * the left-out key ranges as [lo, hi] pairs (2 u64 each, ascending, merged;
 * *n = ranges; NULL ranges: count only) for the caller to redo through
 * kman_extract_marked + kman_sort_range + kman_finish and merge in
 * (kman_merge_runs). */
int kman_dround_failed(kman_ctx *ctx, uint64_t *ranges, uint64_t cap, uint64_t *n);
/* Heavy keys of the last kman_dround_finish (*n; 0 when none or off): keys
 * that every S-th received item's sample saw at least twice (the most often
 * sampled, at most 256 per bucket of the round, held in the pass's LDS while
 * a chain of the bucket runs) are counted apart in its pass 1 -- count mode
 * keeps one copy per pass-1 chain and adds the others to the key's row after
 * the finish, uniq mode drops them all (they occur more than once) -- so a
 * repeat with 10^5 copies does not overflow its regions.  KMAN_HEAVY=0 turns
 * it off, KMAN_HEAVY=1 applies it to rounds of any size (default: >= 2^20
 * items).  Not in the reference: the rows are the same either way. */
int kman_dround_heavy(kman_ctx *ctx, uint32_t *n);
/* After kman_dround_finish (before its arena A is reused): the items of the
 * regions it left out, gathered from its pass-1 output instead of
 * re-extracted from the codes (kman_extract_marked) -- full keys in d_keys
 * and, uniq, the pos its finish would have emitted in d_pos; *n = items
 * (NULL d_keys: count only; cap = room in d_keys / d_pos).  KMAN_EFALLBACK
 * when its pass 1 itself overflowed (its output lacks items): then the
 * marked extraction.  The items' sort + run-length rows equal the left-out
 * regions' rows once kman_dround_heavy_fix has added the heavy keys' dropped
 * copies (count mode).  Not in the reference. */
int kman_dround_left(kman_ctx *ctx, uint64_t *d_keys, uint64_t *d_pos, uint64_t cap, uint64_t *n);
/* Adds the last kman_dround_finish's heavy keys' dropped copies to the rows
 * (d_keys sorted) that hold them: for rows built from kman_dround_left's
 * items (count mode; uniq rows and rows recounted from the codes need none). */
int kman_dround_heavy_fix(kman_ctx *ctx, const uint64_t *d_keys, void *d_vals, uint32_t val_bytes, uint64_t n);

/* Abundance spectrum of a count output (BASELINE config 5; not
 * in the reference): d_hist[c] = number of distinct k-mers seen c times, the
 * last bin collecting every count >= nbins - 1 (bin 0 stays 0).  With
 * KMAN_CANONICAL counts (kman_groups) this is the canonical k-mer spectrum;
 * for odd k those counts equal the `kmer count -r` rows with key <= rc(key)
 * (the reference's -r emits both strands, seq.py:274-282).  d_counts 16-byte aligned. */
int kman_count_hist(kman_ctx *ctx, const void *d_counts, uint32_t count_bytes, uint64_t n, uint64_t *d_hist,
                    uint32_t nbins);

/* k in 33..64 (Sequence.yield_kmers has no k limit, seq.py:285-328): keys
 * as word pairs, hi = the first k - 32 bases (2(k-32) bits), lo = the last 32
 * bases, both 2 bits per base MSB-first, so (hi, lo) in lexicographic order is
 * the reference's str order.
 *   kman_extract_wide  keys (+ pos) in stream order; d_hi = d_lo = NULL only
 *                      counts (*n_kmers); flags KMAN_RC | KMAN_CANONICAL |
 *                      KMAN_WANT_POS as kman_extract
 *   kman_iota_u64      v[i] = i
 *   kman_gather        dst[i] = src[idx[i]] (4 or 8 byte elements)
 *   kman_rle_wide      count / uniq of (hi, lo) pairs sorted lexicographically
 *                      (mode KMAN_FINISH_COUNT: d_ovals = group sizes; UNIQ:
 *                      the pairs of groups of one with their d_vals payload)
 * The sort is two stable kman_sort passes: by lo with an index payload, then
 * by the gathered hi (an LSD sort over 2k bits); the host writers
 * kman_format_*_wide print the pairs. */
int kman_extract_wide(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                      uint64_t *d_hi, uint64_t *d_lo, void *d_pos, uint32_t pos_bytes, uint64_t cap,
                      uint64_t *n_kmers);
int kman_iota_u64(kman_ctx *ctx, uint64_t *d_v, uint64_t n);
int kman_gather(kman_ctx *ctx, const void *d_src, const uint64_t *d_idx, uint64_t n, void *d_dst, uint32_t elem_bytes);
int kman_rle_wide(kman_ctx *ctx, int mode, const uint64_t *d_hi, const uint64_t *d_lo, const void *d_vals,
                  uint32_t val_bytes, uint64_t n, uint64_t *d_ohi, uint64_t *d_olo, void *d_ovals, uint64_t *n_out);

/* Any k >= 2 (the reference has no k limit: Sequence.yield_kmers,
 * seq.py:285-328; FastaBatcher.do asserts only k > 1, batcher.py:477-478):
 * a k-mer as W = ceil(k / 32) words, MSB-first -- word 0 the first
 * k - 32 (W - 1) bases, words 1 .. W-1 32 bases each -- so (w_0 .. w_{W-1})
 * in lexicographic order is the reference's str order (Batch.sorted,
 * batch.py:156-168).  Word-major planes: word j of item i at
 * d_words[j * stride + i] (W = 2 is kman_extract_wide's (hi, lo)).
 *   kman_extract_words  keys (+ pos, (global base << 1) | strand) of the valid
 *                       windows in stream order (records, positions, + then
 *                       - with KMAN_RC; one min(fwd, rc) key per window with
 *                       KMAN_CANONICAL); d_words = d_pos = NULL only counts;
 *                       KMAN_ECAP (with *n_out) when more than cap
 *   kman_rle_words      count / uniq of sorted word keys (Crawler.do_batch +
 *                       join_sequence_count / join_unique, join.py:95-130,
 *                       244-285): KMAN_FINISH_COUNT -> d_ovals = group sizes;
 *                       UNIQ -> the keys of groups of one with their d_vals
 *   kman_batch_tags     d_tags[i] = (start + d_perm[i]) / per_batch: the batch
 *                       of every item of a permutation of stream range
 *                       [start, ..) (Batch.sorted per batch, batch.py:156-168)
 * The sort is LSD over the planes: stable kman_sort passes with an index
 * payload and kman_gather (kman_amd/engine.py sort_words). */
int kman_extract_words(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                       uint64_t *d_words, uint64_t stride, void *d_pos, uint32_t pos_bytes, uint64_t cap,
                       uint64_t *n_out);
int kman_rle_words(kman_ctx *ctx, int mode, const uint64_t *d_words, uint32_t W, uint64_t stride, const void *d_vals,
                   uint32_t val_bytes, uint64_t n, uint64_t *d_owords, uint64_t ostride, void *d_ovals,
                   uint32_t oval_bytes, uint64_t *n_out);
int kman_batch_tags(kman_ctx *ctx, const uint64_t *d_perm, uint64_t n, uint64_t start, uint64_t per_batch,
                    uint64_t *d_tags);

/* Run-length count of sorted keys (join.py:95-130 + 266-285):
 * d_ukeys[j], d_counts[j] (u32 if count_bytes == 4 else u64). */
int kman_rle_count(kman_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint64_t *d_ukeys,
                   void *d_counts, uint32_t count_bytes, uint64_t *n_unique);

/* n-way merge of runs each sorted by key (Crawler.do_records' heapq.merge
 * over sorted batches, kmermaid/join.py:63-93): a tree of stable merge-path
 * 2-way merges in run order, so equal keys keep run order, then in-run order.
 * d_okeys / d_ovals get the merged total; d_tmp_* (same size) is scratch
 * (unused for <= 2 runs).  val_bytes 0 (keys only), 4 or 8.
 * kman_count_descents: number of i with keys[i] < keys[i-1] (0 = sorted). */
typedef struct {
    const uint64_t *keys;
    const void *vals;
    uint64_t n;
} kman_run;
int kman_merge_runs(kman_ctx *ctx, const kman_run *runs, int nruns, uint32_t val_bytes, uint64_t *d_okeys,
                    void *d_ovals, uint64_t *d_tmp_keys, void *d_tmp_vals);
int kman_count_descents(kman_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint64_t *descents);
/* kman_row_digest: a checksum of n result rows (keys + 0 / 4 / 8-byte values)
 * for comparing two joins' outputs without moving them to the host (the
 * at-size tests): out4 = {sum, xor} of h_i = mix(key_i ^ mix(val_i + (first +
 * i) * 0x9E3779B97F4A7C15)) (mix = the murmur3 finaliser), the sum of the
 * values, and the number of i >= 1 with keys[i] <= keys[i-1].  Sums are mod
 * 2^64; slices [a, b) digested with first = a combine by sum / xor / sum. */
int kman_row_digest(kman_ctx *ctx, const uint64_t *d_keys, const void *d_vals, uint32_t val_bytes, uint64_t n,
                    uint64_t first_index, uint64_t *out4);

/* Abundance vectors, KJoiner VEC_COUNT / VEC_COUNT_MASKED (join.py:288-335 ->
 * AbundanceVector.add_count, abundance.py:103-130; the reference's base-class
 * call raises NotImplementedError, so these are its evident semantics): over
 * a key-sorted, stream-stable array with pos payloads ((window << 1) | strand,
 * tagged with the source in bits 56-63 when `tagged`), write d_vec[index] =
 * the size of the item's key run (masked = 0), or (masked = 1) the run's
 * items in other records, only when the run spans several records.  index =
 * pos, or src_base[pos >> 56] + (pos & (2^56 - 1)) when tagged.  Masked:
 * rec_start (nrec ascending, index space) and rec_id (the record identity,
 * one per distinct name) give each item's record.  d_vec (u32) is zeroed by
 * the caller; entries never written stay 0. */
int kman_vec_fill(kman_ctx *ctx, const uint64_t *d_keys, const void *d_pos, uint32_t pos_bytes, uint64_t n,
                  int masked, const uint64_t *d_src_base, uint32_t tagged, const uint64_t *d_rec_start,
                  const uint32_t *d_rec_id, uint64_t nrec, uint32_t *d_vec);
/* Host: one vector as text, "%d\n" per entry v[0], v[stride], .. (n entries;
 * AbundanceVector.write_to, abundance.py:151-168); out NULL: size only. */
int kman_format_vector(const uint32_t *v, uint64_t n, uint64_t stride, char *out, size_t cap, size_t *used,
                       int threads);

/* Keys that occur exactly once, with their payload (join.py:244-263). */
int kman_rle_uniq(kman_ctx *ctx, const uint64_t *d_keys, const void *d_vals, uint32_t val_bytes,
                  uint64_t n, uint64_t *d_okeys, void *d_ovals, uint64_t *n_out);

/* ------------------------------------------------------------ multi-GPU
 * One process per GPU over RCCL (xGMI).  The reference has no collective
 * (joblib pools over temp files); this is the single exchange step that
 * splits the global join by prefix range.
 *   kman_comm_unique_id  rank 0 creates the 128-byte id, the launcher shares it
 *   kman_comm_init       ncclCommInitRank on the context's device
 *   kman_comm_count      the ranks and this rank as the communicator counts
 *                        them (ncclCommCount / ncclCommUserRank)
 *   kman_prefix_hist     d_hist[(key >> shift) & (2^bits - 1)] += 1 (bits <= 14)
 *   kman_allreduce_u64   in-place sum (histograms)
 *   kman_allgather_u64   per-rank counts
 *   kman_alltoallv       grouped send/recv of contiguous per-destination runs
 *   kman_partition       stable partition of keys (+ vals) into nbuckets
 *                        destinations, bucket = d_lut[key >> lut_shift]; one
 *                        onesweep pass; bucket_counts is a host array */
int kman_comm_unique_id(uint8_t *out128);
int kman_comm_init(kman_ctx *ctx, const uint8_t *id128, int nranks, int rank);
int kman_comm_count(kman_ctx *ctx, int *nranks, int *rank);
int kman_comm_destroy(kman_ctx *ctx);
int kman_prefix_hist(kman_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint32_t shift, uint32_t bits,
                     uint64_t *d_hist);
int kman_allreduce_u64(kman_ctx *ctx, uint64_t *d_buf, uint64_t n);
int kman_allgather_u64(kman_ctx *ctx, const uint64_t *d_send, uint64_t *d_recv, uint64_t n);
int kman_alltoallv(kman_ctx *ctx, const void *d_send, const uint64_t *send_counts, const uint64_t *send_offsets,
                   void *d_recv, const uint64_t *recv_counts, const uint64_t *recv_offsets, uint32_t elem_bytes);
/* The same on the context's communication stream, ordered after the work
 * queued so far on its compute stream; completion recorded in event `slot`
 * (0..7).  kman_comm_wait makes the compute stream wait for it: an exchange
 * overlaps the compute on the parts already received (DistPipeline's
 * overlapped rounds). */
int kman_alltoallv_async(kman_ctx *ctx, const void *d_send, const uint64_t *send_counts,
                         const uint64_t *send_offsets, void *d_recv, const uint64_t *recv_counts,
                         const uint64_t *recv_offsets, uint32_t elem_bytes, int slot);
int kman_comm_wait(kman_ctx *ctx, int slot);
int kman_partition(kman_ctx *ctx, const uint64_t *d_keys, uint64_t *d_keys_out, const void *d_vals,
                   void *d_vals_out, uint32_t val_bytes, uint64_t n, const uint8_t *d_lut, uint32_t lut_shift,
                   uint32_t nbuckets, const uint64_t *bucket_counts);

/* ------------------------------------------------------------ helpers
 * kman_tag_batches: keys[i] |= ((first_index + i) / batch_size) << key_bits,
 *   so one stable kman_sort over key_bits + tag bits sorts every stream chunk
 *   of batch_size k-mers on its own (BatcherBase.new_batch, batcher.py:118-131,
 *   then Batch.sorted per batch).  KMAN_EINVAL if the tag does not fit.
 * kman_or_u64 / kman_widen_u32: payload tagging (multi-source joins). */
int kman_tag_batches(kman_ctx *ctx, uint64_t *d_keys, uint64_t n, uint32_t key_bits, uint64_t first_index,
                     uint64_t batch_size);
int kman_or_u64(kman_ctx *ctx, uint64_t *d_v, uint64_t n, uint64_t value);
int kman_widen_u32(kman_ctx *ctx, const uint32_t *d_in, uint64_t *d_out, uint64_t n, uint64_t value);
int kman_memcpy_d2d(kman_ctx *ctx, void *dst, const void *src, size_t bytes);

/* ------------------------------------------------------- abundance filter
 * kman_filter_counts: stable compaction of count rows, keeping those with
 *   lo <= count <= hi in their order; *n_out = the rows kept.
 *   d_keys     W planes of n keys, plane j at d_keys + j * stride (W = 1: the
 *              rows of kman_finish / kman_groups / kman_rle_count, any stride;
 *              W > 1: the word planes of kman_rle_words, stride >= n)
 *   d_counts   n counts of count_bytes (4 or 8)
 *   outputs    both NULL: the rows are only counted (one read of the counts);
 *              equal to the inputs: compacted in place; apart from the inputs
 *              and from each other: written there, the inputs left as they
 *              are (output planes at the same stride).  Anything else
 *              (outputs that overlap the inputs in part, one output NULL) is
 *              KMAN_EINVAL.
 *   n == 0 or lo > hi: *n_out = 0, nothing launched, no error.
 *   One pass over tiles of KMAN_FILTER_TILE rows for W = 1 (12 or 16 B read
 *   per row, as many written per kept row); W > 1: one pass per plane and one
 *   for the counts, each reading the counts.  Synchronises. */
#define KMAN_FILTER_TILE 4096
int kman_filter_counts(kman_ctx *ctx, const uint64_t *d_keys, uint32_t W, uint64_t stride, const void *d_counts,
                       uint32_t count_bytes, uint64_t n, uint64_t lo, uint64_t hi, uint64_t *d_okeys,
                       void *d_ocounts, uint64_t *n_out);

/* ------------------------------------------------------- two count tables
 * kman_match_counts: look every row of table A up in table B.  A and B are
 *   rows (u64 key, count) each STRICTLY ASCENDING in key (distinct, sorted:
 *   the rows of kman_groups / kman_finish / kman_rle_count); this is not
 *   checked -- rows that break it give wrong counts, never a wild address or
 *   an endless loop.  For every row i of A, with ca = its count and cb = the
 *   count of the row of B with the same key ("matched"; none: cb = 0):
 *     KMAN_MATCH_RIGHT    out[i] = cb                      (the plain lookup)
 *     KMAN_MATCH_LEFT     out[i] = matched ? ca : 0
 *     KMAN_MATCH_MIN      out[i] = matched ? min(ca, cb) : 0
 *     KMAN_MATCH_MAX      out[i] = matched ? max(ca, cb) : 0
 *     KMAN_MATCH_SUM      out[i] = matched ? ca + cb : 0
 *     KMAN_MATCH_ABSENT   out[i] = matched ? 0 : ca
 *     KMAN_MATCH_ANY_SUM  out[i] = ca + cb                 (never 0 for ca >= 1)
 *     KMAN_MATCH_ANY_MAX  out[i] = max(ca, cb)
 *   Counts and out are 4 or 8 bytes wide, each chosen on its own; sums are
 *   made in 64 bits, and a value that does not fit out_bytes is stored as the
 *   largest value of that width.  Any other op or width: KMAN_EINVAL.
 *   na == 0: nothing is launched; nb == 0: every row is unmatched and B is
 *   not read.  RIGHT does not read A's counts, LEFT and ABSENT do not read
 *   B's (they may be NULL).  The inputs are never written; d_out (na values)
 *   must not overlap them (not checked).
 *   A merge-path join: a split step cuts the merged order of A and B into
 *   tiles of KMAN_MATCH_TILE rows (the splits in the context's scratch), a
 *   tile kernel matches each tile's A rows against its B rows in LDS, so the
 *   work per block does not depend on na : nb.  8 + a_count_bytes read per A
 *   row, 8 + b_count_bytes per B row, out_bytes written per A row.
 *   Synchronises. */
#define KMAN_MATCH_TILE 2048
#define KMAN_MATCH_RIGHT 0
#define KMAN_MATCH_LEFT 1
#define KMAN_MATCH_MIN 2
#define KMAN_MATCH_MAX 3
#define KMAN_MATCH_SUM 4
#define KMAN_MATCH_ABSENT 5
#define KMAN_MATCH_ANY_SUM 6
#define KMAN_MATCH_ANY_MAX 7
int kman_match_counts(kman_ctx *ctx, const uint64_t *d_akeys, const void *d_acounts, uint32_t a_count_bytes,
                      uint64_t na, const uint64_t *d_bkeys, const void *d_bcounts, uint32_t b_count_bytes,
                      uint64_t nb, int op, void *d_out, uint32_t out_bytes);

/* ------------------------------------------------- reads against a table
 * Not in the reference: for every record of a parsed input, how many of its
 * k-mer windows are rows of a count table, and the sum of those rows' counts.
 *
 * kman_table_index: a prefix index over nt STRICTLY ASCENDING 2k-bit keys
 *   (the rows of kman_groups / kman_finish / kman_rle_count; not checked).
 *   Writes 2^index_bits + 1 words: d_index[p] = the number of rows whose top
 *   index_bits bits (of the 2k-bit key) are < p; d_index[2^index_bits] = nt.
 *   1 <= index_bits <= min(2k, KMAN_SCREEN_MAX_INDEX_BITS), else KMAN_EINVAL.
 *   nt == 0 is legal: an all-zero index, the keys are not read.  One thread
 *   per entry, a lower bound over the keys in bits(nt) <= 64 steps.
 *   Synchronises.
 *
 * kman_screen_records: d_codes, n_bases, k (2..32) and flags as for
 *   kman_extract (codes 16-byte aligned and followed by 64 bytes of padding,
 *   as the parsers write them); flags is 0 or KMAN_CANONICAL, anything else
 *   KMAN_EINVAL.  d_rec_seq: n_records ascending first-base indices (equal
 *   neighbours are empty records).  The table: nt rows (d_tkeys strictly
 *   ascending, d_tcounts of t_count_bytes = 4 or 8) and the index that
 *   kman_table_index made of it with the same k and index_bits.
 *   d_out, three planes of n_records u64, zeroed by the call itself:
 *     d_out[r]                  the valid windows that start in record r (k
 *                               ACGT codes, no record start after the first)
 *     d_out[n_records + r]      how many of them have their key (the canonical
 *                               key under KMAN_CANONICAL) among the table's rows
 *     d_out[2 * n_records + r]  the sum of those rows' counts, modulo 2^64
 *   The record of base b is upper_bound(d_rec_seq, b) - 1: an empty record
 *   gets three zeros, of equal entries the last one owns the bases, windows
 *   before the first entry belong to no record.
 *   n_records == 0: nothing is done.  n_bases < k: nothing is launched and the
 *   planes are zero.  nt == 0: the hit and sum planes are zero, the table is
 *   not read.  An index that does not belong to the table, or keys that are
 *   not ascending, give wrong counts, never a wild address or an endless loop
 *   (bounds are clamped to nt; every search runs a step count fixed before it
 *   starts).
 *   One block per tile of KMAN_SCREEN_TILE windows.  Per valid window: one
 *   index pair, floor(log2(bucket rows)) + 1 key reads at most, one count read
 *   on a hit.  The tile's slice of d_rec_seq is staged in LDS when it has at
 *   most KMAN_SCREEN_REC_CAP entries and searched in global memory otherwise;
 *   each (tile, record, plane) adds to d_out with at most one 64-bit atomic.
 *   Launches are timed under the tag "screen".  Synchronises. */
#define KMAN_SCREEN_MAX_INDEX_BITS 24
#define KMAN_SCREEN_TILE 4096
#define KMAN_SCREEN_REC_CAP 512
int kman_table_index(kman_ctx *ctx, const uint64_t *d_tkeys, uint64_t nt, uint32_t k, uint32_t index_bits,
                     uint64_t *d_index);
int kman_screen_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                        const uint64_t *d_rec_seq, uint64_t n_records, const uint64_t *d_tkeys, const void *d_tcounts,
                        uint32_t t_count_bytes, uint64_t nt, const uint64_t *d_index, uint32_t index_bits,
                        uint64_t *d_out);

/* ------------------------------------------- reads among several references
 * Not in the reference: for every record of a parsed input, how many of its
 * k-mer windows occur in each of up to KMAN_CLASSIFY_MAX_COLORS references.
 * The COLOURED TABLE is the union of the references' k-mers (d_tkeys strictly
 * ascending, as every table here) with one u64 mask per row: bit c is set when
 * reference c holds the key (kman_amd/engine.py color_table builds it from
 * count tables with kman_or_u64, kman_match_counts and kman_merge_runs).
 *
 * kman_classify_records: d_codes, n_bases, k, d_rec_seq, n_records, the table
 *   (d_tkeys, nt), d_index and index_bits are kman_screen_records' arguments,
 *   with its record ownership (upper_bound - 1), its empty records, its
 *   n_bases < k, nt == 0 and n_records == 0 cases and its bounds (a foreign
 *   index or unsorted keys give wrong counts, never a wild address or an
 *   endless loop).  d_tmasks: nt u64 masks.  flags: KMAN_CANONICAL and
 *   KMAN_CLASSIFY_SPECIFIC, anything else KMAN_EINVAL.  n_colors outside
 *   1..KMAN_CLASSIFY_MAX_COLORS: KMAN_EINVAL.  A refused call writes nothing.
 *   d_out, 1 + n_colors planes of n_records u32, zeroed by the call itself:
 *     d_out[r]                        the valid windows that start in record r
 *     d_out[(1 + c) * n_records + r]  how many of them have their key (the
 *                                     canonical key under KMAN_CANONICAL) in a
 *                                     row whose mask has bit c set; under
 *                                     KMAN_CLASSIFY_SPECIFIC only when the
 *                                     mask, cut to its bits < n_colors, is
 *                                     1 << c exactly (no other reference of
 *                                     the call holds the k-mer)
 *   Mask bits at or above n_colors are ignored.  Counts are modulo 2^32 (a
 *   record of 2^32 or more bases: kman_amd/engine.py classify refuses it).
 *   One block per tile of KMAN_SCREEN_TILE windows and ONE lookup per window
 *   whatever n_colors is (kman_screen_records' lookup with the masks as the
 *   counts); the colours are then reduced in chunks of 8 over masks held in
 *   registers: n_colors <= 8 is one chunk, and a chunk none of whose colours
 *   occurs in the tile is skipped.  Each (tile, record, plane) adds to d_out
 *   with at most one 32-bit atomic.  The tile's slice of d_rec_seq is staged
 *   in LDS when it has at most KMAN_SCREEN_REC_CAP entries and searched in
 *   global memory otherwise.  Launches are timed under the tag "classify".
 *   Synchronises.
 *
 * kman_classify_pick: d_planes is kman_classify_records' d_out (1 + n_colors
 *   planes of n_records u32; plane 0 is not read).  d_pick, three planes of
 *   n_records u32, every word written:
 *     d_pick[r]                  the lowest-indexed colour with the largest
 *                                hit count, KMAN_CLASSIFY_NONE when that is 0
 *     d_pick[n_records + r]      that largest count
 *     d_pick[2 * n_records + r]  the largest count among the other colours
 *                                (equal to the largest on a tie; 0 when
 *                                n_colors == 1)
 *   n_colors outside 1..KMAN_CLASSIFY_MAX_COLORS or a NULL pointer with
 *   n_records > 0: KMAN_EINVAL, nothing written.  n_records == 0: nothing is
 *   done.  One thread per record, the planes read coalesced across records.
 *   Launches are timed under "classify_pick".  Synchronises. */
#define KMAN_CLASSIFY_MAX_COLORS 64
#define KMAN_CLASSIFY_SPECIFIC 16u
#define KMAN_CLASSIFY_NONE 0xFFFFFFFFu
int kman_classify_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                          const uint64_t *d_rec_seq, uint64_t n_records, const uint64_t *d_tkeys,
                          const uint64_t *d_tmasks, uint64_t nt, const uint64_t *d_index, uint32_t index_bits,
                          uint32_t n_colors, uint32_t *d_out);
int kman_classify_pick(kman_ctx *ctx, const uint32_t *d_planes, uint64_t n_records, uint32_t n_colors,
                       uint32_t *d_pick);

/* ------------------------------------------- all pairs of a coloured table
 * Not in the reference: how many rows of a coloured table every two of its
 * colours share, the Gram matrix of the bit matrix whose rows are the masks
 * (`kmer compare`: Jaccard, containment and Mash distance of up to 64 inputs
 * from one pass over the table).
 *
 * kman_mask_gram: d_masks, n u64 masks (a coloured table's counts), 8-byte
 *   aligned and no stricter, never written.  Bits at or above n_colors are
 *   ignored: m' = m & (2^n_colors - 1), all 64 bits when n_colors == 64.
 *     d_gram     n_colors x n_colors u64, row-major: G[i][j] = the rows with
 *                bits i and j of m' both set.  Symmetric, both triangles
 *                written; G[c][c] is the row count of colour c.
 *     d_occ      n_colors + 1 u64, may be NULL: occ[p] = the rows with
 *                popcount(m') == p (occ[0]: rows of none of the colours).
 *     d_private  n_colors u64, may be NULL: private[c] = the rows with
 *                m' == 1 << c.
 *   Every non-NULL output is zeroed by the call itself, then filled.  n == 0:
 *   the outputs are zeroed, d_masks is not read and nothing is launched.
 *   n_colors outside 1..KMAN_CLASSIFY_MAX_COLORS, a NULL d_gram, or
 *   n > KMAN_GRAM_MAX_ROWS: KMAN_EINVAL.  A refused call writes nothing.
 *   The work per row does not depend on how many bits the row has set: a wave
 *   takes 64 masks per step (lanes past n contribute 0), forms the n_colors
 *   column words with one 64-lane ballot per colour, lane c keeping column c
 *   and parking it in the wave's own LDS slice; lane i then adds
 *   popcount(col_i AND col_(i+d) mod n_colors) for d = 0 .. n_colors / 2 (every
 *   unordered pair once, at most 33 rounds for the 2080 pairs of 64 colours)
 *   into registers across a grid-stride loop.  occ comes from the ballots of
 *   the seven bits of popcount(m'), private from col_c AND
 *   ballot(popcount(m') == 1).  The accumulators are 32-bit: a step adds at
 *   most 64 and a wave runs at most KMAN_GRAM_MAX_ROWS / (KMAN_GRAM_MAX_BLOCKS *
 *   KMAN_GRAM_THREADS) = 2^22 steps, so a block's sums stay below 2^30.  They
 *   are added up in LDS and flushed ONCE per block, one 64-bit integer atomic
 *   per nonzero entry (two for i != j): two identical calls give identical
 *   bytes.  Grid: min(KMAN_GRAM_MAX_BLOCKS, ceil(n / KMAN_GRAM_THREADS)) blocks
 *   of KMAN_GRAM_THREADS threads (four per CU on 256 CUs), not proportional to
 *   n; one grid stride is KMAN_GRAM_MAX_BLOCKS * KMAN_GRAM_THREADS rows.
 *   Launches are timed under the tag "gram".  Synchronises. */
#define KMAN_GRAM_THREADS 256
#define KMAN_GRAM_MAX_BLOCKS 1024
#define KMAN_GRAM_MAX_ROWS (1ull << 40)
int kman_mask_gram(kman_ctx *ctx, const uint64_t *d_masks, uint64_t n, uint32_t n_colors, uint64_t *d_gram,
                   uint64_t *d_occ, uint64_t *d_private);

/* ------------------------------------------------- unitigs of a count table
 * Not in the reference: the compacted de Bruijn graph of a CANONICAL count
 * table (`kmer unitigs`), whose nodes are the table's rows and whose
 * non-branching paths are merged into unitigs.  k is odd, 3 <= k <= 31, so no
 * k-mer is its own reverse complement.
 *
 * Definition.  Row i holds the canonical k-mer x_i (keys strictly ascending).
 *   A row has two sides, KMAN_GRAPH_R (the right end of the canonical spelling)
 *   and KMAN_GRAPH_L; the pair is packed as (row << 1) | side.
 *   Neighbours of side R of x: for each base b, y = x[1:] + b; when c =
 *   min(y, revcomp(y)) is a row, that row is a neighbour, entered at its side L
 *   when y == c and at its side R otherwise.  Of side L: y = b + x[:-1],
 *   entered at R when y == c, else at L.  deg(x, s) counts the bases that give
 *   a neighbour; two bases that reach one row count twice.
 *   Side (i, s) is LINKED to (j, t) when deg(i, s) == 1, its one neighbour is
 *   (j, t), deg(j, t) == 1 and j != i.  Links are symmetric.
 *   A UNITIG is a connected component of the links, a path or a cycle; a cycle
 *   is cut at side L of its smallest row (that link and its partner go).  A
 *   path starts at the end row with the smaller index.  Walking from there, a
 *   row that is left through R is spelled as its key, one left through L as
 *   the reverse complement (the last row is left through the side opposite
 *   the one it was entered by, a lone row through R); the unitig's text is the
 *   first row's k bases and the last base of every later row.  Unitigs are
 *   ordered by their start row.
 *
 * kman_graph_links: d_tkeys, nt, k and the index that kman_table_index made of
 *   these keys with this k and index_bits.  d_link, 2 nt u32, every word
 *   written: d_link[2 i + s] = the packed partner of side s of row i, or
 *   KMAN_GRAPH_NONE.  k even or outside 3..31, index_bits outside
 *   1..min(2k, KMAN_SCREEN_MAX_INDEX_BITS), nt >= KMAN_GRAPH_MAX_ROWS or a NULL
 *   pointer with nt > 0: KMAN_EINVAL, nothing written.  nt == 0: nothing is
 *   done.  One thread per row: its 8 neighbour keys are looked up with the 8
 *   searches advancing in lockstep, floor(log2(bucket rows)) + 1 key reads each
 *   at most; a second launch applies the mutual rule.  An index that does not
 *   belong to the table, or keys that are not ascending, give wrong links,
 *   never a wild address or an endless loop (bounds are clamped to nt; every
 *   search runs a step count fixed before it starts), and what is written is
 *   still symmetric: d_link[v] == u wherever d_link[u] == v.  The inputs are
 *   not written.  8 nt bytes of the context's scratch.  Launches are timed
 *   under the tag "graph_links".  Synchronises.
 *
 * kman_graph_rank: d_link as kman_graph_links writes it (a word >= 2 nt reads
 *   as KMAN_GRAPH_NONE), never written.  Three outputs of nt u32, every word
 *   written:
 *     d_start[i]  the start row of row i's unitig
 *     d_pos[i]    (position of row i in the walk from the start << 1) |
 *                 orientation: 0 = spelled as its key, 1 = reverse complement
 *     d_nodes[i]  the unitig's rows when row i is its start, 0 otherwise
 *   List ranking over the 2 nt states "leave row i through side s" by pointer
 *   doubling, one launch per round over all states and a device word that
 *   tells the host whether a pointer moved: at most ceil(log2(2 nt)) + 1
 *   rounds, fewer when nothing moves earlier (a path of p rows: ceil(log2(p -
 *   1)) rounds that move).  No kernel loops over a unitig.  States that then
 *   point at no end lie on cycles: each cycle's smallest row comes from a
 *   minimum carried through the rounds, its side-L link and the partner's are
 *   cut in a private copy of the links, those states are set up again and the
 *   rounds repeated.  *rounds (may be NULL): the rounds in which a pointer
 *   moved, both passes; *cycles (may be NULL): the cycles cut.  nt == 0:
 *   nothing is done, both are 0.  nt >= KMAN_GRAPH_MAX_ROWS or a NULL array
 *   with nt > 0: KMAN_EINVAL, nothing written.  Links that are not symmetric
 *   give wrong ranks within the same bounds and round counts.  56 nt + 16
 *   bytes of the context's scratch.  Launches are timed under "graph_rank".
 *   Synchronises (once per round).
 *
 * kman_unitig_spell: the table (d_tkeys, d_tcounts of count_bytes = 4 or 8,
 *   nt, k) and kman_graph_rank's three arrays; none is written.  Outputs, for
 *   *n_unitigs = U unitigs of *n_bases = B bases in all:
 *     d_off     U + 1 u64: unitig u's text is d_seq[d_off[u], d_off[u + 1]);
 *               d_off[U] = B
 *     d_unodes  U u32: its rows (its text has that many + k - 1 bases)
 *     d_kc      U u64: the sum of its rows' counts, modulo 2^64
 *     d_seq     B bytes of ACGT, not terminated
 *   in the order of the start rows.  All four NULL: only *n_unitigs and
 *   *n_bases are set (the call that sizes the buffers; d_tkeys, d_tcounts and
 *   d_start are then not read).  Else d_off holds unitig_cap + 1 words,
 *   d_unodes and d_kc unitig_cap, d_seq seq_cap bytes; a capacity below U or B
 *   is KMAN_ECAP with both numbers set and nothing written.  Some but not all
 *   outputs NULL, k even or outside 3..31, count_bytes not 4 or 8, nt >=
 *   KMAN_GRAPH_MAX_ROWS, a NULL input with nt > 0: KMAN_EINVAL, nothing
 *   written.  nt == 0: both numbers are 0, nothing is launched or written.
 *   One pass of tiles of KMAN_UNITIG_TILE rows counts the starts and sums their
 *   bases (two block scans, two decoupled look-backs); then one thread per row
 *   writes the row's own base (a start: its k bases, offset and rows) and adds
 *   its count to d_kc with one 64-bit integer atomic: two calls give equal
 *   bytes.  Rank arrays that are not kman_graph_rank's give wrong text within
 *   the outputs' bounds.  12 nt + 8 bytes of the context's scratch.  Launches
 *   are timed under "unitig_spell".  Synchronises.
 *
 * kman_format_unitigs (host): ">ID LN:i:BASES KC:i:SUM\nSEQ\n" per unitig, ID
 *   = first_id + u in decimal, the sequence on one line.  seq, off (n + 1
 *   words) and kc are host copies of kman_unitig_spell's outputs.  The
 *   kman_format_* contract: *used is the size, KMAN_ECAP when cap is short or
 *   out is NULL; n == 0 writes nothing.
 *
 * Edges between unitigs (`kmer unitigs --gfa`).  Unitig u has the text T_u that
 *   kman_unitig_spell writes.  Orientation "+" (o = 0) reads T_u, orientation
 *   "-" (o = 1) reads revcomp(T_u).  END e = 2 u + o is the right end of the
 *   oriented text.  There is an EDGE (u, o) -> (v, p) when, for a base b, the
 *   k-mer suffix_{k-1}(oriented T_u) + b is the first k-mer of v's text in
 *   orientation p.  Within an end the edges are ordered by b, A C G T, the base
 *   that extends the oriented text; the ends are ordered by e.
 *   In rows: the "+" end of u is (its last row, the side that row is left
 *   through), the "-" end is (its first row, the side opposite the one it is
 *   left through); such a side's neighbours are those of the definition above.
 *   A neighbour (j, t) names v "+" when j is v's first row and t the side that
 *   row is entered by, v "-" when j is v's last row and t the side it is left
 *   through.  Exactly one of the two holds: a side with a neighbour it is not
 *   linked to is never inside a unitig, the two ends of a cut cycle see each
 *   other, and both sides of a row that neighbours itself are ends.
 *   No edge occurs twice; with (u, o, v, p) the edge (v, !p, u, !o) is present
 *   (an edge can be its own mirror); an end has at most 4 edges, E <= 8 U.
 *
 * kman_unitig_edges: d_tkeys, nt, k, the index of kman_table_index (d_index,
 *   index_bits) and kman_graph_rank's three arrays; none is written.  Outputs
 *   in CSR form, for *n_ends = 2 U ends and *n_edges = E edges:
 *     d_eoff  2 U + 1 u64: the edges of end e are d_edge[d_eoff[e],
 *             d_eoff[e + 1]); d_eoff[2 U] = E
 *     d_edge  E u32: (v << 1) | p
 *   Both NULL: only *n_ends and *n_edges are set (the sizing call; it runs the
 *   lookups too, so a caller that can afford the bound edge_cap = 4 * 2 U makes
 *   one filling call instead).  Else d_eoff holds end_cap + 1 words and d_edge
 *   edge_cap; a capacity below 2 U or E is KMAN_ECAP with both numbers set and
 *   nothing written.  One output NULL, k even or outside 3..31, index_bits
 *   outside 1..min(2k, KMAN_SCREEN_MAX_INDEX_BITS), nt >= KMAN_GRAPH_MAX_ROWS, a
 *   NULL input with nt > 0: KMAN_EINVAL, nothing written.  nt == 0: both
 *   numbers are 0 and d_eoff[0] = 0 when d_eoff is given.
 *   Four passes: kman_unitig_spell's tile pass gives every first row its
 *   unitig's ordinal; one thread per row notes the two ends' (row, side); one
 *   thread per end, in tiles of KMAN_EDGE_TILE ends, looks its 4 extensions up
 *   with the 4 searches advancing in lockstep (once per filling call), maps
 *   every hit through d_start, d_pos and the ordinals to (v << 1) | p, keeps
 *   the up to 4 words and takes its offset from a block scan and a decoupled
 *   look-back over the tiles; a last pass compacts the words into d_edge.  No
 *   atomics: two calls give equal bytes.  An index or rank arrays that do not
 *   belong to the table give wrong edges, never a wild address or an endless
 *   loop (every row, start, ordinal and offset read from memory is compared
 *   with its array's size; every search runs a step count fixed before it
 *   starts).  56 U bytes of the context's scratch and 4 nt of its second
 *   scratch.  Launches are timed under "unitig_edges".  Synchronises.
 *
 * kman_format_gfa_segments (host): "S\tID\tSEQ\tLN:i:BASES\tKC:i:SUM\n" per
 *   unitig, the arguments of kman_format_unitigs.
 * kman_format_gfa_links (host): "L\tU\t+|-\tV\t+|-\t(k-1)M\n" per edge of the
 *   n_units unitigs from first_id on, in CSR order.  eoff points at the first
 *   of the slice's 2 n_units + 1 offsets, whose values are absolute and read
 *   relative to eoff[0]; edge points at the slice's first edge.  V is the
 *   word's unitig as it stands (an absolute ID).  Offsets that descend, k even
 *   or outside 3..31: KMAN_EINVAL.  Both under the kman_format_* contract. */
#define KMAN_GRAPH_R 0
#define KMAN_GRAPH_L 1
#define KMAN_GRAPH_NONE 0xFFFFFFFFu
#define KMAN_GRAPH_MAX_ROWS (1ull << 31)
#define KMAN_UNITIG_TILE 2048
#define KMAN_EDGE_TILE 256
int kman_graph_links(kman_ctx *ctx, const uint64_t *d_tkeys, uint64_t nt, uint32_t k, const uint64_t *d_index,
                     uint32_t index_bits, uint32_t *d_link);
int kman_graph_rank(kman_ctx *ctx, const uint32_t *d_link, uint64_t nt, uint32_t *d_start, uint32_t *d_pos,
                    uint32_t *d_nodes, uint32_t *rounds, uint64_t *cycles);
int kman_unitig_spell(kman_ctx *ctx, const uint64_t *d_tkeys, const void *d_tcounts, uint32_t count_bytes, uint64_t nt,
                      uint32_t k, const uint32_t *d_start, const uint32_t *d_pos, const uint32_t *d_nodes,
                      uint64_t *d_off, uint32_t *d_unodes, uint64_t *d_kc, uint64_t unitig_cap, uint8_t *d_seq,
                      uint64_t seq_cap, uint64_t *n_unitigs, uint64_t *n_bases);
int kman_format_unitigs(const uint8_t *seq, const uint64_t *off, const uint64_t *kc, uint64_t n, uint64_t first_id,
                        char *out, size_t cap, size_t *used, int threads);
int kman_unitig_edges(kman_ctx *ctx, const uint64_t *d_tkeys, uint64_t nt, uint32_t k, const uint64_t *d_index,
                      uint32_t index_bits, const uint32_t *d_start, const uint32_t *d_pos, const uint32_t *d_nodes,
                      uint64_t *d_eoff, uint64_t end_cap, uint32_t *d_edge, uint64_t edge_cap, uint64_t *n_ends,
                      uint64_t *n_edges);
int kman_format_gfa_segments(const uint8_t *seq, const uint64_t *off, const uint64_t *kc, uint64_t n,
                             uint64_t first_id, char *out, size_t cap, size_t *used, int threads);
int kman_format_gfa_links(const uint64_t *eoff, const uint32_t *edge, uint64_t n_units, uint64_t first_id, uint32_t k,
                          char *out, size_t cap, size_t *used, int threads);

/* ------------------------------------------- per-record order statistic
 * Not in the reference: one quantile (the median, by default) of the table
 * counts of a record's k-mer windows.  A sum commutes and an order statistic
 * does not, so the per-window counts are written once and a selection runs
 * inside every record.
 *
 * kman_window_counts: the arguments of kman_screen_records without the
 *   record table and d_out, checked the same way (a refused call writes
 *   nothing), plus d_wc, 16-byte aligned, room for n_bases u32.  For every
 *   b < n_bases:
 *     d_wc[b] = KMAN_WC_NONE   no valid window starts at base b (the windows
 *                              that kman_screen_records' first plane counts
 *                              are the others): the last k - 1 bases of a
 *                              record and of the input; every word when
 *                              n_bases < k (nothing is launched then)
 *               otherwise      the count of the window's key (the canonical
 *                              key under KMAN_CANONICAL) in the table: 0 when
 *                              it is not a row, 0xFFFFFFFE when a u64 count is
 *                              larger than that
 *   Words past n_bases are not written.  One block per tile of
 *   KMAN_SCREEN_TILE windows, the lookup of kman_screen_records (the same
 *   device function, the same bounds: a foreign index or unsorted keys give
 *   wrong counts, never a wild address or an endless loop), a 4 B store per
 *   base in 16-byte vectors.  Launches are timed under "window_counts".
 *   Synchronises.
 *
 * kman_record_quantile: record r owns bases [d_rec_seq[r], d_rec_seq[r + 1]),
 *   the last record runs to n_bases; equal neighbours are empty records,
 *   bases before d_rec_seq[0] belong to nobody, entries are clamped to
 *   n_bases.  With v_0 <= .. <= v_{w-1} the record's words that are not
 *   KMAN_WC_NONE, ascending: d_q[r] = v_{floor((w - 1) * num / den)}, and 0
 *   when w == 0.  1/2 is the lower median, 0/1 the minimum, 1/1 the maximum.
 *   1 <= den <= 65535 and num <= den, else KMAN_EINVAL with nothing written.
 *   d_q: n_records u32.  d_wc (16-byte aligned) is scratch afterwards.
 *   n_records == 0: nothing is done.
 *   Records of at most KMAN_QUANTILE_REC_CAP bases: a chunk of
 *   KMAN_QUANTILE_TILE bases owns the records that start in it, stages them
 *   whole in LDS and a wave per record radix-selects the word (8-bit digits);
 *   the chunk's slice of d_rec_seq is staged when it has at most
 *   KMAN_QUANTILE_SLICE records and read from global memory otherwise.
 *   Longer records are listed, gathered as (slot << 32 | word) keys, sorted
 *   with kman_sort and picked by rank; this needs work memory:
 *   kman_record_quantile_plan (host only) gives the bytes for n_long_records
 *   records longer than KMAN_QUANTILE_REC_CAP bases holding n_long_values
 *   bases together (0, 0: the size every call needs).  d_work 16-byte aligned.
 *   A buffer too small for the records met: KMAN_ECAP, no fault (d_q may then
 *   hold the short records' words already).  An unsorted d_rec_seq gives wrong
 *   or unwritten words, never a wild address.  Launches are timed under
 *   "record_quantile" and, the long records' gather and pick,
 *   "record_quantile_long".  Synchronises. */
#define KMAN_WC_NONE 0xFFFFFFFFu
#define KMAN_QUANTILE_TILE 4096
#define KMAN_QUANTILE_REC_CAP 2048
#define KMAN_QUANTILE_SLICE 1024
int kman_window_counts(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                       const uint64_t *d_tkeys, const void *d_tcounts, uint32_t t_count_bytes, uint64_t nt,
                       const uint64_t *d_index, uint32_t index_bits, uint32_t *d_wc);
int kman_record_quantile_plan(uint64_t n_long_records, uint64_t n_long_values, uint64_t *work_bytes);
int kman_record_quantile(kman_ctx *ctx, uint32_t *d_wc, uint64_t n_bases, const uint64_t *d_rec_seq,
                         uint64_t n_records, uint32_t num, uint32_t den, void *d_work, uint64_t work_bytes,
                         uint32_t *d_q);

/* ------------------------------------------- per-record longest solid run
 * Not in the reference: where in a record the trusted k-mers are.  Over
 * kman_window_counts' words, base b is SOLID when d_wc[b] != KMAN_WC_NONE and
 * d_wc[b] >= min_count.  A RUN of record r is a maximal interval of solid
 * bases inside r's range: it is cut at the record's ends even when the
 * neighbouring record's words are solid (hand-built words need not have the
 * KMAN_WC_NONE gap that kman_window_counts leaves before every record start).
 *
 * kman_record_runs: d_wc, n_bases u32 as kman_window_counts writes them
 *   (16-byte aligned); the call does NOT modify them (kman_record_quantile
 *   leaves them as scratch: on one buffer, runs go first).  Record ownership
 *   is kman_record_quantile's: record r owns bases [d_rec_seq[r],
 *   d_rec_seq[r + 1]), the last record runs to n_bases; entries are clamped to
 *   n_bases; bases before d_rec_seq[0] belong to nobody; of equal entries the
 *   last one owns the bases, the others are empty records.
 *   d_out, two planes of n_records u64, zeroed by the call itself:
 *     d_out[r]              start: the offset from d_rec_seq[r] of the
 *                           leftmost run of that length
 *     d_out[n_records + r]  len: the length, in windows, of r's longest run
 *   Both are 0 when r has no solid base or is empty.
 *   1 <= min_count <= 0xFFFFFFFE, else KMAN_EINVAL; a NULL pointer with
 *   non-zero sizes: KMAN_EINVAL; work_bytes below kman_record_runs_plan's
 *   (host only; d_work 16-byte aligned): KMAN_ECAP.  A refused call writes
 *   nothing.  n_records == 0: nothing is done.  n_bases == 0: both planes are
 *   zero, nothing else is launched, d_wc and d_work may be NULL.
 *   Tiles of KMAN_RUNS_TILE bases, 256 threads, 16 consecutive words per
 *   thread.  Pass 1 writes 1 + the position of each tile's last non-solid base
 *   (read from the tile's end, it stops at the first quarter that holds one);
 *   one block max-scans those words over the tiles; pass 2 reads the tile
 *   again: a run starts at the larger of that carried position and its
 *   record's first base, and at a run's end its length is known.  The tile's
 *   slice of d_rec_seq is staged in LDS when it has at most KMAN_RUNS_REC_CAP
 *   entries and searched in global memory otherwise.  Runs are reduced in LDS
 *   per (tile, record); a record inside one tile is stored directly, one that
 *   reaches out of its tile (at most two per tile) takes one 64-bit atomic max
 *   on len and, from a last kernel over the tiles' candidates, one 64-bit
 *   atomic min on start among those that reach it: the same bytes on every
 *   call.  The words are read at most twice (8 B per base), 16 B are written
 *   per record, 56 B of work memory per tile.
 *   An unsorted d_rec_seq gives wrong or unwritten words, never a wild address
 *   or an unbounded loop: every record index comes from a search over at most
 *   n_records entries and is checked against n_records, every LDS index
 *   against its region.  Launches are timed under "record_runs".
 *   Synchronises. */
#define KMAN_RUNS_TILE 4096
#define KMAN_RUNS_REC_CAP 512
int kman_record_runs_plan(uint64_t n_bases, uint64_t n_records, uint64_t *work_bytes);
int kman_record_runs(kman_ctx *ctx, const void *d_wc, uint64_t n_bases, const void *d_rec_seq, uint64_t n_records,
                     uint32_t min_count, void *d_work, uint64_t work_bytes, void *d_out);

/* ------------------------------------------------- the listed records' text
 * Not in the reference: the records of the input text that a screen lists,
 * written as one text on the device, whole or cut to one column interval, so
 * that only the text crosses PCIe (`kmer screen --reads-out`, `--trim`).
 *
 * kman_cut_records: d_text, n_bytes of input text (16-byte aligned; FASTA or
 *   FASTQ).  d_rec_off: n_records + 1 byte offsets, record r is the bytes
 *   [d_rec_off[r], d_rec_off[r + 1]): the parsers' d_rec_hdr followed by
 *   n_bytes.  The offsets themselves need no alignment.  d_keep: one byte per
 *   record, a record is written when its byte is not 0 (NULL: every record).
 *   Without KMAN_CUT_TRIM a written record is its bytes, verbatim, and d_start
 *   and d_end are NULL.  With it (four-line FASTQ records) they hold one column
 *   interval [START, END) per record, and with L1..L4 the record's first four
 *   lines without their terminators ("\n", "\r\n" or a lone "\r" ends a line;
 *   a line that the record does not have is empty), body = L2 right-stripped
 *   of " \t\v\f" and the bytes 0x1c..0x1f, cols = the offsets of the bytes of
 *   body that are not ' ', c0 = cols[START], c1 = cols[END - 1] + 1, the
 *   record is written as
 *       L1 "\n" L2[c0, c1) "\n" L3 "\n" L4[c0, c1) "\n"
 *   (L4 cut like a Python slice: both ends clamped to its length).  These are
 *   the columns of kman_parse_fastq's codes and of kman_parse_fastq_q's mask.
 *   The text is the written records' texts in input order.  *used = its size.
 *   d_out (16-byte aligned) NULL: sizing only, cap is taken as 0.  A text
 *   larger than cap: KMAN_ECAP, *used is set and d_out is not written at all.
 *   Records are independent: the slice [i0, i0 + m) of d_keep, d_start and
 *   d_end with the m + 1 offsets from d_rec_off + i0 gives the matching slice
 *   of the text.
 *   flags other than KMAN_CUT_TRIM, d_start or d_end given without
 *   KMAN_CUT_TRIM, and, with n_records > 0, a NULL d_rec_off or d_work, a NULL
 *   d_text with n_bytes > 0, a NULL d_start or d_end under KMAN_CUT_TRIM, a
 *   misaligned d_text, d_out or d_work, or more than 2^31 records: KMAN_EINVAL.
 *   work_bytes below kman_cut_records_plan's (host only; 16 B per record, 64
 *   under KMAN_CUT_TRIM, and 16): KMAN_ECAP.  A refused call writes nothing.
 *   n_records == 0: nothing is launched, *used = 0.  The inputs are never
 *   modified.
 *   Bad data gives defined bytes, never a wild address or an unbounded loop:
 *   every offset is clamped to n_bytes; a record with d_rec_off[r + 1] <=
 *   d_rec_off[r] writes nothing; under KMAN_CUT_TRIM a record with START >=
 *   END or START >= len(cols) writes nothing and END is clamped to len(cols);
 *   every line search ends at the record's end.
 *   Pass 1 turns every record into segments (source, output length): one
 *   thread per record, or, under KMAN_CUT_TRIM, one wave per record that walks
 *   it 1024 bytes at a time (a record of any length: about length / 1024
 *   steps of that wave).  The lengths are scanned with the decoupled
 *   look-back.  Pass 2 runs one block per KMAN_CUT_TILE output bytes: its
 *   slice of the segments is staged in LDS when it has at most
 *   KMAN_CUT_SEG_CAP of them and searched in global memory otherwise; every
 *   output word is one 16-byte store, made of two 16-byte text loads and a
 *   byte shift where it lies inside one segment.  Text bytes are read about
 *   once, under KMAN_CUT_TRIM lines 1 and 2 twice.  Launches are timed under
 *   the tag "cut_records".  Synchronises. */
#define KMAN_CUT_TRIM 1u
#define KMAN_CUT_TILE 16384
#define KMAN_CUT_SEG_CAP 1024
int kman_cut_records_plan(uint64_t n_records, uint32_t flags, uint64_t *work_bytes);
int kman_cut_records(kman_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, const uint64_t *d_rec_off,
                     uint64_t n_records, const uint8_t *d_keep, const uint64_t *d_start, const uint64_t *d_end,
                     uint32_t flags, void *d_work, uint64_t work_bytes, char *d_out, size_t cap, size_t *used);

/* ------------------------------------------- isolated substitution errors
 * Not in the reference: the base that one substitution error changed, put back
 * from the table (`kmer screen --solid C --correct`).  Over
 * kman_window_counts' words on these codes, this table, k and flags, window
 * start b is WEAK when d_wc[b] != KMAN_WC_NONE and d_wc[b] < min_count, SOLID
 * when d_wc[b] != KMAN_WC_NONE and d_wc[b] >= min_count.  A WEAK RUN [a, b) of
 * record r (bases [s, e), kman_record_runs' ownership) is a maximal interval
 * of weak window starts inside [s, e).  With
 *     L = a > s and a - 1 is solid          openL = a == s
 *     R = b + k <= e and b is solid         openR = b + k == e + 1
 * the run names a SITE p in exactly these cases:
 *     L and R,     b - a == k    p = b - 1
 *     L and openR, b - a <= k    p = a + k - 1
 *     openL and R, b - a <= k    p = b - 1
 * (a KMAN_WC_NONE neighbour, both sides open, L and R with another length: no
 * site).  The windows of r that cover p are then exactly the run's.  With o
 * the base at p, ok(x) for x != o: every window of the run, read with x at p,
 * has a count >= min_count in the table (its canonical key under
 * KMAN_CANONICAL).  The site is corrected to x when exactly one x is ok.
 * Sites are judged on the codes and words as given; two sites of a record
 * never share a window.
 *
 * kman_correct_sites: d_codes, n_bases, k (2..32), flags (0 or
 *   KMAN_CANONICAL), the table, d_index and index_bits as for
 *   kman_window_counts; d_wc its words on them (16-byte aligned); d_rec_seq,
 *   n_records and min_count (1..0xFFFFFFFE) as for kman_record_runs.  Checked
 *   as those two check them: KMAN_EINVAL, and a refused call writes nothing.
 *   d_fix, n_bases bytes, every one written by the call (it fills the plane
 *   itself): KMAN_FIX_NONE, or the new 2-bit base of a corrected site.
 *   *n_fixed (may be NULL): the corrected bases.  Neither d_codes nor d_wc is
 *   modified.  n_bases < k or n_records == 0: d_fix is KMAN_FIX_NONE
 *   throughout, *n_fixed = 0, nothing else is launched.  n_bases == 0: nothing
 *   is done.
 *   One block of 256 threads per tile of KMAN_CORRECT_TILE bases; the tile's
 *   words and a halo of 36 go to LDS; the tile's slice of d_rec_seq is staged
 *   when it has at most KMAN_CORRECT_REC_CAP entries and searched in global
 *   memory otherwise.  The lane of a run's first base reads at most k more
 *   words (nothing is carried across tiles); a wave then evaluates its lanes'
 *   sites one at a time: 64 codes, at most 3 k lookups (kman_screen_records'
 *   device function and bounds), three votes, one byte stored.  Every byte of
 *   d_fix has one writer after the fill; the count is one atomic add per wave:
 *   the same bytes on every call.  A d_wc, index or d_rec_seq that does not
 *   belong to these codes gives wrong corrections, never a wild address or an
 *   unbounded loop.  Launches are timed under "correct_sites".  Synchronises.
 *
 * kman_apply_fixes: d_fix as kman_correct_sites writes it (16-byte aligned;
 *   a byte other than KMAN_FIX_NONE is taken modulo 4).
 *   Codes: d_codes[b] = d_fix[b] | (d_codes[b] & 8) where d_fix[b] !=
 *   KMAN_FIX_NONE.
 *   Counts: d_nfix[r] (n_records u32, every word written) = the bytes of d_fix
 *   that are not KMAN_FIX_NONE among the bases of record r (kman_record_runs'
 *   ownership).
 *   Text: d_text NULL, or n_bytes of four-line FASTQ text (16-byte aligned)
 *   with d_rec_off, kman_cut_records' n_records + 1 offsets (the parser's
 *   d_rec_hdr followed by n_bytes).  The kept characters of record r are the
 *   bytes of its second line (kman_cut_records' line rule) that are not ' ',
 *   in order: the i-th is the character of base d_rec_seq[r] + i (blanks
 *   inside a sequence line shift code indices), and bytes that the parser's
 *   right strip removed come after the last base.  The text byte of a fixed
 *   base becomes "ACGT"[x], "acgt"[x] when the byte it replaces is a lower-case
 *   letter.  The quality line and every other byte are untouched.
 *   A NULL pointer with non-zero sizes, d_text without d_rec_off, a misaligned
 *   d_fix or d_text, more than 2^31 records: KMAN_EINVAL, nothing written.
 *   One thread per 16 bases for the codes; one wave per record for the count
 *   and the text (a record of L bytes: about L / 1024 steps of that wave,
 *   kman_cut_records' limit for very long reads; a record without a fix is
 *   not searched in the text).  Offsets are clamped to n_bytes and n_bases, a
 *   descending pair is an empty record.  Launches are timed under
 *   "apply_fixes".  Synchronises. */
#define KMAN_FIX_NONE 0xFFu
#define KMAN_CORRECT_TILE 4096
#define KMAN_CORRECT_REC_CAP 512
int kman_correct_sites(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                       const uint32_t *d_wc, const uint64_t *d_rec_seq, uint64_t n_records, const uint64_t *d_tkeys,
                       const void *d_tcounts, uint32_t t_count_bytes, uint64_t nt, const uint64_t *d_index,
                       uint32_t index_bits, uint32_t min_count, uint8_t *d_fix, uint64_t *n_fixed);
int kman_apply_fixes(kman_ctx *ctx, uint8_t *d_codes, uint64_t n_bases, const uint8_t *d_fix,
                     const uint64_t *d_rec_seq, uint64_t n_records, uint8_t *d_text, uint64_t n_bytes,
                     const uint64_t *d_rec_off, uint32_t *d_nfix);

/* ------------------------------------------------- two inputs, zipped by record
 * Not in the reference: the codes of two parsed inputs whose i-th records are
 * the two mates of pair i, interleaved by record in one buffer (`kmer screen
 * --mate`, `kmer classify --mate`): mate 1 of pair 0, mate 2 of pair 0, mate 1
 * of pair 1, ..  The lookup kernels cut windows at bit 3 of the codes and
 * attribute them by the record table they are given: with every second entry
 * of the zipped table they count per pair, with every entry per mate.
 *
 * kman_zip_records: d_codes1, n_bases1 and d_codes2, n_bases2: the codes of
 *   the two inputs as the parsers write them (16-byte aligned).  d_rec_seq1,
 *   d_rec_seq2: their record tables, n_records ascending first-base indices
 *   each (equal neighbours are empty records; the last record runs to
 *   n_bases).  Neither input is modified.
 *   d_codes (16-byte aligned, room for n_bases1 + n_bases2 + 64 bytes) takes
 *   the n_bases1 + n_bases2 codes, every byte copied verbatim (bit 3 and a
 *   quality mask survive), then 64 pad bytes of value 4.  d_rec_seq takes
 *   2 * n_records ascending entries: entry 2i is the first base of mate 1 of
 *   pair i, entry 2i + 1 of its mate 2; an empty mate stays an empty record.
 *   Bases before d_rec_seq1[0] or d_rec_seq2[0] belong to no record, as
 *   everywhere: their places, at the front of d_codes, are written as 4.
 *   n_records == 0 or no bases at all: only the pad is written (at d_codes;
 *   with records and no bases d_rec_seq is all zeros).
 *   A NULL d_codes, a NULL table with n_records > 0, NULL codes with bases, a
 *   misaligned code buffer, more than 2^31 pairs: KMAN_EINVAL, nothing is
 *   written.  A table that is not ascending or points past n_bases gives wrong
 *   bytes, never a wild address or an endless loop: entries are clamped, a
 *   source byte is read only below its n_bases, an output byte is written only
 *   below n_bases1 + n_bases2 + 64, every search runs a step count fixed
 *   before it starts.
 *   The tables are the exclusive scans of the records' lengths already, so the
 *   output offsets are sums of their entries: one thread per pair writes two.
 *   The copy pass runs one block per KMAN_ZIP_TILE output bytes: the block
 *   finds its slice of d_rec_seq by a block-wide search, stages it in LDS when
 *   it has at most KMAN_ZIP_SEG_CAP segments and searches global memory
 *   otherwise; an output word is one aligned 16-byte store, put together from
 *   aligned 16-byte loads of the source of each mate that has bytes in it.
 *   Every byte of d_codes has one writer.  n_bases1 + n_bases2 bytes are read
 *   and as many written, 16 B of table per pair read and 16 B written.
 *   Launches are timed under the tag "zip".  Synchronises. */
#define KMAN_ZIP_TILE 16384
#define KMAN_ZIP_SEG_CAP 1024
int kman_zip_records(kman_ctx *ctx, const uint8_t *d_codes1, uint64_t n_bases1, const uint64_t *d_rec_seq1,
                     const uint8_t *d_codes2, uint64_t n_bases2, const uint64_t *d_rec_seq2, uint64_t n_records,
                     uint8_t *d_codes, uint64_t *d_rec_seq);

/* ------------------------------------------------ homopolymer-compressed codes
 * Not in the reference: every run of one base collapsed to its first base
 * before k-mers are taken (`--hpc`; minimap2 -H, meryl compress), a segmented
 * stream compaction over one byte per base.
 *
 * kman_hpc_records: d_codes, n_bases: codes as the parsers write them (bits
 *   0-1 the base, bit 2 not-ACGT, bit 3 a record's first character; 16-byte
 *   aligned).  Base i is DROPPED exactly when i > 0, bits 2 and 3 of code[i]
 *   are clear and (code[i - 1] & 7) == (code[i] & 7); every other byte is kept
 *   verbatim.  So a record's first base is always kept and no run crosses a
 *   record boundary, N and other not-ACGT characters are never dropped, a base
 *   masked by -q separates the bases on its two sides, and bases before
 *   d_rec_seq[0] follow the same rule.
 *   d_rec_seq: n_records ascending first-base indices (entries are clamped to
 *   n_bases).  d_out_codes (16-byte aligned, room for n_bases + 64 bytes; not
 *   d_codes, nor overlapping it): the kept codes in order, then 64 bytes of
 *   value 4.  d_out_rec_seq[r]: the kept bases with an original index <
 *   d_rec_seq[r] (empty records stay empty records).  d_orig (may be NULL;
 *   room for n_bases u64): the original index of kept base j.  *n_out: the
 *   kept bases.  n_bases == 0: only the pad is written, the table is zeros.
 *   A NULL or misaligned buffer, or d_out_codes over d_codes: KMAN_EINVAL,
 *   nothing written.  A table that is not ascending gives wrong numbers,
 *   never a wild address nor an unbounded loop: every record is looked up on
 *   its own, in a fixed number of steps.
 *   One block per KMAN_HPC_TILE input bytes: 16-byte loads, the predecessor
 *   of a wave's first byte read from d_codes, keep flags by byte-parallel
 *   arithmetic, ranks by one packed DPP wave scan, the tile's offset from the
 *   decoupled look-back; the kept bytes are staged in LDS at the output's
 *   alignment and stored as aligned 16-byte words (the words that two tiles
 *   share byte by byte: every output byte has one writer).  A second kernel,
 *   one thread per record, adds the kept bytes between the record's
 *   KMAN_HPC_GROUP-byte boundary (whose prefix the first kernel noted) and its
 *   first base.  n_bases bytes are read and *n_out written, 8 B per kept base
 *   more with d_orig, 8 B per KMAN_HPC_GROUP input bytes of prefixes.
 *   Launches are timed under the tag "hpc".  Synchronises. */
#define KMAN_HPC_TILE 8192
#define KMAN_HPC_GROUP 256
int kman_hpc_records(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, const uint64_t *d_rec_seq,
                     uint64_t n_records, uint8_t *d_out_codes, uint64_t *d_out_rec_seq, uint64_t *d_orig,
                     uint64_t *n_out);

/* kman_rebase_pos: uniq pos tagged with their source shard (bits 56-63) ->
 *   global pos: (pos & (2^56 - 1)) + (offsets[source] << 1), offsets = the
 *   global base index of each shard's first base (host array, nsrc <= 256).
 * kman_synth_fasta: bytes [byte_lo, byte_lo + n_bytes) of the synthetic
 *   benchmark FASTA into d_out (16-byte aligned): records r = 0.. with header
 *   ">syn<r>\n" at byte rec_tab[3r], first base index rec_tab[3r + 1] and
 *   rec_tab[3r + 2] bases in lines of `line` bases + "\n"; base i of the file
 *   = "ACGT"[splitmix64(seed * 0xD1B54A32D192ED03 + i) >> 62] (the same
 *   generator as tests/golden/inputs.py synth_np). */
int kman_rebase_pos(kman_ctx *ctx, uint64_t *d_pos, uint64_t n, const uint64_t *offsets, uint32_t nsrc);
int kman_synth_fasta(kman_ctx *ctx, uint8_t *d_out, uint64_t byte_lo, uint64_t n_bytes, uint64_t seed,
                     const uint64_t *rec_tab, uint32_t n_records, uint32_t line);

/* ------------------------------------------------------------- formatting
 * Host-side writers that produce the reference's exact bytes.  They run on
 * host threads over host copies of the device results.
 *   names      concatenated record names, name r at names[name_off[r] .. name_off[r+1])
 *   rec_seq    host copy of d_rec_seq (sorted ascending)
 * Each returns the number of bytes written to out (<= cap) in *used, or
 * KMAN_ECAP with the required size in *used. */
int kman_format_count(const uint64_t *ukeys, const void *counts, uint32_t count_bytes, uint64_t n,
                      uint32_t k, char *out, size_t cap, size_t *used, int threads);
int kman_format_uniq(const uint64_t *keys, const void *pos, uint32_t pos_bytes, uint64_t n,
                     uint32_t k, const char *names, const uint64_t *name_off,
                     const uint64_t *rec_seq, uint64_t n_records, char *out, size_t cap,
                     size_t *used, int threads);

/* uniq rows of a multi-source join (several FASTA inputs and reloaded batch
 * files, join.py:63-93 + 244-263): pos are u64 global base indices over one
 * merged record table; rec_kind[r] 0 = a FASTA record (header
 * name:start-end:strand), 1 = a batch-file record printed by its title. */
int kman_format_uniq_mixed(const uint64_t *keys, const uint64_t *pos, uint64_t n, uint32_t k, const char *names,
                           const uint64_t *name_off, const uint64_t *rec_seq, const uint8_t *rec_kind,
                           uint64_t n_records, char *out, size_t cap, size_t *used, int threads);
int kman_format_count_wide(const uint64_t *hi, const uint64_t *lo, const void *counts, uint32_t count_bytes,
                           uint64_t n, uint32_t k, char *out, size_t cap, size_t *used, int threads);
/* any k >= 2 over W word planes (kman_extract_words layout, row i's word j at
 * words[j * stride + i]) */
int kman_format_count_words(const uint64_t *words, uint64_t stride, const void *counts, uint32_t count_bytes,
                            uint64_t n, uint32_t k, char *out, size_t cap, size_t *used, int threads);
int kman_format_uniq_words(const uint64_t *words, uint64_t stride, const void *pos, uint32_t pos_bytes, uint64_t n,
                           uint32_t k, const char *names, const uint64_t *name_off, const uint64_t *rec_seq,
                           uint64_t n_records, char *out, size_t cap, size_t *used, int threads);
int kman_format_uniq_mixed_words(const uint64_t *words, uint64_t stride, const uint64_t *pos, uint64_t n, uint32_t k,
                                 const char *names, const uint64_t *name_off, const uint64_t *rec_seq,
                                 const uint8_t *rec_kind, uint64_t n_records, char *out, size_t cap, size_t *used,
                                 int threads);
int kman_format_uniq_wide(const uint64_t *hi, const uint64_t *lo, const void *pos, uint32_t pos_bytes, uint64_t n,
                          uint32_t k, const char *names, const uint64_t *name_off, const uint64_t *rec_seq,
                          uint64_t n_records, char *out, size_t cap, size_t *used, int threads);

/* kman_screen_records' three planes (out3: windows, hits, count sum, n_records
 * u64 each) as text, one "%s\t%llu\t%llu\t%llu\n" line (name, windows, hits,
 * sum) per record r with keep[r] != 0 (keep == NULL: every record), in input
 * order. */
int kman_format_screen(const uint64_t *out3, uint64_t n_records, const uint8_t *keep, const char *names,
                       const uint64_t *name_off, char *buf, size_t cap, size_t *used, int threads);
/* The same with a fifth column: "%s\t%llu\t%llu\t%llu\t%u\n" (name, windows,
 * hits, sum, median[r]: kman_record_quantile's word of the record). */
int kman_format_screen_median(const uint64_t *out3, const uint32_t *median, uint64_t n_records, const uint8_t *keep,
                              const char *names, const uint64_t *name_off, char *buf, size_t cap, size_t *used,
                              int threads);
/* The same with the record's solid span as two last columns (`kmer screen
 * --solid`): "%s\t%llu\t%llu\t%llu[\t%u]\t%llu\t%llu\n" (name, windows, hits,
 * sum, median[r] unless median == NULL, start[r], end[r]). */
int kman_format_screen_solid(const uint64_t *out3, const uint32_t *median, const uint64_t *start, const uint64_t *end,
                             uint64_t n_records, const uint8_t *keep, const char *names, const uint64_t *name_off,
                             char *buf, size_t cap, size_t *used, int threads);
/* A pair's line (`kmer screen --mate --solid`): out3 and median hold one row
 * per pair (kman_screen_records and kman_record_quantile with every second
 * entry of kman_zip_records' table), start and end one row per mate, 2 *
 * n_pairs each (kman_record_runs with every entry):
 * "%s\t%llu\t%llu\t%llu[\t%u]\t%llu\t%llu\t%llu\t%llu\n" (name, windows, hits,
 * sum, median[r] unless median == NULL, start[2r], end[2r], start[2r + 1],
 * end[2r + 1]); names are the pairs'. */
int kman_format_screen_pair(const uint64_t *out3, const uint32_t *median, const uint64_t *start, const uint64_t *end,
                            uint64_t n_pairs, const uint8_t *keep, const char *names, const uint64_t *name_off,
                            char *buf, size_t cap, size_t *used, int threads);
/* kman_format_screen_solid's lines with the record's corrected bases as one
 * last column (`kmer screen --solid C --correct`):
 * "%s\t%llu\t%llu\t%llu[\t%u]\t%llu\t%llu\t%u\n" (.., start[r], end[r],
 * fixes[r]: kman_apply_fixes' word of the record). */
int kman_format_screen_correct(const uint64_t *out3, const uint32_t *median, const uint64_t *start,
                               const uint64_t *end, const uint32_t *fixes, uint64_t n_records, const uint8_t *keep,
                               const char *names, const uint64_t *name_off, char *buf, size_t cap, size_t *used,
                               int threads);
/* BED lines "%s\t%llu\t%llu\n" (name, start[r], end[r]) for every record r
 * with keep[r] != 0 (keep == NULL: every record) and end[r] > start[r], in
 * input order. */
int kman_format_bed(const uint64_t *start, const uint64_t *end, uint64_t n_records, const uint8_t *keep,
                    const char *names, const uint64_t *name_off, char *buf, size_t cap, size_t *used, int threads);
/* `kmer classify` lines, one "%s\t%u\t%s\t%u\t%u\n" (name, windows[r], LABEL,
 * hits[r], second[r]) per record r with keep[r] != 0 (keep == NULL: every
 * record), in input order.  LABEL: label assign[r] (labels / label_off as
 * names / name_off, n_colors of them) when assign[r] >= 0, "?" when it is -2
 * (ambiguous), "-" for any other negative value (unassigned); an assign[r] >=
 * n_colors is KMAN_EINVAL.  planes != NULL (n_colors planes of n_records u32,
 * kman_classify_records' d_out without its first plane) appends one "\t%u"
 * column per colour, in colour order.  n_colors in
 * 1..KMAN_CLASSIFY_MAX_COLORS. */
int kman_format_classify(const uint32_t *windows, const int32_t *assign, const uint32_t *hits, const uint32_t *second,
                         const uint32_t *planes, uint32_t n_colors, uint64_t n_records, const uint8_t *keep,
                         const char *labels, const uint64_t *label_off, const char *names, const uint64_t *name_off,
                         char *buf, size_t cap, size_t *used, int threads);

/* The same writers on the device: the output text is built in
 * HBM (d_out, 16-byte aligned) from device-resident results, so only the text
 * crosses PCIe.  Byte-identical to kman_format_count / kman_format_uniq.
 * *used = the text size; KMAN_ECAP when it exceeds cap (nothing past cap is
 * written; d_out = NULL sizes only).  The rows are independent: a slice of
 * the result arrays formats to the matching slice of the text. */
int kman_format_count_dev(kman_ctx *ctx, const uint64_t *d_ukeys, const void *d_counts, uint32_t count_bytes,
                          uint64_t n, uint32_t k, char *d_out, size_t cap, size_t *used);
int kman_format_uniq_dev(kman_ctx *ctx, const uint64_t *d_keys, const void *d_pos, uint32_t pos_bytes, uint64_t n,
                         uint32_t k, const char *d_names, const uint64_t *d_name_off, const uint64_t *d_rec_seq,
                         uint64_t n_records, char *d_out, size_t cap, size_t *used);
/* k in 33..64: the same writers over word-pair keys (kman_extract_wide). */
int kman_format_count_wide_dev(kman_ctx *ctx, const uint64_t *d_hi, const uint64_t *d_lo, const void *d_counts,
                               uint32_t count_bytes, uint64_t n, uint32_t k, char *d_out, size_t cap, size_t *used);
int kman_format_uniq_wide_dev(kman_ctx *ctx, const uint64_t *d_hi, const uint64_t *d_lo, const void *d_pos,
                              uint32_t pos_bytes, uint64_t n, uint32_t k, const char *d_names,
                              const uint64_t *d_name_off, const uint64_t *d_rec_seq, uint64_t n_records, char *d_out,
                              size_t cap, size_t *used);

/* any k >= 2: the device writers over W word planes */
int kman_format_count_words_dev(kman_ctx *ctx, const uint64_t *d_words, uint64_t stride, const void *d_counts,
                                uint32_t count_bytes, uint64_t n, uint32_t k, char *d_out, size_t cap, size_t *used);
int kman_format_uniq_words_dev(kman_ctx *ctx, const uint64_t *d_words, uint64_t stride, const void *d_pos,
                               uint32_t pos_bytes, uint64_t n, uint32_t k, const char *d_names,
                               const uint64_t *d_name_off, const uint64_t *d_rec_seq, uint64_t n_records,
                               char *d_out, size_t cap, size_t *used);

#ifdef __cplusplus
}
#endif
#endif /* KMAN_H */

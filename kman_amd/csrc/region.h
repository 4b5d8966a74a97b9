// region.h — the region path: `kmer count` / `kmer uniq` of one FASTA stream in three
// kernels, through padded regions of packed items (kman_groups).
//
// Replaces, for one device-resident batch stream, the whole chain
//   Sequence.yield_kmers (kmermaid/seq.py:285-328) -> Batch.sorted
//   (batch.py:156-168, forced by batcher.py:392) -> Crawler.do_records /
//   do_batch (join.py:63-130) -> join_sequence_count / join_unique
//   (join.py:244-285)
// for the inputs whose shape allows it (uniform-ish prefix distribution, k <=
// 25; anything else returns KMAN_EFALLBACK and the caller runs
// kman_extract_sorted + kman_finish, which handle every input).
//
// MSD instead of the LSD prefix passes of sort.hip:
//   pass 0 (rg_extract)  rolls the windows of a tile and scatters them by the
//                        top 8 key bits b into region (b, s) of capacity C0,
//                        s = one of RS position segments (own look-back
//                        chains).  b is implied by the region from here on, so
//                        an item is ONE u64: (key minus its top 8 bits) << Q |
//                        window index (Q bits; Q = 0 in count mode).
//   pass 1 (rg_pass)     per bucket b (its own chain over the regions (b, *)):
//                        scatter by the next B2 key bits d into region
//                        r = (b << B2 | d) of capacity C1 <= FCAP.
//   finish (rg_finish)   one 512-thread block per region r: load it (<= FCAP
//                        items, 68 KiB of LDS), LSD-sort the remaining key
//                        bits in LDS, run-length pass, emit (key, count) or the
//                        keys that occur once with their pos, compacted by one
//                        look-back over the regions in key order.
// No digit histogram is computed before any pass: every region has a fixed
// capacity (1.5x its expected fill), the passes publish their final region
// counts themselves, and a region that would overflow raises a device flag
// (nothing is written past a capacity) that turns the call into
// KMAN_EFALLBACK.  Algorithmic HBM bytes per k-mer: 1 code read + 8 (pass 0)
// + 16 (pass 1) + 8 (finish read) + the output, against 13 + 2 x 24 + 12 for
// the LSD pipeline of the same workload.
//
// The stages, one translation unit each; a kernel template is defined and
// instantiated in its stage's file only, and the other files reach it through
// the plain functions declared at the end of this header:
//   region_extract.hip  rg_extract, rg_hist and their launchers
//   region_pass.hip     rg_pass, rg_merge_regions
//   region_finish.hip   rg_finish, its launch ladder and stamp report
//   region_groups.hip   make_plan and the kman_groups* entry points
//   region_rounds.hip   the multi-GPU key rounds (kman_dshard_*, kman_dround_*)
#pragma once
#include "common.h"

namespace kman::region {

constexpr int RT = 512;           // threads of passes 0 and 1
constexpr int RS = 64;            // position segments of pass 0 (one wave of counts)
constexpr int FCAP = 8704;        // finish capacity: 68 KiB of 8-byte items
constexpr uint32_t ERR_REGION = 1u << 8;  // a region would overflow (not an engine fault)
// the uniq finish's early row count was not its rows', or a singleton mark
// not the row its sorted keys give: raised by the checked kernels
// (KMAN_RG_CHECK) only -- the plain kernel's rows ARE the marked items and
// their count (its compacting last pass), so it has nothing to compare
constexpr uint32_t ERR_EARLY = 1u << 9;
constexpr uint32_t B1 = 8;        // pass-0 digit: top 8 key bits
// kman_groups' pass-0 bits.  (9, with 9 more in pass 1, leaves regions of ~3.8
// K items per 1 G k-mers that a GCAP finish holds in 40 KiB -- three blocks
// per CU -- but the finish's per-region costs dominate there: 5.96 vs 5.62
// ms, and the 512-bucket pass 0 4.0 vs 3.6 ms)
// (Round 5, with the cursor adds cheap: 9 + 8 bits measured equal to 8 + 9,
// `r05xy_pass_geometry_ab.txt`)
constexpr uint32_t G1 = 8;
// finish capacities (items): FCAP (68 KiB of 8-byte items, two blocks per
// CU) and GCAP (40 KiB, three blocks per CU) for the round path's small
// regions (a pass 1b over many ranks' items leaves ~4 K per region)
constexpr int GCAP = 5120;
// expected region fills the plans aim at (<= T) and accept (<= M): M keeps
// > 10 sd of a uniform fill below the capacity
constexpr uint64_t FFILL_T = 6144, FFILL_M = 7800;

// phase stamps (s_memrealtime, 100 MHz) per tile, thread 0, into `stp`: only
// in diagnostic builds (make EXTRA=-DKMAN_RG_STAMPS OUT=../lib_stamps,
// tools/regionstamps.py); `stp` is null otherwise
#ifdef KMAN_RG_STAMPS
#define RSTAMP(id, i)                                                                                 \
    do {                                                                                              \
        if (stp && threadIdx.x == 0) stp[(uint64_t)(id) * 16 + (i)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#else
#define RSTAMP(id, i) \
    do {              \
        (void)stp;    \
    } while (0)
#endif

struct RegionPlan {
    uint32_t K, Q, B2, rest;
    bool rc;
    uint64_t W;          // windows (x2 with rc): bound on the k-mers
    bool canon;          // canonical keys (KMAN_CANONICAL)
    bool mix;            // canonical keys through mix_key (KMAN_MIXED: spectra)
    uint64_t C0, C1;     // region capacities (items)
    uint32_t H;          // pass-1 chains (sub-regions) per bucket
    uint64_t C1h;        // pass-1 sub-region capacity
    uint32_t n_tiles0, seg_tiles, maxt1;
    uint32_t ei;         // windows per thread of pass 0
    uint64_t off_r1, off_c0, off_c1, off_lim, bytes;
};

inline uint32_t bitlen(uint64_t x) { return x ? 64u - (uint32_t)__builtin_clzll(x) : 0u; }

// The input of a digit pass: nbk buckets, each the concatenation of nsg <= 64
// segments (bucket bk, segment s: seg_cnt[bk * nsg + s] items at seg_base[..],
// or at (bk * nsg + s) * stride when seg_base is null).  Digit = item bits
// [shift, shift + bits), bits <= 9.  Output region of digit d: ((bk / gsub)
// << bits | d) * gsub + bk % gsub (gsub > 1 keeps the sub-buckets' outputs
// apart, as sub-regions of one region), split into H sub-regions (one per
// chain of the bucket) of capacity C1.  With tag, bits [tag_shift, tag_shift +
// tag_bits) of each item are replaced by its segment index / tag_div as it is
// loaded (the source rank on N > 1).
struct PassArgs {
    const void *in;  // items of TI (rg_pass's template): 8 bytes, or 4 (narrow count items)
    const uint64_t *seg_base;
    const uint32_t *seg_cnt;
    uint32_t cnt_sb;  // seg_cnt indexed [segment][bucket] (pass 0's cursors), else [bucket][segment]
    uint64_t stride;
    uint32_t nbk, nsg, gsub, maxt;
    uint32_t H;        // chains (parts) per bucket: outputs are H sub-regions per region
    uint32_t tag_div;  // tag = segment index / tag_div
    uint32_t shift, bits;
    uint32_t tag, tag_shift, tag_bits;
    void *out;  // items of TO
    uint64_t C1;
    uint32_t *cnt1;
    // optional: a sub-region that overflows C1 flags the finish regions
    // [(sub / fail_div) << fail_shift, +2^fail_shift) in fail[] (the round
    // path then leaves them out and redoes only their keys)
    uint8_t *fail;
    uint32_t fail_div, fail_shift;
    uint32_t big;  // a pass of <= 8 bits on the 1024-thread instance anyway (8192-item tiles: 256-byte digit runs)
    // 8-byte items on that instance without a staged tile, through 256-byte
    // lines (rg_pass<..., LN = true>; kman_groups); line1 (KMAN_PASS_LINE1, for
    // tests): one line per digit at any digit width, so that small inputs take
    // many placement rounds per tile
    uint32_t lines, line1;
    // optional (pass 1 of a key round, rg_pass<..., HV = true): the heavy
    // keys of the round, per bucket j of the round an open-addressing table
    // of HV_BSLOTS key rests (the item's key bits, item >> hv_q; HV_EMPTY
    // where free) at hv_tab[j * HV_BSLOTS], copied to LDS when a chain of
    // the bucket starts (a bucket holds <= HV_BMAX of them).  An item whose
    // key rest is in it is counted per slot in LDS; count mode keeps the
    // chain's first copy (hv_keep = 1) and drops the rest, uniq mode drops
    // every copy (a heavy key occurs more than once: no uniq row); the chain's
    // dropped copies go to hv_drop[hv_idx[j * HV_BSLOTS + slot]] when it ends
    const uint64_t *hv_tab;
    const uint32_t *hv_idx;
    uint64_t *hv_drop;
    uint32_t hv_q, hv_keep;
};

// heavy keys of a key round (kman_dround_finish): found by sampling the
// received items, counted apart in pass 1 so that a satellite or repeat-family
// k-mer with 10^5 copies does not overflow its regions (and send the key range
// through the partial redo)
constexpr uint32_t HV_BSLOTS = 1024, HV_BMAX = 256, HV_MAX = 1u << 16;
constexpr uint64_t HV_EMPTY = ~0ull;
constexpr uint32_t HV_FBITS = 1u << 16;
__host__ __device__ inline uint32_t hv_fbit(uint64_t rest) { return ((uint32_t)rest * 0x85EBCA6Bu) >> 16; }
__host__ __device__ inline uint32_t hv_slot(uint64_t rest) {
    return (((uint32_t)rest ^ (uint32_t)(rest >> 29)) * 0x9E3779B1u) >> 22;  // (one 32-bit multiply)
}
// the heavy-key scratch (kman_ctx::d_hv): what outlives find_heavy
constexpr size_t HVO_TAB = 0, HVO_IDX = HVO_TAB + 256 * HV_BSLOTS * 8, HVO_KEYS = HVO_IDX + 256 * HV_BSLOTS * 4,
                 HVO_DROP = HVO_KEYS + HV_MAX * 8, HVO_END = HVO_DROP + HV_MAX * 8;

struct FinishArgs {
    const uint64_t *in;
    uint64_t C1;
    const uint32_t *cnt;
    uint32_t Q, rest, rc;
    uint64_t rbase;
    uint32_t tag_shift;
    uint32_t nreg;
    uint32_t fsub = 1;  // sub-regions per region (cnt and in indexed per sub-region)
    uint8_t *freg = nullptr;  // per-region overflow flags (the round path), else null
    int cap = FCAP;  // the finish's region capacity: FCAP (kman_groups) or GCAP / FCAP chosen by the round plan
    bool in4 = false;  // 4-byte items (the pass wrote them narrow: only with the narrow finish, narrow_ok)
};

// ---- region_extract.hip
// pass 0 of kman_groups over the whole stream (n_launch = 0) or over the next
// n_launch tiles
void launch_extract_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                        uint64_t *r0, uint32_t *c0, uint32_t epoch, uint32_t *counter, uint64_t *stp,
                        uint32_t n_launch = 0);
// the shard's exact (bucket, segment) counts, and pass 0 of a key round into
// the regions of rtab (kman_dshard_hist / kman_dshard_extract)
void launch_hist_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                     uint32_t *hist);
void launch_extract_ex_any(kman_ctx *ctx, const RegionPlan &p, const uint8_t *codes, uint64_t n_bases, uint32_t k,
                           uint64_t *out, const uint32_t *cnt, const uint64_t *rtab, uint32_t epoch);
// ---- region_pass.hip
// in4 / out4: the pass reads / writes 4-byte items (out4 only when every key
// bit below the digit fits 32 bits: pa.shift <= 32, and no tag); pa.bits >= 1
int launch_pass(kman_ctx *ctx, const PassArgs &pa, uint32_t *counter, uint64_t *stp, bool in4 = false,
                bool out4 = false);
// pass 1b with 0 bits (rg_merge_regions): region r takes its nsg sub-regions
// one after another; narrow: 4-byte items in and out
int launch_merge_regions(kman_ctx *ctx, bool narrow, const void *in, uint64_t C1s, const uint32_t *c1, uint32_t nsg,
                         uint32_t H, void *out, uint64_t C1, uint32_t *c2, uint8_t *freg, uint32_t nreg, uint32_t tag,
                         uint32_t tag_shift);
// ---- region_finish.hip
bool narrow_ok(const kman_ctx *ctx, int mode, uint32_t Q, uint32_t rest, uint32_t tag_shift);
int run_finish(kman_ctx *ctx, const FinishArgs &f, int mode, uint64_t *okeys, void *ovals, uint32_t oval_bytes,
               uint64_t *stp);
int report_finish_stamps(kman_ctx *ctx, uint64_t *st, uint64_t nreg);
// ---- region_groups.hip
int region_fault(kman_ctx *ctx, uint32_t e, const char *what);

}  // namespace kman::region

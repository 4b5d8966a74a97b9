// region_rounds.hip — the region path (region.h) at N > 1:
// the region path across G ranks, in key rounds (one process per GPU;
// kman_amd/dist.py drives the collectives between the calls).  Each rank holds
// one byte-range shard of the FASTA (codes + a (k-1)-base halo):
//   kman_dshard_hist     exact item counts per (top-8-bit bucket b, position
//                        segment s) of the shard, in rg_extract's tile geometry
//   (host)               all-gather of the per-bucket counts; the 256 buckets
//                        cut into G x R contiguous parts of ~equal k-mers:
//                        rank q owns parts q*R .. q*R+R-1, round r handles part
//                        q*R + r of every rank q, so a rank's rounds produce
//                        its key range in order and the ranks' outputs in
//                        rank order are the global output
//   per round r:
//   kman_dshard_extract  pass 0 of the shard over the round's buckets only,
//                        written straight into the send buffer: region (b, s)
//                        at rtab[b * RS + s] (exact, destination-major, so no
//                        gather pass and no padding)
//   (host)               one all-to-all of the packed items (RCCL, xGMI)
//   kman_dround_finish   per (bucket, source) chain: pass 1 by 9 bits into
//                        sub-regions (b, d, src, h); pass 1b per (b, d) by g
//                        more bits (g >= ceil(log2 G), more when the round's
//                        buckets are large), tagging each item with its source
//                        rank in the now implied d field; then the LDS finish,
//                        appending the round's rows to the rank's output.
// Uniq pos carry the source rank in bits 56-63.  The round working set is
// two arenas: A = the send buffer, then pass-1 sub-regions; B = the receive
// buffer, then pass-1b regions (the receive buffer is dead after pass 1).
#include "region.h"
#include "onesweep.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace kman::region;

namespace {

// KMAN_RG_VERBOSE: synchronise after each pass of kman_dgroups_finish and
// report which one raised a region overflow (diagnostics only)
int rg_check(kman_ctx *ctx, const char *what, const uint32_t *cnt = nullptr, uint64_t n = 0) {
    static const bool verbose = getenv("KMAN_RG_VERBOSE") != nullptr;
    if (!verbose) return KMAN_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t e = 0;
    HIP_TRY(ctx, hipMemcpy(&e, ctx->d_err, 4, hipMemcpyDeviceToHost));
    uint64_t mx = 0, sum = 0, nz = 0;
    if (cnt && n) {
        std::vector<uint32_t> h(n);
        HIP_TRY(ctx, hipMemcpy(h.data(), cnt, n * 4, hipMemcpyDeviceToHost));
        for (uint32_t v : h) {
            mx = v > mx ? v : mx;
            sum += v;
            nz += v != 0;
        }
        // nonzero counts per block of n/16 entries
        fprintf(stderr, "  nonzero per 1/16:");
        for (int q = 0; q < 16; q++) {
            uint64_t z = 0;
            for (uint64_t i = q * n / 16; i < (q + 1) * n / 16; i++) z += h[i] != 0;
            fprintf(stderr, " %llu", (unsigned long long)z);
        }
        fprintf(stderr, "\n  first 8:");
        for (int q = 0; q < 8 && q < (int)n; q++) fprintf(stderr, " %u", h[q]);
        fprintf(stderr, "\n");
    }
    fprintf(stderr, "kman_dgroups: after %s err=%u counts n=%llu nonzero=%llu sum=%llu max=%llu\n", what, e,
            (unsigned long long)n, (unsigned long long)nz, (unsigned long long)sum, (unsigned long long)mx);
    return KMAN_OK;
}

// the shard's pass-0 geometry (rg_extract / rg_hist): no capacity limits,
// no region area (the exact layout needs none); Q from the common bound
int make_shard_plan(uint64_t n_bases, uint64_t n_bases_q, uint32_t k, uint32_t flags, int mode, RegionPlan *pl) {
    if (mode != KMAN_FINISH_COUNT && mode != KMAN_FINISH_UNIQ) return KMAN_EINVAL;
    if (k < 2 || k > 32 || n_bases_q < n_bases) return KMAN_EINVAL;
    if (getenv("KMAN_NO_REGION")) return KMAN_EFALLBACK;
    if (mode == KMAN_FINISH_UNIQ && k > 25) return KMAN_EFALLBACK;  // (the tile-local window index above the key)
    RegionPlan p{};
    p.canon = flags & KMAN_CANONICAL;
    p.mix = p.canon && (flags & KMAN_MIXED);
    p.rc = (flags & KMAN_RC) && !p.canon;
    p.K = 2 * k;
    if (p.K < B1 + 9 + 1) return KMAN_EFALLBACK;  // (the rounds' passes need 8 + 9 key bits and one more)
    p.W = n_bases * (p.rc ? 2 : 1);
    const uint64_t Wq = n_bases_q * (p.rc ? 2 : 1);
    p.Q = mode == KMAN_FINISH_UNIQ ? (bitlen(Wq - 1) ? bitlen(Wq - 1) : 1u) : 0u;
    if (p.K - B1 + p.Q > 64) return KMAN_EFALLBACK;
    // the shard extraction's tiles (rg_hist counts in the same geometry): 16
    // windows per thread (8 with -r) for shards that one key round takes
    // (1 GB per rank: 2.80-2.88 vs 3.05-3.45 ms with 12), 12 (6) for the big
    // ones, whose rounds keep 1/R of the windows each (config 4's 12.5 GB:
    // 63.8-64.2 vs 71.8-72.2 ms with 16, `r04aj_tiles_ab.txt`); decided on
    // the common bound, so every rank takes the same
    // (KMAN_ONCE: every window of the shard is kept by one extraction for all
    // rounds, so the 16-window tiles as well)
    const bool wide = n_bases_q <= (4ull << 30) || (flags & KMAN_ONCE);
    p.ei = p.rc ? (wide ? 8u : 6u) : (wide ? 16u : 12u);
    const uint64_t win = (uint64_t)RT * p.ei;
    p.n_tiles0 = (uint32_t)ceil_div(n_bases ? n_bases : 1, win);
    p.seg_tiles = (uint32_t)ceil_div(p.n_tiles0, RS);
    *pl = p;
    return KMAN_OK;
}

struct RoundPlan {
    uint32_t K, Q, g, rest, G, nb;
    uint32_t H;           // pass-1 chains per (bucket, source)
    bool p1b;             // pass 1b runs (by g >= 0 bits); else the finish reads pass 1's sub-regions
    bool rc;
    uint64_t C1s, C1;     // pass-1 sub-region / pass-1b region capacities
    int cap;              // the finish's capacity: GCAP when the planned regions fit it (three blocks per CU)
    uint64_t nsub, nreg;
    // arena A: r1 | c1 | pass-1 segment bases (u64) + counts (u32) | region
    // overflow flags (u8); arena B: r2 | c2
    uint64_t off_c1, off_tab, off_fail, a_bytes, off_c2, b_bytes;
};

// Capacity of a region that expects e items: e + max(e / 8, 8 sd of a
// Poisson fill) -- the round path's arenas are most of a rank's HBM, and at
// config 4's size (12.5 G k-mers per rank) a 1.5 x slack cost one key round (a
// re-read and re-roll of the whole shard).  A region that overflows anyway (a
// repeat) is redone by key range.
uint64_t round_cap(uint64_t e, uint64_t extra) {
    const uint64_t sd8 = (uint64_t)(8.0 * sqrt((double)e)) + 1;
    return ceil_div(e + (e / 8 > sd8 ? e / 8 : sd8) + extra, 64) * 64;
}

// counts[src * nb + j] = items of bucket b_lo + j from rank src
int make_rplan(uint32_t k, uint32_t flags, int mode, uint32_t world, uint64_t n_bases_q, uint32_t nb,
               const uint64_t *counts, RoundPlan *rp) {
    if (mode != KMAN_FINISH_COUNT && mode != KMAN_FINISH_UNIQ) return KMAN_EINVAL;
    if (k < 2 || k > 32 || world < 1 || world > 32 || nb > (uint32_t)RADIX) return KMAN_EINVAL;
    if (nb && !counts) return KMAN_EINVAL;
    RoundPlan d{};
    const bool canon = flags & KMAN_CANONICAL;
    d.rc = (flags & KMAN_RC) && !canon;
    d.K = 2 * k;
    d.G = world;
    d.nb = nb;
    const uint64_t Wq = n_bases_q * (d.rc ? 2 : 1);
    d.Q = mode == KMAN_FINISH_UNIQ ? (bitlen(Wq - 1) ? bitlen(Wq - 1) : 1u) : 0u;
    if (d.K - B1 + d.Q > 64) return KMAN_EFALLBACK;
    uint64_t maxsb = 0, maxb = 0;  // largest (bucket, source) chunk, largest bucket
    for (uint32_t j = 0; j < nb; j++) {
        uint64_t t = 0;
        for (uint32_t src = 0; src < world; src++) {
            const uint64_t c = counts[(uint64_t)src * nb + j];
            if (c > 0xffffffffull) return KMAN_EFALLBACK;  // (pass-1 chain lengths are u32)
            maxsb = c > maxsb ? c : maxsb;
            t += c;
        }
        maxb = t > maxb ? t : maxb;
    }
    // pass 1: H block-owned chains per (bucket, source), enough chains to
    // fill the CUs (a round of few buckets on few ranks has few chains);
    // pass 1b concatenates the G * H sub-regions of a (b, d): at most 64
    // H: the fewest chains with the shortest makespan on the 256 CUs (one
    // 1024-thread pass block each): ceil(nb G H / 256) / H bucket-chunks per
    // CU -- 85 buckets take H = 3 (255 chains), not 4 (340: a second wave of
    // 84 chains on 84 CUs, pass 1 19.7 vs 10.1 ms per config-4 round)
    {
        const uint64_t ch1 = (uint64_t)nb * world;
        d.H = 2;
        double best = 1e30;
        for (uint32_t h = 2; h <= 16 && world * h <= 64; h++) {
            const double ms = (double)ceil_div(ch1 * h, 256) / h;
            if (ms < best * 0.95) {  // (more chains only for a clear gain)
                best = ms;
                d.H = h;
            }
        }
    }
    // pass 1b bits g: until a final region expects <= FFILL_T items (the
    // LDS finish holds FCAP = 8704).  g = 0 (no pass 1b, the finish reads the
    // pass-1 sub-regions) when one rank's 9-bit regions already fit: with one
    // source and two chains (N > 1 needs pass 1b anyway, to tag each item with
    // its source rank for uniq and to merge the ranks' sub-regions)
    // Pass 1b runs whenever the finish cannot read the pass-1 sub-regions
    // itself (more than two per region: N > 1, or H > 2) -- with g = 0 bits
    // (a pass that only merges the sources' sub-regions and tags uniq items
    // with their rank) while a (b, d) region's expected fill is <= FFILL_M,
    // as kman_groups keeps its 17-bit regions: N > 1 at 1 G k-mers per rank
    // then finishes ~7.6 K-item regions, not twice as many of half the size
    // (finish 6.3 vs 5.3 ms per 1 G uniq k-mers at world 1, KMAN_DROUND_P1B)
    uint32_t g = 0;
    {
        const char *e = getenv("KMAN_DROUND_MIN_G");  // tests: the wide pass-1b digits of huge rounds
        g = e ? (uint32_t)atoi(e) : 0u;
        g = g <= 9 ? g : 9;
    }
    const uint64_t e2f = maxb >> 9;
    const bool p1b = g > 0 || getenv("KMAN_DROUND_P1B") != nullptr || world * d.H > 2 || e2f > FFILL_M;
    while (p1b && g < 9 && (e2f >> g) > FFILL_T && (g > 0 || e2f > FFILL_M)) g++;
    if ((e2f >> g) > FFILL_M) return KMAN_EFALLBACK;
    d.p1b = p1b;
    if (d.K < B1 + 9 + g + 1) return KMAN_EFALLBACK;
    d.g = g;
    d.rest = d.K - B1 - 9 - g;
    const uint64_t e1 = maxsb / (512ull * d.H);
    d.C1s = round_cap((flags & KMAN_ROOMY) ? 2 * e1 : e1, 256);
    if ((uint64_t)512 * world * d.H * d.C1s >= (1ull << 31)) return KMAN_EFALLBACK;  // (32-bit WC offsets)
    const uint64_t e2 = (maxb >> 9) >> g;
    const uint64_t c2 = round_cap(e2, 512);
    d.C1 = c2 < (uint64_t)FCAP ? c2 : (uint64_t)FCAP;
    // the finish at GCAP (40 KiB, three blocks per CU) when the regions the
    // plan expects fit it with the same margin; else FCAP (68 KiB, two)
    d.cap = round_cap(e2, 512) <= (uint64_t)GCAP ? GCAP : FCAP;
    if (d.cap == GCAP) d.C1 = d.C1 < (uint64_t)GCAP ? d.C1 : (uint64_t)GCAP;
    d.nsub = (uint64_t)nb * 512 * world * d.H;
    d.nreg = (uint64_t)nb * 512 << g;
    d.off_c1 = d.nsub * d.C1s * 8;
    d.off_tab = ceil_div(d.off_c1 + d.nsub * 4, 64) * 64;
    d.off_fail = d.off_tab + ceil_div((uint64_t)nb * world * 12 + 64, 64) * 64;
    d.a_bytes = d.off_fail + ceil_div(d.nreg + 64, 64) * 64;
    d.off_c2 = p1b ? d.nreg * d.C1 * 8 : 0;
    d.b_bytes = p1b ? d.off_c2 + ceil_div(d.nreg * 4 + 64, 64) * 64 : 64;
    *rp = d;
    return KMAN_OK;
}

int read_err(kman_ctx *ctx, uint32_t *e) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small + 8, ctx->d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(e, ctx->h_small + 8, 4);
    if (*e) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, 4, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (*e != ERR_REGION) return region_fault(ctx, *e, "kman_dround_finish");
    }
    return KMAN_OK;
}

// Pass 1b's width g, refitted from the pass-1 counts.  The plan takes g from
// the largest bucket, and a genome's repeats inflate every bucket that holds
// one (a satellite k-mer with 10^5 copies): g = 4 instead of 2 on the
// GRCh38-shaped input, 2 M finish regions of 1.4 K items where per-region
// costs dominate (16.6 us per region at 1.4 K items, 20 us at 3.8 K).  Here g
// covers all but the largest 0.5 % of the (b, d) sub-buckets (the ones a
// repeat fills, which overflow at any g and are redone by key range), never
// above the plan's.  Pass 1 flagged overflowing sub-buckets per (b, d);
// they are spread over their 2^g regions here.
int refit_g(kman_ctx *ctx, RoundPlan &d, const uint32_t *c1, uint8_t *freg, uint32_t G, bool *p1_lost) {
    const uint64_t nbd = (uint64_t)d.nb * 512, gh = (uint64_t)G * d.H;
    std::vector<uint32_t> hc(d.nsub);
    std::vector<uint8_t> hf(nbd);
    HIP_TRY(ctx, hipMemcpyAsync(hc.data(), c1, d.nsub * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(hf.data(), freg, nbd, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t gmin = 1;
    if (const char *e = getenv("KMAN_DROUND_MIN_G")) gmin = std::max<uint32_t>(gmin, std::min(9, atoi(e)));
    std::vector<uint8_t> need(nbd);
    std::vector<uint64_t> size(nbd);
    for (uint64_t j = 0; j < nbd; j++) {
        uint64_t t = 0;
        for (uint64_t q = 0; q < gh; q++) t += hc[j * gh + q];
        size[j] = t;
        uint32_t g = gmin;
        while (g < 9 && (t >> g) > FFILL_T) g++;
        need[j] = (uint8_t)g;
    }
    std::vector<uint64_t> ss(size);
    const uint64_t qi = (uint64_t)(0.995 * (double)(nbd - 1));
    std::nth_element(ss.begin(), ss.begin() + qi, ss.end());
    std::vector<uint8_t> ns(need);
    std::nth_element(ns.begin(), ns.begin() + qi, ns.end());
    uint32_t g = std::max<uint32_t>(gmin, ns[qi]);
    if (g < d.g) {
        const uint64_t nreg = nbd << g;
        const uint64_t e2 = ss[qi] >> g;
        uint64_t C1 = std::min<uint64_t>(round_cap(e2, 512), (uint64_t)FCAP);
        C1 = std::max<uint64_t>(C1, d.C1);  // (never tighter than planned)
        C1 = std::min<uint64_t>(C1, (uint64_t)FCAP);
        const uint64_t off_c2 = nreg * C1 * 8;
        if (off_c2 + ceil_div(nreg * 4 + 64, 64) * 64 <= d.b_bytes) {
            d.g = g;
            d.rest = d.K - B1 - 9 - g;
            d.nreg = nreg;
            d.C1 = C1;
            d.cap = C1 <= (uint64_t)GCAP ? GCAP : FCAP;
            d.off_c2 = off_c2;
        }
    }
    // pass 1's (b, d) flags -> the regions they feed
    bool any = false;
    for (uint64_t j = 0; j < nbd; j++) any |= hf[j] != 0;
    *p1_lost = any;
    if (any && getenv("KMAN_DROUND_LOG")) {
        uint64_t nl = 0, big = 0;
        for (uint64_t j = 0; j < nbd; j++)
            if (hf[j]) {
                nl++;
                big = std::max(big, size[j]);
            }
        fprintf(stderr, "refit_g: pass 1 lost items in %llu of %llu sub-buckets (C1s %llu; the largest kept %llu)\n",
                (unsigned long long)nl, (unsigned long long)nbd, (unsigned long long)d.C1s, (unsigned long long)big);
    }
    if (any) {
        std::vector<uint8_t> fr(d.nreg, 0);
        for (uint64_t j = 0; j < nbd; j++)
            if (hf[j]) memset(&fr[j << d.g], 1, (size_t)1 << d.g);
        HIP_TRY(ctx, hipMemcpyAsync(freg, fr.data(), d.nreg, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (fr leaves scope)
    } else {
        HIP_TRY(ctx, hipMemsetAsync(freg, 0, nbd, ctx->stream));
    }
    return KMAN_OK;
}

// ---------------------------------------------------------------- heavy keys
// A key round's heavy keys (PassArgs::hv_tab): every S-th received item's
// full key is sampled, the samples sorted and run-length counted, and the
// keys sampled at least twice (so they occur at least twice: a uniq round may
// drop all their copies) -- the most often sampled, at most HV_BMAX per bucket --
// go into an open-addressing table that pass 1 probes per item.  Pass 1 adds
// each key's dropped copies to drop[slot]; rg_hv_fix then adds them to the
// key's row (count mode: pass 1 kept one copy per chain, so the row exists
// unless its region was left out, in which case the partial redo recounts
// the whole key range from the codes).

// sample i = the item at i * S; runs (src, j) lie in src-major order, run t =
// src * nb + j starting at rs[t] (the last run starting at or before p holds p)
__global__ __launch_bounds__(256) void rg_hv_sample(const uint64_t *__restrict__ in, const uint64_t *__restrict__ rs,
                                                    uint32_t nrun, uint32_t nb, uint64_t S, uint64_t ns, uint32_t b_lo,
                                                    uint32_t kb, uint32_t q, uint64_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ns) return;
    const uint64_t p = i * S;
    uint32_t lo = 0, hi = nrun;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rs[mid] <= p) lo = mid;
        else hi = mid;
    }
    out[i] = ((uint64_t)(b_lo + lo % nb) << kb) | (in[p] >> q);
}

// One block per bucket j of the round: its sampled keys (the run-length
// output ukeys / cnt, sorted) seen >= 2 times, the most often sampled of them
// (hits >= a cut-off that leaves <= HV_BMAX; the first HV_BMAX in key order
// when more than that were sampled >= 63 times) into the bucket's table of key
// rests (an LDS open-addressing table of HV_BSLOTS, filled by CAS, then
// written out with each slot's index j * HV_BMAX + i into keys), *total +=
// the keys taken
__global__ __launch_bounds__(256) void rg_hv_build(const uint64_t *__restrict__ ukeys, const uint32_t *__restrict__ cnt,
                                                   uint64_t nu, uint32_t b_lo, uint32_t kb, uint64_t *__restrict__ tab,
                                                   uint32_t *__restrict__ idx, uint64_t *__restrict__ keys,
                                                   uint32_t *__restrict__ total) {
    __shared__ unsigned long long t_[HV_BSLOTS];
    __shared__ uint32_t ti[HV_BSLOTS];
    __shared__ uint32_t hist[64], wsum[4], s_cut;
    __shared__ uint64_t s_lo, s_hi;
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const int lane = lane_id(), w = tid >> 6;
    for (uint32_t q = tid; q < HV_BSLOTS; q += 256) {
        t_[q] = HV_EMPTY;
        ti[q] = 0;
    }
    if (tid < 64) hist[tid] = 0;
    if (tid < 2) {  // the bucket's range [lo, hi) of ukeys
        const uint64_t want = (uint64_t)(b_lo + j + tid) << kb;
        uint64_t lo = 0, hi = nu;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (ukeys[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        if (tid == 0) s_lo = lo;
        else s_hi = lo;
    }
    __syncthreads();
    const uint64_t lo = s_lo, hi = s_hi;
    for (uint64_t i = lo + tid; i < hi; i += 256) {
        const uint32_t c = cnt[i];
        if (c >= 2) atomicAdd(&hist[c < 63 ? c : 63], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t above = 0, cut = 64;
        for (uint32_t t = 63; t >= 2; t--) {
            if (above + hist[t] > HV_BMAX) break;
            above += hist[t];
            cut = t;
        }
        s_cut = cut == 64 && hist[63] ? 63 : cut;  // (64: none)
    }
    __syncthreads();
    const uint32_t cut = s_cut;
    // the keys >= cut in key order, 256 at a time (cut 64: none; the
    // bucket's table and keys are written empty all the same -- they hold a
    // previous round's otherwise)
    uint32_t base = 0;
    for (uint64_t c0 = lo; cut < 64 && c0 < hi && base < HV_BMAX; c0 += 256) {
        const uint64_t i = c0 + tid;
        const bool take = i < hi && cnt[i] >= cut;
        const uint64_t m = __ballot(take);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, tot = 0;
        for (int q = 0; q < 4; q++) {
            before += q < w ? wsum[q] : 0u;
            tot += wsum[q];
        }
        const uint32_t at = base + before + (uint32_t)__popcll(m & lanemask_lt());
        if (take && at < HV_BMAX) {
            const uint64_t key = ukeys[i], kr = key & ((1ull << kb) - 1);
            uint32_t sl = hv_slot(kr);
            while (atomicCAS(&t_[sl], (unsigned long long)HV_EMPTY, (unsigned long long)kr) != HV_EMPTY)
                sl = (sl + 1) & (HV_BSLOTS - 1);
            ti[sl] = j * HV_BMAX + at;
            keys[(uint64_t)j * HV_BMAX + at] = key;
        }
        base += tot;
        __syncthreads();
    }
    const uint32_t n = base < HV_BMAX ? base : HV_BMAX;
    for (uint32_t q = n + tid; q < HV_BMAX; q += 256) keys[(uint64_t)j * HV_BMAX + q] = HV_EMPTY;
    for (uint32_t q = tid; q < HV_BSLOTS; q += 256) {
        tab[(uint64_t)j * HV_BSLOTS + q] = t_[q];
        idx[(uint64_t)j * HV_BSLOTS + q] = ti[q];
    }
    if (tid == 0) atomicAdd(total, n);
}

// each heavy key's dropped copies onto its row (rows sorted by key)
template <typename V>
__global__ __launch_bounds__(256) void rg_hv_fix(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ drop,
                                                 uint32_t m, const uint64_t *__restrict__ okeys, V *__restrict__ ovals,
                                                 uint64_t n) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const uint64_t key = keys[s], d = drop[s];
    if (!d || !n || key == HV_EMPTY) return;
    uint64_t lo = 0, hi = n;  // first row >= key
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (okeys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && okeys[lo] == key) ovals[lo] += (V)d;
}

// kman_dround_left: the items of the left-out regions, from the pass-1
// sub-regions (bd, src, h) = subs[i] of their sub-buckets bd (a sub-bucket's
// 2^g regions are left out one by one: an item is kept when freg flags its
// region) as full keys (+ uniq pos, as the finish emits them).  Block
// (i, y) takes the sub-region's 2048-item chunks y, y + Y, ...; WRITE = false
// counts its items into bcnt[block], WRITE = true writes them from
// boff[block] on (a scan of those counts), in chunk order
template <typename TI, bool WRITE>
__global__ __launch_bounds__(256) void rg_left_gather(const TI *__restrict__ r1, uint64_t C1s,
                                                      const uint32_t *__restrict__ subs,
                                                      const uint32_t *__restrict__ cnts, const uint8_t *__restrict__ freg,
                                                      uint32_t g, uint32_t G, uint32_t H, uint32_t b_lo, uint32_t kb,
                                                      uint32_t Q, uint32_t rc, uint64_t *__restrict__ bco,
                                                      uint64_t *__restrict__ okeys, uint64_t *__restrict__ opos) {
    constexpr int E = 8;
    __shared__ uint32_t wsum[4];
    const uint32_t i = blockIdx.x, bid = blockIdx.x * gridDim.y + blockIdx.y;
    const uint32_t s = subs[i], n = cnts[i];
    const uint32_t bd = s / (G * H), src = (s / H) % G;
    const uint64_t hi = (uint64_t)(b_lo + (bd >> 9)) << kb;
    const uint64_t kmask = (1ull << kb) - 1, qmask = Q ? (1ull << Q) - 1 : 0ull;
    const uint32_t rsh = kb - 9 - g;  // key bits below the region
    const TI *in = r1 + (uint64_t)s * C1s;
    const int lane = lane_id(), w = threadIdx.x >> 6;
    uint64_t base = WRITE ? bco[bid] : 0;
    uint32_t mine = 0;
    for (uint32_t c0 = blockIdx.y * 256 * E; c0 < n; c0 += gridDim.y * 256 * E) {
        uint64_t kk[E], vv[E];
        uint32_t km = 0;
#pragma unroll
        for (int e = 0; e < E; e++) {
            const uint32_t j = c0 + e * 256 + threadIdx.x;
            kk[e] = vv[e] = 0;
            if (j < n) {
                const uint64_t v = in[j];
                uint64_t key;
                if constexpr (sizeof(TI) == 4) key = hi | ((uint64_t)(bd & 511u) << (kb - 9)) | (v & ((1ull << (kb - 9)) - 1));
                else key = hi | ((v >> Q) & kmask);
                const uint64_t r = ((uint64_t)bd << g) | ((key >> rsh) & ((1ull << g) - 1));
                if (freg[r]) km |= 1u << e;
                kk[e] = key;
                vv[e] = v;
            }
        }
        const uint32_t c = (uint32_t)__popc(km);
        if constexpr (!WRITE) {
            mine += c;
            continue;
        }
        // the chunk's block-wide exclusive offsets
        const uint32_t inc = wave_inclusive_scan(c, SumU32());
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        uint32_t before = 0, tot = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            before += q < w ? wsum[q] : 0u;
            tot += wsum[q];
        }
        __syncthreads();
        uint64_t at = base + before + inc - c;
#pragma unroll
        for (int e = 0; e < E; e++) {
            if (!((km >> e) & 1u)) continue;
            okeys[at] = kk[e];
            if (sizeof(TI) == 8 && opos) {
                const uint64_t idx = vv[e] & qmask;
                opos[at] = (rc ? idx : idx << 1) | ((uint64_t)src << 56);
            }
            at++;
        }
        base += tot;
    }
    if constexpr (!WRITE) {
        const uint32_t inc = wave_inclusive_scan(mine, SumU32());
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        if (threadIdx.x == 0) bco[bid] = (uint64_t)wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

__global__ __launch_bounds__(256) void rg_left_counts(const uint32_t *__restrict__ c1, const uint32_t *__restrict__ subs,
                                                      uint32_t n, uint64_t C1s, uint32_t *__restrict__ cnts) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const uint32_t c = c1[subs[i]];
        cnts[i] = c < C1s ? c : (uint32_t)C1s;
    }
}

struct HeavyRound {
    uint32_t n = 0;  // heavy keys in the table (0: none, pass 1 as usual)
    uint32_t slots = 0;  // the keys list's length (HV_BMAX per bucket, HV_EMPTY where unused)
    char *w = nullptr;  // kman_ctx::d_hv (HVO_* parts)
};

int hv_fix(kman_ctx *ctx, const char *w, uint32_t m, const uint64_t *okeys, void *ovals, uint32_t vb, uint64_t n) {
    const uint64_t *keys = (const uint64_t *)(w + HVO_KEYS), *drop = (const uint64_t *)(w + HVO_DROP);
    const dim3 grid((m + 255) / 256);
    if (vb == 4)
        hipLaunchKernelGGL(rg_hv_fix<uint32_t>, grid, dim3(256), 0, ctx->stream, keys, drop, m, okeys,
                           (uint32_t *)ovals, n);
    else
        hipLaunchKernelGGL(rg_hv_fix<uint64_t>, grid, dim3(256), 0, ctx->stream, keys, drop, m, okeys,
                           (uint64_t *)ovals, n);
    HIP_TRY(ctx, hipGetLastError());
    return KMAN_OK;
}

int hv_buffer(kman_ctx *ctx, size_t bytes, char **p) {
    if (bytes > ctx->hv_bytes) {
        if (ctx->d_hv) {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(ctx->d_hv));
            ctx->d_hv = nullptr;
            ctx->hv_bytes = 0;
        }
        HIP_TRY(ctx, hipMalloc(&ctx->d_hv, bytes));
        ctx->hv_bytes = bytes;
    }
    *p = (char *)ctx->d_hv;
    return KMAN_OK;
}

// The round's heavy keys (see above).  hb[j * G + src] = run (j, src)'s start
// in d_recv, total = the round's items.  KMAN_HEAVY=0 turns it off.
int find_heavy(kman_ctx *ctx, const RoundPlan &d, const uint64_t *d_recv, const std::vector<uint64_t> &hb,
               uint64_t total, uint32_t b_lo, HeavyRound *hv) {
    hv->n = 0;
    const char *e = getenv("KMAN_HEAVY");  // "0": off; "1": any round (tests); else rounds of >= 2^20 items
    if (e && !strcmp(e, "0")) return KMAN_OK;
    const bool force = e && !strcmp(e, "1");
    if (d.K > 62 || (!force && total < (1u << 20)) || !total) return KMAN_OK;  // (table keys < HV_EMPTY)
    const uint32_t nb = d.nb, G = d.G, nrun = nb * G;
    // samples: every S-th item, S >= 64, at most HV_NS
    const uint64_t HV_NS = 1ull << 23;
    const uint64_t S = std::max<uint64_t>(64, ceil_div(total, HV_NS));
    const uint64_t ns = ceil_div(total, S);
    const size_t o_misc = HVO_END, o_rs = o_misc + 512, o_s = o_rs + ceil_div(nrun * 8, 256) * 256, o_a = o_s + ns * 8, o_u = o_a + ns * 8, o_c = o_u + ns * 8,
                 bytes = o_c + ns * 4 + 256;
    char *w;
    KMAN_TRY(hv_buffer(ctx, bytes, &w));
    uint64_t *rs = (uint64_t *)(w + o_rs), *smp = (uint64_t *)(w + o_s), *alt = (uint64_t *)(w + o_a),
             *uk = (uint64_t *)(w + o_u);
    uint32_t *uc = (uint32_t *)(w + o_c);
    std::vector<uint64_t> hrs(nrun);
    for (uint32_t src = 0; src < G; src++)
        for (uint32_t j = 0; j < nb; j++) hrs[(size_t)src * nb + j] = hb[(size_t)j * G + src];
    HIP_TRY(ctx, hipMemcpyAsync(rs, hrs.data(), nrun * 8, hipMemcpyHostToDevice, ctx->stream));
    // the samples sorted and run-length counted: first 2^16 of them (every
    // S1-th item; all distinct -- uniform keys -- ends it here), then ns
    uint64_t nu = 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms_since = [&](std::chrono::steady_clock::time_point a) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    };
    for (int stage = 0; stage < 2; stage++) {
        const uint64_t S_ = stage ? S : std::max<uint64_t>(S, ceil_div(total, 1ull << 16)),
                       ns_ = stage ? ns : ceil_div(total, S_);
        if (stage && S_ == std::max<uint64_t>(S, ceil_div(total, 1ull << 16))) break;  // (stage 0 took them all)
        {
            KTimer kt_(ctx, "heavy_sample");
            hipLaunchKernelGGL(rg_hv_sample, dim3((uint32_t)ceil_div(ns_, 256)), dim3(256), 0, ctx->stream, d_recv,
                               rs, nrun, nb, S_, ns_, b_lo, d.K - B1, d.Q, smp);
            HIP_TRY(ctx, hipGetLastError());
        }
        int in_alt = 0;
        KMAN_TRY(kman_sort(ctx, smp, alt, nullptr, nullptr, 0, ns_, d.K, nullptr, &in_alt));
        KMAN_TRY(kman_rle_count(ctx, in_alt ? alt : smp, ns_, uk, uc, 4, &nu));  // (synchronises)
        if (nu == ns_) return KMAN_OK;  // every sample distinct: no heavy key
    }
    const double t_sort = ms_since(t0);
    const auto t1 = std::chrono::steady_clock::now();
    // the tables built on the device (the buckets without a key sampled
    // twice get empty ones: their chains probe and find nothing)
    uint32_t *d_total = (uint32_t *)(w + o_misc);
    HIP_TRY(ctx, hipMemsetAsync(d_total, 0, 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w + HVO_DROP, 0, HV_MAX * 8, ctx->stream));
    hipLaunchKernelGGL(rg_hv_build, dim3(nb), dim3(256), 0, ctx->stream, uk, uc, nu, b_lo, d.K - B1,
                       (uint64_t *)(w + HVO_TAB), (uint32_t *)(w + HVO_IDX), (uint64_t *)(w + HVO_KEYS), d_total);
    HIP_TRY(ctx, hipGetLastError());
    uint32_t m = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&m, d_total, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (getenv("KMAN_DROUND_LOG"))
        fprintf(stderr, "find_heavy: %llu samples, %llu distinct, %u keys; sample + sort %.2f ms, tables %.2f\n",
                (unsigned long long)ns, (unsigned long long)nu, m, t_sort, ms_since(t1));
    if (!m) return KMAN_OK;
    hv->n = m;
    hv->slots = nb * HV_BMAX;
    hv->w = w;
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_dshard_plan(uint64_t n_bases, uint64_t n_bases_q, uint32_t k, uint32_t flags, int mode) {
    RegionPlan p;
    return make_shard_plan(n_bases, n_bases_q, k, flags, mode, &p);
}

extern "C" int kman_dshard_hist(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint64_t n_bases_q,
                                uint32_t k, uint32_t flags, int mode, uint32_t *d_hist, uint32_t *hist) {
    if (!ctx || !d_hist || !hist) return KMAN_EINVAL;
    RegionPlan p;
    const int pr = make_shard_plan(n_bases, n_bases_q, k, flags, mode, &p);
    if (pr == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_dshard_hist: bad arguments");
    if (pr != KMAN_OK) return pr;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, (size_t)RADIX * RS * 4, ctx->stream));
    if (n_bases) {
        if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "null codes");
        KTimer kt_(ctx, "shard_hist");
        launch_hist_any(ctx, p, d_codes, n_bases, k, d_hist);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipMemcpyAsync(hist, d_hist, (size_t)RADIX * RS * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_dshard_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint64_t n_bases_q,
                                   uint32_t k, uint32_t flags, int mode, const uint32_t *d_hist,
                                   const uint64_t *d_rtab, uint64_t *d_send) {
    if (!ctx) return KMAN_EINVAL;
    RegionPlan p;
    const int pr = make_shard_plan(n_bases, n_bases_q, k, flags, mode, &p);
    if (pr == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_dshard_extract: bad arguments");
    if (pr != KMAN_OK) return pr;
    if (!n_bases) return KMAN_OK;
    if (!d_codes || !d_hist || !d_rtab || !d_send) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));  // (the XCD ticket counters only)
    {
        KTimer kt_(ctx, "region_extract");
        const uint32_t *cnt = d_hist;  // the exact region sizes (read-only)
        launch_extract_ex_any(ctx, p, d_codes, n_bases, k, d_send, cnt, d_rtab, epoch);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint32_t e;
    KMAN_TRY(read_err(ctx, &e));
    if (e) return kman_fail(ctx, KMAN_EHIP, "kman_dshard_extract: a region outgrew its rg_hist count");
    return KMAN_OK;
}

extern "C" int kman_dround_plan(uint32_t k, uint32_t flags, int mode, uint32_t world, uint64_t n_bases_q, uint32_t nb,
                                const uint64_t *counts, uint64_t *a_bytes, uint64_t *b_bytes) {
    if (!a_bytes || !b_bytes) return KMAN_EINVAL;
    *a_bytes = *b_bytes = 0;
    RoundPlan d;
    const int r = make_rplan(k, flags, mode, world, n_bases_q, nb, counts, &d);
    if (r != KMAN_OK) return r;
    *a_bytes = d.a_bytes;
    *b_bytes = d.b_bytes;
    return KMAN_OK;
}

extern "C" int kman_dround_finish(kman_ctx *ctx, const uint64_t *d_recv, uint32_t k, uint32_t flags, int mode,
                                  uint32_t world, uint64_t n_bases_q, uint32_t b_lo, uint32_t nb,
                                  const uint64_t *counts, void *d_a, uint64_t a_bytes, void *d_b, uint64_t b_bytes,
                                  uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes, uint64_t *n_out) {
    if (!ctx || !n_out) return KMAN_EINVAL;
    *n_out = 0;
    RoundPlan d;
    const int pr = make_rplan(k, flags, mode, world, n_bases_q, nb, counts, &d);
    if (pr == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_dround_finish: bad arguments");
    if (pr != KMAN_OK) return pr;
    if (b_lo + nb > (uint32_t)RADIX) return kman_fail(ctx, KMAN_EINVAL, "bucket range past 256");
    if (a_bytes < d.a_bytes || b_bytes < d.b_bytes)
        return kman_fail(ctx, KMAN_ECAP, "round arenas %llu / %llu < %llu / %llu bytes", (unsigned long long)a_bytes,
                         (unsigned long long)b_bytes, (unsigned long long)d.a_bytes, (unsigned long long)d.b_bytes);
    if (oval_bytes != 4 && oval_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "oval_bytes must be 4 or 8");
    if (mode == KMAN_FINISH_UNIQ && oval_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "uniq pos on N > 1 are u64");
    if (nb == 0) return KMAN_OK;
    if (!d_recv || !d_a || !d_b || !d_okeys || !d_ovals) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    char *wa = (char *)d_a, *wb = (char *)d_b;
    uint64_t *r1 = (uint64_t *)wa;
    uint32_t *c1 = (uint32_t *)(wa + d.off_c1);
    uint64_t *sbase = (uint64_t *)(wa + d.off_tab);
    uint32_t *scnt = (uint32_t *)(sbase + (uint64_t)nb * world);
    uint64_t *r2 = (uint64_t *)wb;
    uint32_t *c2 = (uint32_t *)(wb + d.off_c2);
    uint8_t *freg = (uint8_t *)(wa + d.off_fail);
    const uint32_t G = world;
    ctx->failed.clear();
    ctx->heavy_keys = 0;
    ctx->left.valid = false;
    ctx->left.bd.clear();
    // pass-1 segments: bucket (b, src) = one contiguous run of src's chunk
    std::vector<uint64_t> hb((size_t)nb * G);
    std::vector<uint32_t> hn((size_t)nb * G);
    uint64_t roff = 0;
    for (uint32_t src = 0; src < G; src++) {
        for (uint32_t j = 0; j < nb; j++) {
            const uint64_t c = counts[(uint64_t)src * nb + j];
            hb[(size_t)j * G + src] = roff;
            hn[(size_t)j * G + src] = (uint32_t)c;
            roff += c;
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(sbase, hb.data(), hb.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(scnt, hn.data(), hn.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(c1, 0, d.nsub * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(freg, 0, d.nreg, ctx->stream));
    HeavyRound hv;
    const auto t_hv0 = std::chrono::steady_clock::now();
    {
        // (no room for the samples: the round runs without the table)
        const int hr = find_heavy(ctx, d, d_recv, hb, roff, b_lo, &hv);
        if (hr == KMAN_ENOMEM) {
            hv = HeavyRound{};
            ctx->err.clear();
            (void)hipGetLastError();
        } else if (hr != KMAN_OK) {
            return hr;
        }
    }
    const double hv_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_hv0).count();
    uint32_t epoch, *counter;
    // 4-byte count items out of pass 1 when the key bits below its digit
    // (rest + g, whatever refit_g makes of the split) fit 32 bits
    const bool narrow1 = narrow_ok(ctx, mode, d.Q, d.K - B1 - 9, 0) && !getenv("KMAN_WIDE_ITEMS");
    bool p1_lost = true;  // (no pass 1b: the finish reads pass 1's output, whose overflow loses items)
    // pass 1: by the 9 bits below the bucket, H chains per (b, src) into
    // sub-regions (b, d, src, h)
    {
        KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));
        KTimer kt_(ctx, "region_pass");
        PassArgs pa{};
        pa.in = d_recv;
        pa.seg_base = sbase;
        pa.seg_cnt = scnt;
        pa.nbk = nb * G;
        pa.nsg = 1;
        pa.gsub = G;
        pa.H = d.H;
        pa.shift = d.Q + d.K - B1 - 9;
        pa.bits = 9;
        pa.out = r1;
        pa.C1 = d.C1s;
        pa.cnt1 = c1;
        pa.fail = freg;  // sub-region (b, d, src, h) -> flag (b, d) (spread over its 2^g regions below)
        pa.fail_div = G * d.H;
        pa.fail_shift = 0;
        if (hv.n) {
            pa.hv_tab = (const uint64_t *)(hv.w + HVO_TAB);
            pa.hv_idx = (const uint32_t *)(hv.w + HVO_IDX);
            pa.hv_drop = (uint64_t *)(hv.w + HVO_DROP);
            pa.hv_q = d.Q;
            pa.hv_keep = mode == KMAN_FINISH_COUNT;
        }
        KMAN_TRY(launch_pass(ctx, pa, counter, nullptr, false, narrow1));
        HIP_TRY(ctx, hipGetLastError());
    }
    KMAN_TRY(rg_check(ctx, "pass 1", c1, d.nsub));
    if (d.p1b) {
        KMAN_TRY(refit_g(ctx, d, c1, freg, G, &p1_lost));
        c2 = (uint32_t *)(wb + d.off_c2);
    }
    uint64_t *fst = nullptr;
#ifdef KMAN_RG_STAMPS
    if (getenv("KMAN_RG_STAMPS")) {
        HIP_TRY(ctx, hipMalloc((void **)&fst, d.nreg * 128));
        HIP_TRY(ctx, hipMemsetAsync(fst, 0, d.nreg * 128, ctx->stream));
    }
#endif
    if (!d.p1b) {
        // one source, two chains: the finish reads the pass-1 sub-regions
        FinishArgs f{r1, d.C1s, c1, d.Q, d.rest, (uint32_t)d.rc, (uint64_t)b_lo << 9, 0u, (uint32_t)d.nreg};
        f.fsub = d.H;
        f.freg = freg;
        f.in4 = narrow1;
        f.cap = d.cap;
        KMAN_TRY(run_finish(ctx, f, mode, d_okeys, d_ovals, oval_bytes, fst));
    } else {
        // (c2 may lie in the receive buffer: cleared only once pass 1 has read it)
        HIP_TRY(ctx, hipMemsetAsync(c2, 0, d.nreg * 4, ctx->stream));
        // pass 1b's items: 4 bytes out when the narrow finish takes them (always
        // when pass 1's were: rest <= rest + g)
        const bool narrow1b = narrow1 || (narrow_ok(ctx, mode, d.Q, d.rest, 0) && !getenv("KMAN_WIDE_ITEMS"));
        // pass 1b: per (b, d), its 2G sub-regions concatenated, by g more bits;
        // the source rank (segment index / 2) goes into the d field
        {
            KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));
            KTimer kt_(ctx, "region_pass1b");
            // count mode: a chain takes 2^m consecutive sub-buckets (their G x H
            // sub-regions lie one after another) and sorts by the g bits and the
            // low m bits of d above them -- the same regions, in the same order,
            // from fewer and longer chains (a sub-bucket alone is a few tiles,
            // whose per-chain setup and partial lines dominated); m keeps >= 1024
            // chains, <= 64 segments, <= 8 bits, and the d bits a 4-byte item holds
            // (and stops once a chain averages 64 K items: config 4's
            // sub-buckets, ~100 K each, stay one per chain)
            uint32_t m = 0;
            if (mode == KMAN_FINISH_COUNT) {
                const uint32_t kb = d.K - B1;
                const uint64_t per_sub = roff / ((uint64_t)nb * 512);
                while (m < 5 && (per_sub << m) < 65536 && ((d.H * G) << (m + 1)) <= 64 && d.g + m + 1 <= 8 &&
                       ((nb * 512u) >> (m + 1)) >= 1024 && (!narrow1 || m + 1 + (kb - 9) <= 32))
                    m++;
            }
            if (d.g == 0) {
                // (0 bits: a merge of the sources' sub-regions, rg_merge_regions)
                const uint32_t nsg = d.H * G, tg = mode == KMAN_FINISH_UNIQ, ts = d.Q + d.rest;
                if (narrow1b != narrow1) return kman_fail(ctx, KMAN_EHIP, "pass 1b: 0-bit merge changes the item width");
                KMAN_TRY(launch_merge_regions(ctx, narrow1, r1, d.C1s, c1, nsg, d.H, r2, d.C1, c2, freg,
                                              (uint32_t)d.nreg, tg, ts));
            } else {
                PassArgs pa{};
                pa.in = r1;
                pa.seg_base = nullptr;
                pa.seg_cnt = c1;
                pa.stride = d.C1s;
                pa.nbk = (nb * 512) >> m;
                pa.nsg = (d.H * G) << m;
                pa.gsub = 1;
                pa.H = 1;
                pa.shift = d.Q + d.rest;
                pa.bits = d.g + m;
                pa.tag = mode == KMAN_FINISH_UNIQ;
                pa.tag_div = d.H;
                pa.tag_shift = d.Q + d.rest + d.g;
                pa.tag_bits = 9;
                pa.out = r2;
                pa.C1 = d.C1;
                pa.cnt1 = c2;
                pa.fail = freg;
                pa.fail_div = 1;
                pa.fail_shift = 0;
                KMAN_TRY(launch_pass(ctx, pa, counter, nullptr, narrow1, narrow1b));
                HIP_TRY(ctx, hipGetLastError());
            }
        }
        KMAN_TRY(rg_check(ctx, "pass 1b", c2, d.nreg));
        if (const char *t = getenv("KMAN_TEST_LEAVE_OUT")) {
            // tests: every n-th region left out as if it had overflowed (the
            // partial redo's paths on inputs too small to overflow)
            const uint64_t every = strtoull(t, nullptr, 10);
            if (every) {
                std::vector<uint8_t> fr(d.nreg);
                HIP_TRY(ctx, hipMemcpy(fr.data(), freg, d.nreg, hipMemcpyDeviceToHost));
                for (uint64_t r = 0; r < d.nreg; r += every) fr[r] = 1;
                HIP_TRY(ctx, hipMemcpy(freg, fr.data(), d.nreg, hipMemcpyHostToDevice));
                const uint32_t ev = ERR_REGION;
                HIP_TRY(ctx, hipMemcpy(ctx->d_err, &ev, 4, hipMemcpyHostToDevice));
            }
        }
        {
            FinishArgs f{r2, d.C1, c2, d.Q, d.rest, (uint32_t)d.rc, (uint64_t)b_lo << (9 + d.g),
                         mode == KMAN_FINISH_UNIQ ? d.Q + d.rest + d.g : 0u, (uint32_t)d.nreg};
            f.freg = freg;
            f.in4 = narrow1b;
            f.cap = d.cap;
            KMAN_TRY(run_finish(ctx, f, mode, d_okeys, d_ovals, oval_bytes, fst));
        }
    }
    if (fst) KMAN_TRY(report_finish_stamps(ctx, fst, d.nreg));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_small + 4, ctx->d_status + (d.nreg - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    uint32_t e;
    KMAN_TRY(read_err(ctx, &e));  // synchronises
    const uint64_t wd = ctx->h_small[4];
    if (((wd >> 56) & 63u) != ctx->epoch || (wd >> 62) != ST_INCL)
        return kman_fail(ctx, KMAN_EHIP, "region output total not published");
    *n_out = wd & ST_VMASK;
    ctx->heavy_keys = hv.n;
    ctx->heavy_slots = hv.slots;
    ctx->heavy_mode = mode;
    {
        // pass 1's output stays in arena A until the caller reuses it
        auto &L = ctx->left;
        L.valid = !e || (d.p1b && !p1_lost);
        L.r1 = r1;
        L.c1 = c1;
        L.C1s = d.C1s;
        L.nb = nb;
        L.G = G;
        L.H = d.H;
        L.K = d.K;
        L.Q = d.Q;
        L.b_lo = b_lo;
        L.rc = d.rc;
        L.narrow = narrow1;
        L.mode = mode;
        L.g = d.g;
        L.freg = freg;
    }
    if (hv.n && mode == KMAN_FINISH_COUNT && *n_out) {
        // the heavy keys' dropped copies onto their rows
        KTimer kt_(ctx, "heavy_fix");
        KMAN_TRY(hv_fix(ctx, hv.w, hv.slots, d_okeys, d_ovals, oval_bytes, *n_out));
    }
    if (!e) return KMAN_OK;
    // regions that overflowed a capacity (skewed keys: repeats) emitted
    // nothing; the rows of every other region are in place, in key order.
    // Their key ranges, merged, for the caller to redo (kman_dround_failed)
    std::vector<uint8_t> hf(d.nreg);
    HIP_TRY(ctx, hipMemcpy(hf.data(), freg, d.nreg, hipMemcpyDeviceToHost));
    const uint64_t rbase = (uint64_t)b_lo << (9 + d.g);
    const uint64_t top = d.rest >= 64 ? ~0ull : ((1ull << d.rest) - 1);
    for (uint64_t r = 0; r < d.nreg; r++) {
        if (!hf[r]) continue;
        if (ctx->left.valid && (ctx->left.bd.empty() || ctx->left.bd.back() != (uint32_t)(r >> d.g)))
            ctx->left.bd.push_back((uint32_t)(r >> d.g));
        const uint64_t lo = (rbase + r) << d.rest, hi = lo | top;
        if (!ctx->failed.empty() && ctx->failed.back() + 1 == lo) ctx->failed.back() = hi;
        else {
            ctx->failed.push_back(lo);
            ctx->failed.push_back(hi);
        }
    }
    if (getenv("KMAN_DROUND_LOG")) {
        uint64_t nf = 0;
        for (uint64_t r = 0; r < d.nreg; r++) nf += hf[r] != 0;
        fprintf(stderr, "kman_dround_finish: %llu items, nb %u G %u H %u g %u C1s %llu C1 %llu, heavy %u, pass 1 %s, "
                "%llu of %llu regions left out (%zu sub-buckets for a local redo); finding the heavy keys %.2f ms\n",
                (unsigned long long)roff, nb, G, d.H, d.g, (unsigned long long)d.C1s, (unsigned long long)d.C1, hv.n,
                p1_lost ? "lost items" : "complete", (unsigned long long)nf, (unsigned long long)d.nreg,
                ctx->left.bd.size(), hv_ms);
    }
    if (ctx->failed.empty())  // (an overflow that flagged no region: not expected)
        return kman_fail(ctx, KMAN_EHIP, "kman_dround_finish: overflow without a flagged region");
    return KMAN_EPARTIAL;
}

extern "C" int kman_dround_left(kman_ctx *ctx, uint64_t *d_keys, uint64_t *d_pos, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return KMAN_EINVAL;
    *n = 0;
    const auto &L = ctx->left;
    if (!L.valid) return KMAN_EFALLBACK;
    if (L.bd.empty()) return KMAN_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t GH = L.G * L.H;
    const uint32_t ns = (uint32_t)L.bd.size() * GH;
    std::vector<uint32_t> subs(ns);
    for (size_t i = 0; i < L.bd.size(); i++)
        for (uint32_t q = 0; q < GH; q++) subs[i * GH + q] = L.bd[i] * GH + q;
    // (the heavy-key scratch holds the sub-region list, counts and offsets)
    const size_t o_subs = HVO_END, o_cnt = o_subs + ceil_div((uint64_t)ns * 4, 256) * 256,
                 o_off = o_cnt + ceil_div((uint64_t)ns * 4, 256) * 256, bytes = o_off + (size_t)ns * 16 * 8 + 256;
    if (bytes > ctx->hv_bytes) {
        // (grows the buffer: its heavy table is copied along)
        void *nb_ = nullptr;
        if (hipMalloc(&nb_, bytes) != hipSuccess) {  // (no room: the caller's marked-extraction redo)
            (void)hipGetLastError();
            return KMAN_EFALLBACK;
        }
        if (ctx->d_hv) {
            HIP_TRY(ctx, hipMemcpyAsync(nb_, ctx->d_hv, std::min(ctx->hv_bytes, HVO_END), hipMemcpyDeviceToDevice,
                                        ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            HIP_TRY(ctx, hipFree(ctx->d_hv));
        }
        ctx->d_hv = nb_;
        ctx->hv_bytes = bytes;
    }
    char *w = (char *)ctx->d_hv;
    uint32_t *d_subs = (uint32_t *)(w + o_subs), *d_cnt = (uint32_t *)(w + o_cnt);
    uint64_t *d_bco = (uint64_t *)(w + o_off);  // (ns x Y <= 16 per-block counts / offsets)
    HIP_TRY(ctx, hipMemcpyAsync(d_subs, subs.data(), (size_t)ns * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(rg_left_counts, dim3((ns + 255) / 256), dim3(256), 0, ctx->stream, L.c1, d_subs, ns, L.C1s,
                       d_cnt);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> cnt(ns);
    HIP_TRY(ctx, hipMemcpyAsync(cnt.data(), d_cnt, (size_t)ns * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t mx = 0;
    for (uint32_t i = 0; i < ns; i++) mx = std::max(mx, cnt[i]);
    if (d_keys && L.mode == KMAN_FINISH_UNIQ && !d_pos) return kman_fail(ctx, KMAN_EINVAL, "uniq: null pos");
    KTimer kt_(ctx, "left_gather");
    const uint32_t Y = std::max<uint32_t>(1, std::min<uint32_t>(16, (mx + 2047) / 2048));
    const dim3 grid(ns, Y);
    const uint64_t nbk = (uint64_t)ns * Y;
    // the per-block counts, then (writing) their exclusive scan, in d_bco
    const auto launch = [&](bool write) {
        uint64_t *pos = write && L.mode == KMAN_FINISH_UNIQ ? d_pos : nullptr;
        uint64_t *ok = write ? d_keys : nullptr;
        if (L.narrow) {
            if (write)
                hipLaunchKernelGGL((rg_left_gather<uint32_t, true>), grid, dim3(256), 0, ctx->stream,
                                   (const uint32_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
            else
                hipLaunchKernelGGL((rg_left_gather<uint32_t, false>), grid, dim3(256), 0, ctx->stream,
                                   (const uint32_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
        } else {
            if (write)
                hipLaunchKernelGGL((rg_left_gather<uint64_t, true>), grid, dim3(256), 0, ctx->stream,
                                   (const uint64_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
            else
                hipLaunchKernelGGL((rg_left_gather<uint64_t, false>), grid, dim3(256), 0, ctx->stream,
                                   (const uint64_t *)L.r1, L.C1s, d_subs, d_cnt, L.freg, L.g, L.G, L.H, L.b_lo,
                                   L.K - B1, L.Q, (uint32_t)L.rc, d_bco, ok, pos);
        }
        return hipGetLastError();
    };
    HIP_TRY(ctx, launch(false));
    std::vector<uint64_t> bc(nbk);
    HIP_TRY(ctx, hipMemcpyAsync(bc.data(), d_bco, nbk * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t tot = 0;
    for (uint64_t q = 0; q < nbk; q++) {
        const uint64_t c = bc[q];
        bc[q] = tot;
        tot += c;
    }
    *n = tot;
    if (!d_keys || !tot) return KMAN_OK;
    if (tot > cap)
        return kman_fail(ctx, KMAN_ECAP, "kman_dround_left: %llu items > cap %llu", (unsigned long long)tot,
                         (unsigned long long)cap);
    HIP_TRY(ctx, hipMemcpyAsync(d_bco, bc.data(), nbk * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, launch(true));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (bc leaves scope)
    return KMAN_OK;
}

extern "C" int kman_dround_heavy_fix(kman_ctx *ctx, const uint64_t *d_keys, void *d_vals, uint32_t val_bytes,
                                     uint64_t n) {
    if (!ctx) return KMAN_EINVAL;
    if (!ctx->heavy_keys || ctx->heavy_mode != KMAN_FINISH_COUNT || !n) return KMAN_OK;
    if (!d_keys || !d_vals) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (val_bytes != 4 && val_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "val_bytes must be 4 or 8");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    KMAN_TRY(hv_fix(ctx, (const char *)ctx->d_hv, ctx->heavy_slots, d_keys, d_vals, val_bytes, n));
    return KMAN_OK;
}

extern "C" int kman_dround_heavy(kman_ctx *ctx, uint32_t *n) {
    if (!ctx || !n) return KMAN_EINVAL;
    *n = ctx->heavy_keys;
    return KMAN_OK;
}

extern "C" int kman_dround_failed(kman_ctx *ctx, uint64_t *ranges, uint64_t cap, uint64_t *n) {
    if (!ctx || !n) return KMAN_EINVAL;
    *n = ctx->failed.size() / 2;
    if (!ranges) return KMAN_OK;
    if (cap < *n) return KMAN_ECAP;
    memcpy(ranges, ctx->failed.data(), ctx->failed.size() * 8);
    return KMAN_OK;
}

// region_finish.hip — the finish of the region path (region.h): rg_finish, one
// block per region, its launch ladder (item width, rank method, the early-count
// check) and the stamp report of the round finish.
#include "region.h"

#include <cstdio>
#include <cstdlib>

using namespace kman::region;

namespace {

constexpr int FT = 512;           // finish threads (more threads per region: 640 or 576 -- a second
                                  // block no longer fits the CU's SIMDs, 9.5 / 11.5 vs 5.7 ms; 768,
                                  // two blocks at 80 VGPRs -- 6.7 ms, the sort phase's barriers over
                                  // 12 waves cost more than the waves gain)
constexpr int FBITS = 9;          // finish LSD digit (26 bits: 3 passes)
constexpr int FRAD = 1 << FBITS;
constexpr int FWORD = FRAD / 2;   // per-wave counters: two u16 per word

// ---------------------------------------------------------------- finish
// One block per region r (regions in key order = grab order): LSD sort of the
// item bits [Q, Q + rest) in LDS (<= 9-bit digits, per-wave counters, stable),
// run-length pass, output compacted through one look-back over the regions.
// COUNT: okeys[j], ovals[j] = group size; UNIQ: keys of groups of one and
// their pos ((window << 1) | strand).
// T = uint32_t (count mode, rest <= 32 bits, no tag): items held as their key
// rest in 4 bytes, half the LDS (three blocks per CU); rows staged in two
// rounds (keys, then counts).
// CHK (uniq): the early row count (below) is checked against the rows the
// sorted keys give -- per thread, the singleton marks against heads & tails
// computed from the keys -- and a disagreement raises ERR_EARLY; CHK = 2 also
// flips one mark of region `hook` (a test of the check itself).  CHK = 0 with
// atomic ranks: the last pass moves the marked items only and its scatter is
// the compacted row list (COMPACT below).
enum { RG_COUNT = 1, RG_UNIQ = 2 };

// waves per SIMD the launch bounds ask for: 8-byte items of a GCAP region
// (40 KiB) and 4-byte items: three blocks per CU; 8-byte items of an FCAP
// region (68 KiB) and the ballot ranks (their registers): two
template <typename T, bool ATOMIC, int CAP>
constexpr int fin_waves() {
    // (4-byte items of a GCAP region, 28 KiB: four blocks per CU in 64
    // VGPRs, 6.46 vs 7.07 ms per 1 G k-mers at three)
    if (sizeof(T) == 4 && CAP <= GCAP) return 8;
    return sizeof(T) == 4 || (ATOMIC && CAP <= GCAP) ? 6 : 4;
}

template <int MODE, typename O, bool ATOMIC, typename T = uint64_t, int CHK = 0, int CAP = FCAP>
__global__ __launch_bounds__(FT, (fin_waves<T, ATOMIC, CAP>())) void rg_finish(
    const uint64_t *__restrict__ in, uint64_t C1, const uint32_t *__restrict__ cnt1, uint32_t Q, uint32_t rest,
    uint32_t rc, uint64_t rbase, uint32_t tag_shift, uint32_t fsub, uint64_t *__restrict__ okeys,
    O *__restrict__ ovals, uint64_t *__restrict__ status, uint32_t *__restrict__ counter, uint32_t epoch,
    uint32_t *__restrict__ err, uint32_t hook, uint64_t *__restrict__ stp, uint32_t nreg,
    uint8_t *__restrict__ freg, uint32_t in4) {
    constexpr int NT = FT, NW_ = NT / 64;
    constexpr int IPT = (CAP + NT - 1) / NT;  // items per thread
    constexpr bool NARROW = sizeof(T) == 4;
    static_assert(!NARROW || MODE == RG_COUNT, "narrow items: count mode");
    // PIPE: the rank atomics and slot reads of a pass issue back to back
    // (8-byte items of an FCAP region, 128 VGPRs).  The 80- and 64-VGPR
    // instances spill so: their ranks stay one round trip at a time and
    // their slot reads go four at a time (count finish 5.34 -> 5.27 ms);
    // the GCAP instance with 3 dwords of spills was no faster on the round
    // path (`r04q_ab.txt`)
    constexpr bool PIPE = ATOMIC && !NARROW && CAP == FCAP;
    static_assert(CHK == 0 || MODE == RG_UNIQ, "the early count is uniq's");
    __shared__ __attribute__((aligned(16))) T s[CAP];
    // per-wave digit counters, u16 pairs; words FWORD + lane: where the
    // lanes without an item add (so every rank atomic is unconditional).
    // TWO (4-byte count items, rest <= 21 bits: the round path's regions):
    // two passes instead of three -- the first by up to 11 bits on ONE
    // block-wide counter array (an LSD sort's first pass need not be stable),
    // the second by up to 10 bits on per-wave counters of 512 words
    constexpr bool TWO_OK = NARROW;
    // the two-pass scans cover their counter words with one word pair per
    // thread (first pass: <= 11 bits, 1024 words) and one word per thread
    // (second pass: <= 10 bits, 512 words)
    static_assert(!TWO_OK || (2 * NT >= 1024 && NT >= 512), "the two-pass finish needs >= 512 threads");
    constexpr uint32_t WSTR = TWO_OK ? 512 + 64 : FWORD + 64;
    __shared__ uint32_t wh[NW_][WSTR];
    __shared__ uint32_t lds_scan[NW_], lds_scan2[NW_];
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_out;

    const int t = threadIdx.x, lane = lane_id(), w = t >> 6;
    const uint64_t rmask = (1ull << rest) - 1;
    const uint32_t pw = (uint32_t)w * (IPT * 64) + (uint32_t)lane;  // wave-striped positions
    // region rr's size m0 (first sub-region) and m (0: emits nothing), and
    // its items into v (wave-striped positions)
    auto region_size = [&](uint32_t rr, uint32_t &m0_) -> uint32_t {
        m0_ = cnt1[(uint64_t)rr * fsub];
        const uint32_t m1_ = fsub > 1 ? cnt1[(uint64_t)rr * fsub + 1] : 0u;
        // freg (the round path): a region flagged by a pass (a sub-region
        // overflowed) or here (more than the LDS holds) emits nothing
        const uint32_t mm = m0_ + m1_;
        if (freg && freg[rr]) return 0u;  // (block-uniform)
        if (mm > (uint32_t)CAP) {
            if (t == 0) {
                atomicOr(err, ERR_REGION);  // (block-uniform) more than the LDS holds
                if (freg) freg[rr] = 1;
            }
            return 0u;
        }
        return mm;
    };
    auto load_items = [&](uint32_t rr, uint32_t m0_, uint32_t mm, T (&v)[IPT]) {
        // (a uniform base and one 32-bit offset per item: few address VGPRs)
        const uint32_t skip = (uint32_t)C1 - m0_;
        if (NARROW && in4) {  // (4-byte count items from the pass: rg_pass<.., uint32_t>)
            const uint32_t *src = reinterpret_cast<const uint32_t *>(in) + (uint64_t)rr * fsub * C1;
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t p = pw + i * 64;
                v[i] = p < mm ? (T)src[p < m0_ ? p : p + skip] : (T)0;
            }
            return;
        }
        const uint64_t *src = in + (uint64_t)rr * fsub * C1;
#pragma unroll
        for (int i = 0; i < IPT; i++) {
            const uint32_t p = pw + i * 64;
            v[i] = p < mm ? (T)src[p < m0_ ? p : p + skip] : (T)0;
        }
    };
    // NARROW (three blocks per CU): wave priority 2 while a region's loads and
    // row stores issue, 0 while it sorts, so the memory phases go ahead of
    // the other blocks' sorting (count finish 5.17 -> 5.08 ms; the uniq
    // instance, two blocks per CU, slows down with it: 5.29 vs 5.21,
    // `r04am_prio_ab.txt`)
    if (NARROW) __builtin_amdgcn_s_setprio(2);
    // one region per block.  (Persistent blocks that load the next region's
    // items into registers while this one is written: 15 vs 6 ms, spilled at
    // three blocks per CU; round 2's at two: 11.1 vs 5.7 ms.)
    if (t == 0) s_tile = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t r = __builtin_amdgcn_readfirstlane(s_tile);
    if (r >= nreg) return;
    uint32_t m0;
    const uint32_t m = region_size(r, m0);
    T x[IPT];
    load_items(r, m0, m, x);
    RSTAMP(r, 0);
    if (NARROW) __builtin_amdgcn_s_setprio(0);  // (the sort)
#ifdef KMAN_RG_STAMPS
    __builtin_amdgcn_s_waitcnt(0);  // (diagnostic build: phase 1 = the wait for the region's items)
    if (stp && t == 0) stp[(uint64_t)r * 16 + 15] = m;  // (the region's items, beside its phase stamps)
#endif
    RSTAMP(r, 1);

    // stable LSD passes of <= 9 bits.  Ranks: per-wave u16 counters packed two
    // to a word (a wave ranks <= 64 * IPT items), same-word LDS atomics of one
    // wave return in lane order (probed: ATOMIC), else ballot match-any.
    const bool two = TWO_OK && rest >= 2 && rest <= 21;
    // U32C (8-byte items of an FCAP region: the uniq finish): a block-wide
    // first pass of <= 11 bits, then 8-bit passes on u32 counters (below)
    constexpr bool U32C = PIPE;
    static_assert(!U32C || (NW_ * (FWORD + 64) >= 2048 + 64 && FWORD + 64 >= 256 + 64), "u32 counters fit wh");
    static_assert(!U32C || NT * IPT <= CAP, "an item past m writes its own position");
    const uint32_t np = two ? 2u : U32C ? (rest <= 11 ? 1u : 1u + (rest - 11 + 7) / 8) : (rest + FBITS - 1) / FBITS;
    const uint32_t bw_two = rest / 2;  // (two: the stable second pass's bits, <= 10)
    // EARLY (uniq): the region's row count is found after the second-to-last
    // pass, when equal keys already share a run of equal low bits (a run of
    // one item almost always), and published then, so the look-back after the
    // last pass finds its predecessors' counts in place instead of waiting
    // for the slowest region in flight (1.0 of 5.8 ms).  A singleton's mark
    // rides in item bit 63 (above the key rest and the pos: the top bit of the
    // pass-1 digit, constant in a region and never read here, so it is
    // overwritten) through the last pass.
    constexpr uint64_t MARK = 1ull << 63;
    // (the round path's items carry the source rank in the 9 bits at
    // tag_shift, read as 8 bits below: bit 63 is free there as well)
    const bool early = MODE == RG_UNIQ && (!tag_shift || tag_shift + 8 <= 63) && np >= 2;
    // COMPACT (the plain uniq finish with atomic ranks): which items are rows
    // and how many is settled by early_marks() before the last pass, so that
    // pass ranks and scatters the marked items only -- the marked keys are
    // distinct, the pass is stable and the earlier passes ordered the low
    // bits -- and leaves s[0, etot) holding the region's rows compacted in key
    // order: no run-length pass, no offset scan, no staging, and the look-back
    // runs inside the pass (compact_lookback).  The checked instances sort every
    // item and compare the marks with the rows the sorted keys give; a call
    // where `early` does not hold takes the run-length pass here as well.
    constexpr bool COMPACT = MODE == RG_UNIQ && CHK == 0 && ATOMIC && !NARROW;
    uint32_t etot = 0;
    uint32_t at = 0;
    uint32_t p0 = 0;
    if constexpr (TWO_OK) {
        if (two) {
            // the first pass, by the low rest - bw_two bits on one block-wide
            // counter array (u16 pairs; the waves' adds interleave, so the
            // pass is not stable, which a first LSD pass need not be)
            uint32_t *const flat = &wh[0][0];
            const uint32_t bw = rest - bw_two, dm = (1u << bw) - 1, nwd = 1u << (bw - 1);
            for (uint32_t q = t; q < nwd; q += NT) flat[q] = 0;
            __syncthreads();
            uint32_t rk[IPT];
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t d = (uint32_t)(x[i] >> Q) & dm, hs = (d & 1u) * 16u;
                rk[i] = pw + i * 64 < m ? (atomicAdd(&flat[d >> 1], 1u << hs) >> hs) & 0xffffu : 0u;
            }
            __syncthreads();
            {
                // thread t: words 2t, 2t+1 (digits 4t .. 4t+3) -> their starts
                // (the scan's barrier orders every word read before the writes)
                const uint32_t c0 = 2 * t < nwd ? flat[2 * t] : 0u, c1 = 2 * t + 1 < nwd ? flat[2 * t + 1] : 0u;
                const uint32_t a0 = c0 & 0xffffu, a1 = c0 >> 16, a2 = c1 & 0xffffu, a3 = c1 >> 16;
                const uint32_t ls =
                    block_exclusive_scan1<NT>(a0 + a1 + a2 + a3, SumU32(), 0u, lds_scan, (uint32_t *)nullptr);
                if (2 * t < nwd) flat[2 * t] = ls | ((ls + a0) << 16);
                if (2 * t + 1 < nwd) flat[2 * t + 1] = (ls + a0 + a1) | ((ls + a0 + a1 + a2) << 16);
            }
            __syncthreads();
#pragma unroll
            for (int i0 = 0; i0 < IPT; i0 += 4) {
                uint32_t sl[4];
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++) {
                    const uint32_t d = (uint32_t)(x[i] >> Q) & dm;
                    sl[i - i0] = ((flat[d >> 1] >> ((d & 1u) * 16u)) & 0xffffu) + rk[i];
                }
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++)
                    if (pw + i * 64 < m) s[sl[i - i0]] = x[i];
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (pw + i * 64 < m) x[i] = s[pw + i * 64];
            at = bw;
            p0 = 1;
        }
    }
    // EARLY's marks, after the second-to-last pass (items sorted by their low
    // `at` rest bits, wave-striped in x)
    auto early_marks = [&]() {
            // The items are sorted by their low `at` rest bits, and x holds
            // them wave-striped (item (i, lane) at position pw + i * 64), so a
            // neighbour in position is a neighbouring lane (DPP) or the next /
            // previous row's edge lane (readlane); only the wave's two edges
            // come from LDS.  A key is a singleton iff no item of its run of
            // equal low bits has its whole rest: runs of one or two decide
            // from the neighbours, the rare runs of three or more scan LDS.
            const uint64_t lm = ((1ull << at) - 1) << Q, km = rmask << Q;
            const uint32_t wb = (uint32_t)w * (IPT * 64), we = wb + IPT * 64;
            auto rl64 = [](uint64_t v, int l) -> uint64_t {
                return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), l) << 32) |
                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
            };
            auto eq = [](uint64_t a, uint64_t b, uint64_t mask) { return !((a ^ b) & mask); };
            // the wave's edges: positions wb - 2, wb - 1 and we, we + 1
            const uint64_t eL = wb >= 1 && wb - 1 < m ? (uint64_t)s[wb - 1] : 0;
            const uint64_t eLL = wb >= 2 && wb - 2 < m ? (uint64_t)s[wb - 2] : 0;
            const uint64_t eR = we < m ? (uint64_t)s[we] : 0;
            const uint64_t eRR = we + 1 < m ? (uint64_t)s[we + 1] : 0;
            // LE / FE bit i: item (i, lane) has the low bits / the whole rest
            // of its left neighbour (position - 1)
            uint32_t LE = 0, FE = 0, V = 0;
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t pos = pw + i * 64;
                const uint64_t v = x[i];
                const uint64_t left = wave_shr1(v, i ? rl64(x[i - 1], 63) : eL);
                const bool ok = pos < m && pos > 0;
                const bool le = ok && eq(left, v, lm);
                LE |= (uint32_t)le << i;
                FE |= (uint32_t)(le && eq(left, v, km)) << i;
                V |= (uint32_t)(pos < m) << i;
            }
            // the same of position + 1 (RE, RF), of position - 1 (LL) and of
            // position + 2 (RR): lane shifts, rows carried through lanes 0 / 63
            const uint64_t vlast = rl64(x[IPT - 1], 63);
            const bool eRle = we < m && eq(eR, vlast, lm), eRfe = eRle && eq(eR, vlast, km);
            const bool eRRle = we + 1 < m && eq(eRR, eR, lm);
            const bool eLle = wb >= 2 && wb - 1 < m && eq(eL, eLL, lm);
            const uint32_t top = 1u << (IPT - 1);
            const uint32_t RE = wave_shl1(LE, ((uint32_t)__builtin_amdgcn_readlane((int)LE, 0) >> 1) | (eRle ? top : 0u));
            const uint32_t RF = wave_shl1(FE, ((uint32_t)__builtin_amdgcn_readlane((int)FE, 0) >> 1) | (eRfe ? top : 0u));
            const uint32_t LL = wave_shr1(LE, ((uint32_t)__builtin_amdgcn_readlane((int)LE, 63) << 1) | (eLle ? 1u : 0u));
            const uint32_t RR = wave_shl1(RE, ((uint32_t)__builtin_amdgcn_readlane((int)RE, 0) >> 1) | (eRRle ? top : 0u));
            const uint32_t lng = ((LE & RE) | (LE & LL) | (RE & RR)) & V;  // in a run of three or more
            uint32_t S = V & ~FE & ~RF & ~lng;
            for (uint32_t sl = lng; sl;) {  // (rare: the exact scan over the run in LDS)
                const int i = __ffs(sl) - 1;
                sl &= sl - 1;
                const uint32_t q = pw + (uint32_t)i * 64;
                const uint64_t v = s[q];
                bool single = true;
                for (uint32_t a2 = q; single && a2 > 0;) {
                    const uint64_t u = s[--a2];
                    if (!eq(u, v, lm)) break;
                    if (eq(u, v, km)) single = false;
                }
                for (uint32_t a2 = q + 1; single && a2 < m; a2++) {
                    const uint64_t u = s[a2];
                    if (!eq(u, v, lm)) break;
                    if (eq(u, v, km)) single = false;
                }
                S |= (uint32_t)single << i;
            }
            if (CHK == 2 && r == hook && t == 0) S ^= 1u;  // (the check's own test: one wrong mark)
            // (bit 63 is the top bit of the region's pass-1 digit before it
            // becomes the mark: set or cleared on every item)
#pragma unroll
            for (int i = 0; i < IPT; i++) x[i] = (x[i] & ~(T)MARK) | (((S >> i) & 1u) ? (T)MARK : (T)0);
            (void)block_exclusive_scan1<NT>((uint32_t)__popc(S), SumU32(), 0u, lds_scan2, &etot);
            if (t == 0) publish_agg<0>(status, r, etot, epoch);
    };
    // item i of the thread takes part in a pass: inside the region, and in the
    // compacting last pass (cp) marked (an item past m holds 0: no mark)
    auto live = [&](int i, bool cp) -> bool {
        if constexpr (COMPACT) {
            if (cp) return (int32_t)((uint64_t)x[i] >> 32) < 0;
        }
        return pw + i * 64 < m;
    };
    // the compacting pass's look-back: the rows will be s[0, etot), and the
    // region's predecessors published their counts a pass ago, so the last
    // wave (the one with the fewest items: a region fills 7 of its 8 waves
    // and a little) looks back once the digit starts are in place, while the
    // other waves read their slots and scatter; the pass's last barrier
    // publishes s_out.  (By wave 0 after its scatter, every wave waiting at
    // that barrier for the status loads: finish 5.03-5.04 vs 4.91-4.95 ms,
    // `finish_compact_ab.txt`)
    auto compact_lookback = [&]() {
        if (w == NW_ - 1) {
            const uint64_t ob = wave_lookback_published<0>(status, r, etot, epoch, err);
            if (lane == 0) s_out = ob;
        }
    };
    if constexpr (U32C) {
        // the 8-byte-item finish: a first pass by up to 11 bits on ONE
        // block-wide array of u32 counters (unstable, as a first LSD pass may
        // be), then stable passes of <= 8 bits on per-wave u32 counters (256
        // words: no u16 halves to shift in and out); every item's LDS write
        // and read unconditional (an item past m writes its own position,
        // >= m, so no branch per item)
        uint32_t *const flat = &wh[0][0];
        for (uint32_t p = 0; p < np; p++) {
            const bool blk = p == 0;
            const bool cp = COMPACT && early && p + 1 == np;  // (block-uniform)
            const uint32_t bw = blk ? rest - 8 * (np - 1) : 8u;
            const uint32_t sh = Q + at, dm = (1u << bw) - 1;
            at += bw;
            const uint32_t nd = 1u << bw;  // counters of the array
            uint32_t *const wc = blk ? flat : &wh[w][0];
            if (blk) {
                for (uint32_t q = t; q < nd; q += NT) flat[q] = 0;
                __syncthreads();
            } else {
#pragma unroll
                for (int q = 0; q < 256 / 64; q++) wc[lane + 64 * q] = 0;
                __builtin_amdgcn_wave_barrier();
            }
            uint32_t rk[IPT];
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const bool valid = live(i, cp);
                const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
                rk[i] = atomicAdd(&wc[valid ? d : nd + lane], 1u);
            }
            __syncthreads();
            if (blk) {
                // thread t: counters [t * cp, (t + 1) * cp), cp = nd / NT (<= 4)
                const uint32_t cp = nd > (uint32_t)NT ? nd / NT : 1u;
                uint32_t c[4] = {0, 0, 0, 0};
                const uint32_t b0 = t * cp;
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (q < cp && b0 + q < nd) c[q] = flat[b0 + q];
                uint32_t run = block_exclusive_scan1<NT>(c[0] + c[1] + c[2] + c[3], SumU32(), 0u, lds_scan,
                                                         (uint32_t *)nullptr);
#pragma unroll
                for (uint32_t q = 0; q < 4; q++)
                    if (q < cp && b0 + q < nd) flat[b0 + q] = run, run += c[q];
            } else {
                // thread t < 256: digit t -> its total over the waves, block
                // scan -> digit start, each wave's first slot in place
                uint32_t cw[NW_], tot = 0;
                if (t < 256) {
#pragma unroll
                    for (int ww = 0; ww < NW_; ww++) tot += (cw[ww] = wh[ww][t]);
                }
                uint32_t run = block_exclusive_scan1<NT>(t < 256 ? tot : 0u, SumU32(), 0u, lds_scan,
                                                         (uint32_t *)nullptr);
                if (t < 256) {
#pragma unroll
                    for (int ww = 0; ww < NW_; ww++) wh[ww][t] = run, run += cw[ww];
                }
            }
            __syncthreads();
            if (cp) compact_lookback();
#pragma unroll
            for (int i = 0; i < IPT; i++) rk[i] += wc[(uint32_t)(x[i] >> sh) & dm];
            // (only the items: the slot grid past m is 12-14 % of a region's
            // LDS, and writing it unconditionally cost more LDS cycles than
            // the branches: 5.72 vs 5.21 ms, `r06e`)
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (live(i, cp)) s[rk[i]] = x[i];
            __syncthreads();
            if (p + 1 < np) {
#pragma unroll
                for (int i = 0; i < IPT; i++)
                    if (pw + i * 64 < m) x[i] = s[pw + i * 64];
            }
            if (early && p + 2 == np) early_marks();
        }
    }
    if constexpr (!U32C)
    for (uint32_t p = p0; p < np; p++) {
        const uint32_t bw = two ? bw_two : (rest - at + (np - p) - 1) / (np - p);
        const uint32_t sh = Q + at, dm = (1u << bw) - 1;
        at += bw;
        const bool cp = COMPACT && early && p + 1 == np;  // (block-uniform)
        // (two: the second pass's per-wave counters, 2^(bw - 1) <= 512 words)
        const uint32_t nwd = two ? 1u << (bw - 1) : (uint32_t)FWORD;
        if (TWO_OK && two) {
            for (uint32_t q = lane; q < nwd; q += 64) wh[w][q] = 0;
        } else {
#pragma unroll
            for (int q = 0; q < FWORD / 64; q++) wh[w][lane + 64 * q] = 0;
        }
        __builtin_amdgcn_wave_barrier();
        uint32_t rk[IPT];
#pragma unroll
        for (int i = 0; i < IPT; i++) {
            const bool valid = live(i, cp);
            const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
            const uint32_t hs = (d & 1u) * 16u;
            if (PIPE) {
                // (no branch around the atomic: in a branch its return is
                // waited for before the next item's atomic issues, 17 LDS
                // round trips in a row per pass)
                rk[i] = (atomicAdd(&wh[w][valid ? d >> 1 : (uint32_t)FWORD + lane], 1u << hs) >> hs) & 0xffffu;
            } else if (ATOMIC) {
                rk[i] = valid ? (atomicAdd(&wh[w][d >> 1], 1u << hs) >> hs) & 0xffffu : 0u;
            } else {
                uint64_t peers = __ballot(valid);
                for (uint32_t bb = 0; bb < bw; bb++) {
                    const bool set = (d >> bb) & 1u;
                    const uint64_t mm = __ballot(set);
                    peers &= set ? mm : ~mm;
                }
                const uint32_t before = valid ? (wh[w][d >> 1] >> hs) & 0xffffu : 0u;
                rk[i] = before + (uint32_t)__popcll(peers & lanemask_lt());
                __builtin_amdgcn_wave_barrier();
                const int leader = __ffsll((unsigned long long)peers) - 1;
                if (valid && lane == leader) atomicAdd(&wh[w][d >> 1], (uint32_t)__popcll(peers) << hs);
                __builtin_amdgcn_wave_barrier();
            }
        }
        __syncthreads();
        {
            // thread t < words: digits 2t, 2t+1 -> their totals, block scan
            // of the totals -> digit starts, then each wave's first slot per
            // digit (digit start + the earlier waves' counts, < 2^16) in place
            // of its counters, so the scatter reads one word per item
            const uint32_t nw_ = nwd;
            uint32_t tlo = 0, thi = 0, cw[NW_];
            if (t < nw_) {
#pragma unroll
                for (int ww = 0; ww < NW_; ww++) {
                    cw[ww] = wh[ww][t];
                    tlo += cw[ww] & 0xffffu;
                    thi += cw[ww] >> 16;
                }
            }
            const uint32_t ls = block_exclusive_scan1<NT>(tlo + thi, SumU32(), 0u, lds_scan, (uint32_t *)nullptr);
            if (t < nw_) {
                uint32_t plo = ls, phi = ls + tlo;
#pragma unroll
                for (int ww = 0; ww < NW_; ww++) {
                    wh[ww][t] = plo | (phi << 16);
                    plo += cw[ww] & 0xffffu;
                    phi += cw[ww] >> 16;
                }
            }
        }
        __syncthreads();
        if (PIPE) {
            // every item's slot first (unconditional reads, issued back to
            // back; an item past m reads a slot it does not use), then the
            // writes
#pragma unroll
            for (int i = 0; i < IPT; i++) {
                const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
                rk[i] += (wh[w][d >> 1] >> ((d & 1u) * 16u)) & 0xffffu;
            }
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (live(i, cp)) s[rk[i]] = x[i];
        } else {
#pragma unroll
            for (int i0 = 0; i0 < IPT; i0 += 4) {
                uint32_t sl[4];
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++) {
                    const uint32_t d = (uint32_t)(x[i] >> sh) & dm;
                    sl[i - i0] = ((wh[w][d >> 1] >> ((d & 1u) * 16u)) & 0xffffu) + rk[i];
                }
#pragma unroll
                for (int i = i0; i < i0 + 4 && i < IPT; i++)
                    if (live(i, cp)) s[sl[i - i0]] = x[i];
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // (after the scatter here: ahead of it the 80-VGPR instance spills)
        if (cp) compact_lookback();
        __syncthreads();
        if (p + 1 < np) {
#pragma unroll
            for (int i = 0; i < IPT; i++)
                if (pw + i * 64 < m) x[i] = s[pw + i * 64];
        }
        if (early && p + 2 == np) early_marks();
    }
    if (np == 0) {
#pragma unroll
        for (int i = 0; i < IPT; i++)
            if (pw + i * 64 < m) s[pw + i * 64] = x[i];
        __syncthreads();
    }

    RSTAMP(r, 2);
    // the compacting last pass ran: the rows are in place and counted
    const bool compacted = COMPACT && early;  // (block-uniform)
    // ---- run-length pass (thread t: sorted positions t*IPT ..)
    const uint32_t q0 = (uint32_t)t * IPT;
    uint32_t heads = 0, tails = 0, emit = 0, lh_before = 0, off = 0;
    // (compacted: etot, the same in every thread -- block_exclusive_scan1
    // hands each thread the sum of all the waves' totals)
    uint32_t total = etot;
#define RKEY(v) (((v) >> Q) & rmask)
    T kv[IPT];
    // the emitted rows compacted in LDS as one word each: the item itself
    // (UNIQ: key rest + pos) or key rest | group size << rest (COUNT); every
    // read of s above came before the scan's barriers.  NARROW: the key
    // rests, then (after they are written) the group sizes
    auto stage = [&](bool sizes) {
        uint32_t o = off, cur = lh_before;  // head position + 1 of the open group
#pragma unroll
        for (int j = 0; j < IPT; j++) {
            const uint32_t q = q0 + j;
            if (MODE != RG_UNIQ && ((heads >> j) & 1u)) cur = q + 1;
            if ((emit >> j) & 1u) {
                if constexpr (NARROW)
                    s[o++] = sizes ? (T)(q + 2 - cur) : kv[j];
                else
                    s[o++] = MODE == RG_UNIQ ? kv[j] : (T)(RKEY(kv[j]) | ((uint64_t)(q + 2 - cur) << rest));
            }
        }
    };
    if (!compacted) {
#pragma unroll
        for (int j = 0; j < IPT; j++) kv[j] = q0 + j < m ? s[q0 + j] : 0;
        // (a COMPACT instance comes here without the early count only)
        if (!COMPACT && early) {
            // the early count's marks are the rows (heads & tails below)
            uint32_t marks = 0;
#pragma unroll
            for (int j = 0; j < IPT; j++) marks |= (uint32_t)(q0 + j < m && ((uint64_t)kv[j] & MARK)) << j;
            heads = tails = marks;
            if (CHK) {
                // the rows the sorted keys give: a singleton differs from both
                // neighbours in its whole rest
                uint32_t single = 0;
                const uint64_t kl = q0 > 0 && q0 - 1 < m ? RKEY((uint64_t)s[q0 - 1]) : ~0ull;
                const uint64_t kr = q0 + IPT < m ? RKEY((uint64_t)s[q0 + IPT]) : ~0ull;
#pragma unroll
                for (int j = 0; j < IPT; j++) {
                    const uint32_t q = q0 + j;
                    const uint64_t kq = RKEY((uint64_t)kv[j]);
                    const bool h = q == 0 || kq != (j ? RKEY((uint64_t)kv[j - 1]) : kl);
                    const bool e = q + 1 == m || kq != (j + 1 < IPT ? RKEY((uint64_t)kv[j + 1]) : kr);
                    single |= (uint32_t)(q < m && h && e) << j;
                }
                if (single != marks) atomicOr(err, ERR_EARLY);
            }
        } else {
#pragma unroll
            for (int j = 0; j < IPT; j++) {
                const uint32_t q = q0 + j;
                if (q < m) {
                    const uint64_t kq = RKEY(kv[j]);
                    const bool h = q == 0 || kq != RKEY(j ? kv[j - 1] : s[q - 1]);
                    const bool e = q + 1 == m || kq != RKEY(j + 1 < IPT ? kv[j + 1] : s[q + 1]);
                    heads |= (uint32_t)h << j;
                    tails |= (uint32_t)e << j;
                }
            }
        }
        if constexpr (MODE == RG_UNIQ) {
            emit = heads & tails;
        } else {
            emit = tails;
            const uint32_t lh = heads ? q0 + (31 - __clz(heads)) + 1 : 0u;
            lh_before = block_exclusive_scan1<NT>(
                lh, [](uint32_t a, uint32_t b) { return a > b ? a : b; }, 0u, lds_scan2, (uint32_t *)nullptr);
        }
        const uint32_t ne = (uint32_t)__popc(emit);
        // (its barrier orders every read of s above before the staging writes below)
        off = block_exclusive_scan1<NT>(ne, SumU32(), 0u, lds_scan, &total);
        // ERR_EARLY, the published count is not the rows': raised by the
        // checked instances only -- a COMPACT instance has no second count to
        // compare with, its rows ARE the marked items (total = etot above)
        if (!COMPACT && early && t == 0 && total != etot) atomicOr(err, ERR_EARLY);
        RSTAMP(r, 3);
        if (w == 0) {
            const uint64_t ob = !COMPACT && early ? wave_lookback_published<0>(status, r, total, epoch, err)
                                                  : wave_lookback<0>(status, r, total, epoch, err);
            if (lane == 0) s_out = ob;
        }
        stage(false);
        __syncthreads();
    } else {
        RSTAMP(r, 3);
    }
    RSTAMP(r, 4);
    if (NARROW) __builtin_amdgcn_s_setprio(2);  // (the row stores)
    const uint64_t ob = s_out;
    // the rows leave with non-temporal stores (a stream of GBs that no cache
    // keeps until it is read): 5.52-5.58 vs 5.58-5.62 ms (`r04k_nt_ab.txt`;
    // on the passes' scattered line stores they lose L2's write combining:
    // rg_pass 6.3-8.0 vs 3.5 ms)
    const uint64_t qmask = Q ? ((1ull << Q) - 1) : 0ull;
    // OB rows per trip, their LDS reads first, back to back (rows outside
    // the region's read slot 0 and are not written).  Lane l of a wave
    // writes a global row = l mod 64 (the region's first row shifted by
    // ob % 64), so a wave's store covers whole 128-byte lines: non-temporal
    // stores of part lines are not merged in L2 (finish writes 12.35 GB per
    // launch unaligned, 11.74 aligned, `r04s_ab.txt`; same time)
    const uint32_t mis = (uint32_t)(ob & 63);
    constexpr uint32_t OB = 4;
    auto each_row = [&](auto &&put) {
        for (uint32_t q0 = t; q0 < total + mis; q0 += OB * NT) {
            uint64_t v4[OB];
#pragma unroll
            for (uint32_t u = 0; u < OB; u++) {
                const uint32_t q = q0 + u * NT - mis;
                v4[u] = (uint64_t)s[q < total ? q : 0u];
            }
#pragma unroll
            for (uint32_t u = 0; u < OB; u++) {
                const uint32_t q = q0 + u * NT - mis;
                if (q < total) put(q, v4[u]);
            }
        }
    };
    auto put_key = [&](uint32_t q, uint64_t v) {
        __builtin_nontemporal_store(((uint64_t)(r + rbase) << rest) | RKEY(v), okeys + ob + q);
    };
    auto put_val = [&](uint32_t q, uint64_t v) {
        if constexpr (MODE == RG_UNIQ) {
            const uint64_t idx = v & qmask;
            const uint64_t pos = rc ? idx : (idx << 1);
            // N > 1: the source rank (tagged into the item by the pass after
            // the exchange) in bits 56-63, as DistPipeline's payloads
            // (ranks < 256: 8 tag bits, so bit 63 -- the early count's mark -- is not read)
            __builtin_nontemporal_store((O)(tag_shift ? pos | (((v >> tag_shift) & 0xffull) << 56) : pos), ovals + ob + q);
        } else if constexpr (NARROW) {
            __builtin_nontemporal_store((O)v, ovals + ob + q);
        } else {
            __builtin_nontemporal_store((O)(v >> rest), ovals + ob + q);
        }
    };
    if constexpr (MODE == RG_UNIQ && CHK == 0) {
        // a uniq row is read once for its key and its pos: global row ob + q
        // of lane 0 is a multiple of 64 in both streams, so the 4- or 8-byte
        // pos stores of a wave cover whole lines as the key stores do
        each_row([&](uint32_t q, uint64_t v) {
            put_key(q, v);
            put_val(q, v);
        });
    } else {
        each_row(put_key);
        if constexpr (NARROW) {
            __syncthreads();  // (every key read before the sizes overwrite them)
            stage(true);
            __syncthreads();
        }
        each_row(put_val);
    }
#undef RKEY
    RSTAMP(r, 5);
}

template <int MODE, typename O, int CAP, bool ATOMIC, typename T = uint64_t, int CHK = 0>
void launch_finish_as(kman_ctx *ctx, const FinishArgs &f, uint64_t *okeys, void *ovals, uint32_t epoch,
                      uint32_t *counter, uint32_t hook, uint64_t *stp) {
    hipLaunchKernelGGL((rg_finish<MODE, O, ATOMIC, T, CHK, CAP>), dim3(f.nreg), dim3(FT), 0, ctx->stream, f.in, f.C1,
                       f.cnt, f.Q, f.rest, f.rc, f.rbase, f.tag_shift, f.fsub, okeys, (O *)ovals, ctx->d_status,
                       counter, epoch, ctx->d_err, hook, stp, f.nreg, f.freg, (uint32_t)f.in4);
}

// The early-count check of the uniq finish (rg_finish CHK): KMAN_RG_CHECK=1
// (or "hook=<region>": also one wrong mark in that region, the check's own
// GPU test) selects the checked kernel; 0 / unset, the plain one.
struct EarlyCheck {
    int chk;
    uint32_t hook;
};
EarlyCheck early_check() {
    const char *e = getenv("KMAN_RG_CHECK");
    if (!e || !*e || !strcmp(e, "0")) return {0, ~0u};
    if (!strncmp(e, "hook=", 5)) return {2, (uint32_t)strtoul(e + 5, nullptr, 10)};
    return {1, ~0u};
}

// one block per region; count rows whose key rest fits 32 bits hold 4-byte
// items in LDS (three blocks per CU: count finish 5.95 -> 5.68 ms, config-4
// shard 84.7 -> 78.3 ms).  Without the probed lane-ordered LDS atomics the
// ranks are ballots (8-byte items: the ballot ranks overflow the 80 VGPRs of
// three blocks per CU -- 2.5 KB of spills per lane -- so no narrow variant).
template <int MODE, typename O, int CAP>
void launch_finish(kman_ctx *ctx, const FinishArgs &f, uint64_t *okeys, void *ovals, uint32_t epoch,
                   uint32_t *counter, uint64_t *stp) {
    if constexpr (MODE == RG_COUNT) {
        if (narrow_ok(ctx, KMAN_FINISH_COUNT, f.Q, f.rest, f.tag_shift)) {
            launch_finish_as<MODE, O, CAP, true, uint32_t>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
            return;
        }
    }
    if (!ctx->lds_atomic_ordered) {
        launch_finish_as<MODE, O, CAP, false>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
        return;
    }
    if constexpr (MODE == RG_UNIQ) {
        const EarlyCheck ck = early_check();
        if (ck.chk == 1) {
            launch_finish_as<MODE, O, CAP, true, uint64_t, 1>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
            return;
        }
        if (ck.chk == 2) {
            launch_finish_as<MODE, O, CAP, true, uint64_t, 2>(ctx, f, okeys, ovals, epoch, counter, ck.hook, stp);
            return;
        }
    }
    launch_finish_as<MODE, O, CAP, true>(ctx, f, okeys, ovals, epoch, counter, ~0u, stp);
}

template <int CAP>
void launch_finish_cap(kman_ctx *ctx, const FinishArgs &f, int mode, uint64_t *okeys, void *ovals,
                       uint32_t oval_bytes, uint32_t epoch, uint32_t *counter, uint64_t *stp) {
    if (mode == KMAN_FINISH_UNIQ) {
        if (oval_bytes == 4) launch_finish<RG_UNIQ, uint32_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
        else launch_finish<RG_UNIQ, uint64_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
    } else {
        if (oval_bytes == 4) launch_finish<RG_COUNT, uint32_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
        else launch_finish<RG_COUNT, uint64_t, CAP>(ctx, f, okeys, ovals, epoch, counter, stp);
    }
}

}  // namespace

// the narrow (4-byte) count finish's condition -- also when the pass before
// it writes 4-byte items (FinishArgs::in4)
bool kman::region::narrow_ok(const kman_ctx *ctx, int mode, uint32_t Q, uint32_t rest, uint32_t tag_shift) {
    return mode == KMAN_FINISH_COUNT && ctx->lds_atomic_ordered && rest <= 32 && Q == 0 && tag_shift == 0;
}

int kman::region::run_finish(kman_ctx *ctx, const FinishArgs &f, int mode, uint64_t *okeys, void *ovals,
                             uint32_t oval_bytes, uint64_t *stp) {
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, f.nreg + 1, &epoch, &counter));
    KTimer kt_(ctx, "region_finish");
    if (f.cap == GCAP) launch_finish_cap<GCAP>(ctx, f, mode, okeys, ovals, oval_bytes, epoch, counter, stp);
    else launch_finish_cap<FCAP>(ctx, f, mode, okeys, ovals, oval_bytes, epoch, counter, stp);
    HIP_TRY(ctx, hipGetLastError());
    return KMAN_OK;
}

// the round finish's regions (KMAN_RG_STAMPS diagnostic build): mean phases,
// the spread of per-region times and of the look-back wait, by region size
int kman::region::report_finish_stamps(kman_ctx *ctx, uint64_t *st, uint64_t nreg) {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> h(nreg * 16);
    HIP_TRY(ctx, hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipFree(st));
    std::vector<double> tot, wait;
    double ph[7] = {0}, sz_t[4] = {0};
    uint64_t n = 0, sz_n[4] = {0}, t0 = ~0ull, t1 = 0;
    for (uint64_t r = 0; r < nreg; r++) {
        const uint64_t *x = &h[r * 16];
        if (!x[0] || !x[5]) continue;
        t0 = x[0] < t0 ? x[0] : t0;
        t1 = x[5] > t1 ? x[5] : t1;
        for (int i = 1; i < 6; i++) ph[i] += (double)(x[i] - x[i - 1]) / 100.0;
        tot.push_back((double)(x[5] - x[0]) / 100.0);
        wait.push_back((double)(x[4] - x[3]) / 100.0);
        const int b = x[15] < 2048 ? 0 : x[15] < 4096 ? 1 : x[15] < 6144 ? 2 : 3;
        sz_t[b] += tot.back();
        sz_n[b]++;
        n++;
    }
    if (!n) return KMAN_OK;
    auto pct = [](std::vector<double> v, double q) {
        std::sort(v.begin(), v.end());
        return v[(size_t)(q * (double)(v.size() - 1))];
    };
    fprintf(stderr, "stamps round finish: regions %llu span %.1f us  mean us/region %.2f  phases:",
            (unsigned long long)n, (double)(t1 - t0) / 100.0, pct(tot, 0.5));
    for (int i = 1; i < 6; i++) fprintf(stderr, " %d:%.2f", i, ph[i] / (double)n);
    fprintf(stderr, "\n  total p50 %.2f p90 %.2f p99 %.2f max %.2f | look-back wait p50 %.2f p90 %.2f p99 %.2f max %.2f\n",
            pct(tot, 0.5), pct(tot, 0.9), pct(tot, 0.99), pct(tot, 1.0), pct(wait, 0.5), pct(wait, 0.9),
            pct(wait, 0.99), pct(wait, 1.0));
    fprintf(stderr, "  mean us by items <2K %.2f (%llu) <4K %.2f (%llu) <6K %.2f (%llu) >=6K %.2f (%llu)\n",
            sz_n[0] ? sz_t[0] / sz_n[0] : 0.0, (unsigned long long)sz_n[0], sz_n[1] ? sz_t[1] / sz_n[1] : 0.0,
            (unsigned long long)sz_n[1], sz_n[2] ? sz_t[2] / sz_n[2] : 0.0, (unsigned long long)sz_n[2],
            sz_n[3] ? sz_t[3] / sz_n[3] : 0.0, (unsigned long long)sz_n[3]);
    return KMAN_OK;
}

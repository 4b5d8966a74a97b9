// gram.hip — all-pairs shared rows of a coloured table: the Gram matrix of the
// bit matrix whose rows are the table's u64 masks (engine.color_table).
//   G[i][j]     rows whose mask has bits i and j
//   occ[p]      rows whose mask has p bits
//   private[c]  rows whose mask is 1 << c
// all for masks cut to their bits < n_colors.
//
// The work per row does not depend on the row's bits.  A wave takes 64 rows per
// step, one mask per lane (lanes past n hold 0), and turns them by 90 degrees:
//   columns   col_c = __ballot(bit c of the lane's mask), c < n_colors: the 64
//             rows' bit c as one 64-bit word.  The ballot is wave-uniform; lane
//             c alone keeps it (two v_cndmask), so after the loop lane c
//             HOLDS col_c (lanes >= n_colors hold 0).  Sixty-four
//             column words would be 128 SGPRs: they are never kept scalar.
//   LDS       every lane parks its column in the wave's own slice, twice:
//             slice[c] and slice[n_colors + c] (GSLICE = 128 words, 1 KiB per
//             wave), so that column (c + d) mod n_colors is slice[c + d] and a
//             read needs no wrap.
//   pairs     the unordered pairs {i, j} are walked along the diagonals of the
//             circulant: in round d = 0 .. n_colors / 2, lane i < n_colors owns
//             the pair (i, (i + d) mod n_colors) and adds
//             popcount(col_i & slice[i + d]) to its register acc[d]: one LDS
//             read, two ANDs and two v_bcnt per pair, col_i from the lane's own
//             registers.  Every pair occurs once (d = 0 is the diagonal of G);
//             for an even n_colors the last round holds each pair twice and only
//             the lanes i < n_colors / 2 flush it.  GROUNDS = 33 rounds of 64
//             lanes cover the 2080 pairs of 64 colours.
//   occ       seven ballots of the bits of popcount(mask) (0..64) give seven
//             planes; lane p < 64 ANDs plane k or its complement, by bit k of p,
//             into the rows with exactly p bits, cut to the rows < n.  64 bits
//             (n_colors == 64 only) is plane 6 itself, counted wave-uniformly.
//   private   popcount(col_c & ballot(popcount(mask) == 1)) in lane c.
// The next step's mask is loaded before the current one is reduced.
//
// Accumulators are 32-bit: a step adds at most 64 to each, a wave of a full
// grid runs at most ceil(n / GSTRIDE) steps, and the call refuses n > 2^40
// (KMAN_GRAM_MAX_ROWS), so a wave's sum stays below 64 * 2^22 = 2^28 and a
// block's (four waves, added in LDS) below 2^30.  They are flushed ONCE per
// block: every wave adds its registers into the block's LDS table (distinct
// addresses within a wave), and after a barrier each nonzero entry is one
// 64-bit atomicAdd to G[i][j], one more to G[j][i] when i != j, to occ[p] or to
// private[c].  Integer adds commute: two identical calls give identical bytes.
//
// Grid: min(KMAN_GRAM_MAX_BLOCKS, ceil(n / 256)) blocks of 256 threads, four
// per CU on 256 CUs, not proportional to n; a grid stride is GSTRIDE =
// KMAN_GRAM_MAX_BLOCKS * 256 rows.
//
// Bounds, not values: a mask is read only at an index < n; slice indices are
// lane + d <= 63 + 32 < GSLICE; the LDS table is indexed [round < GROUNDS + 2]
// [lane < 64] plus its one last word; G indices i, j < n_colors, occ index
// <= n_colors and private index < n_colors are checked where they are formed.
//
// Algorithmic bytes: 8 B read per row; per block at most
// 8 * (n_colors^2 + 2 n_colors + 1) B of atomics.
#include "common.h"

namespace {

constexpr int GT = KMAN_GRAM_THREADS;
constexpr int GW = GT / 64;     // waves per block
constexpr int GSLICE = 128;     // column words of a wave's LDS slice: slice[c] and slice[n_colors + c]
constexpr int GROUNDS = KMAN_CLASSIFY_MAX_COLORS / 2 + 1;  // diagonals of the circulant: 33 x 64 >= 2080 pairs
constexpr int GROW_OCC = GROUNDS, GROW_PRIV = GROUNDS + 1;  // rows of the block's table after the pair rounds
constexpr int GSUM = (GROUNDS + 2) * 64 + 1;  // the block's table; its last word: the rows with all 64 bits
static_assert(GT == 256 && KMAN_CLASSIFY_MAX_COLORS == 64, "one lane per colour, four waves per block");
static_assert(63 + GROUNDS - 1 < GSLICE, "lane + d stays inside the slice");
// a block's 32-bit sums: 64 per step, KMAN_GRAM_MAX_ROWS / GSTRIDE steps, GW waves
static_assert(64ull * GW * (KMAN_GRAM_MAX_ROWS / ((uint64_t)KMAN_GRAM_MAX_BLOCKS * GT)) < (1ull << 32),
              "the 32-bit accumulators cannot overflow");

KMAN_DEV uint32_t popc64(uint64_t x) { return (uint32_t)__popcll((unsigned long long)x); }

__global__ __launch_bounds__(GT) void gram_kernel(const uint64_t *__restrict__ masks, uint64_t n, uint32_t nc,
                                                  unsigned long long *__restrict__ gram,
                                                  unsigned long long *__restrict__ occ,
                                                  unsigned long long *__restrict__ priv) {
    __shared__ uint64_t s_cols[GW * GSLICE];
    __shared__ uint32_t s_sum[GSUM];

    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *slice = s_cols + wave * GSLICE;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(GW * GSLICE); i += GT) s_cols[i] = 0;
    for (uint32_t i = threadIdx.x; i < (uint32_t)GSUM; i += GT) s_sum[i] = 0;
    __syncthreads();

    const uint64_t cut = nc >= 64 ? ~0ull : ((1ull << nc) - 1);
    const uint32_t half = nc >> 1;  // the last round
    uint32_t acc[GROUNDS], a_occ = 0, a_occ64 = 0, a_priv = 0;
#pragma unroll
    for (int d = 0; d < GROUNDS; d++) acc[d] = 0;

    // wave-uniform: the first row of this wave's step, the grid stride in rows
    const uint64_t stride = (uint64_t)gridDim.x * GT;
    uint64_t base = ((uint64_t)blockIdx.x * GW + wave) * 64;
    // (every load is of a row < n: the index is clamped, n >= 1 here, and a row past n counts as 0; an
    // unconditional load lets the wait for this step's mask leave the next step's in flight)
    auto load = [&](uint64_t row) {
        const uint64_t v = masks[row < n ? row : n - 1];
        return row < n ? v : 0ull;
    };
    uint64_t m_next = load(base + lane);
    while (base < n) {
        const uint64_t m = m_next & cut;
        const uint64_t live = n - base >= 64 ? ~0ull : ((1ull << (n - base)) - 1);  // the rows < n of this step
        const uint64_t nb = base + stride;
        m_next = load(nb + lane);

        // ---- columns: lane c gets col_c, in groups of 8 colours (a group past n_colors is skipped by the
        // whole wave; inside the last group a colour >= n_colors has no bit in the cut masks)
        const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
        uint64_t col = 0;
#pragma unroll 1
        for (uint32_t c0 = 0; c0 < nc; c0 += 8) {  // (not unrolled: 64 lane == c masks would not fit the SGPRs)
            const uint32_t w = (c0 < 32 ? lo : hi) >> (c0 & 31), rel = lane - c0;
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                const uint64_t b = __ballot((w & (1u << j)) != 0);
                col = rel == j ? b : col;
            }
        }
        slice[lane] = col;  // (lanes >= nc store 0)
        if (lane < nc) slice[nc + lane] = col;  // (after the store above: entries nc .. 2 nc - 1 are the columns again)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

        // ---- pairs: round d, lane i: (i, (i + d) mod nc); a lane >= nc has col == 0
#pragma unroll
        for (int d = 0; d < GROUNDS; d++)
            if ((uint32_t)d <= half) acc[d] += popc64(col & slice[lane + d]);

        // ---- occ and private from the popcount's bit planes
        const uint32_t pc = popc64(m);
        uint64_t rows = live;  // lane p: the rows with exactly p bits
#pragma unroll
        for (int kbit = 0; kbit < 6; kbit++) {
            const uint64_t plane = __ballot((pc >> kbit) & 1u);
            rows &= ((lane >> kbit) & 1u) ? plane : ~plane;
        }
        const uint64_t full = __ballot(pc == 64u);  // plane 6: all 64 bits
        a_occ += popc64(rows & ~full);
        a_occ64 += popc64(full);
        a_priv += popc64(col & __ballot(pc == 1u));

        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the slice is read before the next step overwrites it
        base = nb;
    }

    // ---- one flush per block
#pragma unroll
    for (int d = 0; d < GROUNDS; d++)
        if (acc[d]) atomicAdd(&s_sum[d * 64 + lane], acc[d]);
    if (a_occ) atomicAdd(&s_sum[GROW_OCC * 64 + lane], a_occ);
    if (a_priv) atomicAdd(&s_sum[GROW_PRIV * 64 + lane], a_priv);
    if (lane == 0 && a_occ64) atomicAdd(&s_sum[GSUM - 1], a_occ64);  // (wave-uniform: one lane adds it)
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < (uint32_t)GSUM; e += GT) {
        const uint32_t v = s_sum[e];
        if (v == 0) continue;
        const uint32_t d = e >> 6, i = e & 63u;
        if (e == (uint32_t)GSUM - 1) {
            if (occ && nc == 64) atomicAdd(&occ[64], (unsigned long long)v);
        } else if (d == (uint32_t)GROW_OCC) {
            if (occ && i <= nc) atomicAdd(&occ[i], (unsigned long long)v);
        } else if (d == (uint32_t)GROW_PRIV) {
            if (priv && i < nc) atomicAdd(&priv[i], (unsigned long long)v);
        } else {
            if (i >= nc || d > half) continue;  // (cannot happen: such a lane or round adds 0)
            if (d && 2 * d == nc && i >= half) continue;  // the last round of an even nc holds each pair twice
            uint32_t j = i + d;
            if (j >= nc) j -= nc;
            atomicAdd(&gram[(uint64_t)i * nc + j], (unsigned long long)v);
            if (j != i) atomicAdd(&gram[(uint64_t)j * nc + i], (unsigned long long)v);
        }
    }
}

}  // namespace

extern "C" int kman_mask_gram(kman_ctx *ctx, const uint64_t *d_masks, uint64_t n, uint32_t n_colors, uint64_t *d_gram,
                              uint64_t *d_occ, uint64_t *d_private) {
    if (!ctx) return KMAN_EINVAL;
    if (n_colors < 1 || n_colors > KMAN_CLASSIFY_MAX_COLORS)
        return kman_fail(ctx, KMAN_EINVAL, "n_colors must be in [1, %d], got %u", KMAN_CLASSIFY_MAX_COLORS, n_colors);
    if (!d_gram || (n && !d_masks)) return kman_fail(ctx, KMAN_EINVAL, "kman_mask_gram: null buffer");
    if (((uintptr_t)d_masks & 7) != 0) return kman_fail(ctx, KMAN_EINVAL, "masks must be 8-byte aligned");
    if (n > KMAN_GRAM_MAX_ROWS)
        return kman_fail(ctx, KMAN_EINVAL, "%llu rows: kman_mask_gram takes at most 2^40", (unsigned long long)n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemsetAsync(d_gram, 0, (size_t)8 * n_colors * n_colors, ctx->stream));
    if (d_occ) HIP_TRY(ctx, hipMemsetAsync(d_occ, 0, (size_t)8 * (n_colors + 1), ctx->stream));
    if (d_private) HIP_TRY(ctx, hipMemsetAsync(d_private, 0, (size_t)8 * n_colors, ctx->stream));
    if (n) {
        const uint64_t want = ceil_div(n, GT);
        const uint32_t blocks = (uint32_t)(want < (uint64_t)KMAN_GRAM_MAX_BLOCKS ? want : KMAN_GRAM_MAX_BLOCKS);
        KTimer kt_(ctx, "gram");
        hipLaunchKernelGGL(gram_kernel, dim3(blocks), dim3(GT), 0, ctx->stream, d_masks, n, n_colors,
                           (unsigned long long *)d_gram, (unsigned long long *)d_occ,
                           (unsigned long long *)d_private);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

// filter.hip — abundance filter: stable stream compaction of count rows.
//
// kman_filter_counts keeps the rows (key, count) with lo <= count <= hi, in
// their order (jellyfish -L/-U, KMC -ci/-cx), on the device: the rows that a
// `count -L 2` drops (most distinct k-mers of real reads occur once) are then
// never formatted nor sent over PCIe.
//
// One pass of tile kernels (256 threads x 16 rows = KMAN_FILTER_TILE rows):
// a tile loads its counts (and keys) as 16-byte vectors, builds keep flags,
// ranks them with one packed DPP wave scan, gets its output offset from the
// decoupled look-back of common.h (dynamic tile ids, flag:2|epoch:6|value:56
// status words) and writes the kept rows coalesced through LDS.
//
// Algorithmic bytes (W = 1): 12 (16 with u64 counts) read per row, as many
// written per kept row.  State carried between tiles: one status word each.
//
// Word planes (W > 1): W is unbounded, so the same kernel runs once per plane
// (keep flags from the counts, that plane compacted) and once more for the
// counts themselves, last: 4 B more read per row and plane.
#include "common.h"

namespace {

constexpr int FT = 256;                      // threads per tile
constexpr int FR = 4;                        // consecutive rows per group: one 16-byte vector of u32 counts
constexpr int FG = 4;                        // groups per thread
constexpr int FWAVE = 64 * FG * FR;          // consecutive rows of one wave
constexpr int FTILE = (FT / 64) * FWAVE;     // rows per tile
static_assert(FTILE == KMAN_FILTER_TILE, "include/kman.h states the tile size");

// what a launch moves: the keep flags always come from the counts
constexpr int F_COUNT = 0;  // nothing (the number of kept rows only)
constexpr int F_ROWS = 1;   // keys and counts (W = 1)
constexpr int F_PLANE = 2;  // one key plane
constexpr int F_CNTS = 3;   // the counts

// rows [g0, g0 + FR) of p (0 past n): 16-byte vector loads when VEC (p is
// 16-byte aligned; g0 is a multiple of FR) and the group is whole
template <bool VEC, typename T>
KMAN_DEV void load_group(const T *p, uint64_t g0, uint64_t n, T (&v)[FR]) {
    if (VEC && g0 + FR <= n) {
        constexpr int E = 16 / sizeof(T);
        typedef T vec_t __attribute__((ext_vector_type(E)));
#pragma unroll
        for (int q = 0; q < FR / E; q++) {
            const vec_t x = *reinterpret_cast<const vec_t *>(p + g0 + q * E);
#pragma unroll
            for (int e = 0; e < E; e++) v[q * E + e] = x[e];
        }
    } else {
#pragma unroll
        for (int r = 0; r < FR; r++) v[r] = g0 + r < n ? p[g0 + r] : (T)0;
    }
}

// keys / counts / okeys / ocounts may alias (in place): no __restrict__.
// Wave w of a tile owns its rows [w * FWAVE, (w + 1) * FWAVE); lane l's group
// j is the FR rows from (j * 64 + l) * FR there, so a vector load of a wave
// reads one contiguous KiB (counts) or two (keys), and the rank order is
// (wave, j, lane, row).
template <typename C, int MODE, bool VEC>
__global__ __launch_bounds__(FT) void filter_kernel(const uint64_t *keys, const C *counts, uint64_t n, uint64_t lo,
                                                    uint64_t hi, uint64_t *okeys, C *ocounts, uint64_t *status,
                                                    uint32_t *counter, uint32_t epoch, uint32_t *err) {
    constexpr bool KEYS = MODE == F_ROWS || MODE == F_PLANE;
    constexpr bool CNTS = MODE == F_ROWS || MODE == F_CNTS;
    __shared__ __attribute__((aligned(16))) uint64_t sk[KEYS ? FTILE : 1];
    __shared__ __attribute__((aligned(16))) C sc[CNTS ? FTILE : 1];
    __shared__ uint32_t lds_w[FT / 64];
    __shared__ uint64_t lds_base;
    __shared__ uint32_t lds_tile;
    const int64_t tile = grab_tile(counter, &lds_tile);
    const int lane = lane_id();
    const int w = threadIdx.x >> 6;
    const uint64_t wb = (uint64_t)tile * FTILE + (uint64_t)w * FWAVE;
    uint64_t k[FG][FR];
    C c[FG][FR];
#pragma unroll
    for (int j = 0; j < FG; j++) load_group<VEC>(counts, wb + (uint64_t)(j * 64 + lane) * FR, n, c[j]);
    if constexpr (KEYS) {
#pragma unroll
        for (int j = 0; j < FG; j++) load_group<VEC>(keys, wb + (uint64_t)(j * 64 + lane) * FR, n, k[j]);
    }
    // every load of this thread's rows has returned (not merely the counts
    // that the flags below depend on): see the publish
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t f[FG];
    uint64_t packed = 0;  // the kept rows of group j in bits [16 j, 16 j + 16): a wave's sum is <= 256 each
#pragma unroll
    for (int j = 0; j < FG; j++) {
        const uint64_t g0 = wb + (uint64_t)(j * 64 + lane) * FR;
        f[j] = 0;
#pragma unroll
        for (int r = 0; r < FR; r++) {
            const uint64_t x = (uint64_t)c[j][r];
            f[j] |= (uint32_t)(g0 + r < n && x >= lo && x <= hi) << r;
        }
        packed |= (uint64_t)__popc(f[j]) << (16 * j);
    }
    const uint64_t inc = wave_inclusive_scan(packed, SumU64(), (uint64_t)0);
    const uint64_t tot = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(inc >> 32), 63) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)inc, 63);
    const uint64_t exc = inc - packed;
    uint32_t wave_cnt = 0, goff[FG];  // goff[j]: the wave's kept rows before this lane's group j
#pragma unroll
    for (int j = 0; j < FG; j++) {
        goff[j] = wave_cnt + (uint32_t)((exc >> (16 * j)) & 0xffffu);
        wave_cnt += (uint32_t)((tot >> (16 * j)) & 0xffffu);
    }
    if (lane == 0) lds_w[w] = wave_cnt;
    __syncthreads();
    uint32_t wpre = 0, tile_cnt = 0;
#pragma unroll
    for (int i = 0; i < FT / 64; i++) {
        const uint32_t x = lds_w[i];
        if (i < w) wpre += x;
        tile_cnt += x;
    }
    if (w == 0) {
        // The publish (wave_lookback stores this tile's aggregate first).  In
        // place, the outputs are the inputs, and that is safe only because of
        // what is true HERE: every thread of the tile passed its
        // `s_waitcnt vmcnt(0)` before the barrier above, so every load of the
        // tile's own rows -- keys too, on which no count depends -- has
        // returned.  Tile m's offset exists only once every tile before m has
        // published, hence loaded.  Its kept rows land in
        // [kept before m, kept before m + kept in m), which lies inside
        // [0, end of tile m): rows of tiles <= m, all of them already read.
        // Tiles before m write below `kept before m`: no two tiles write one
        // row.  So no row is overwritten before it was read.
        const uint64_t b = wave_lookback<0>(status, tile, tile_cnt, epoch, err);
        if (lane == 0) lds_base = b;
    }
    if constexpr (MODE == F_COUNT) return;
    // the kept rows to their tile-local ranks in LDS, then out coalesced
#pragma unroll
    for (int j = 0; j < FG; j++) {
        uint32_t o = wpre + goff[j];
#pragma unroll
        for (int r = 0; r < FR; r++) {
            if ((f[j] >> r) & 1u) {
                if constexpr (KEYS) sk[o] = k[j][r];
                if constexpr (CNTS) sc[o] = c[j][r];
                o++;
            }
        }
    }
    __syncthreads();
    const uint64_t base = lds_base;
    for (uint32_t q = threadIdx.x; q < tile_cnt; q += FT) {
        if constexpr (KEYS) okeys[base + q] = sk[q];
        if constexpr (CNTS) ocounts[base + q] = sc[q];
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

template <typename C, int MODE>
int launch_mode(kman_ctx *ctx, const uint64_t *keys, const C *counts, uint64_t n, uint64_t lo, uint64_t hi,
                uint64_t *okeys, C *ocounts, uint64_t T) {
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, T, &epoch, &counter));
    const bool vec = aligned16(counts) && (MODE == F_COUNT || MODE == F_CNTS || aligned16(keys));
    if (vec)
        hipLaunchKernelGGL((filter_kernel<C, MODE, true>), dim3((uint32_t)T), dim3(FT), 0, ctx->stream, keys, counts, n,
                           lo, hi, okeys, ocounts, ctx->d_status, counter, epoch, ctx->d_err);
    else
        hipLaunchKernelGGL((filter_kernel<C, MODE, false>), dim3((uint32_t)T), dim3(FT), 0, ctx->stream, keys, counts,
                           n, lo, hi, okeys, ocounts, ctx->d_status, counter, epoch, ctx->d_err);
    HIP_TRY(ctx, hipGetLastError());
    return KMAN_OK;
}

template <typename C>
int filter_run(kman_ctx *ctx, const uint64_t *keys, uint32_t W, uint64_t stride, const C *counts, uint64_t n,
               uint64_t lo, uint64_t hi, uint64_t *okeys, C *ocounts, uint64_t T) {
    if (!okeys) return launch_mode<C, F_COUNT>(ctx, nullptr, counts, n, lo, hi, nullptr, nullptr, T);
    if (W == 1) return launch_mode<C, F_ROWS>(ctx, keys, counts, n, lo, hi, okeys, ocounts, T);
    // the counts keep every plane's flags: they are compacted last
    for (uint32_t j = 0; j < W; j++)
        KMAN_TRY((launch_mode<C, F_PLANE>(ctx, keys + j * stride, counts, n, lo, hi, okeys + j * stride, nullptr, T)));
    return launch_mode<C, F_CNTS>(ctx, nullptr, counts, n, lo, hi, nullptr, ocounts, T);
}

bool overlap(const void *a, uint64_t an, const void *b, uint64_t bn) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + bn && y < x + an;
}

}  // namespace

extern "C" int kman_filter_counts(kman_ctx *ctx, const uint64_t *d_keys, uint32_t W, uint64_t stride,
                                  const void *d_counts, uint32_t count_bytes, uint64_t n, uint64_t lo, uint64_t hi,
                                  uint64_t *d_okeys, void *d_ocounts, uint64_t *n_out) {
    if (!ctx || !n_out) return KMAN_EINVAL;
    *n_out = 0;
    if (count_bytes != 4 && count_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "count_bytes must be 4 or 8");
    if (W == 0 || (W > 1 && stride < n)) return kman_fail(ctx, KMAN_EINVAL, "W planes need W >= 1 and stride >= n");
    if ((d_okeys == nullptr) != (d_ocounts == nullptr))
        return kman_fail(ctx, KMAN_EINVAL, "output keys and counts: both or neither");
    if (n == 0 || lo > hi) return KMAN_OK;
    if (!d_counts || (d_okeys && !d_keys)) return KMAN_EINVAL;
    const uint64_t T = ceil_div(n, FTILE);
    if (T > 0x7fffffffull) return kman_fail(ctx, KMAN_EINVAL, "%llu rows: too many tiles", (unsigned long long)n);
    const bool in_place = d_okeys == d_keys && d_ocounts == d_counts;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto run = [&](uint64_t *ok_, void *oc_) -> int {
        {
            KTimer kt_(ctx, "filter_counts");  // (the launches alone, not the read-back of the total)
            if (count_bytes == 4)
                KMAN_TRY(filter_run<uint32_t>(ctx, d_keys, W, stride, (const uint32_t *)d_counts, n, lo, hi, ok_,
                                              (uint32_t *)oc_, T));
            else
                KMAN_TRY(filter_run<uint64_t>(ctx, d_keys, W, stride, (const uint64_t *)d_counts, n, lo, hi, ok_,
                                              (uint64_t *)oc_, T));
        }
        return kman_lookback_total(ctx, T, n_out);
    };
    if (d_okeys && !in_place) {
        // outputs of `rows` rows must lie apart from the inputs and from each other
        const uint64_t ikb = 8 * ((uint64_t)(W - 1) * stride + n), icb = (uint64_t)count_bytes * n;
        auto clash = [&](uint64_t rows) {
            const uint64_t kb = 8 * ((uint64_t)(W - 1) * stride + rows), cb = (uint64_t)count_bytes * rows;
            return overlap(d_okeys, kb, d_keys, ikb) || overlap(d_okeys, kb, d_counts, icb) ||
                   overlap(d_ocounts, cb, d_keys, ikb) || overlap(d_ocounts, cb, d_counts, icb) ||
                   overlap(d_okeys, kb, d_ocounts, cb);
        };
        bool bad = clash(1);  // an output that starts inside an input
        if (!bad && clash(n)) {
            // apart only if few enough rows are kept (an output allocated for
            // the kept rows, just below an input): count them first
            KMAN_TRY(run(nullptr, nullptr));
            bad = clash(*n_out);
            *n_out = 0;
        }
        if (bad) return kman_fail(ctx, KMAN_EINVAL, "outputs overlap the inputs in part (equal to them, or apart)");
    }
    return run(d_okeys, d_ocounts);
}

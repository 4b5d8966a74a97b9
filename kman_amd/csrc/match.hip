// match.hip — look one count table up in another: a balanced merge-path join.
//
// kman_match_counts takes two tables of (u64 key, count) rows, each strictly
// ascending in key (the rows of kman_groups / kman_finish / kman_rle_count),
// and writes, for every row i of A, out[i] = op(count of A's row, count of the
// row of B with the same key or "none").  Intersection, subtraction and union
// of two k-mer sets are this vector plus kman_filter_counts (engine.set_op).
//
// Two kernels:
//   match_split   one thread per tile boundary t: the merge-path split a_t of
//                 diagonal d_t = min(t * MTILE, na + nb), the number of A rows
//                 among the first d_t rows of the merged order (ties: A first).
//                 b_t = d_t - a_t.  One binary search in global memory per
//                 tile (<= 64 steps), tiles + 1 words of context scratch.
//   match_tile    256 threads per tile of MTILE = KMAN_MATCH_TILE merged rows:
//                 A[a_t, a_t+1) and B[b_t, b_t+1] (keys, and B's counts when
//                 the op reads them) go to LDS as 16-byte vectors, each A row
//                 finds its partner by a lower bound over the B slice in LDS
//                 (MSTEPS = 12 steps), and out[a_t ..] is written coalesced.
//
// Why B[b_t+1] (one row past the slice) and no more: keys are distinct in each
// table and ties put A first, so in the merged order the B row equal to A[i]
// is the very next row after A[i].  A[i] lies in [d_t, d_t+1), so its partner
// lies in [d_t + 1, d_t+1]: inside the tile's B slice, or the first B row of
// the next tile.  It cannot lie before b_t (it comes after A[i]).
//
// Work per block is MTILE rows whatever na : nb is: 10^6 B rows between two
// neighbouring A keys are 10^6 / MTILE tiles with no A row, which read their
// two split words and leave.
//
// Bounds, not values: slices are cut by index (rows past a slice are never
// compared), so keys 0 and 2^64 - 1 are ordinary keys.  Every loop count comes
// from MTILE; the splits are clamped to [a_t, a_t + rows of the tile] and every
// global index is below na / nb, so an input that breaks the precondition
// (unsorted, duplicate keys) gives wrong counts but no wild address and no
// unbounded loop.
//
// Algorithmic bytes: 8 + a_count_bytes read per A row (8 for RIGHT), 8 +
// b_count_bytes per B row (8 for LEFT and ABSENT), out_bytes written per A row.
// A slice that does not start on a 16-byte boundary is loaded from the vector
// that holds its first row (at most 3 rows of the neighbouring tile, read twice).
//
// Resources (gfx950, hipcc -O3, the compiler's report): match_tile 44 VGPRs at
// most, no scratch memory in any of the eight instances, LDS 8 * (MTILE + 8)
// bytes of keys + count bytes * (MTILE + 8) of B counts = 24,672 B (u32 B
// counts) or 32,896 B (u64): 6 or 4 blocks per CU.  match_split: 16 VGPRs, no
// LDS, no scratch memory.
#include "common.h"

namespace {

constexpr int MT = 256;                  // threads per tile
constexpr int MTILE = 2048;              // merged rows (A + B) per tile
constexpr int MROWS = MTILE / MT;        // A rows per thread at most
constexpr int MSTEPS = 12;               // lower bound over <= MTILE + 1 rows: 2049 -> 0 in 12 halvings
constexpr int MPAD = 8;                  // LDS rows for the alignment offsets and B's extra row
static_assert(MTILE == KMAN_MATCH_TILE, "include/kman.h states the tile size");
static_assert((MTILE + 1) >> MSTEPS == 0, "MSTEPS halvings empty the B slice");

// the number of A rows among the first d rows of the merged order, ties A first
KMAN_DEV uint64_t merge_split(const uint64_t *__restrict__ ak, uint64_t na, const uint64_t *__restrict__ bk,
                              uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = umin64(d, na);
    for (int s = 0; s < 64 && lo < hi; s++) {
        const uint64_t mid = lo + ((hi - lo) >> 1);  // (lo <= mid < hi <= d, mid >= d - nb: 0 <= d - 1 - mid < nb)
        if (ak[mid] <= bk[d - 1 - mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(MT) void match_split(const uint64_t *__restrict__ ak, uint64_t na,
                                                  const uint64_t *__restrict__ bk, uint64_t nb, uint64_t tiles,
                                                  uint64_t *__restrict__ split) {
    const uint64_t t = (uint64_t)blockIdx.x * MT + threadIdx.x;
    if (t > tiles) return;
    split[t] = merge_split(ak, na, bk, nb, umin64(t * MTILE, na + nb));
}

// Rows [i0, i1) of src (n rows in all) to LDS: dst[i - base] = src[i], where
// base is i0 rounded down to a whole 16-byte vector when `vec` (src is 16-byte
// aligned), else i0.  Returns i0 - base.  i1 - i0 <= MTILE + 1; dst is 16-byte
// aligned and has room for MTILE + 1 rows and two partial vectors.
template <typename TY>
KMAN_DEV uint32_t stage(TY *dst, const TY *__restrict__ src, uint64_t i0, uint64_t i1, uint64_t n, bool vec) {
    constexpr int E = 16 / sizeof(TY);
    typedef TY vec_t __attribute__((ext_vector_type(E)));
    const uint64_t base = vec ? i0 & ~(uint64_t)(E - 1) : i0;
    const uint32_t cnt = (uint32_t)(i1 - base);
    if (vec) {
        const uint32_t nv = (cnt + E - 1) / E;
        constexpr int MAXV = ((MTILE + 1 + 2 * (E - 1)) / E + MT - 1) / MT;
#pragma unroll
        for (int j = 0; j < MAXV; j++) {
            const uint32_t v = threadIdx.x + j * MT;
            const uint64_t g = base + (uint64_t)v * E;
            if (v < nv && g + E <= n) {
                *reinterpret_cast<vec_t *>(dst + v * E) = *reinterpret_cast<const vec_t *>(src + g);
            } else if (v < nv) {
#pragma unroll
                for (int e = 0; e < E; e++)
                    if (g + e < n) dst[v * E + e] = src[g + e];
            }
        }
    } else {
        constexpr int MAXQ = (MTILE + 1 + MT - 1) / MT;
#pragma unroll
        for (int j = 0; j < MAXQ; j++) {
            const uint32_t q = threadIdx.x + j * MT;
            if (q < cnt) dst[q] = src[base + q];
        }
    }
    return (uint32_t)(i0 - base);
}

KMAN_DEV uint64_t add_sat(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}

// vec bits: 1 = A keys, 2 = B keys, 4 = B counts are 16-byte aligned
template <typename CA, typename CB, typename CO>
__global__ __launch_bounds__(MT) void match_tile(const uint64_t *__restrict__ ak, const CA *__restrict__ ac,
                                                 uint64_t na, const uint64_t *__restrict__ bk,
                                                 const CB *__restrict__ bc, uint64_t nb, int op, uint32_t vec,
                                                 const uint64_t *__restrict__ split, CO *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint64_t sk[MTILE + MPAD];  // the A slice, then the B slice
    __shared__ __attribute__((aligned(16))) CB sc[MTILE + MPAD];        // the B slice's counts
    const bool need_a = op != KMAN_MATCH_RIGHT;
    const bool need_b = op != KMAN_MATCH_LEFT && op != KMAN_MATCH_ABSENT;
    const uint64_t N = na + nb;
    const uint64_t d0 = umin64((uint64_t)blockIdx.x * MTILE, N), d1 = umin64(d0 + MTILE, N);
    // the clamps change nothing for sorted input (a_t <= a_t+1 <= a_t + d1 - d0)
    const uint64_t a0 = umin64(split[blockIdx.x], umin64(d0, na));
    uint64_t a1 = split[blockIdx.x + 1];
    a1 = a1 < a0 ? a0 : umin64(a1, umin64(a0 + (d1 - d0), na));
    const uint32_t nA = (uint32_t)(a1 - a0);
    if (nA == 0) return;  // a tile of B rows only: nothing to write
    const uint64_t b0 = umin64(d0 - a0, nb), b1 = umin64(d1 - a1, nb);
    const uint64_t b1x = umin64((b1 < b0 ? b0 : b1) + 1, nb);  // B's slice and the row past it
    const uint32_t nB = (uint32_t)(b1x - b0);                 // <= MTILE - nA + 1
    // this thread's A counts: in flight while the slices are staged
    uint64_t ca[MROWS];
#pragma unroll
    for (int j = 0; j < MROWS; j++) {
        const uint32_t ia = threadIdx.x + j * MT;
        ca[j] = need_a && ia < nA ? (uint64_t)ac[a0 + ia] : 0;
    }
    const uint32_t offA = stage(sk, ak, a0, a1, na, vec & 1u);
    uint64_t *skb = sk + ((offA + nA + 1) & ~1u);  // (16-byte aligned; <= nA + 2 rows in)
    const uint32_t offB = stage(skb, bk, b0, b1x, nb, (vec & 2u) != 0);
    uint32_t offC = 0;
    if (need_b) offC = stage(sc, bc, b0, b1x, nb, (vec & 4u) != 0);
    __syncthreads();
    const uint64_t *ska = sk + offA;
    skb += offB;
    const CB *scb = sc + offC;
    constexpr uint64_t OMAX = sizeof(CO) == 4 ? 0xffffffffull : ~0ull;
#pragma unroll
    for (int j = 0; j < MROWS; j++) {
        const uint32_t ia = threadIdx.x + j * MT;
        if (ia >= nA) continue;
        const uint64_t x = ska[ia];
        uint32_t lo = 0, len = nB;  // the first row of the B slice with key >= x
#pragma unroll
        for (int s = 0; s < MSTEPS; s++) {
            const uint32_t half = len >> 1;
            if (len != 0 && skb[lo + half] < x) {  // (len == 0: done, nothing is read)
                lo += half + 1;
                len -= half + 1;
            } else {
                len = half;
            }
        }
        const bool hit = lo < nB && skb[lo] == x;
        const uint64_t cb = hit && need_b ? (uint64_t)scb[lo] : 0;
        const uint64_t a = ca[j];
        uint64_t r;
        switch (op) {
        case KMAN_MATCH_RIGHT: r = cb; break;
        case KMAN_MATCH_LEFT: r = hit ? a : 0; break;
        case KMAN_MATCH_MIN: r = hit ? (a < cb ? a : cb) : 0; break;
        case KMAN_MATCH_MAX: r = hit ? (a > cb ? a : cb) : 0; break;
        case KMAN_MATCH_SUM: r = hit ? add_sat(a, cb) : 0; break;
        case KMAN_MATCH_ABSENT: r = hit ? 0 : a; break;
        case KMAN_MATCH_ANY_SUM: r = add_sat(a, cb); break;
        default: r = a > cb ? a : cb; break;  // KMAN_MATCH_ANY_MAX
        }
        out[a0 + ia] = (CO)(r < OMAX ? r : OMAX);
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

template <typename CA, typename CB, typename CO>
void launch_tiles(kman_ctx *ctx, const uint64_t *ak, const void *ac, uint64_t na, const uint64_t *bk, const void *bc,
                  uint64_t nb, int op, uint32_t vec, const uint64_t *split, void *out, uint64_t tiles) {
    hipLaunchKernelGGL((match_tile<CA, CB, CO>), dim3((uint32_t)tiles), dim3(MT), 0, ctx->stream, ak, (const CA *)ac,
                       na, bk, (const CB *)bc, nb, op, vec, split, (CO *)out);
}

}  // namespace

extern "C" int kman_match_counts(kman_ctx *ctx, const uint64_t *d_akeys, const void *d_acounts,
                                 uint32_t a_count_bytes, uint64_t na, const uint64_t *d_bkeys, const void *d_bcounts,
                                 uint32_t b_count_bytes, uint64_t nb, int op, void *d_out, uint32_t out_bytes) {
    if (!ctx) return KMAN_EINVAL;
    if (op < KMAN_MATCH_RIGHT || op > KMAN_MATCH_ANY_MAX) return kman_fail(ctx, KMAN_EINVAL, "unknown match op %d", op);
    for (uint32_t w : {a_count_bytes, b_count_bytes, out_bytes})
        if (w != 4 && w != 8) return kman_fail(ctx, KMAN_EINVAL, "count and output widths must be 4 or 8 bytes");
    if (na == 0) return KMAN_OK;
    const bool need_a = op != KMAN_MATCH_RIGHT, need_b = op != KMAN_MATCH_LEFT && op != KMAN_MATCH_ABSENT;
    if (!d_akeys || !d_out || (need_a && !d_acounts) || (nb && (!d_bkeys || (need_b && !d_bcounts))))
        return kman_fail(ctx, KMAN_EINVAL, "kman_match_counts: null buffer");
    if (na + nb < na) return kman_fail(ctx, KMAN_EINVAL, "too many rows");
    const uint64_t tiles = ceil_div(na + nb, MTILE);
    if (tiles > 0x7ffffffeull) return kman_fail(ctx, KMAN_EINVAL, "%llu rows: too many tiles", (unsigned long long)(na + nb));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *scr;
    KMAN_TRY(kman_scratch(ctx, 8 * (tiles + 1), &scr));
    uint64_t *split = (uint64_t *)scr;
    const uint32_t vec = (aligned16(d_akeys) ? 1u : 0u) | (aligned16(d_bkeys) ? 2u : 0u) | (aligned16(d_bcounts) ? 4u : 0u);
    {
        KTimer kt_(ctx, "match_counts");
        hipLaunchKernelGGL(match_split, dim3((uint32_t)ceil_div(tiles + 1, MT)), dim3(MT), 0, ctx->stream, d_akeys, na,
                           d_bkeys, nb, tiles, split);
        HIP_TRY(ctx, hipGetLastError());
        const int sel = (a_count_bytes == 8 ? 4 : 0) | (b_count_bytes == 8 ? 2 : 0) | (out_bytes == 8 ? 1 : 0);
#define KMAN_MATCH_CASE(i, CA, CB, CO)                                                                        \
    case i:                                                                                                   \
        launch_tiles<CA, CB, CO>(ctx, d_akeys, d_acounts, na, d_bkeys, d_bcounts, nb, op, vec, split, d_out, tiles); \
        break;
        switch (sel) {
            KMAN_MATCH_CASE(0, uint32_t, uint32_t, uint32_t)
            KMAN_MATCH_CASE(1, uint32_t, uint32_t, uint64_t)
            KMAN_MATCH_CASE(2, uint32_t, uint64_t, uint32_t)
            KMAN_MATCH_CASE(3, uint32_t, uint64_t, uint64_t)
            KMAN_MATCH_CASE(4, uint64_t, uint32_t, uint32_t)
            KMAN_MATCH_CASE(5, uint64_t, uint32_t, uint64_t)
            KMAN_MATCH_CASE(6, uint64_t, uint64_t, uint32_t)
            KMAN_MATCH_CASE(7, uint64_t, uint64_t, uint64_t)
        }
#undef KMAN_MATCH_CASE
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

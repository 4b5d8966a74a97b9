// unitig.hip — the compacted de Bruijn graph of a canonical count table: the
// table's rows are the nodes, non-branching paths are merged into unitigs
// (`kmer unitigs`; include/kman.h states the definition).
//
// kman_graph_links, one thread per row, two kernels:
//   neighbours  the 4 keys that extend the row's k-mer to the right (side R)
//               and the 4 that extend it to the left (side L) are folded to
//               their canonical form and looked up through the prefix index of
//               kman_table_index: the 8 searches advance in lockstep
//               (screen_lookup.h's table_rows), and a hit keeps the ROW its
//               lower bound ended on.  A side with exactly one hit writes
//               (row << 1 | side entered) to a scratch word, every other side
//               KMAN_GRAPH_NONE.
//   mutual      side u keeps its word v when v's own word is u and v is a side
//               of another row; else KMAN_GRAPH_NONE.
//
// kman_graph_rank, list ranking over the 2 nt states "leave row i through side
// s" (state 2 i + s): the successor of a state is its partner's opposite side,
// a state without a link is terminal (it points at itself).  Pointer doubling
// with the rounds driven from the host: a round reads (pointer, distance, least
// row) of every state and of the state it points at from one buffer and writes
// the other (no state is read and written in one launch), and sets a device
// word when a pointer moved; the host stops when none did, after at most
// ceil(log2(2 nt)) + 1 rounds.  No kernel holds a loop over a unitig.  States
// that then do not point at a terminal lie on cycles: the least row carried
// through the rounds names each cycle's smallest row, whose side-L link and its
// partner are removed from a private copy of the links, those states alone are
// set up again and the rounds repeated.  Per row the two states give the two
// end rows of its path (the smaller one is the unitig's start), the distance
// to each, and with that the position, the orientation and the node count.
//
// kman_unitig_spell, two kernels:
//   layout   tiles of UTILE rows: the heads (position 0) are counted and their
//            nodes + k - 1 bases summed, one block scan each, and the tile's
//            two offsets come from two decoupled look-backs of common.h
//            (dynamic tile ids; the second one in the upper half of the status
//            words): every head gets its ordinal and its first base's offset.
//   spell    one thread per row: a head writes its k bases and its unitig's
//            offset and node count, every other row the one base it adds;
//            every row adds its count to its unitig's KC with one 64-bit
//            integer atomic (integer adds commute: two calls, equal bytes).
//
// kman_unitig_edges, four kernels:
//   layout   the spelling's tile pass without its base sums (BASES = false):
//            every head gets its ordinal.
//   ends     one thread per row: a head notes (row, side opposite its exit) as
//            its unitig's "-" end, a last row (pos >> 1 == nodes[start] - 1)
//            (row, exit side) as the "+" end.
//   edges    one thread per END, tiles of ETILE: the 4 extensions of the end's
//            oriented k-mer are looked up in lockstep (table_rows<4>), each hit
//            (j, t) becomes (ord[start[j]] << 1) | p, "+" when j is a head
//            entered at t; the up to 4 words and the end's offset (block scan,
//            decoupled look-back) go to scratch.
//   write    offsets and words into the outputs, once the capacities hold.
//
// Bounds, not values: every index read from memory (index pair, link, pointer,
// start row, ordinal, offset) is compared with its array's size before it is
// used, every search runs a step count fixed before it starts and every round
// count is fixed by nt; a foreign index, unsorted keys or links that are no
// links give wrong unitigs, never a wild address or an unbounded loop.
//
// Algorithmic bytes per row: links 8 B key, 8 index pairs, at most
// 8 (floor(log2 bucket) + 1) random key reads, 8 + 24 B of link words; a rank
// round 2 x (12 B read + 12 B random read + 12 B written); spell 24 B read,
// two dependent random reads (ordinal, offset), one byte and one atomic.
// Edges, per row: 4 B in the layout, 12 B and one random ordinal in ends; per
// END: 4 B end word, 8 B key, 4 index pairs, at most 4 (floor(log2 bucket) +
// 1) random key reads, per hit three dependent random words (start, pos,
// ordinal), 24 B of scratch written and read again, 8 B + 4 B per edge out.
#include "common.h"
#include "screen_lookup.h"

namespace {

constexpr int UT = 256;
constexpr int UR = 8;  // consecutive rows per thread of the layout kernel
constexpr int UTILE = UT * UR;
constexpr uint32_t NONE = KMAN_GRAPH_NONE;
constexpr int ETILE = UT;  // ends per tile of the edges kernel, one per thread
static_assert(UTILE == KMAN_UNITIG_TILE, "include/kman.h states the tile size");
static_assert(ETILE == KMAN_EDGE_TILE, "include/kman.h states the tile size");
static_assert(KMAN_GRAPH_R == 0 && KMAN_GRAPH_L == 1, "a state's opposite side is its word ^ 1");

// the reverse complement of a 2k-bit key
KMAN_DEV uint64_t rc_key(uint64_t x, uint32_t k) {
    x = ~x;
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
    return __builtin_bswap64(x) >> (64 - 2 * k);
}

// ---------------------------------------------------------------- links
__global__ __launch_bounds__(UT) void neighbours_kernel(const uint64_t *__restrict__ tkeys, uint32_t nt, uint32_t k,
                                                        const uint64_t *__restrict__ index, uint32_t shift,
                                                        uint32_t *__restrict__ nb) {
    const uint32_t i = blockIdx.x * UT + threadIdx.x;
    if (i >= nt) return;
    const uint64_t mask = (1ull << (2 * k)) - 1;  // (k <= 31)
    const uint64_t x = tkeys[i] & mask;
    uint64_t kf[8], row[8];
    uint32_t fwd = 0;  // bit j: the extension is its own canonical form
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint64_t b = (uint64_t)(j & 3);
        const uint64_t y = j < 4 ? (((x << 2) | b) & mask) : ((x >> 2) | (b << (2 * k - 2)));
        const uint64_t r = rc_key(y, k);
        kf[j] = y < r ? y : r;
        fwd |= (uint32_t)(y < r) << j;
    }
    const uint32_t hit = table_rows<8>(~0u, kf, shift, index, tkeys, (uint64_t)nt, row);
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const uint32_t h = (hit >> (4 * s)) & 15u;
        uint32_t w = NONE;
        if (__popc(h) == 1) {
            const int j = 4 * s + (__ffs((int)h) - 1);
            uint64_t rj = 0;
#pragma unroll
            for (int q = 0; q < 8; q++) rj = q == j ? row[q] : rj;  // (no indexed register array)
            // out of R a forward neighbour is entered at its L, a reversed one at its R; out of L the other way
            const uint32_t f = (fwd >> j) & 1u;
            const uint32_t t = s == KMAN_GRAPH_R ? (f ? KMAN_GRAPH_L : KMAN_GRAPH_R) : (f ? KMAN_GRAPH_R : KMAN_GRAPH_L);
            w = ((uint32_t)rj << 1) | t;  // (rj < nt < 2^31)
        }
        nb[2 * (uint64_t)i + s] = w;
    }
}

__global__ __launch_bounds__(UT) void mutual_kernel(const uint32_t *__restrict__ nb, uint32_t n2,
                                                    uint32_t *__restrict__ link) {
    const uint32_t u = blockIdx.x * UT + threadIdx.x;
    if (u >= n2) return;
    const uint32_t v = nb[u];
    const bool ok = v < n2 && (v >> 1) != (u >> 1) && nb[v] == u;
    link[u] = ok ? v : NONE;
}

// ----------------------------------------------------------------- rank
// a state's word: its pointer in the low half, the distance to it in the high half
KMAN_DEV uint32_t ptr_of(uint64_t s, uint32_t self, uint32_t n2) {
    const uint32_t p = (uint32_t)s;
    return p < n2 ? p : self;
}

__global__ __launch_bounds__(UT) void rank_init_kernel(const uint32_t *__restrict__ link, uint32_t n2,
                                                       uint32_t *__restrict__ mine, uint64_t *__restrict__ S,
                                                       uint32_t *__restrict__ M) {
    const uint32_t u = blockIdx.x * UT + threadIdx.x;
    if (u >= n2) return;
    const uint32_t l = link[u];
    const bool on = l < n2;
    mine[u] = on ? l : NONE;
    S[u] = on ? ((uint64_t)(l ^ 1u) | (1ull << 32)) : (uint64_t)u;
    M[u] = u >> 1;
}

__global__ __launch_bounds__(UT) void rank_round_kernel(const uint64_t *__restrict__ S, const uint32_t *__restrict__ M,
                                                        uint32_t n2, uint64_t *__restrict__ S2,
                                                        uint32_t *__restrict__ M2, uint32_t *__restrict__ moved) {
    const uint32_t u = blockIdx.x * UT + threadIdx.x;
    bool mv = false;
    if (u < n2) {
        const uint64_t s = S[u];
        const uint32_t p = ptr_of(s, u, n2);
        const uint64_t t = S[p];
        const uint32_t q = ptr_of(t, p, n2);
        const uint32_t a = M[u], b = M[p];
        // (the distance wraps on a cycle alone, where it is never used)
        S2[u] = (uint64_t)q | ((uint64_t)((uint32_t)(s >> 32) + (uint32_t)(t >> 32)) << 32);
        M2[u] = a < b ? a : b;
        mv = q != p;
    }
    if (__ballot(mv) != 0 && lane_id() == 0) *moved = 1u;
}

// row i is its cycle's smallest: its side-L link and the partner's go
__global__ __launch_bounds__(UT) void cycle_cut_kernel(const uint32_t *__restrict__ link, const uint64_t *__restrict__ S,
                                                       const uint32_t *__restrict__ M, uint32_t nt,
                                                       uint32_t *__restrict__ mine, uint32_t *__restrict__ ncut) {
    const uint32_t i = blockIdx.x * UT + threadIdx.x;
    if (i >= nt) return;
    const uint32_t n2 = 2 * nt, u = 2 * i + KMAN_GRAPH_L;
    const uint32_t p = ptr_of(S[u], u, n2);
    if (link[p] >= n2 || M[u] != i) return;  // (points at a terminal: a path)
    const uint32_t q = mine[u];
    mine[u] = NONE;
    if (q < n2) mine[q] = NONE;
    atomicAdd(ncut, 1u);
}

// the states that point at no terminal start again from the cut links
__global__ __launch_bounds__(UT) void rank_again_kernel(const uint32_t *__restrict__ link,
                                                        const uint32_t *__restrict__ mine, uint32_t n2,
                                                        uint64_t *__restrict__ S, uint32_t *__restrict__ M) {
    const uint32_t u = blockIdx.x * UT + threadIdx.x;
    if (u >= n2) return;
    const uint32_t p = ptr_of(S[u], u, n2);
    if (link[p] >= n2) return;
    const uint32_t l = mine[u];
    S[u] = l < n2 ? ((uint64_t)(l ^ 1u) | (1ull << 32)) : (uint64_t)u;
    M[u] = u >> 1;
}

__global__ __launch_bounds__(UT) void rank_finish_kernel(const uint64_t *__restrict__ S, uint32_t nt,
                                                         uint32_t *__restrict__ start, uint32_t *__restrict__ pos,
                                                         uint32_t *__restrict__ nodes) {
    const uint32_t i = blockIdx.x * UT + threadIdx.x;
    if (i >= nt) return;
    const uint32_t n2 = 2 * nt;
    const uint64_t sr = S[2 * i + KMAN_GRAPH_R], sl = S[2 * i + KMAN_GRAPH_L];
    const uint32_t er = ptr_of(sr, 2 * i, n2) >> 1, el = ptr_of(sl, 2 * i + 1, n2) >> 1;  // the end rows
    const uint32_t dr = (uint32_t)(sr >> 32), dl = (uint32_t)(sl >> 32);
    // the start lies behind side L: the walk leaves this row through R, the canonical spelling
    const bool canon = el <= er;
    const uint32_t p = canon ? dl : dr;
    start[i] = canon ? el : er;
    pos[i] = (p << 1) | (canon ? 0u : 1u);
    nodes[i] = p == 0 ? dr + dl + 1 : 0u;
}

// ---------------------------------------------------------------- spell
// BASES false: the ordinals alone, for kman_unitig_edges (nodes and hoff are not touched, one look-back)
template <bool BASES>
__global__ __launch_bounds__(UT) void layout_kernel(const uint32_t *__restrict__ pos, const uint32_t *__restrict__ nodes,
                                                    uint32_t nt, uint32_t k, uint32_t *__restrict__ ord,
                                                    uint64_t *__restrict__ hoff, uint64_t *status, uint64_t n_tiles,
                                                    uint32_t *counter, uint32_t epoch, uint32_t *err) {
    __shared__ uint32_t lds_c[UT / 64];
    __shared__ uint64_t lds_b[UT / 64];
    __shared__ uint64_t lds_base[2];
    __shared__ uint32_t lds_tile;
    const int64_t tile = grab_tile(counter, &lds_tile);
    const uint64_t r0 = (uint64_t)tile * UTILE + (uint64_t)threadIdx.x * UR;
    uint32_t heads = 0, nn[UR];
    uint64_t bases = 0;
#pragma unroll
    for (int r = 0; r < UR; r++) {
        const uint64_t i = r0 + r;
        const bool head = i < nt && (pos[i < nt ? i : 0] >> 1) == 0;
        nn[r] = BASES && head ? nodes[i] : 0u;
        heads |= (uint32_t)head << r;
        bases += head ? (uint64_t)nn[r] + (k - 1) : 0ull;
    }
    uint32_t tc = 0;
    uint64_t tb = 0;
    uint32_t c = block_exclusive_scan<UT>((uint32_t)__popc(heads), SumU32(), 0u, lds_c, &tc);
    uint64_t b = BASES ? block_exclusive_scan<UT>(bases, SumU64(), (uint64_t)0, lds_b, &tb) : 0ull;
    if ((threadIdx.x >> 6) == 0) {
        const uint64_t bc = wave_lookback<0>(status, tile, (uint64_t)tc, epoch, err);
        const uint64_t bb = BASES ? wave_lookback<0>(status + n_tiles, tile, tb, epoch, err) : 0ull;
        if (lane_id() == 0) {
            lds_base[0] = bc;
            lds_base[1] = bb;
        }
    }
    __syncthreads();
    c += (uint32_t)lds_base[0];
    b += lds_base[1];
#pragma unroll
    for (int r = 0; r < UR; r++) {
        const uint64_t i = r0 + r;
        if (i >= nt) break;
        const bool head = (heads >> r) & 1u;
        ord[i] = head ? c : NONE;
        if (head) {
            if (BASES) hoff[i] = b;
            c++;
            b += (uint64_t)nn[r] + (k - 1);
        }
    }
}

template <typename CT>
__global__ __launch_bounds__(UT) void spell_kernel(const uint64_t *__restrict__ tkeys, const CT *__restrict__ tcounts,
                                                   uint32_t nt, uint32_t k, const uint32_t *__restrict__ start,
                                                   const uint32_t *__restrict__ pos, const uint32_t *__restrict__ nodes,
                                                   const uint32_t *__restrict__ ord, const uint64_t *__restrict__ hoff,
                                                   uint64_t nu, uint64_t total, uint64_t *__restrict__ off,
                                                   uint32_t *__restrict__ unodes, unsigned long long *__restrict__ kc,
                                                   uint8_t *__restrict__ seq) {
    const uint32_t i = blockIdx.x * UT + threadIdx.x;
    if (i >= nt) return;
    if (i == 0) off[nu] = total;
    const uint32_t a = start[i];
    if (a >= nt) return;
    const uint32_t o = ord[a];
    if ((uint64_t)o >= nu) return;  // (NONE: the start is no head; cannot happen on kman_graph_rank's output)
    const uint64_t at = hoff[a];
    const uint32_t pw = pos[i], p = pw >> 1;
    const uint64_t x = tkeys[i] & ((1ull << (2 * k)) - 1);
    const uint64_t s = (pw & 1u) ? rc_key(x, k) : x;
    const uint32_t B = 0x54474341u;  // "ACGT"
    if (p == 0) {
        off[o] = at;
        unodes[o] = nodes[i];
        for (uint32_t j = 0; j < k; j++)  // (k <= 31)
            if (at + j < total) seq[at + j] = (uint8_t)(B >> (8 * ((s >> (2 * (k - 1 - j))) & 3u)));
    } else {
        const uint64_t w = at + (k - 1) + p;
        if (w < total) seq[w] = (uint8_t)(B >> (8 * (s & 3u)));
    }
    atomicAdd(&kc[o], (unsigned long long)tcounts[i]);
}

// ---------------------------------------------------------------- edges
// endw[2 u + o] = (row << 1) | side of end o of unitig u: the last row and the
// side it is left through ("+"), the first row and the opposite side ("-")
__global__ __launch_bounds__(UT) void ends_kernel(const uint32_t *__restrict__ start, const uint32_t *__restrict__ pos,
                                                  const uint32_t *__restrict__ nodes, const uint32_t *__restrict__ ord,
                                                  uint32_t nt, uint64_t nu, uint32_t *__restrict__ endw) {
    const uint32_t i = blockIdx.x * UT + threadIdx.x;
    if (i >= nt) return;
    const uint32_t a = start[i];
    if (a >= nt) return;
    const uint32_t u = ord[a];
    if ((uint64_t)u >= nu) return;  // (NONE: the start is no head)
    const uint32_t pw = pos[i], p = pw >> 1, o = pw & 1u;
    if (p == 0) endw[2 * (uint64_t)u + 1] = (i << 1) | (o ^ 1u);
    if (p + 1 == nodes[a]) endw[2 * (uint64_t)u] = (i << 1) | o;  // (p < 2^31)
}

// One thread per end, tiles of ETILE ends: the 4 keys that extend the end's
// oriented k-mer are looked up in lockstep, each hit (j, t) is resolved to
// (v << 1) | p through start, pos and ord, the up to 4 words go to ew[e] and
// the end's offset, from a block scan and a look-back over the tiles, to
// eoff[e].
__global__ __launch_bounds__(UT) void edges_kernel(const uint64_t *__restrict__ tkeys, uint32_t nt, uint32_t k,
                                                   const uint64_t *__restrict__ index, uint32_t shift,
                                                   const uint32_t *__restrict__ start, const uint32_t *__restrict__ pos,
                                                   const uint32_t *__restrict__ ord,
                                                   const uint32_t *__restrict__ endw, uint64_t n_ends,
                                                   uint4 *__restrict__ ew, uint64_t *__restrict__ eoff,
                                                   uint64_t *status, uint32_t *counter, uint32_t epoch, uint32_t *err) {
    __shared__ uint32_t lds_c[UT / 64];
    __shared__ uint64_t lds_base;
    __shared__ uint32_t lds_tile;
    const int64_t tile = grab_tile(counter, &lds_tile);
    const uint64_t e = (uint64_t)tile * ETILE + threadIdx.x;
    const uint32_t me = e < n_ends ? endw[e] : NONE;
    uint32_t w[4] = {NONE, NONE, NONE, NONE}, c = 0;
    if ((me >> 1) < nt) {  // (NONE >> 1 = 2^31 - 1 >= nt)
        const uint64_t mask = (1ull << (2 * k)) - 1;  // (k <= 31)
        const uint64_t x = tkeys[me >> 1] & mask;
        const uint64_t z = (me & 1u) == KMAN_GRAPH_R ? x : rc_key(x, k);  // the k-mer as the end's orientation reads it
        uint64_t kf[4], row[4];
        uint32_t fwd = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint64_t y = ((z << 2) | (uint64_t)j) & mask;
            const uint64_t r = rc_key(y, k);
            kf[j] = y < r ? y : r;
            fwd |= (uint32_t)(y < r) << j;
        }
        const uint32_t hit = table_rows<4>(~0u, kf, shift, index, tkeys, (uint64_t)nt, row);
        const uint64_t nu = n_ends >> 1;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (!((hit >> j) & 1u)) continue;
            const uint32_t rj = (uint32_t)row[j];  // (< nt)
            // a forward neighbour is entered at its L, a reversed one at its R
            const uint32_t t = ((fwd >> j) & 1u) ? KMAN_GRAPH_L : KMAN_GRAPH_R;
            const uint32_t a = start[rj], pw = pos[rj];
            const uint32_t v = a < nt ? ord[a] : NONE;
            if ((uint64_t)v >= nu) continue;
            // v "+": entered at its first row's entry side; else at its last row's exit side, v "-"
            const bool plus = (pw >> 1) == 0 && t == ((pw & 1u) ^ 1u);
            const uint32_t word = (v << 1) | (plus ? 0u : 1u);  // (v < nu <= nt < 2^31)
#pragma unroll
            for (int q = 0; q < 4; q++) w[q] = q == (int)c ? word : w[q];  // (no indexed register array)
            c++;
        }
    }
    uint32_t tc = 0;
    const uint32_t ex = block_exclusive_scan<UT>(c, SumU32(), 0u, lds_c, &tc);
    if ((threadIdx.x >> 6) == 0) {
        const uint64_t base = wave_lookback<0>(status, tile, (uint64_t)tc, epoch, err);
        if (lane_id() == 0) lds_base = base;
    }
    __syncthreads();
    if (e < n_ends) {
        eoff[e] = lds_base + ex;
        ew[e] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

__global__ __launch_bounds__(UT) void edges_write_kernel(const uint4 *__restrict__ ew, const uint64_t *__restrict__ eoff,
                                                         uint64_t n_ends, uint64_t total,
                                                         uint64_t *__restrict__ d_eoff, uint32_t *__restrict__ d_edge) {
    const uint64_t e = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (e >= n_ends) return;
    if (e == 0) d_eoff[n_ends] = total;
    const uint64_t a = umin64(eoff[e], total);
    const uint64_t b = umin64(e + 1 < n_ends ? eoff[e + 1] : total, total);
    d_eoff[e] = a;
    const uint64_t c = b > a ? umin64(b - a, 4) : 0;  // (a + c <= b <= total)
    const uint4 w = ew[e];
    if (c > 0) d_edge[a] = w.x;
    if (c > 1) d_edge[a + 1] = w.y;
    if (c > 2) d_edge[a + 2] = w.z;
    if (c > 3) d_edge[a + 3] = w.w;
}

inline uint32_t blocks_of(uint64_t n) { return (uint32_t)ceil_div(n, UT); }

int graph_args(kman_ctx *ctx, const char *who, uint64_t nt) {
    if (nt >= KMAN_GRAPH_MAX_ROWS)
        return kman_fail(ctx, KMAN_EINVAL, "%s: %llu rows, a packed (row, side) word takes fewer than 2^31", who,
                         (unsigned long long)nt);
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_graph_links(kman_ctx *ctx, const uint64_t *d_tkeys, uint64_t nt, uint32_t k,
                                const uint64_t *d_index, uint32_t index_bits, uint32_t *d_link) {
    if (!ctx) return KMAN_EINVAL;
    if (k < 3 || k > 31 || (k & 1u) == 0)
        return kman_fail(ctx, KMAN_EINVAL, "kman_graph_links: k must be odd and in [3, 31], got %u", k);
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    KMAN_TRY(graph_args(ctx, "kman_graph_links", nt));
    if (nt == 0) return KMAN_OK;
    if (!d_tkeys || !d_index || !d_link) return kman_fail(ctx, KMAN_EINVAL, "kman_graph_links: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *scr = nullptr;
    KMAN_TRY(kman_scratch(ctx, (size_t)8 * nt, &scr));
    uint32_t *nb = (uint32_t *)scr;
    {
        KTimer kt_(ctx, "graph_links");
        hipLaunchKernelGGL(neighbours_kernel, dim3(blocks_of(nt)), dim3(UT), 0, ctx->stream, d_tkeys, (uint32_t)nt, k,
                           d_index, 2 * k - index_bits, nb);
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(mutual_kernel, dim3(blocks_of(2 * nt)), dim3(UT), 0, ctx->stream, nb, (uint32_t)(2 * nt),
                           d_link);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_graph_rank(kman_ctx *ctx, const uint32_t *d_link, uint64_t nt, uint32_t *d_start, uint32_t *d_pos,
                               uint32_t *d_nodes, uint32_t *rounds, uint64_t *cycles) {
    if (!ctx) return KMAN_EINVAL;
    KMAN_TRY(graph_args(ctx, "kman_graph_rank", nt));
    if (rounds) *rounds = 0;
    if (cycles) *cycles = 0;
    if (nt == 0) return KMAN_OK;
    if (!d_link || !d_start || !d_pos || !d_nodes) return kman_fail(ctx, KMAN_EINVAL, "kman_graph_rank: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint32_t n2 = (uint32_t)(2 * nt);
    // scratch: two flag words, two state buffers, two least-row buffers, the links' copy
    void *scr = nullptr;
    KMAN_TRY(kman_scratch(ctx, 16 + (size_t)n2 * (8 + 8 + 4 + 4 + 4), &scr));
    uint32_t *flags = (uint32_t *)scr;  // [0]: a pointer moved; [1]: cycles cut
    uint64_t *S[2] = {(uint64_t *)((char *)scr + 16), (uint64_t *)((char *)scr + 16) + n2};
    uint32_t *M[2] = {(uint32_t *)(S[1] + n2), (uint32_t *)(S[1] + n2) + n2};
    uint32_t *mine = M[1] + n2;
    uint32_t max_rounds = 1;  // ceil(log2(2 nt)) + 1
    while ((1ull << (max_rounds - 1)) < n2) max_rounds++;
    int cur = 0;
    uint32_t done = 0;
    uint32_t *h = (uint32_t *)ctx->h_small;
    auto run_rounds = [&]() -> int {
        for (uint32_t r = 0; r < max_rounds; r++) {
            HIP_TRY(ctx, hipMemsetAsync(flags, 0, 4, ctx->stream));
            hipLaunchKernelGGL(rank_round_kernel, dim3(blocks_of(n2)), dim3(UT), 0, ctx->stream, S[cur], M[cur], n2,
                               S[cur ^ 1], M[cur ^ 1], flags);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(h, flags, 4, hipMemcpyDeviceToHost, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            cur ^= 1;  // (a round in which nothing moved copied the states)
            if (h[0] == 0) break;
            done++;
        }
        return KMAN_OK;
    };
    {
        KTimer kt_(ctx, "graph_rank");
        HIP_TRY(ctx, hipMemsetAsync(flags, 0, 16, ctx->stream));
        hipLaunchKernelGGL(rank_init_kernel, dim3(blocks_of(n2)), dim3(UT), 0, ctx->stream, d_link, n2, mine, S[0],
                           M[0]);
        HIP_TRY(ctx, hipGetLastError());
        KMAN_TRY(run_rounds());
        hipLaunchKernelGGL(cycle_cut_kernel, dim3(blocks_of(nt)), dim3(UT), 0, ctx->stream, d_link, S[cur], M[cur],
                           (uint32_t)nt, mine, flags + 1);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(h, flags + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t ncut = h[0];
        if (cycles) *cycles = ncut;
        if (ncut) {
            hipLaunchKernelGGL(rank_again_kernel, dim3(blocks_of(n2)), dim3(UT), 0, ctx->stream, d_link, mine, n2,
                               S[cur], M[cur]);
            HIP_TRY(ctx, hipGetLastError());
            KMAN_TRY(run_rounds());
        }
        hipLaunchKernelGGL(rank_finish_kernel, dim3(blocks_of(nt)), dim3(UT), 0, ctx->stream, S[cur], (uint32_t)nt,
                           d_start, d_pos, d_nodes);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (rounds) *rounds = done;
    return KMAN_OK;
}

extern "C" int kman_unitig_spell(kman_ctx *ctx, const uint64_t *d_tkeys, const void *d_tcounts, uint32_t count_bytes,
                                 uint64_t nt, uint32_t k, const uint32_t *d_start, const uint32_t *d_pos,
                                 const uint32_t *d_nodes, uint64_t *d_off, uint32_t *d_unodes, uint64_t *d_kc,
                                 uint64_t unitig_cap, uint8_t *d_seq, uint64_t seq_cap, uint64_t *n_unitigs,
                                 uint64_t *n_bases) {
    if (!ctx || !n_unitigs || !n_bases) return KMAN_EINVAL;
    if (k < 3 || k > 31 || (k & 1u) == 0)
        return kman_fail(ctx, KMAN_EINVAL, "kman_unitig_spell: k must be odd and in [3, 31], got %u", k);
    if (count_bytes != 4 && count_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "count widths must be 4 or 8 bytes");
    KMAN_TRY(graph_args(ctx, "kman_unitig_spell", nt));
    const bool count_only = !d_off && !d_unodes && !d_kc && !d_seq;
    if (!count_only && (!d_off || !d_unodes || !d_kc || !d_seq))
        return kman_fail(ctx, KMAN_EINVAL, "kman_unitig_spell: the four outputs go together (all, or none to count)");
    *n_unitigs = *n_bases = 0;
    if (nt == 0) return KMAN_OK;
    if (!d_pos || !d_nodes || (!count_only && (!d_tkeys || !d_tcounts || !d_start)))
        return kman_fail(ctx, KMAN_EINVAL, "kman_unitig_spell: null buffer");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    void *scr = nullptr;
    KMAN_TRY(kman_scratch(ctx, (size_t)12 * nt + 8, &scr));
    uint64_t *hoff = (uint64_t *)scr;
    uint32_t *ord = (uint32_t *)(hoff + nt);
    const uint64_t T = ceil_div(nt, UTILE);
    uint64_t nu = 0, total = 0;
    {
        KTimer kt_(ctx, "unitig_spell");
        uint32_t epoch, *counter;
        KMAN_TRY(kman_lookback_begin(ctx, 2 * T, &epoch, &counter));
        hipLaunchKernelGGL(layout_kernel<true>, dim3((uint32_t)T), dim3(UT), 0, ctx->stream, d_pos, d_nodes, (uint32_t)nt, k,
                           ord, hoff, ctx->d_status, T, counter, epoch, ctx->d_err);
        HIP_TRY(ctx, hipGetLastError());
    }
    KMAN_TRY(kman_lookback_total(ctx, T, &nu));
    KMAN_TRY(kman_lookback_total(ctx, 2 * T, &total));
    *n_unitigs = nu;
    *n_bases = total;
    if (count_only) return KMAN_OK;
    if (nu > unitig_cap || total > seq_cap)
        return kman_fail(ctx, KMAN_ECAP, "kman_unitig_spell: %llu unitigs of %llu bases for capacities %llu and %llu",
                         (unsigned long long)nu, (unsigned long long)total, (unsigned long long)unitig_cap,
                         (unsigned long long)seq_cap);
    HIP_TRY(ctx, hipMemsetAsync(d_kc, 0, (size_t)8 * nu, ctx->stream));
    {
        KTimer kt_(ctx, "unitig_spell");
        if (count_bytes == 4)
            hipLaunchKernelGGL((spell_kernel<uint32_t>), dim3(blocks_of(nt)), dim3(UT), 0, ctx->stream, d_tkeys,
                               (const uint32_t *)d_tcounts, (uint32_t)nt, k, d_start, d_pos, d_nodes, ord, hoff, nu,
                               total, d_off, d_unodes, (unsigned long long *)d_kc, d_seq);
        else
            hipLaunchKernelGGL((spell_kernel<uint64_t>), dim3(blocks_of(nt)), dim3(UT), 0, ctx->stream, d_tkeys,
                               (const uint64_t *)d_tcounts, (uint32_t)nt, k, d_start, d_pos, d_nodes, ord, hoff, nu,
                               total, d_off, d_unodes, (unsigned long long *)d_kc, d_seq);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_unitig_edges(kman_ctx *ctx, const uint64_t *d_tkeys, uint64_t nt, uint32_t k,
                                 const uint64_t *d_index, uint32_t index_bits, const uint32_t *d_start,
                                 const uint32_t *d_pos, const uint32_t *d_nodes, uint64_t *d_eoff, uint64_t end_cap,
                                 uint32_t *d_edge, uint64_t edge_cap, uint64_t *n_ends, uint64_t *n_edges) {
    if (!ctx || !n_ends || !n_edges) return KMAN_EINVAL;
    if (k < 3 || k > 31 || (k & 1u) == 0)
        return kman_fail(ctx, KMAN_EINVAL, "kman_unitig_edges: k must be odd and in [3, 31], got %u", k);
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    KMAN_TRY(graph_args(ctx, "kman_unitig_edges", nt));
    const bool count_only = !d_eoff && !d_edge;
    if (!count_only && (!d_eoff || !d_edge))
        return kman_fail(ctx, KMAN_EINVAL, "kman_unitig_edges: the two outputs go together (both, or none to count)");
    if (nt > 0 && (!d_tkeys || !d_index || !d_start || !d_pos || !d_nodes))
        return kman_fail(ctx, KMAN_EINVAL, "kman_unitig_edges: null buffer");
    *n_ends = *n_edges = 0;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (nt == 0) {
        if (d_eoff) {
            HIP_TRY(ctx, hipMemsetAsync(d_eoff, 0, 8, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        return KMAN_OK;
    }
    // the heads' ordinals live in the second scratch: the first one is sized once the ends are counted
    void *aux = nullptr;
    KMAN_TRY(kman_aux(ctx, (size_t)4 * nt, &aux));
    uint32_t *ord = (uint32_t *)aux;
    const uint64_t T = ceil_div(nt, UTILE);
    uint64_t nu = 0, ne = 0, total = 0;
    {
        KTimer kt_(ctx, "unitig_edges");
        uint32_t epoch, *counter;
        KMAN_TRY(kman_lookback_begin(ctx, T, &epoch, &counter));
        hipLaunchKernelGGL(layout_kernel<false>, dim3((uint32_t)T), dim3(UT), 0, ctx->stream, d_pos,
                           (const uint32_t *)nullptr, (uint32_t)nt, k, ord, (uint64_t *)nullptr, ctx->d_status, T,
                           counter, epoch, ctx->d_err);
        HIP_TRY(ctx, hipGetLastError());
    }
    KMAN_TRY(kman_lookback_total(ctx, T, &nu));
    if (nu > nt) return kman_fail(ctx, KMAN_EHIP, "kman_unitig_edges: %llu heads in %llu rows", (unsigned long long)nu,
                                  (unsigned long long)nt);
    ne = 2 * nu;
    uint4 *ew = nullptr;
    uint64_t *eoff = nullptr;
    if (ne) {
        void *scr = nullptr;
        KMAN_TRY(kman_scratch(ctx, (size_t)28 * ne, &scr));
        ew = (uint4 *)scr;
        eoff = (uint64_t *)(ew + ne);
        uint32_t *endw = (uint32_t *)(eoff + ne);
        const uint64_t T2 = ceil_div(ne, ETILE);
        {
            KTimer kt_(ctx, "unitig_edges");
            HIP_TRY(ctx, hipMemsetAsync(endw, 0xFF, (size_t)4 * ne, ctx->stream));
            hipLaunchKernelGGL(ends_kernel, dim3(blocks_of(nt)), dim3(UT), 0, ctx->stream, d_start, d_pos, d_nodes, ord,
                               (uint32_t)nt, nu, endw);
            HIP_TRY(ctx, hipGetLastError());
            uint32_t epoch, *counter;
            KMAN_TRY(kman_lookback_begin(ctx, T2, &epoch, &counter));
            hipLaunchKernelGGL(edges_kernel, dim3((uint32_t)T2), dim3(UT), 0, ctx->stream, d_tkeys, (uint32_t)nt, k,
                               d_index, 2 * k - index_bits, d_start, d_pos, ord, endw, ne, ew, eoff, ctx->d_status,
                               counter, epoch, ctx->d_err);
            HIP_TRY(ctx, hipGetLastError());
        }
        KMAN_TRY(kman_lookback_total(ctx, T2, &total));
    }
    *n_ends = ne;
    *n_edges = total;
    if (count_only) return KMAN_OK;
    if (ne > end_cap || total > edge_cap)
        return kman_fail(ctx, KMAN_ECAP, "kman_unitig_edges: %llu ends with %llu edges for capacities %llu and %llu",
                         (unsigned long long)ne, (unsigned long long)total, (unsigned long long)end_cap,
                         (unsigned long long)edge_cap);
    {
        KTimer kt_(ctx, "unitig_edges");
        if (ne) {
            hipLaunchKernelGGL(edges_write_kernel, dim3(blocks_of(ne)), dim3(UT), 0, ctx->stream, ew, eoff, ne, total,
                               d_eoff, d_edge);
            HIP_TRY(ctx, hipGetLastError());
        } else {
            HIP_TRY(ctx, hipMemsetAsync(d_eoff, 0, 8, ctx->stream));
        }
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

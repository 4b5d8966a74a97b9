// quantile.hip — a per-record order statistic of the k-mer counts of a read:
// kman_window_counts writes one u32 per base (the table count of the window
// that starts there), kman_record_quantile selects one quantile of those
// words inside every record (`kmer screen --median`).
//
// kman_window_counts, one block of 256 threads per tile of WTILE = 4096
// windows: screen_kernel's staging (stage_codes), roll<16, CANON> and lookup
// (screen_lookup.h, the same function), then, instead of the per-record
// reduction, each thread stores the words of its 16 consecutive windows as
// four 16-byte vectors.  Per valid window the lookup's bytes (screen.hip) and
// a 4 B store.
//
// kman_record_quantile, short records (<= QCAP bases): one block of 256
// threads per chunk of QC = 4096 bases.  A chunk owns the records that start
// in it (segsort.hip's rule): it stages d_wc from the chunk's first base to the
// end of its last short record (region = QC + QCAP words of LDS) and the
// chunk's slice of d_rec_seq (<= QSLICE records; a larger slice is read from
// global memory, record by record).  A wave takes every fourth record and
// radix-selects its quantile: four passes over the record's staged words, most
// significant 8-bit digit first, each into the wave's own 256 counters
// (LDS atomics), the digit that holds the rank found by one wave scan over the
// counters.  KMAN_WC_NONE words are counted in the first pass (w = length -
// NONE words) and sort last, so rank floor((w - 1) num / den) never selects
// one.  One d_q word per record, a direct store; no block barrier after the
// staging.  Every word of d_wc is read from HBM once, plus the chunk's tail.
//
// Long records (> QCAP bases) are listed by the chunk that owns their start
// (ordinal, first base, length).  The host reads the list, lays the records'
// words out contiguously as u64 keys (slot << 32) | word, sorts them with
// kman_sort over 32 + bits(slots) key bits (KMAN_WC_NONE sorts last inside
// its slot) and one thread per long record picks keys[start + rank], w from a
// lower bound on the slot's first NONE.  All of it lives in the caller's work
// buffer (kman_record_quantile_plan).
//
// Bounds, not values: entries of d_rec_seq are clamped to n_bases, a record is
// staged only when its first base lies in the chunk and its length is <= QCAP
// (so every LDS index is < QC + QCAP), every record index is < n_records,
// every list slot is < its capacity, every search runs a step count fixed
// before it starts.  An unsorted d_rec_seq gives wrong (or unwritten) values,
// never a wild address.
#include "common.h"
#include "kmer.h"
#include "screen_lookup.h"
#include "tile_records.h"

namespace {

constexpr int WT = 256;
constexpr int WEI = 16;
constexpr int WTILE = WT * WEI;
static_assert(WTILE == KMAN_SCREEN_TILE, "kman_window_counts runs on kman_screen_records' tile");

#define WC_NONE KMAN_WC_NONE
#define WC_MAX 0xFFFFFFFEu  // the largest count a word holds: larger ones saturate

constexpr int QT = 256;         // threads per chunk
constexpr int QW = QT / 64;     // waves: one record each at a time
constexpr int QC = 4096;        // chunk: records that start here are owned
constexpr int QCAP = 2048;      // the longest record staged in LDS
constexpr int QR = QC + QCAP;   // region: chunk + tail of its last short record
constexpr int QSLICE = 1024;    // records of a chunk whose d_rec_seq entries are staged
constexpr size_t QHDR = 256;    // work buffer: the list count lives in its first bytes
static_assert(QC == KMAN_QUANTILE_TILE, "include/kman.h states the chunk size");
static_assert(QCAP == KMAN_QUANTILE_REC_CAP, "include/kman.h states the longest staged record");
static_assert(QSLICE == KMAN_QUANTILE_SLICE, "include/kman.h states the staged slice of d_rec_seq");
static_assert(QC % 4 == 0 && QR % 4 == 0, "16-byte staging");

template <int CANON, typename CT>
__global__ __launch_bounds__(WT) void window_counts_kernel(const uint8_t *__restrict__ codes, uint64_t n_bases, int k,
                                                           const uint64_t *__restrict__ tkeys,
                                                           const CT *__restrict__ tcounts, uint64_t nt,
                                                           const uint64_t *__restrict__ index, uint32_t shift,
                                                           uint32_t *__restrict__ wc) {
    __shared__ __attribute__((aligned(16))) uint8_t scodes[WTILE + 64];
    const uint64_t tb = (uint64_t)blockIdx.x * WTILE;
    stage_codes<WT, WEI>(codes, n_bases, tb, scodes);
    __syncthreads();

    const uint64_t mask = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    uint64_t kf[WEI], kr[WEI];
    const uint64_t p0 = tb + (uint64_t)threadIdx.x * WEI;
    const uint32_t valid = roll<WEI, CANON>(scodes, threadIdx.x * WEI, k, mask, p0, n_bases, kf, kr);
    uint64_t cnt[WEI];
    table_lookup<WEI, CT>(valid, kf, shift, index, tkeys, tcounts, nt, cnt);

    uint32_t word[WEI];
#pragma unroll
    for (int j = 0; j < WEI; j++)
        word[j] = ((valid >> j) & 1u) ? (cnt[j] > (uint64_t)WC_MAX ? WC_MAX : (uint32_t)cnt[j]) : WC_NONE;
    if (p0 + WEI <= n_bases) {
        // 64 contiguous bytes per thread (p0 is a multiple of 16 words, wc 16-byte aligned)
        uint4 *dst = reinterpret_cast<uint4 *>(wc + p0);
#pragma unroll
        for (int q = 0; q < WEI / 4; q++) dst[q] = make_uint4(word[4 * q], word[4 * q + 1], word[4 * q + 2], word[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < WEI; j++)
            if (p0 + j < n_bases) wc[p0 + j] = word[j];
    }
}

template <int CANON, typename CT>
void launch_window_counts(kman_ctx *ctx, const uint8_t *codes, uint64_t n_bases, uint32_t k, const uint64_t *tkeys,
                          const void *tcounts, uint64_t nt, const uint64_t *index, uint32_t shift, uint32_t *wc,
                          uint64_t tiles) {
    hipLaunchKernelGGL((window_counts_kernel<CANON, CT>), dim3((uint32_t)tiles), dim3(WT), 0, ctx->stream, codes,
                       n_bases, (int)k, tkeys, (const CT *)tcounts, nt, index, shift, wc);
}

// ------------------------------------------------------------ record quantile

// LDS writes of this wave before, its LDS reads after
KMAN_DEV void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// floor((w - 1) * num / den) for w >= 1: < w since num <= den
KMAN_DEV uint64_t rank_of(uint64_t w, uint32_t num, uint32_t den) { return (w - 1) * (uint64_t)num / (uint64_t)den; }

// One wave: the word of rank floor((w - 1) num / den) among the non-NONE
// words of v[0, len), 0 when there is none.  wh: the wave's 256 counters.
// Called with all 64 lanes active and wave-uniform arguments.
KMAN_DEV uint32_t wave_select(const uint32_t *v, uint32_t len, uint32_t num, uint32_t den, uint32_t *wh) {
    const int lane = lane_id();
    uint32_t prefix = 0, pmask = 0, t = 0;
#pragma unroll 1
    for (int pass = 0; pass < 4; pass++) {
        const uint32_t sh = 24u - 8u * (uint32_t)pass;
        *reinterpret_cast<uint4 *>(wh + 4 * lane) = make_uint4(0, 0, 0, 0);
        wave_sync_lds();
        uint32_t n_none = 0;
        for (uint32_t i0 = 0; i0 < len; i0 += 64) {
            const uint32_t i = i0 + (uint32_t)lane;
            const uint32_t x = i < len ? v[i] : 0u;
            if (pass == 0) n_none += (uint32_t)__popcll(__ballot(i < len && x == WC_NONE));
            if (i < len && (x & pmask) == prefix) atomicAdd(&wh[(x >> sh) & 255u], 1u);
        }
        if (pass == 0) {
            const uint32_t w = len - n_none;
            if (w == 0) return 0u;  // (wave-uniform)
            t = (uint32_t)rank_of(w, num, den);
        }
        wave_sync_lds();
        const uint4 c = *reinterpret_cast<const uint4 *>(wh + 4 * lane);
        const uint32_t s = c.x + c.y + c.z + c.w;
        const uint32_t inc = wave_inclusive_scan(s, SumU32());
        const uint64_t over = __ballot(t < inc);
        // (t < the pass's candidates, so a lane exists; lane 63 otherwise keeps the digit in range)
        const int src = over ? __ffsll((unsigned long long)over) - 1 : 63;
        uint32_t tt = t - (inc - s), d = 0;
        if (tt >= c.x) {
            tt -= c.x;
            d = 1;
            if (tt >= c.y) {
                tt -= c.y;
                d = 2;
                if (tt >= c.z) {
                    tt -= c.z;
                    d = 3;
                }
            }
        }
        const uint32_t digit = (uint32_t)__shfl((int)(4u * (uint32_t)lane + d), src, 64);
        t = (uint32_t)__shfl((int)tt, src, 64);
        prefix |= digit << sh;
        pmask |= 255u << sh;
        wave_sync_lds();  // (the counters are read before the next pass clears them)
    }
    return prefix;
}

__global__ __launch_bounds__(QT) void record_quantile_kernel(const uint32_t *__restrict__ wc, uint64_t n_bases,
                                                             const uint64_t *__restrict__ rec_seq, uint64_t n_records,
                                                             uint32_t num, uint32_t den, uint32_t *__restrict__ q,
                                                             uint32_t *__restrict__ n_long, uint64_t *__restrict__ list,
                                                             uint64_t list_cap) {
    __shared__ __attribute__((aligned(16))) uint32_t sv[QR];
    __shared__ uint64_t srec[QSLICE + 1];
    __shared__ __attribute__((aligned(16))) uint32_t wh[QW][256];
    __shared__ uint64_t s_rlo, s_rhi, s_need;

    const uint64_t cb = (uint64_t)blockIdx.x * QC;  // (cb <= n_bases: the grid is n_bases / QC + 1 chunks)
    if (threadIdx.x == 0) {
        // the records whose first base, clamped to n_bases, lies in [cb, cb + QC)
        const uint64_t rlo = lower_count(rec_seq, n_records, cb);
        uint64_t rhi = cb + QC > n_bases ? n_records : lower_count(rec_seq, n_records, cb + QC);
        if (rhi < rlo) rhi = rlo;  // (unsorted entries)
        // staged: the chunk, and the tail of its last record when that one is short
        uint64_t need = umin64(cb + QC, n_bases);
        if (rhi > rlo) {
            const uint64_t s = umin64(rec_seq[rhi - 1], n_bases);
            const uint64_t e = rhi < n_records ? umin64(rec_seq[rhi], n_bases) : n_bases;
            if (e > need && e >= s && e - s <= (uint64_t)QCAP) need = e;
        }
        s_rlo = rlo;
        s_rhi = rhi;
        s_need = umin64(need, cb + QR);
    }
    __syncthreads();
    const uint64_t rlo = s_rlo, rhi = s_rhi, need = s_need;
    if (rhi == rlo) return;
    const uint64_t ns = rhi - rlo;
    const bool staged = ns <= (uint64_t)QSLICE;
    if (staged)
        for (uint32_t i = threadIdx.x; i <= (uint32_t)ns; i += QT)
            srec[i] = rlo + i < n_records ? umin64(rec_seq[rlo + i], n_bases) : n_bases;
    for (uint32_t i = threadIdx.x; i < (uint32_t)(QR / 4); i += QT) {
        const uint64_t b = cb + 4ull * i;
        if (b + 4 <= need) {
            *reinterpret_cast<uint4 *>(sv + 4 * i) = *reinterpret_cast<const uint4 *>(wc + b);
        } else {
            for (int j = 0; j < 4; j++)
                if (b + j < need) sv[4 * i + j] = wc[b + j];
        }
    }
    __syncthreads();

    const int w = threadIdx.x >> 6;
    const int lane = lane_id();
    for (uint64_t r = rlo + (uint64_t)w; r < rhi; r += QW) {
        uint64_t s, e;
        if (staged) {
            s = srec[r - rlo];
            e = srec[r - rlo + 1];
        } else {
            s = umin64(rec_seq[r], n_bases);
            e = r + 1 < n_records ? umin64(rec_seq[r + 1], n_bases) : n_bases;
        }
        if (s < cb || s - cb >= (uint64_t)QC) continue;  // (unsorted entries: not this chunk's)
        const uint64_t len = e > s ? e - s : 0;
        if (len > (uint64_t)QCAP) {
            if (lane == 0) {
                const uint32_t slot = atomicAdd(n_long, 1u);
                if ((uint64_t)slot < list_cap) {
                    list[3 * (uint64_t)slot] = r;
                    list[3 * (uint64_t)slot + 1] = s;
                    list[3 * (uint64_t)slot + 2] = len;
                }
            }
            continue;
        }
        // (s - cb < QC and len <= QCAP: inside sv)
        const uint32_t res = len ? wave_select(sv + (uint32_t)(s - cb), (uint32_t)len, num, den, wh[w]) : 0u;
        if (lane == 0) q[r] = res;
    }
}

// long records: tab[4 g ..] = (record, first base, offset among the gathered words, length)
__global__ __launch_bounds__(256) void long_gather_kernel(const uint32_t *__restrict__ wc,
                                                          const uint64_t *__restrict__ tab, uint32_t n_long,
                                                          uint64_t total, uint64_t *__restrict__ keys) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total;
         j += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_long;  // the last slot whose offset is <= j
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (tab[4 * (uint64_t)mid + 2] <= j) lo = mid;
            else hi = mid;
        }
        const uint64_t at = j - tab[4 * (uint64_t)lo + 2];
        if (at >= tab[4 * (uint64_t)lo + 3]) continue;  // (cannot happen: the offsets are the lengths' prefix sums)
        keys[j] = ((uint64_t)lo << 32) | (uint64_t)wc[tab[4 * (uint64_t)lo + 1] + at];
    }
}

__global__ __launch_bounds__(256) void long_pick_kernel(const uint64_t *__restrict__ keys,
                                                        const uint64_t *__restrict__ tab, uint32_t n_long,
                                                        uint64_t n_records, uint32_t num, uint32_t den,
                                                        uint32_t *__restrict__ q) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_long) return;
    const uint64_t r = tab[4 * (uint64_t)g], off = tab[4 * (uint64_t)g + 2], len = tab[4 * (uint64_t)g + 3];
    if (r >= n_records) return;
    const uint64_t *seg = keys + off;
    const uint64_t none = ((uint64_t)g << 32) | (uint64_t)WC_NONE;
    const uint64_t w = lower_count(seg, len, none);  // NONE sorts last inside the slot
    q[r] = w ? (uint32_t)seg[rank_of(w, num, den)] : 0u;
}

uint32_t host_bits(uint64_t v) {
    uint32_t b = 0;
    for (; v; v >>= 1) b++;
    return b;
}

}  // namespace

extern "C" int kman_window_counts(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                                  const uint64_t *d_tkeys, const void *d_tcounts, uint32_t t_count_bytes, uint64_t nt,
                                  const uint64_t *d_index, uint32_t index_bits, uint32_t *d_wc) {
    if (!ctx) return KMAN_EINVAL;
    if (k < 2 || k > 32) return kman_fail(ctx, KMAN_EINVAL, "k must be in [2, 32] on the GPU path, got %u", k);
    if (flags & ~KMAN_CANONICAL) return kman_fail(ctx, KMAN_EINVAL, "kman_window_counts: flags 0x%x", flags);
    if (t_count_bytes != 4 && t_count_bytes != 8)
        return kman_fail(ctx, KMAN_EINVAL, "count widths must be 4 or 8 bytes");
    if (!index_bits_ok(k, index_bits))
        return kman_fail(ctx, KMAN_EINVAL, "index_bits must be in [1, min(2k, %d)], got %u (k = %u)",
                         KMAN_SCREEN_MAX_INDEX_BITS, index_bits, k);
    if (n_bases == 0) return KMAN_OK;
    if (!d_wc) return kman_fail(ctx, KMAN_EINVAL, "kman_window_counts: null buffer");
    if (((uintptr_t)d_wc & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "d_wc must be 16-byte aligned");
    if (n_bases >= k) {
        if (!d_codes || !d_index || (nt && (!d_tkeys || !d_tcounts)))
            return kman_fail(ctx, KMAN_EINVAL, "kman_window_counts: null buffer");
        if (((uintptr_t)d_codes & 15) != 0) return kman_fail(ctx, KMAN_EINVAL, "codes must be 16-byte aligned");
    }
    const uint64_t tiles = ceil_div(n_bases, WTILE);
    if (tiles > 0x7ffffffeull)
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases: too many tiles", (unsigned long long)n_bases);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (n_bases < k) {
        // no window at all: every word is KMAN_WC_NONE
        HIP_TRY(ctx, hipMemsetAsync(d_wc, 0xFF, (size_t)(4 * n_bases), ctx->stream));
    } else {
        const uint32_t shift = 2 * k - index_bits;
        KTimer kt_(ctx, "window_counts");
        if (flags & KMAN_CANONICAL) {
            if (t_count_bytes == 4)
                launch_window_counts<1, uint32_t>(ctx, d_codes, n_bases, k, d_tkeys, d_tcounts, nt, d_index, shift,
                                                  d_wc, tiles);
            else
                launch_window_counts<1, uint64_t>(ctx, d_codes, n_bases, k, d_tkeys, d_tcounts, nt, d_index, shift,
                                                  d_wc, tiles);
        } else {
            if (t_count_bytes == 4)
                launch_window_counts<0, uint32_t>(ctx, d_codes, n_bases, k, d_tkeys, d_tcounts, nt, d_index, shift,
                                                  d_wc, tiles);
            else
                launch_window_counts<0, uint64_t>(ctx, d_codes, n_bases, k, d_tkeys, d_tcounts, nt, d_index, shift,
                                                  d_wc, tiles);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

extern "C" int kman_record_quantile_plan(uint64_t n_long_records, uint64_t n_long_values, uint64_t *work_bytes) {
    if (!work_bytes) return KMAN_EINVAL;
    *work_bytes = 0;
    if (n_long_records > 0xffffffffull || n_long_values > (~0ull >> 6)) return KMAN_EINVAL;
    // the list count; one (record, first base, offset, length) row per long
    // record (the first run's list of three words per record fits it); the
    // keys and their sort's second buffer
    *work_bytes = QHDR + 32 * n_long_records + 16 * n_long_values;
    return KMAN_OK;
}

extern "C" int kman_record_quantile(kman_ctx *ctx, uint32_t *d_wc, uint64_t n_bases, const uint64_t *d_rec_seq,
                                    uint64_t n_records, uint32_t num, uint32_t den, void *d_work, uint64_t work_bytes,
                                    uint32_t *d_q) {
    if (!ctx) return KMAN_EINVAL;
    if (den < 1 || den > 65535 || num > den)
        return kman_fail(ctx, KMAN_EINVAL, "quantile %u / %u: 1 <= den <= 65535 and num <= den", num, den);
    if (n_records == 0) return KMAN_OK;
    if (!d_rec_seq || !d_q || !d_work || (n_bases && !d_wc))
        return kman_fail(ctx, KMAN_EINVAL, "kman_record_quantile: null buffer");
    if (((uintptr_t)d_wc & 15) != 0 || ((uintptr_t)d_work & 15) != 0)
        return kman_fail(ctx, KMAN_EINVAL, "d_wc and d_work must be 16-byte aligned");
    const uint64_t chunks = n_bases / QC + 1;
    if (chunks > 0x7ffffffeull)
        return kman_fail(ctx, KMAN_EINVAL, "%llu bases: too many chunks", (unsigned long long)n_bases);
    if (work_bytes < QHDR)
        return kman_fail(ctx, KMAN_ECAP, "work buffer of %llu bytes: kman_record_quantile_plan asks for at least %llu",
                         (unsigned long long)work_bytes, (unsigned long long)QHDR);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    uint32_t *d_nlong = (uint32_t *)d_work;
    uint64_t *d_body = (uint64_t *)((char *)d_work + QHDR);
    const uint64_t list_cap = (work_bytes - QHDR) / 24;
    HIP_TRY(ctx, hipMemsetAsync(d_nlong, 0, QHDR, ctx->stream));
    {
        KTimer kt_(ctx, "record_quantile");
        hipLaunchKernelGGL(record_quantile_kernel, dim3((uint32_t)chunks), dim3(QT), 0, ctx->stream, d_wc, n_bases,
                           d_rec_seq, n_records, num, den, d_q, d_nlong, d_body, list_cap);
        HIP_TRY(ctx, hipGetLastError());
    }
    uint32_t nl = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&nl, d_nlong, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (nl == 0) return KMAN_OK;
    if ((uint64_t)nl > list_cap)
        return kman_fail(ctx, KMAN_ECAP, "%u long records do not fit the work buffer (kman_record_quantile_plan)", nl);
    // ---- the long records: gathered as (slot, word) keys, sorted, picked
    std::vector<uint64_t> list(3 * (size_t)nl), tab(4 * (size_t)nl);
    HIP_TRY(ctx, hipMemcpyAsync(list.data(), d_body, 24 * (size_t)nl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> order(nl);
    for (uint32_t i = 0; i < nl; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return list[3 * (size_t)a] < list[3 * (size_t)b]; });
    uint64_t nv = 0;
    for (uint32_t g = 0; g < nl; g++) {
        const size_t i = order[g];
        tab[4 * (size_t)g] = list[3 * i];
        tab[4 * (size_t)g + 1] = list[3 * i + 1];
        tab[4 * (size_t)g + 2] = nv;
        tab[4 * (size_t)g + 3] = list[3 * i + 2];
        nv += list[3 * i + 2];  // (each <= n_bases: no overflow for any nl < 2^32)
    }
    uint64_t want = 0;
    KMAN_TRY(kman_record_quantile_plan(nl, nv, &want));
    if (want > work_bytes)
        return kman_fail(ctx, KMAN_ECAP, "%u long records of %llu words need a work buffer of %llu bytes, got %llu", nl,
                         (unsigned long long)nv, (unsigned long long)want, (unsigned long long)work_bytes);
    uint64_t *d_tab = d_body, *d_k0 = d_body + 4 * (size_t)nl, *d_k1 = d_k0 + nv;
    HIP_TRY(ctx, hipMemcpyAsync(d_tab, tab.data(), 32 * (size_t)nl, hipMemcpyHostToDevice, ctx->stream));
    {
        KTimer kt_(ctx, "record_quantile_long");
        const uint32_t cg = (uint32_t)(ceil_div(nv, 256) < 65536 ? ceil_div(nv, 256) : 65536);
        hipLaunchKernelGGL(long_gather_kernel, dim3(cg), dim3(256), 0, ctx->stream, d_wc, d_tab, nl, nv, d_k0);
        HIP_TRY(ctx, hipGetLastError());
    }
    int in_alt = 0;
    const uint32_t key_bits = 32 + (nl > 1 ? host_bits((uint64_t)nl - 1) : 1);
    KMAN_TRY(kman_sort(ctx, d_k0, d_k1, nullptr, nullptr, 0, nv, key_bits, nullptr, &in_alt));
    {
        KTimer kt_(ctx, "record_quantile_long");
        hipLaunchKernelGGL(long_pick_kernel, dim3((nl + 255) / 256), dim3(256), 0, ctx->stream, in_alt ? d_k1 : d_k0,
                           d_tab, nl, n_records, num, den, d_q);
        HIP_TRY(ctx, hipGetLastError());
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return KMAN_OK;
}

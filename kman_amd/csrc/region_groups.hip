// region_groups.hip — kman_groups: the plan of one region-path call (region.h)
// and the entry points that run its three stages on one device.
#include "region.h"

#include <cstdio>
#include <cstdlib>

using namespace kman::region;

namespace {

constexpr int RSI = 16;           // items per thread, pass 1
constexpr uint64_t T1 = (uint64_t)RT * RSI;  // pass-1 tile

int make_plan(uint64_t n_bases, uint32_t k, uint32_t flags, int mode, RegionPlan *pl) {
    if (mode != KMAN_FINISH_COUNT && mode != KMAN_FINISH_UNIQ) return KMAN_EINVAL;
    if (k < 2 || k > 32) return KMAN_EINVAL;
    if (getenv("KMAN_NO_REGION")) return KMAN_EFALLBACK;  // (tests: the general path)
    // uniq: k <= 25 (the tile-local window index rides above the key bits in
    // pass 0); count items carry no index: k <= 32
    if ((mode == KMAN_FINISH_UNIQ && k > 25) || n_bases == 0) return KMAN_EFALLBACK;
    RegionPlan p{};
    // canonical: one key per window, min(forward, reverse complement)
    p.canon = flags & KMAN_CANONICAL;
    p.mix = p.canon && (flags & KMAN_MIXED);
    p.rc = (flags & KMAN_RC) && !p.canon;
    p.K = 2 * k;
    p.W = n_bases * (p.rc ? 2 : 1);
    p.Q = mode == KMAN_FINISH_UNIQ ? (bitlen(p.W - 1) ? bitlen(p.W - 1) : 1u) : 0u;
    if (p.K - G1 + p.Q > 64) return KMAN_EFALLBACK;
    // B2: fewest bits with an expected region fill <= FFILL_T (at most 9); up
    // to FFILL_M expected keeps > 10 sd (uniform data) below the capacity
    uint32_t b2 = 1;
    // (17 region bits in all while their fill stays <= FFILL_M: the finish's
    // per-region costs make more, smaller regions slower)
    while (b2 < 9 && (p.W >> (G1 + b2)) > FFILL_T && (G1 + b2 < 17 || (p.W >> (G1 + b2)) > FFILL_M)) b2++;
    if ((p.W >> (G1 + b2)) > FFILL_M) return KMAN_EFALLBACK;
    if (p.K < G1 + b2 + 1) return KMAN_EFALLBACK;
    p.B2 = b2;
    p.rest = p.K - G1 - b2;
    // windows per thread: 16 (8 with -r: two items per window) makes
    // 8192-item tiles, 69 KiB of LDS, two blocks per CU: with the atomic
    // region cursors a tile waits on nothing and the longer digit runs win
    // (3.27 vs 3.35 ms with 12 windows, three blocks per CU; 8, four blocks:
    // 3.83)
    p.ei = p.rc ? 8u : 16u;
    const uint64_t win = (uint64_t)RT * p.ei;
    p.n_tiles0 = (uint32_t)ceil_div(n_bases, win);
    p.seg_tiles = (uint32_t)ceil_div(p.n_tiles0, RS);
    const uint64_t nb0 = 1ull << G1;  // pass-0 buckets
    const uint64_t e0 = p.W / (nb0 * RS);
    p.C0 = ceil_div(e0 + e0 / 2 + 256, 64) * 64;
    if (nb0 * RS * p.C0 >= (1ull << 32)) return KMAN_EFALLBACK;  // (32-bit item indices)
    const uint64_t e1 = p.W >> (G1 + b2);
    uint64_t c1 = ceil_div(e1 + e1 / 2 + 512, 64) * 64;
    // (a multiple of 32 either way, and off_r1 of 512 bytes: pass 1's 256-byte lines)
    static_assert(FCAP % 32 == 0, "a sub-region ends on a 256-byte line");
    p.C1 = c1 < (uint64_t)FCAP ? c1 : (uint64_t)FCAP;
    // pass 1 runs H = 2 block-owned chains per bucket (its first and second
    // half of tiles) into H sub-regions per region that the finish
    // concatenates: 512 chains for the 256 resident blocks
    p.H = 2;
    p.C1h = p.C1;  // either half may hold most of a region (position-skewed repeats)
    p.maxt1 = (uint32_t)ceil_div((uint64_t)ceil_div(RS, p.H) * p.C0, T1);
    const uint64_t nreg = 1ull << (G1 + b2);
    p.off_r1 = nb0 * RS * p.C0 * 8;
    p.off_c0 = p.off_r1 + nreg * p.H * p.C1h * 8;
    p.off_c1 = p.off_c0 + nb0 * RS * 4;
    p.off_lim = p.off_c1 + nreg * p.H * 4;
    p.bytes = p.off_lim + 64;
    *pl = p;
    return KMAN_OK;
}

// mean phase durations (us) per kernel from the stamp rows; frees the buffers
int report_stamps(kman_ctx *ctx, uint64_t **st, const uint64_t *rows) {
    static const char *names[3] = {"rg_extract", "rg_pass", "rg_finish"};
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < 3; q++) {
        std::vector<uint64_t> h(rows[q] * 16);
        HIP_TRY(ctx, hipMemcpy(h.data(), st[q], h.size() * 8, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipFree(st[q]));
        double sum[16] = {0}, tot = 0;
        uint64_t n[16] = {0}, nt = 0;
        for (uint64_t r = 0; r < rows[q]; r++) {
            const uint64_t *x = &h[r * 16];
            int last = 0;
            for (int i = 1; i < 15; i++)
                if (x[i] && x[i - 1]) {
                    sum[i] += (double)(x[i] - x[i - 1]) / 100.0;
                    n[i]++;
                    last = i;
                }
            if (x[0] && last) {
                tot += (double)(x[last] - x[0]) / 100.0;
                nt++;
            }
        }
        fprintf(stderr, "stamps %-10s tiles %8llu  mean us/tile %.2f  phases:", names[q], (unsigned long long)nt,
                nt ? tot / nt : 0.0);
        for (int i = 1; i < 15; i++)
            if (n[i]) fprintf(stderr, " %d:%.2f", i, sum[i] / n[i]);
        fprintf(stderr, "\n");
    }
    return KMAN_OK;
}

}  // namespace

// The error word of the region kernels: ERR_REGION alone is not a fault (a
// region that would overflow: the caller redoes the input, or its key ranges,
// by another path); any other bit is, and each has its own message.
int kman::region::region_fault(kman_ctx *ctx, uint32_t e, const char *what) {
    const uint32_t f = e & ~ERR_REGION;
    if (f & ERR_EARLY)
        return kman_fail(ctx, KMAN_EHIP,
                         "%s: a region's early row count disagreed with the rows its sorted keys give (device "
                         "check, error word %u)", what, e);
    return kman_fail(ctx, KMAN_ETIMEOUT, "%s: device look-back wait exceeded its bound (error word %u)", what, e);
}

extern "C" int kman_groups_plan(uint64_t n_bases, uint32_t k, uint32_t flags, int mode, uint64_t *work_bytes) {
    if (!work_bytes) return KMAN_EINVAL;
    RegionPlan p;
    const int rc = make_plan(n_bases, k, flags, mode, &p);
    *work_bytes = rc == KMAN_OK ? p.bytes : 0;
    return rc;
}

namespace {

// one kman_groups call: the plan and the work-area carve-up
struct GroupsCall {
    RegionPlan p;
    uint64_t *r0, *r1;
    uint32_t *c0, *c1;
    uint32_t nreg;
};

int groups_setup(kman_ctx *ctx, uint64_t n_bases, uint32_t k, uint32_t flags, int mode, void *d_work,
                 uint64_t work_bytes, GroupsCall *g) {
    RegionPlan &p = g->p;
    const int prc = make_plan(n_bases, k, flags, mode, &p);
    if (prc == KMAN_EINVAL) return kman_fail(ctx, KMAN_EINVAL, "kman_groups: bad mode or k");
    if (prc != KMAN_OK) return prc;
    if (!d_work) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (work_bytes < p.bytes)
        return kman_fail(ctx, KMAN_ECAP, "work area %llu < %llu bytes", (unsigned long long)work_bytes,
                         (unsigned long long)p.bytes);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    g->r0 = (uint64_t *)d_work;
    g->r1 = (uint64_t *)((char *)d_work + p.off_r1);
    g->c0 = (uint32_t *)((char *)d_work + p.off_c0);
    g->c1 = (uint32_t *)((char *)d_work + p.off_c1);
    g->nreg = 1u << (G1 + p.B2);
    return KMAN_OK;
}

int groups_outputs_ok(kman_ctx *ctx, const GroupsCall &g, int mode, const void *d_okeys, const void *d_ovals,
                      uint32_t oval_bytes, uint64_t n_bases) {
    if (!d_okeys || !d_ovals) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (oval_bytes != 4 && oval_bytes != 8) return kman_fail(ctx, KMAN_EINVAL, "oval_bytes must be 4 or 8");
    if (oval_bytes == 4 && mode == KMAN_FINISH_UNIQ && (g.p.rc ? g.p.W : 2 * g.p.W) - 1 > 0xffffffffull)
        return kman_fail(ctx, KMAN_EINVAL, "u32 pos cannot address %llu bases", (unsigned long long)n_bases);
    return KMAN_OK;
}

// pass 1 (per bucket, by the next B2 bits), the finish (one block per
// region) and the results: output count (the last region's inclusive),
// region-0 counts (k-mers), error word
int groups_tail(kman_ctx *ctx, const GroupsCall &g, int mode, uint64_t *d_okeys, void *d_ovals, uint32_t oval_bytes,
                uint64_t **stamps, const uint64_t *stamp_rows, uint64_t *n_kmers, uint64_t *n_out) {
    const RegionPlan &p = g.p;
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));  // (the chain counter only)
    // count items leave pass 1 as 4 bytes when the narrow finish takes them
    // (KMAN_WIDE_ITEMS=1: 8 bytes, for A/B)
    const bool narrow4 = narrow_ok(ctx, mode, p.Q, p.rest, 0) && !getenv("KMAN_WIDE_ITEMS");
    {
        KTimer kt_(ctx, "region_pass");
        PassArgs pa{};
        pa.in = g.r0;
        pa.seg_base = nullptr;
        pa.seg_cnt = g.c0;
        pa.cnt_sb = 1;  // (rg_extract's cursors: [segment][bucket])
        pa.stride = p.C0;
        pa.nbk = 1u << G1;
        pa.nsg = RS;
        pa.gsub = 1;
        pa.H = p.H;
        pa.shift = p.Q + p.rest;
        pa.bits = p.B2;
        pa.out = g.r1;
        pa.C1 = p.C1h;
        pa.cnt1 = g.c1;
        pa.big = 1;
        pa.lines = 1;
        pa.line1 = getenv("KMAN_PASS_LINE1") ? 1 : 0;
        KMAN_TRY(launch_pass(ctx, pa, counter, stamps[1], false, narrow4));
        HIP_TRY(ctx, hipGetLastError());
    }
    {
        FinishArgs f{g.r1, p.C1h, g.c1, p.Q, p.rest, (uint32_t)p.rc, 0, 0, g.nreg};
        f.fsub = p.H;
        f.in4 = narrow4;
        KMAN_TRY(run_finish(ctx, f, mode, d_okeys, d_ovals, oval_bytes, stamps[2]));
    }
    if (stamps[0]) KMAN_TRY(report_stamps(ctx, stamps, stamp_rows));
    uint64_t *h = ctx->h_small;
    HIP_TRY(ctx, hipMemcpyAsync(h + 4, ctx->d_status + (g.nreg - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(h + 8, ctx->d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    std::vector<uint32_t> hc((size_t)RS << G1);
    HIP_TRY(ctx, hipMemcpyAsync(hc.data(), g.c0, hc.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    uint32_t e;
    memcpy(&e, h + 8, 4);
    if (e) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->d_err, 0, sizeof(uint32_t), ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (e & ERR_REGION) return KMAN_EFALLBACK;  // a region overflowed: outputs invalid, redone elsewhere
        return region_fault(ctx, e, "kman_groups");
    }
    const uint64_t wd = h[4];
    if (((wd >> 56) & 63u) != ctx->epoch || (wd >> 62) != ST_INCL)
        return kman_fail(ctx, KMAN_EHIP, "region output total not published");
    uint64_t nk = 0;
    for (uint32_t v : hc) nk += v;
    *n_kmers = nk;
    *n_out = wd & ST_VMASK;
    return KMAN_OK;
}

}  // namespace

extern "C" int kman_groups(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                           int mode, void *d_work, uint64_t work_bytes, uint64_t *d_okeys, void *d_ovals,
                           uint32_t oval_bytes, uint64_t *n_kmers, uint64_t *n_out) {
    if (!ctx || !n_kmers || !n_out) return KMAN_EINVAL;
    *n_kmers = 0;
    *n_out = 0;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    KMAN_TRY(groups_outputs_ok(ctx, g, mode, d_okeys, d_ovals, oval_bytes, n_bases));
    const RegionPlan &p = g.p;
    HIP_TRY(ctx, hipMemsetAsync(g.c0, 0, p.bytes - p.off_c0, ctx->stream));
    uint64_t *stamps[3] = {nullptr, nullptr, nullptr};
    const uint64_t stamp_rows[3] = {p.n_tiles0, (uint64_t)p.maxt1 << G1, g.nreg};
    if (getenv("KMAN_RG_STAMPS"))
        for (int q = 0; q < 3; q++) {
            HIP_TRY(ctx, hipMalloc((void **)&stamps[q], stamp_rows[q] * 128));
            HIP_TRY(ctx, hipMemsetAsync(stamps[q], 0, stamp_rows[q] * 128, ctx->stream));
        }
    uint32_t epoch, *counter;
    // pass 0: extraction by the top 8 bits
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));  // (the ticket counters only)
    {
        KTimer kt_(ctx, "region_extract");
        launch_extract_any(ctx, p, d_codes, n_bases, k, g.r0, g.c0, epoch, counter, stamps[0]);
        HIP_TRY(ctx, hipGetLastError());
    }
    return groups_tail(ctx, g, mode, d_okeys, d_ovals, oval_bytes, stamps, stamp_rows, n_kmers, n_out);
}

extern "C" int kman_groups_begin(kman_ctx *ctx, uint64_t n_bases, uint32_t k, uint32_t flags, int mode,
                                 void *d_work, uint64_t work_bytes, uint32_t *n_tiles, uint64_t *tile_bases) {
    if (!ctx || !n_tiles || !tile_bases) return KMAN_EINVAL;
    *n_tiles = 0;
    *tile_bases = 0;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    const RegionPlan &p = g.p;
    HIP_TRY(ctx, hipMemsetAsync(g.c0, 0, p.bytes - p.off_c0, ctx->stream));
    uint32_t epoch, *counter;
    KMAN_TRY(kman_lookback_begin(ctx, 1, &epoch, &counter));
    ctx->grp_epoch = epoch;
    ctx->grp_next = 0;
    ctx->grp_tiles = p.n_tiles0;
    *n_tiles = p.n_tiles0;
    *tile_bases = (uint64_t)RT * p.ei;
    return KMAN_OK;
}

namespace {
int groups_extract_to(kman_ctx *ctx, const GroupsCall &g, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                      uint32_t tile_hi) {
    const RegionPlan &p = g.p;
    if (ctx->grp_epoch == 0 || ctx->grp_epoch != ctx->epoch || ctx->grp_tiles != p.n_tiles0)
        return kman_fail(ctx, KMAN_EINVAL, "kman_groups_extract: no kman_groups_begin of this input before it, or "
                                           "another look-back call in between");
    if (!d_codes) return kman_fail(ctx, KMAN_EINVAL, "null buffer");
    if (tile_hi > p.n_tiles0) tile_hi = p.n_tiles0;
    uint32_t *counter = ctx->d_counters + ctx->grp_epoch;
    if (tile_hi <= ctx->grp_next) return KMAN_OK;
    {
        KTimer kt_(ctx, "region_extract");
        launch_extract_any(ctx, p, d_codes, n_bases, k, g.r0, g.c0, ctx->grp_epoch, counter, nullptr,
                           tile_hi - ctx->grp_next);
        HIP_TRY(ctx, hipGetLastError());
    }
    ctx->grp_next = tile_hi;
    return KMAN_OK;
}
}  // namespace

extern "C" int kman_groups_extract(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k,
                                   uint32_t flags, int mode, void *d_work, uint64_t work_bytes, uint32_t tile_hi) {
    if (!ctx) return KMAN_EINVAL;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    return groups_extract_to(ctx, g, d_codes, n_bases, k, tile_hi);
}

extern "C" int kman_groups_end(kman_ctx *ctx, const uint8_t *d_codes, uint64_t n_bases, uint32_t k, uint32_t flags,
                               int mode, void *d_work, uint64_t work_bytes, uint64_t *d_okeys, void *d_ovals,
                               uint32_t oval_bytes, uint64_t *n_kmers, uint64_t *n_out) {
    if (!ctx || !n_kmers || !n_out) return KMAN_EINVAL;
    *n_kmers = 0;
    *n_out = 0;
    GroupsCall g;
    KMAN_TRY(groups_setup(ctx, n_bases, k, flags, mode, d_work, work_bytes, &g));
    KMAN_TRY(groups_outputs_ok(ctx, g, mode, d_okeys, d_ovals, oval_bytes, n_bases));
    KMAN_TRY(groups_extract_to(ctx, g, d_codes, n_bases, k, g.p.n_tiles0));
    ctx->grp_epoch = 0;
    uint64_t *stamps[3] = {nullptr, nullptr, nullptr};
    const uint64_t stamp_rows[3] = {0, 0, 0};
    return groups_tail(ctx, g, mode, d_okeys, d_ovals, oval_bytes, stamps, stamp_rows, n_kmers, n_out);
}

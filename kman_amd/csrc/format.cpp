// format.cpp — byte-exact output writers (host side).
//
//   count  "%s\t%d\n" % (seq, len(headers))       kmermaid/join.py:283-284
//   uniq   ">%s\n%s\n" % (header, seq)            kmermaid/join.py:261-262
//   batch  KMer.as_fasta ">%s\n%s\n"               kmermaid/seq.py:489-495
//   header "%s:%d-%d:%s" % (ref, start, end, +/-)  kmermaid/seq.py:103-104
//
// The formatting runs on host threads over host copies of the device results:
// each thread sizes its slice, an exclusive scan gives the slice offsets, then
// every thread writes its slice in place.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/kman.h"

namespace {

inline int ndigits(uint64_t v) {
    int n = 1;
    while (v >= 10) {
        v /= 10;
        n++;
    }
    return n;
}

inline char *put_u64(char *p, uint64_t v) {
    char t[24];
    int n = 0;
    do {
        t[n++] = (char)('0' + v % 10);
        v /= 10;
    } while (v);
    while (n) *p++ = t[--n];
    return p;
}

inline char *put_seq(char *p, uint64_t key, uint32_t k) {
    static const char B[4] = {'A', 'C', 'G', 'T'};
    for (int j = (int)k - 1; j >= 0; j--) *p++ = B[(key >> (2 * j)) & 3];
    return p;
}

// k > 32: the first k - 32 bases in hi, the last 32 in lo
inline char *put_seq_wide(char *p, uint64_t hi, uint64_t lo, uint32_t k) {
    p = put_seq(p, hi, k - 32);
    return put_seq(p, lo, 32);
}

// any k: W word planes (words.hip layout), row i's word j at w[j * stride + i]
struct Words {
    const uint64_t *w;
    uint64_t stride;
    uint32_t W;
    char *put(char *p, uint64_t i, uint32_t k) const {
        const uint32_t h = k - 32 * (W - 1);
        for (uint32_t j = 0; j < W; j++) p = put_seq(p, w[j * stride + i], j ? 32u : h);
        return p;
    }
};

inline uint64_t get_val(const void *a, uint32_t bytes, uint64_t i) {
    return bytes == 4 ? ((const uint32_t *)a)[i] : ((const uint64_t *)a)[i];
}

template <typename SizeF, typename WriteF>
int run_sliced(uint64_t n, char *out, size_t cap, size_t *used, int threads, SizeF size_of, WriteF write_at) {
    if (threads < 1) threads = 1;
    if ((uint64_t)threads > n / 4096 + 1) threads = (int)(n / 4096 + 1);
    std::vector<size_t> sz(threads + 1, 0);
    auto slice = [&](int t, uint64_t *b, uint64_t *e) {
        *b = n * t / threads;
        *e = n * (t + 1) / threads;
    };
    {
        std::vector<std::thread> th;
        for (int t = 0; t < threads; t++)
            th.emplace_back([&, t] {
                uint64_t b, e;
                slice(t, &b, &e);
                size_t s = 0;
                for (uint64_t i = b; i < e; i++) s += size_of(i);
                sz[t + 1] = s;
            });
        for (auto &x : th) x.join();
    }
    for (int t = 0; t < threads; t++) sz[t + 1] += sz[t];
    *used = sz[threads];
    if (sz[threads] > cap || !out) return KMAN_ECAP;
    {
        std::vector<std::thread> th;
        for (int t = 0; t < threads; t++)
            th.emplace_back([&, t] {
                uint64_t b, e;
                slice(t, &b, &e);
                char *p = out + sz[t];
                for (uint64_t i = b; i < e; i++) p = write_at(i, p);
            });
        for (auto &x : th) x.join();
    }
    return KMAN_OK;
}

struct Names {
    const char *names;
    const uint64_t *off;
    const uint64_t *rec_seq;
    uint64_t R;
    // record owning global base p: the last record whose first base is <= p
    uint64_t find(uint64_t p) const {
        const uint64_t *it = std::upper_bound(rec_seq, rec_seq + R, p);
        return (uint64_t)(it - rec_seq) - 1;
    }
};

int format_fasta_impl(const uint64_t *keys, const void *pos, uint32_t pos_bytes, uint64_t n, uint32_t k,
                      const Names &nm, char *out, size_t cap, size_t *used, int threads,
                      const uint64_t *hi = nullptr, const Words *wd = nullptr) {
    auto size_of = [&](uint64_t i) -> size_t {
        const uint64_t v = get_val(pos, pos_bytes, i);
        const uint64_t p = v >> 1;
        const uint64_t r = nm.find(p);
        const uint64_t st = p - nm.rec_seq[r];
        // ">" name ":" start "-" end ":" s "\n" seq "\n"
        return 1 + (nm.off[r + 1] - nm.off[r]) + 1 + ndigits(st) + 1 + ndigits(st + k) + 2 + 1 + k + 1;
    };
    auto write_at = [&](uint64_t i, char *p) -> char * {
        const uint64_t v = get_val(pos, pos_bytes, i);
        const uint64_t g = v >> 1;
        const uint64_t r = nm.find(g);
        const uint64_t st = g - nm.rec_seq[r];
        *p++ = '>';
        const uint64_t L = nm.off[r + 1] - nm.off[r];
        memcpy(p, nm.names + nm.off[r], L);
        p += L;
        *p++ = ':';
        p = put_u64(p, st);
        *p++ = '-';
        p = put_u64(p, st + k);
        *p++ = ':';
        *p++ = (v & 1) ? '-' : '+';
        *p++ = '\n';
        p = wd ? wd->put(p, i, k) : hi ? put_seq_wide(p, hi[i], keys[i], k) : put_seq(p, keys[i], k);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

}  // namespace

extern "C" int kman_format_count(const uint64_t *ukeys, const void *counts, uint32_t count_bytes, uint64_t n,
                                 uint32_t k, char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n && (!ukeys || !counts)) || k < 1 || k > 32) return KMAN_EINVAL;
    if (count_bytes != 4 && count_bytes != 8) return KMAN_EINVAL;
    auto size_of = [&](uint64_t i) -> size_t { return k + 2 + ndigits(get_val(counts, count_bytes, i)); };
    auto write_at = [&](uint64_t i, char *p) -> char * {
        p = put_seq(p, ukeys[i], k);
        *p++ = '\t';
        p = put_u64(p, get_val(counts, count_bytes, i));
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

// one abundance vector as text, "%d\n" per entry (AbundanceVector.write_to,
// abundance.py:151-168, after its "# k=%d" line): entries v[0], v[stride], ..
extern "C" int kman_format_vector(const uint32_t *v, uint64_t n, uint64_t stride, char *out, size_t cap,
                                  size_t *used, int threads) {
    if (!used || (n && !v) || stride == 0) return KMAN_EINVAL;
    auto size_of = [&](uint64_t i) -> size_t { return ndigits(v[i * stride]) + 1; };
    auto write_at = [&](uint64_t i, char *p) -> char * {
        p = put_u64(p, v[i * stride]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

extern "C" int kman_format_uniq(const uint64_t *keys, const void *pos, uint32_t pos_bytes, uint64_t n, uint32_t k,
                                const char *names, const uint64_t *name_off, const uint64_t *rec_seq,
                                uint64_t n_records, char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n && (!keys || !pos || !name_off || !rec_seq || !n_records)) || k < 1 || k > 32) return KMAN_EINVAL;
    if (pos_bytes != 4 && pos_bytes != 8) return KMAN_EINVAL;
    Names nm{names, name_off, rec_seq, n_records};
    return format_fasta_impl(keys, pos, pos_bytes, n, k, nm, out, cap, used, threads);
}

// uniq rows over several sources (a multi-source join: FASTA inputs and
// reloaded batch files): one merged record table in global base indices;
// rec_kind[r] = 0: a FASTA record (header name:start-end:strand), 1: a batch
// file record whose title is the header as written (the k-mer's own
// "ref:start-end:strand").
namespace {
int uniq_mixed_impl(const uint64_t *keys, const Words *wd, const uint64_t *pos, uint64_t n, uint32_t k,
                    const char *names, const uint64_t *name_off, const uint64_t *rec_seq, const uint8_t *rec_kind,
                    uint64_t n_records, char *out, size_t cap, size_t *used, int threads) {
    Names nm{names, name_off, rec_seq, n_records};
    auto size_of = [&](uint64_t i) -> size_t {
        const uint64_t g = pos[i] >> 1;
        const uint64_t r = nm.find(g);
        const size_t L = nm.off[r + 1] - nm.off[r];
        if (rec_kind[r]) return 1 + L + 1 + k + 1;
        const uint64_t st = g - nm.rec_seq[r];
        return 1 + L + 1 + ndigits(st) + 1 + ndigits(st + k) + 2 + 1 + k + 1;
    };
    auto write_at = [&](uint64_t i, char *p) -> char * {
        const uint64_t v = pos[i], g = v >> 1;
        const uint64_t r = nm.find(g);
        const uint64_t L = nm.off[r + 1] - nm.off[r];
        *p++ = '>';
        memcpy(p, nm.names + nm.off[r], L);
        p += L;
        if (!rec_kind[r]) {
            const uint64_t st = g - nm.rec_seq[r];
            *p++ = ':';
            p = put_u64(p, st);
            *p++ = '-';
            p = put_u64(p, st + k);
            *p++ = ':';
            *p++ = (v & 1) ? '-' : '+';
        }
        *p++ = '\n';
        p = wd ? wd->put(p, i, k) : put_seq(p, keys[i], k);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}
}  // namespace

extern "C" int kman_format_uniq_mixed(const uint64_t *keys, const uint64_t *pos, uint64_t n, uint32_t k,
                                      const char *names, const uint64_t *name_off, const uint64_t *rec_seq,
                                      const uint8_t *rec_kind, uint64_t n_records, char *out, size_t cap,
                                      size_t *used, int threads) {
    if (!used || (n && (!keys || !pos || !name_off || !rec_seq || !rec_kind || !n_records)) || k < 1 || k > 32)
        return KMAN_EINVAL;
    return uniq_mixed_impl(keys, nullptr, pos, n, k, names, name_off, rec_seq, rec_kind, n_records, out, cap, used,
                           threads);
}

// the same over W word planes (any k >= 2; words.hip layout)
extern "C" int kman_format_uniq_mixed_words(const uint64_t *words, uint64_t stride, const uint64_t *pos, uint64_t n,
                                            uint32_t k, const char *names, const uint64_t *name_off,
                                            const uint64_t *rec_seq, const uint8_t *rec_kind, uint64_t n_records,
                                            char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n && (!words || !pos || !name_off || !rec_seq || !rec_kind || !n_records)) || k < 2 || stride < n)
        return KMAN_EINVAL;
    const Words wd{words, stride, (k + 31) / 32};
    return uniq_mixed_impl(nullptr, &wd, pos, n, k, names, name_off, rec_seq, rec_kind, n_records, out, cap, used,
                           threads);
}

// any k >= 2 over W word planes: the count table and the uniq / batch FASTA
extern "C" int kman_format_count_words(const uint64_t *words, uint64_t stride, const void *counts,
                                       uint32_t count_bytes, uint64_t n, uint32_t k, char *out, size_t cap,
                                       size_t *used, int threads) {
    if (!used || (n && (!words || !counts)) || k < 2 || stride < n) return KMAN_EINVAL;
    if (count_bytes != 4 && count_bytes != 8) return KMAN_EINVAL;
    const Words wd{words, stride, (k + 31) / 32};
    auto size_of = [&](uint64_t i) -> size_t { return k + 2 + ndigits(get_val(counts, count_bytes, i)); };
    auto write_at = [&](uint64_t i, char *p) -> char * {
        p = wd.put(p, i, k);
        *p++ = '\t';
        p = put_u64(p, get_val(counts, count_bytes, i));
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

extern "C" int kman_format_uniq_words(const uint64_t *words, uint64_t stride, const void *pos, uint32_t pos_bytes,
                                      uint64_t n, uint32_t k, const char *names, const uint64_t *name_off,
                                      const uint64_t *rec_seq, uint64_t n_records, char *out, size_t cap,
                                      size_t *used, int threads) {
    if (!used || (n && (!words || !pos || !name_off || !rec_seq || !n_records)) || k < 2 || stride < n)
        return KMAN_EINVAL;
    if (pos_bytes != 4 && pos_bytes != 8) return KMAN_EINVAL;
    Names nm{names, name_off, rec_seq, n_records};
    const Words wd{words, stride, (k + 31) / 32};
    return format_fasta_impl(nullptr, pos, pos_bytes, n, k, nm, out, cap, used, threads, nullptr, &wd);
}

// kman_screen_records' planes: "%s\t%d\t%d\t%d\n" % (name, windows, hits, sum)
// per kept record (`kmer screen`; not in the reference)
extern "C" int kman_format_screen(const uint64_t *out3, uint64_t n_records, const uint8_t *keep, const char *names,
                                  const uint64_t *name_off, char *buf, size_t cap, size_t *used, int threads) {
    if (!used || (n_records && (!out3 || !name_off))) return KMAN_EINVAL;
    const uint64_t *w = out3, *h = out3 + n_records, *s = out3 + 2 * n_records;
    auto size_of = [&](uint64_t r) -> size_t {
        if (keep && !keep[r]) return 0;
        return (name_off[r + 1] - name_off[r]) + 4 + ndigits(w[r]) + ndigits(h[r]) + ndigits(s[r]);
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (keep && !keep[r]) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, w[r]);
        *p++ = '\t';
        p = put_u64(p, h[r]);
        *p++ = '\t';
        p = put_u64(p, s[r]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_records, buf, cap, used, threads, size_of, write_at);
}

// the same lines with kman_record_quantile's word as a fifth column
// (`kmer screen --median`)
extern "C" int kman_format_screen_median(const uint64_t *out3, const uint32_t *median, uint64_t n_records,
                                         const uint8_t *keep, const char *names, const uint64_t *name_off, char *buf,
                                         size_t cap, size_t *used, int threads) {
    if (!used || (n_records && (!out3 || !median || !name_off))) return KMAN_EINVAL;
    const uint64_t *w = out3, *h = out3 + n_records, *s = out3 + 2 * n_records;
    auto size_of = [&](uint64_t r) -> size_t {
        if (keep && !keep[r]) return 0;
        return (name_off[r + 1] - name_off[r]) + 5 + ndigits(w[r]) + ndigits(h[r]) + ndigits(s[r]) +
               ndigits(median[r]);
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (keep && !keep[r]) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, w[r]);
        *p++ = '\t';
        p = put_u64(p, h[r]);
        *p++ = '\t';
        p = put_u64(p, s[r]);
        *p++ = '\t';
        p = put_u64(p, median[r]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_records, buf, cap, used, threads, size_of, write_at);
}

// the same lines with the record's solid span as two last columns, after the
// median when there is one (`kmer screen --solid`)
extern "C" int kman_format_screen_solid(const uint64_t *out3, const uint32_t *median, const uint64_t *start,
                                        const uint64_t *end, uint64_t n_records, const uint8_t *keep,
                                        const char *names, const uint64_t *name_off, char *buf, size_t cap,
                                        size_t *used, int threads) {
    if (!used || (n_records && (!out3 || !start || !end || !name_off))) return KMAN_EINVAL;
    const uint64_t *w = out3, *h = out3 + n_records, *s = out3 + 2 * n_records;
    auto size_of = [&](uint64_t r) -> size_t {
        if (keep && !keep[r]) return 0;
        return (name_off[r + 1] - name_off[r]) + 6 + ndigits(w[r]) + ndigits(h[r]) + ndigits(s[r]) +
               (median ? 1 + ndigits(median[r]) : 0) + ndigits(start[r]) + ndigits(end[r]);
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (keep && !keep[r]) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, w[r]);
        *p++ = '\t';
        p = put_u64(p, h[r]);
        *p++ = '\t';
        p = put_u64(p, s[r]);
        if (median) {
            *p++ = '\t';
            p = put_u64(p, median[r]);
        }
        *p++ = '\t';
        p = put_u64(p, start[r]);
        *p++ = '\t';
        p = put_u64(p, end[r]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_records, buf, cap, used, threads, size_of, write_at);
}

// a pair's line: the joint planes and median, then the solid span of mate 1
// and of mate 2 (`kmer screen --mate --solid`); the span arrays hold the mates'
// rows interleaved, 2 * n_pairs each
extern "C" int kman_format_screen_pair(const uint64_t *out3, const uint32_t *median, const uint64_t *start,
                                       const uint64_t *end, uint64_t n_pairs, const uint8_t *keep, const char *names,
                                       const uint64_t *name_off, char *buf, size_t cap, size_t *used, int threads) {
    if (!used || (n_pairs && (!out3 || !start || !end || !name_off))) return KMAN_EINVAL;
    const uint64_t *w = out3, *h = out3 + n_pairs, *s = out3 + 2 * n_pairs;
    auto size_of = [&](uint64_t r) -> size_t {
        if (keep && !keep[r]) return 0;
        return (name_off[r + 1] - name_off[r]) + 8 + ndigits(w[r]) + ndigits(h[r]) + ndigits(s[r]) +
               (median ? 1 + ndigits(median[r]) : 0) + ndigits(start[2 * r]) + ndigits(end[2 * r]) +
               ndigits(start[2 * r + 1]) + ndigits(end[2 * r + 1]);
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (keep && !keep[r]) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, w[r]);
        *p++ = '\t';
        p = put_u64(p, h[r]);
        *p++ = '\t';
        p = put_u64(p, s[r]);
        if (median) {
            *p++ = '\t';
            p = put_u64(p, median[r]);
        }
        for (uint64_t m = 2 * r; m < 2 * r + 2; m++) {
            *p++ = '\t';
            p = put_u64(p, start[m]);
            *p++ = '\t';
            p = put_u64(p, end[m]);
        }
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_pairs, buf, cap, used, threads, size_of, write_at);
}

// the same lines with the record's corrected bases as one last column
// (`kmer screen --solid C --correct`)
extern "C" int kman_format_screen_correct(const uint64_t *out3, const uint32_t *median, const uint64_t *start,
                                          const uint64_t *end, const uint32_t *fixes, uint64_t n_records,
                                          const uint8_t *keep, const char *names, const uint64_t *name_off, char *buf,
                                          size_t cap, size_t *used, int threads) {
    if (!used || (n_records && (!out3 || !start || !end || !fixes || !name_off))) return KMAN_EINVAL;
    const uint64_t *w = out3, *h = out3 + n_records, *s = out3 + 2 * n_records;
    auto size_of = [&](uint64_t r) -> size_t {
        if (keep && !keep[r]) return 0;
        return (name_off[r + 1] - name_off[r]) + 7 + ndigits(w[r]) + ndigits(h[r]) + ndigits(s[r]) +
               (median ? 1 + ndigits(median[r]) : 0) + ndigits(start[r]) + ndigits(end[r]) + ndigits(fixes[r]);
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (keep && !keep[r]) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, w[r]);
        *p++ = '\t';
        p = put_u64(p, h[r]);
        *p++ = '\t';
        p = put_u64(p, s[r]);
        if (median) {
            *p++ = '\t';
            p = put_u64(p, median[r]);
        }
        *p++ = '\t';
        p = put_u64(p, start[r]);
        *p++ = '\t';
        p = put_u64(p, end[r]);
        *p++ = '\t';
        p = put_u64(p, fixes[r]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_records, buf, cap, used, threads, size_of, write_at);
}

// "%s\t%d\t%d\n" % (name, start, end) per kept record with end > start: the
// BED of the solid spans (`kmer screen --solid C --bed FILE`)
extern "C" int kman_format_bed(const uint64_t *start, const uint64_t *end, uint64_t n_records, const uint8_t *keep,
                               const char *names, const uint64_t *name_off, char *buf, size_t cap, size_t *used,
                               int threads) {
    if (!used || (n_records && (!start || !end || !name_off))) return KMAN_EINVAL;
    auto listed = [&](uint64_t r) -> bool { return (!keep || keep[r]) && end[r] > start[r]; };
    auto size_of = [&](uint64_t r) -> size_t {
        if (!listed(r)) return 0;
        return (name_off[r + 1] - name_off[r]) + 3 + ndigits(start[r]) + ndigits(end[r]);
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (!listed(r)) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, start[r]);
        *p++ = '\t';
        p = put_u64(p, end[r]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_records, buf, cap, used, threads, size_of, write_at);
}

// "%s\t%d\t%s\t%d\t%d\n" % (name, windows, label | "?" | "-", hits, second)
// per kept record, with one "\t%d" per colour appended when `planes` is given
// (`kmer classify`, `--hits`; not in the reference)
extern "C" int kman_format_classify(const uint32_t *windows, const int32_t *assign, const uint32_t *hits,
                                    const uint32_t *second, const uint32_t *planes, uint32_t n_colors,
                                    uint64_t n_records, const uint8_t *keep, const char *labels,
                                    const uint64_t *label_off, const char *names, const uint64_t *name_off, char *buf,
                                    size_t cap, size_t *used, int threads) {
    if (!used || n_colors < 1 || n_colors > KMAN_CLASSIFY_MAX_COLORS || !label_off) return KMAN_EINVAL;
    if (n_records && (!windows || !assign || !hits || !second || !name_off)) return KMAN_EINVAL;
    for (uint64_t r = 0; r < n_records; r++)
        if (assign[r] >= 0 && (uint32_t)assign[r] >= n_colors) return KMAN_EINVAL;
    auto label_len = [&](uint64_t r) -> size_t {
        return assign[r] >= 0 ? (size_t)(label_off[assign[r] + 1] - label_off[assign[r]]) : 1;
    };
    auto size_of = [&](uint64_t r) -> size_t {
        if (keep && !keep[r]) return 0;
        size_t s = (name_off[r + 1] - name_off[r]) + 5 + ndigits(windows[r]) + label_len(r) + ndigits(hits[r]) +
                   ndigits(second[r]);
        if (planes)
            for (uint32_t c = 0; c < n_colors; c++) s += 1 + ndigits(planes[(uint64_t)c * n_records + r]);
        return s;
    };
    auto write_at = [&](uint64_t r, char *p) -> char * {
        if (keep && !keep[r]) return p;
        const uint64_t L = name_off[r + 1] - name_off[r];
        if (L) memcpy(p, names + name_off[r], L);
        p += L;
        *p++ = '\t';
        p = put_u64(p, windows[r]);
        *p++ = '\t';
        if (assign[r] >= 0) {
            const size_t n = label_len(r);
            if (n) memcpy(p, labels + label_off[assign[r]], n);
            p += n;
        } else {
            *p++ = assign[r] == -2 ? '?' : '-';
        }
        *p++ = '\t';
        p = put_u64(p, hits[r]);
        *p++ = '\t';
        p = put_u64(p, second[r]);
        if (planes)
            for (uint32_t c = 0; c < n_colors; c++) {
                *p++ = '\t';
                p = put_u64(p, planes[(uint64_t)c * n_records + r]);
            }
        *p++ = '\n';
        return p;
    };
    return run_sliced(n_records, buf, cap, used, threads, size_of, write_at);
}

// ">%d LN:i:%d KC:i:%d\n%s\n" % (first_id + u, bases, kc, seq) per unitig, the
// sequence on one line (`kmer unitigs`; not in the reference)
extern "C" int kman_format_unitigs(const uint8_t *seq, const uint64_t *off, const uint64_t *kc, uint64_t n,
                                   uint64_t first_id, char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n && (!seq || !off || !kc))) return KMAN_EINVAL;
    for (uint64_t u = 0; u < n; u++)
        if (off[u + 1] < off[u]) return KMAN_EINVAL;
    auto size_of = [&](uint64_t u) -> size_t {
        const uint64_t len = off[u + 1] - off[u];
        return 1 + ndigits(first_id + u) + 6 + ndigits(len) + 6 + ndigits(kc[u]) + 1 + len + 1;
    };
    auto write_at = [&](uint64_t u, char *p) -> char * {
        const uint64_t len = off[u + 1] - off[u];
        *p++ = '>';
        p = put_u64(p, first_id + u);
        memcpy(p, " LN:i:", 6);
        p = put_u64(p + 6, len);
        memcpy(p, " KC:i:", 6);
        p = put_u64(p + 6, kc[u]);
        *p++ = '\n';
        if (len) memcpy(p, seq + off[u], len);
        p += len;
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

// "S\t%d\t%s\tLN:i:%d\tKC:i:%d\n" % (first_id + u, seq, bases, kc) per unitig (`kmer unitigs --gfa`)
extern "C" int kman_format_gfa_segments(const uint8_t *seq, const uint64_t *off, const uint64_t *kc, uint64_t n,
                                        uint64_t first_id, char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n && (!seq || !off || !kc))) return KMAN_EINVAL;
    for (uint64_t u = 0; u < n; u++)
        if (off[u + 1] < off[u]) return KMAN_EINVAL;
    auto size_of = [&](uint64_t u) -> size_t {
        const uint64_t len = off[u + 1] - off[u];
        return 2 + ndigits(first_id + u) + 1 + len + 6 + ndigits(len) + 6 + ndigits(kc[u]) + 1;
    };
    auto write_at = [&](uint64_t u, char *p) -> char * {
        const uint64_t len = off[u + 1] - off[u];
        *p++ = 'S';
        *p++ = '\t';
        p = put_u64(p, first_id + u);
        *p++ = '\t';
        if (len) memcpy(p, seq + off[u], len);
        p += len;
        memcpy(p, "\tLN:i:", 6);
        p = put_u64(p + 6, len);
        memcpy(p, "\tKC:i:", 6);
        p = put_u64(p + 6, kc[u]);
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

// "L\t%d\t%c\t%d\t%c\t%dM\n" % (first_id + u, "+-"[o], v, "+-"[p], k - 1) per edge, one item per end: end e of the
// slice has the edges edge[eoff[e] - eoff[0], eoff[e + 1] - eoff[0]), words (v << 1) | p
extern "C" int kman_format_gfa_links(const uint64_t *eoff, const uint32_t *edge, uint64_t n_units, uint64_t first_id,
                                     uint32_t k, char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n_units && !eoff) || k < 3 || k > 31 || (k & 1u) == 0) return KMAN_EINVAL;
    const uint64_t n_ends = 2 * n_units;
    for (uint64_t e = 0; e < n_ends; e++)
        if (eoff[e + 1] < eoff[e]) return KMAN_EINVAL;
    if (n_ends && eoff[n_ends] > eoff[0] && !edge) return KMAN_EINVAL;
    const size_t fixed = 2 + 1 + 1 + 1 + 1 + 1 + 1 + ndigits(k - 1) + 2;  // all but the two numbers
    auto size_of = [&](uint64_t e) -> size_t {
        const size_t du = ndigits(first_id + (e >> 1));
        size_t s = 0;
        for (uint64_t i = eoff[e] - eoff[0]; i < eoff[e + 1] - eoff[0]; i++) s += fixed + du + ndigits(edge[i] >> 1);
        return s;
    };
    auto write_at = [&](uint64_t e, char *p) -> char * {
        for (uint64_t i = eoff[e] - eoff[0]; i < eoff[e + 1] - eoff[0]; i++) {
            *p++ = 'L';
            *p++ = '\t';
            p = put_u64(p, first_id + (e >> 1));
            *p++ = '\t';
            *p++ = (e & 1) ? '-' : '+';
            *p++ = '\t';
            p = put_u64(p, edge[i] >> 1);
            *p++ = '\t';
            *p++ = (edge[i] & 1u) ? '-' : '+';
            *p++ = '\t';
            p = put_u64(p, k - 1);
            *p++ = 'M';
            *p++ = '\n';
        }
        return p;
    };
    return run_sliced(n_ends, out, cap, used, threads, size_of, write_at);
}

// k in 33..64: keys as (hi, lo) word pairs (kman_extract_wide)
extern "C" int kman_format_count_wide(const uint64_t *hi, const uint64_t *lo, const void *counts, uint32_t count_bytes,
                                      uint64_t n, uint32_t k, char *out, size_t cap, size_t *used, int threads) {
    if (!used || (n && (!hi || !lo || !counts)) || k < 33 || k > 64) return KMAN_EINVAL;
    if (count_bytes != 4 && count_bytes != 8) return KMAN_EINVAL;
    auto size_of = [&](uint64_t i) -> size_t { return k + 2 + ndigits(get_val(counts, count_bytes, i)); };
    auto write_at = [&](uint64_t i, char *p) -> char * {
        p = put_seq_wide(p, hi[i], lo[i], k);
        *p++ = '\t';
        p = put_u64(p, get_val(counts, count_bytes, i));
        *p++ = '\n';
        return p;
    };
    return run_sliced(n, out, cap, used, threads, size_of, write_at);
}

extern "C" int kman_format_uniq_wide(const uint64_t *hi, const uint64_t *lo, const void *pos, uint32_t pos_bytes,
                                     uint64_t n, uint32_t k, const char *names, const uint64_t *name_off,
                                     const uint64_t *rec_seq, uint64_t n_records, char *out, size_t cap, size_t *used,
                                     int threads) {
    if (!used || (n && (!hi || !lo || !pos || !name_off || !rec_seq || !n_records)) || k < 33 || k > 64)
        return KMAN_EINVAL;
    if (pos_bytes != 4 && pos_bytes != 8) return KMAN_EINVAL;
    Names nm{names, name_off, rec_seq, n_records};
    return format_fasta_impl(lo, pos, pos_bytes, n, k, nm, out, cap, used, threads, hi);
}

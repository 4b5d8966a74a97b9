// bytes16.h — a byte stream read as aligned 16-byte words: the helpers of the
// kernels that walk text or codes one uint4 per lane (cut.hip, correct.hip,
// pair.hip, hpc.hip).
#pragma once
#include "common.h"

namespace {

// the aligned 16-byte word of src at p (p % 16 == 0); bytes at or past n read
// as FILL.  (n - p >= 16 and not p + 16 <= n: no overflow for p near 2^64.)
template <uint32_t FILL = 0>
KMAN_DEV uint4 load16(const uint8_t *__restrict__ src, uint64_t n, uint64_t p) {
    if (p < n && n - p >= 16) return *reinterpret_cast<const uint4 *>(src + p);
    auto dword = [&](int d) -> uint32_t {
        uint32_t acc = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint64_t q = p + (uint64_t)(4 * d + b);
            if (q < n) acc |= (uint32_t)src[q] << (8 * b);
            else if (FILL) acc |= FILL << (8 * b);
        }
        return acc;
    };
    return make_uint4(dword(0), dword(1), dword(2), dword(3));
}

// the sixteen bytes of src from a on (any alignment): the words at a - a % 16
// and after it, a dword select and four v_alignbyte
KMAN_DEV uint4 shifted16(const uint8_t *__restrict__ src, uint64_t n, uint64_t a) {
    const uint32_t q = (uint32_t)(a & 15), dq = q >> 2, sh = q & 3;
    const uint4 A = load16(src, n, a - q);
    const uint4 B = q ? load16(src, n, a - q + 16) : make_uint4(0, 0, 0, 0);
    const uint32_t x0 = dq == 0 ? A.x : dq == 1 ? A.y : dq == 2 ? A.z : A.w;
    const uint32_t x1 = dq == 0 ? A.y : dq == 1 ? A.z : dq == 2 ? A.w : B.x;
    const uint32_t x2 = dq == 0 ? A.z : dq == 1 ? A.w : dq == 2 ? B.x : B.y;
    const uint32_t x3 = dq == 0 ? A.w : dq == 1 ? B.x : dq == 2 ? B.y : B.z;
    const uint32_t x4 = dq == 0 ? B.x : dq == 1 ? B.y : dq == 2 ? B.z : B.w;
    uint4 w;
    w.x = __builtin_amdgcn_alignbyte(x1, x0, sh);
    w.y = __builtin_amdgcn_alignbyte(x2, x1, sh);
    w.z = __builtin_amdgcn_alignbyte(x3, x2, sh);
    w.w = __builtin_amdgcn_alignbyte(x4, x3, sh);
    return w;
}

// byte j (0 .. 15) of a 16-byte word
KMAN_DEV uint32_t byte_of(const uint4 &v, int j) {
    const uint32_t w = (j >> 2) == 0 ? v.x : (j >> 2) == 1 ? v.y : (j >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (j & 3))) & 0xffu;
}

// the first byte of the line after the terminator that starts at t (t >= b: none)
KMAN_DEV uint64_t line_after(const uint8_t *text, uint64_t t, uint64_t b) {
    if (t >= b) return b;
    uint64_t n = t + 1;
    if (text[t] == '\r' && n < b && text[n] == '\n') n++;
    return n;
}

}  // namespace

// xor_expect.h -- the CRC a stripe's XOR parity must have, from the stored
// CRCs of its blocks alone (photon_crc32c_xor_expect_n /
// photon_crc64ecma_xor_expect_n), written once for the device
// kernel (xor_expect_kernel in xor_kernels.h) and for the CPU replay of it
// (photon_crc_test_xor_expect, tuning.h).
//
// Both CRCs are affine in the data: crc(B, s) = R(B) ^ crc(0^n, s), R the raw
// CRC from a zero register. For m blocks of n bytes and P their XOR, R(P) is
// the XOR of the R(B_i), so
//   crc(P, s) = crc(B_0, s) ^ ... ^ crc(B_{m-1}, s) ^ (m even ? crc(0^n, s) : 0):
// an odd number of zero-run terms leaves the one crc(P, s) needs, an even
// number cancels it. The zero-run term is the seed register moved over n
// bytes, fold_shift (fold_parts.h): one table multiply per set bit of the
// 64-bit n. `inv` is the inversion of the CRC's register on the way in and
// out: 0 for CRC-32C, ~0 for CRC-64/ECMA.
#pragma once
#include <stdint.h>

#include "fold_parts.h"

namespace pcrc {

// The words [*s0, *s1) of stripe s. A null grp_start: k words per stripe.
// Both ends are clamped into [0, ncrc] and s0 <= s1 (patch_bounds' rule):
// whatever grp_start holds, no word outside the array is read.
PCRC_HD void xor_expect_bounds(const uint64_t* grp_start, uint64_t ncrc, uint32_t k, uint64_t s, uint64_t* s0,
                               uint64_t* s1) {
    uint64_t a = grp_start ? grp_start[s] : s * k, b = grp_start ? grp_start[s + 1] : s * k + k;
    b = b < ncrc ? b : ncrc;
    *s0 = a < b ? a : b;
    *s1 = b;
}

// crc_extend(n zero bytes, seed).
template <typename G>
PCRC_HD typename G::T xor_expect_zeros(uint64_t n, typename G::T seed, typename G::T inv, const typename G::T* tab) {
    return fold_shift<G>(seed ^ inv, n, tab) ^ inv;
}

// The per-stripe step (one thread of the kernel).
template <typename G>
PCRC_HD typename G::T xor_expect_stripe(const typename G::T* crc, uint64_t ncrc, const uint64_t* grp_start, uint32_t k,
                                        const uint64_t* len, uint64_t nbytes, uint64_t s, typename G::T seed,
                                        typename G::T inv, const typename G::T* tab) {
    uint64_t s0 = 0, s1 = 0;
    xor_expect_bounds(grp_start, ncrc, k, s, &s0, &s1);
    typename G::T x = 0;
    for (uint64_t i = s0; i < s1; ++i) x ^= crc[i];
    if (((s1 - s0) & 1) == 0) x ^= xor_expect_zeros<G>(len ? len[s] : nbytes, seed, inv, tab);
    return x;
}

// Every stripe in order (the CPU replay of the kernel).
template <typename G>
inline void xor_expect_replay(const typename G::T* crc, uint64_t ncrc, const uint64_t* grp_start, uint32_t k,
                              const uint64_t* len, uint64_t nbytes, uint64_t count, typename G::T seed,
                              typename G::T inv, typename G::T* want, const typename G::T* tab) {
    for (uint64_t s = 0; s < count; ++s)
        want[s] = xor_expect_stripe<G>(crc, ncrc, grp_start, k, len, nbytes, s, seed, inv, tab);
}

}  // namespace pcrc

// seg_unscan.h -- per-segment CRCs from the running CRCs that the two-sided
// walk stores (photon_crc32c_copy_msg_iov_seg2_n /
// photon_crc64ecma_copy_msg_iov_seg2_n), written once for the
// device kernel (seg_unscan_kernel in crc32c_kernels.h) and for the CPU replay
// of it (unscan_replay below, tests/cpp/seg_unscan_replay.cpp).
//
// The walk leaves P[j] = the CRC chained from seed_m of every byte of the
// message up to the end of segment j (or up to the end of the copy, in the
// segment in which it ended) in the entry of every segment its cursor reached.
// The combine identity read backwards gives the segment's own CRC from seed 0:
//   crc(B, 0) = crc(AB, seed) ^ crc(A, seed) * x^(8 |B|)
// so, with n_j = the bytes of segment j that landed,
//   seg[j] = n_j ? P[j] ^ Pprev_j * x^(8 n_j) : 0,
//   Pprev_j = seed_m for the side's first segment of the message, else P[j-1].
// It holds on the values the calls return: for raw CRC-32C, and for
// CRC-64/ECMA with its inverted register (the inversions of AB and A cancel
// against the one of B's start value).
//
// Which entries hold a running value: exactly those of the segments the cursor
// reached, and a segment with `before` bytes of its side in front of it was
// reached if before < k_m (a byte at or behind that position landed, so the
// cursor went through the segment, empty or not). n_j > 0 implies that for j
// and for j - 1. Every other entry holds whatever the caller left there and is
// only written, with 0.
#pragma once
#include <stdint.h>

#include "fold_parts.h"

// as PCRC_HD, for the steps that walk arrays (not constant expressions)
#ifndef PCRC_VHD
#ifdef __HIPCC__
#define PCRC_VHD __host__ __device__ inline
#else
#define PCRC_VHD inline
#endif
#endif

namespace pcrc {

constexpr uint32_t kUnscanStep = 64;  // segments of one message and side per step: a wavefront

PCRC_HD uint64_t unscan_sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// k_m: the bytes the walk copies.
PCRC_HD uint64_t unscan_copied(uint64_t size, uint64_t src_sum, uint64_t dst_sum) {
    const uint64_t k = size < src_sum ? size : src_sum;
    return k < dst_sum ? k : dst_sum;
}

// Did the walk's cursor reach (and store the entry of) a segment with `before`
// bytes of its side in front of it?
PCRC_HD bool unscan_reached(uint64_t k, uint64_t before) { return before < k; }

// n_j = clamp(k - before, 0, len).
PCRC_HD uint64_t unscan_landed(uint64_t k, uint64_t before, uint64_t len) {
    const uint64_t room = k > before ? k - before : 0;
    return len < room ? len : room;
}

// x^(8n) for n > 0 as fold_xpow8, without the multiply by one at the first set
// bit of n: a block length that is a power of two costs no multiply here (the
// un-scan kernel is bound by instruction issue, and the multiplies are it).
template <typename G>
PCRC_HD typename G::T unscan_xpow8(uint64_t n, const typename G::T* tab) {
    typename G::T k = 0;  // no factor yet (a product of powers of x is never 0)
    for (int i = 0; n; ++i, n >>= 1)
        if (n & 1) k = k ? G::mul(k, tab[i]) : tab[i];
    return k;
}

// The segment's CRC from seed 0: p = its running value, prev = the one before
// it (both unused when nothing of it landed).
template <typename G>
PCRC_HD typename G::T unscan_diff(typename G::T p, typename G::T prev, uint64_t n, const typename G::T* tab) {
    if (!n) return 0;
    return prev ? p ^ G::mul(prev, unscan_xpow8<G>(n, tab)) : p;
}

// One side of one message as the kernel runs it, over host arrays: steps of
// `width` lanes (the kernel's: kUnscanStep), every load of a step before its
// first store, the last lane's running value carried to the next step. seg:
// the side's entries [s0, s1), rewritten in place.
template <typename G>
inline void unscan_replay(const uint64_t* len, uint64_t s0, uint64_t s1, uint64_t k, typename G::T seed,
                          typename G::T* seg, const typename G::T* tab, uint32_t width = kUnscanStep) {
    typedef typename G::T T;
    uint64_t carry_bytes = 0;
    T carry_p = seed;
    uint64_t* n = new uint64_t[width];
    T* p = new T[width];
    for (uint64_t base = s0; base < s1; base += width) {
        const uint32_t cnt = s1 - base < width ? (uint32_t)(s1 - base) : width;
        uint64_t run = carry_bytes;
        for (uint32_t l = 0; l < cnt; ++l) {  // the loads
            n[l] = unscan_landed(k, run, len[base + l]);
            p[l] = unscan_reached(k, run) ? seg[base + l] : 0;
            run = unscan_sat_add(run, len[base + l]);
        }
        for (uint32_t l = 0; l < cnt; ++l)  // the stores
            seg[base + l] = unscan_diff<G>(p[l], l ? p[l - 1] : carry_p, n[l], tab);
        carry_bytes = run;
        carry_p = p[cnt - 1];
    }
    delete[] n;
    delete[] p;
}

// Message m of a call as one wavefront of the kernel runs it: k_m from the
// lengths (saturating sums), the seed, then the source and the destination
// side. src_len / dst_len: the descriptors' lengths.
template <typename G>
inline void unscan_replay_msg(const uint64_t* src_len, const uint64_t* src_start, const uint64_t* dst_len,
                              const uint64_t* dst_start, uint64_t m, const uint64_t* size, typename G::T seed0,
                              const typename G::T* seeds, typename G::T* src_seg, typename G::T* dst_seg,
                              const typename G::T* tab, uint32_t width = kUnscanStep) {
    uint64_t ssum = 0, dsum = 0;
    for (uint64_t s = src_start[m]; s < src_start[m + 1]; ++s) ssum = unscan_sat_add(ssum, src_len[s]);
    for (uint64_t s = dst_start[m]; s < dst_start[m + 1]; ++s) dsum = unscan_sat_add(dsum, dst_len[s]);
    const uint64_t k = unscan_copied(size ? size[m] : ~0ull, ssum, dsum);
    const typename G::T seed = seeds ? seeds[m] : seed0;
    unscan_replay<G>(src_len, src_start[m], src_start[m + 1], k, seed, src_seg, tab, width);
    unscan_replay<G>(dst_len, dst_start[m], dst_start[m + 1], k, seed, dst_seg, tab, width);
}

}  // namespace pcrc

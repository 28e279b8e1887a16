// window_finish.h -- the finish of the windowed copy + CRC
// (photon_crc32c_copy_msg_iov_window_n / photon_crc64ecma_copy_msg_iov_window_n,
// DESIGN.md §4.15), written once for the device kernel (window_finish_kernel in
// crc32c_kernels.h) and for the CPU replay of it (window_replay_msg below,
// tests/cpp/window_finish_replay.cpp).
//
// The walk reads every source segment of the message in full and leaves
//   P[j]  = the CRC chained from seed 0 of every byte of the source stream up
//           to the end of segment j, in the entry of EVERY source segment, and
//   R(a), R(b) = the same running value in front of the window's first byte
//           and behind its last one, in the message's two work words
// (both work words only when the window is not empty). The per-segment CRCs
// are the un-scan of seg_unscan.h with every segment reached and seed 0. The
// window's CRC from seed_m follows from the same identity,
//   crc(W, 0)    = R(b) ^ R(a) * x^(8k)          (A = the bytes in front, k = |W|)
//   crc(W, seed) = crc(W, 0) ^ seed * x^(8k)  =  (seed ^ R(a)) * x^(8k) ^ R(b),
// on the values the calls return: for raw CRC-32C, and for CRC-64/ECMA with its
// inverted register (R(a) = ~(~0 * x^(8a) ^ raw(A)), so seed ^ R(a) carries
// ~seed and the complement of R(b) is the one of the result; the terms in
// ~0 * x^(8(a+k)) and raw(A) * x^(8k) cancel).
#pragma once
#include <stdint.h>

#include "seg_unscan.h"

namespace pcrc {

// The window of a message: source-stream bytes [a, a + k).
struct Window {
    uint64_t a, k;
};

// skip, size: the caller's (size ~0 = unlimited); L, D: the saturating sums of
// the source and of the destination lengths. No sum of skip and size is formed.
PCRC_HD Window window_bounds(uint64_t skip, uint64_t size, uint64_t L, uint64_t D) {
    const uint64_t a = skip < L ? skip : L;
    uint64_t k = size < D ? size : D;
    k = k < L - a ? k : L - a;
    return Window{a, k};
}

// d_out[m]: ra, rb are read by the caller only when k > 0.
template <typename G>
PCRC_HD typename G::T window_crc(typename G::T seed, typename G::T ra, typename G::T rb, uint64_t k,
                                 const typename G::T* tab) {
    if (!k) return seed;
    const typename G::T v = seed ^ ra;
    return v ? G::mul(v, unscan_xpow8<G>(k, tab)) ^ rb : rb;
}

// Message m of a call as one wavefront of the kernel runs it: L and D from the
// descriptors' lengths, the bounds, the source entries un-scanned in place
// (every segment reached: k = L, seed 0), then the window's CRC and k.
// work: the call's work words, two per message.
template <typename G>
inline void window_replay_msg(const uint64_t* src_len, const uint64_t* src_start, const uint64_t* dst_len,
                              const uint64_t* dst_start, uint64_t m, const uint64_t* skip, const uint64_t* size,
                              typename G::T seed0, const typename G::T* seeds, typename G::T* src_seg,
                              const uint64_t* work, typename G::T* out, uint64_t* copied, const typename G::T* tab,
                              uint32_t width = kUnscanStep) {
    typedef typename G::T T;
    uint64_t L = 0, D = 0;
    for (uint64_t s = src_start[m]; s < src_start[m + 1]; ++s) L = unscan_sat_add(L, src_len[s]);
    for (uint64_t s = dst_start[m]; s < dst_start[m + 1]; ++s) D = unscan_sat_add(D, dst_len[s]);
    const Window w = window_bounds(skip ? skip[m] : 0, size ? size[m] : ~0ull, L, D);
    unscan_replay<G>(src_len, src_start[m], src_start[m + 1], L, (T)0, src_seg, tab, width);
    const T seed = seeds ? seeds[m] : seed0;
    out[m] = w.k ? window_crc<G>(seed, (T)work[2 * m], (T)work[2 * m + 1], w.k, tab) : seed;
    if (copied) copied[m] = w.k;
}

}  // namespace pcrc

// patch_crc.h -- stored CRCs patched by the deltas of overwrites
// (photon_crc32c_patch_n / photon_crc64ecma_patch_n), written
// once for the device kernel (patch_kernel in crc32c_kernels.h) and for the
// CPU replay of it (photon_crc_test_patch, tuning.h).
//
// A write i replaces the bytes O by N of equal length inside a target (a
// block, an object) with `tail[i]` bytes of the target behind the write's end.
// delta[i] = R(O xor N), the raw CRC from a zero register, and by linearity
//   crc(pre N suf, s) = crc(pre O suf, s) ^ delta[i] * x^(8 tail[i])
// for every seed s (the seed's and the prefix's terms are the same on both
// sides and cancel). Target t owns the writes [tgt_start[t], tgt_start[t+1]):
//   out[t] = in[t] ^ XOR_i delta[i] * x^(8 tail[i]).
// The multiply is fold_shift (fold_parts.h): one table multiply per set bit
// of the 64-bit tail, none for a tail of 0 or a delta of 0. NT threads take
// the target's writes round robin (patch_thread) and their values are XORed.
#pragma once
#include <stdint.h>

#include "fold_parts.h"

namespace pcrc {

// The writes [*s0, *s1) of target m. A null tgt_start: write m alone. Both
// ends are clamped into [0, nwrites] and s0 <= s1: whatever tgt_start holds,
// no write outside the arrays is read.
PCRC_HD void patch_bounds(const uint64_t* tgt_start, uint64_t nwrites, uint64_t m, uint64_t* s0, uint64_t* s1) {
    uint64_t a = tgt_start ? tgt_start[m] : m, b = tgt_start ? tgt_start[m + 1] : m + 1;
    b = b < nwrites ? b : nwrites;
    *s0 = a < b ? a : b;
    *s1 = b;
}

// Thread t of nt: the XOR over the writes s0 + t, s0 + t + nt, ... below s1
// of delta * x^(8 tail).
template <typename G>
PCRC_HD typename G::T patch_thread(const typename G::T* delta, const uint64_t* tail, uint64_t s0, uint64_t s1,
                                   uint32_t t, uint32_t nt, const typename G::T* tab) {
    typename G::T v = 0;
    for (uint64_t i = s0 + t; i < s1; i += nt) v ^= fold_shift<G>(delta[i], tail[i], tab);
    return v;
}

// Every target as workgroups of nt threads patch it, in order (the CPU replay
// of the kernel; the kernel XORs the threads' values over the wave and LDS).
template <typename G>
inline void patch_replay(const typename G::T* delta, const uint64_t* tail, uint64_t nwrites,
                         const uint64_t* tgt_start, uint64_t ntgt, const typename G::T* in, typename G::T* out,
                         uint32_t nt, const typename G::T* tab) {
    for (uint64_t m = 0; m < ntgt; ++m) {
        uint64_t s0, s1;
        patch_bounds(tgt_start, nwrites, m, &s0, &s1);
        typename G::T x = 0;
        for (uint32_t t = 0; t < nt; ++t) x ^= patch_thread<G>(delta, tail, s0, s1, t, nt, tab);
        out[m] = in[m] ^ x;
    }
}

}  // namespace pcrc

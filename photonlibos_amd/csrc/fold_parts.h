// fold_parts.h -- the fold of an object's part CRCs into the object's CRC
// (photon_crc32c_fold_parts_n / photon_crc64ecma_fold_parts_n, DESIGN.md
// §4.8), written once for the device kernels (crc32c_fold_parts_kernel,
// crc64_fold_parts_kernel) and for the CPU replay of them
// (photon_crc_test_fold_parts, tuning.h).
//
// The object's parts s = 0..n-1 with CRCs c_s (from seed 0) and lengths l_s
// fold as acc = seed; acc = acc * x^(8 l_s) ^ c_s (the identity of
// extend_spans, crc.cpp:393-405), i.e.
//   out = seed * x^(8 L) ^ XOR_s c_s * x^(8 A_s),   L = sum l, A_s = sum_{u>s} l_u.
// NT threads split the sum: thread t Horner-folds a contiguous run of parts
// (fold_run: the run's value relative to the run's END, and the run's bytes),
// a suffix sum over the runs' bytes gives the bytes AFTER each run, each
// thread shifts its value by them (fold_shift), one thread adds the seed term
// (fold_finish's, seed shifted by L), and the values are XORed.
#pragma once
#include <stdint.h>

#include "gf2.h"

namespace pcrc {

struct Gf32 {
    typedef uint32_t T;
    static PCRC_HD T one() { return kOne; }
    static PCRC_HD T mul(T a, T b) { return mulmod(a, b); }
};
struct Gf64 {
    typedef uint64_t T;
    static PCRC_HD T one() { return 1ull << 63; }
    static PCRC_HD T mul(T a, T b) { return mulmod64(a, b); }
};

// x^(8n): the product of tab[i] = x^(8 * 2^i) over the set bits of n (i < 64,
// so any 64-bit byte count is at most 64 multiplies).
template <typename G>
PCRC_HD typename G::T fold_xpow8(uint64_t n, const typename G::T* tab) {
    typename G::T k = G::one();
    for (int i = 0; n; ++i, n >>= 1)
        if (n & 1) k = G::mul(k, tab[i]);
    return k;
}

// The run of thread t of nt over n parts: ceil(n / nt) parts per thread, the
// last runs short or empty.
PCRC_HD void fold_run_bounds(uint64_t n, uint32_t nt, uint32_t t, uint64_t* lo, uint64_t* hi) {
    const uint64_t per = (n + nt - 1) / nt;
    const uint64_t a = (uint64_t)t * per < n ? (uint64_t)t * per : n;
    *lo = a;
    *hi = n - a < per ? n : a + per;
}

template <typename T>
struct FoldRun {
    T acc;           // XOR over the run of crc[s] * x^(8 * bytes of the run after s)
    uint64_t bytes;  // the run's lengths summed (mod 2^64)
};

// The per-thread step: Horner over parts [lo, hi). The multiplier x^(8 len)
// is kept while consecutive lengths repeat (as crc64_msg_fold_kernel).
template <typename G>
PCRC_HD FoldRun<typename G::T> fold_run(const typename G::T* crc, const uint64_t* len, uint64_t lo, uint64_t hi,
                                        const typename G::T* tab) {
    typedef typename G::T T;
    FoldRun<T> r = {0, 0};
    uint64_t klen = 0;
    T k = G::one();  // x^(8 * klen)
    for (uint64_t s = lo; s < hi; ++s) {
        const uint64_t n = len[s];
        const T c = crc[s];
        if (r.acc) {  // 0 * k = 0: a run's first part (and leading zero CRCs) cost no multiply
            if (n != klen) {
                k = fold_xpow8<G>(n, tab);
                klen = n;
            }
            r.acc = G::mul(r.acc, k);
        }
        r.acc ^= c;
        r.bytes += n;
    }
    return r;
}

// The combine step: a run's value moved from the run's end to the object's
// end, `after` = the bytes of every later run.
// (The table entries are applied to the value itself: one multiply per set bit
// of `after`, none for the constant.)
template <typename G>
PCRC_HD typename G::T fold_shift(typename G::T acc, uint64_t after, const typename G::T* tab) {
    if (!acc) return acc;
    for (int i = 0; after; ++i, after >>= 1)
        if (after & 1) acc = G::mul(acc, tab[i]);
    return acc;
}

// The seed term, one more value in the XOR: seed * x^(8 * total). x = the XOR
// of every shifted run, total = the object's bytes.
template <typename G>
PCRC_HD typename G::T fold_finish(typename G::T x, typename G::T seed, uint64_t total, const typename G::T* tab) {
    return x ^ fold_shift<G>(seed, total, tab);
}

// The whole fold of one object as nt threads run it, in order (the CPU replay
// of the kernels; the kernels do the suffix sum and the XOR in LDS).
template <typename G>
inline typename G::T fold_replay(const typename G::T* crc, const uint64_t* len, uint64_t n, typename G::T seed,
                                 uint32_t nt, const typename G::T* tab, uint64_t* total) {
    typedef typename G::T T;
    T x = 0;
    uint64_t after = 0;  // bytes of the runs behind thread t
    for (uint32_t t = nt; t-- > 0;) {
        uint64_t lo, hi;
        fold_run_bounds(n, nt, t, &lo, &hi);
        const FoldRun<T> r = fold_run<G>(crc, len, lo, hi, tab);
        x ^= fold_shift<G>(r.acc, after, tab);
        after += r.bytes;
    }
    if (total) *total = after;
    return fold_finish<G>(x, seed, after, tab);
}

}  // namespace pcrc

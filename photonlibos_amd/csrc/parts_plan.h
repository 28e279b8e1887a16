// parts_plan.h -- the cut of the many-large-parts calls
// (photon_crc32c_copy_parts_n / photon_crc32c_batch_parts_n and the CRC-64
// forms), written once for the piece kernels, the part fold
// kernels and the host (photon_crc_parts_work_bytes,
// photon_crc_test_parts_plan), as long_plan.h is for the one-long-buffer
// kernels.
//
// Part i is the first n = min(len, max_part_bytes) bytes at address a. A =
// the first 4 KiB boundary at or after a; head = min(A - a, n) (0..4095); the
// body [head, n) is cut into pieces of `piece` bytes (a multiple of 4 KiB),
// the last one short. Piece 0 is the head together with the first body piece
// (the long plan's merged head): [0, head + min(piece, n - head)). Piece j >=
// 1 is [head + j piece, head + min((j + 1) piece, n - head)). So every piece
// but the first starts at a multiple of 4 KiB of the SOURCE address (a
// destination that is co-aligned modulo 16 never has a 16-byte block shared by
// two pieces), every piece between the first and the last is `piece` bytes,
// and a part has count = max(1, ceil((n - head) / piece)) pieces, 0 when n ==
// 0. The host knows max_part_bytes only: the task space gives every part
// P = max(1, ceil(max_part_bytes / piece)) slots (count <= P: the merged head
// needs no slot of its own), and slot j >= count is an empty task.
#pragma once
#include <stdint.h>

#include "fold_parts.h"

namespace pcrc {

constexpr uint64_t kPartsAlign = 4096;              // piece granule, and the boundary the cut is anchored at
constexpr uint64_t kPartsMaxPiece = 1ull << 30;     // photon_crc_set_parts_piece's upper bound
constexpr uint64_t kPartsMaxBytes = 1ull << 62;     // max_part_bytes is clamped here (no part is longer)
constexpr uint64_t kPartsMaxTasks = 1ull << 40;     // nparts * P beyond this: -EINVAL
constexpr uint32_t kPartsFoldRuns = 62;             // lanes of the fold's wave that take a run of pieces

struct PartsPiece {
    uint64_t off, len;  // [off, off + len) of the part; len == 0: an empty task
};

// P: the slots of one part.
PCRC_HD uint64_t parts_bound(uint64_t max_part_bytes, uint64_t piece) {
    const uint64_t c = max_part_bytes / piece + (max_part_bytes % piece ? 1 : 0);
    return c ? c : 1;
}

PCRC_HD uint64_t parts_head(uint64_t addr, uint64_t n) {
    const uint64_t h = (0 - addr) & (kPartsAlign - 1);
    return h < n ? h : n;
}

// The pieces of a part of n (capped) bytes at addr.
PCRC_HD uint64_t parts_count(uint64_t addr, uint64_t n, uint64_t piece) {
    if (!n) return 0;
    const uint64_t m = n - parts_head(addr, n);
    return m ? (m + piece - 1) / piece : 1;
}

// Piece j of the part (j < P; j * piece cannot wrap: P * piece <= max + piece).
PCRC_HD PartsPiece parts_piece(uint64_t addr, uint64_t n, uint64_t piece, uint64_t j) {
    const uint64_t head = parts_head(addr, n), m = n - head;
    const uint64_t lo = j * piece;
    PartsPiece p = {0, 0};
    if (j && lo >= m) return p;  // behind the end of the part
    const uint64_t hi = m - lo < piece ? m : lo + piece;
    p.off = j ? head + lo : 0;
    p.len = head + hi - p.off;
    return p;
}

// The part fold, one wavefront per part: lane t's term of
//   out = seed * x^(8 n) ^ XOR_j w[j] * x^(8 * bytes behind piece j),
// w[j] = the CRC of piece j from seed 0; the XOR of the 64 lanes' values is
// the part's CRC from `seed`. The pieces 1 .. count-2 all have `piece` bytes,
// so the bytes behind piece j < count-1 are (count-2-j) pieces and the last
// piece's L: lanes 0 .. kPartsFoldRuns-1 each Horner-fold a contiguous run of
// the pieces [0, count-1) with K = x^(8 piece) (ktab[0]), shift by the pieces
// behind the run with ktab[i] = K^(2^i) (as crc32c_combine_series_kernel) and
// by L with tab[i] = x^(8 * 2^i); lane 62 shifts the seed by n (the first
// piece's length enters only here); lane 63 holds the last piece's CRC. Every
// lane makes the same two fold_shift calls, so the wave runs them together.
template <typename G>
PCRC_HD typename G::T parts_fold_lane(const typename G::T* w, uint64_t addr, uint64_t n, uint64_t piece,
                                      typename G::T seed, uint32_t t, const typename G::T* ktab,
                                      const typename G::T* tab) {
    typedef typename G::T T;
    const uint64_t count = parts_count(addr, n, piece);
    T v = 0;
    uint64_t behind_pieces = 0, behind_bytes = 0;
    if (t == kPartsFoldRuns) {
        v = seed;
        behind_bytes = n;
    } else if (count) {
        const uint64_t m = count - 1;
        if (t == kPartsFoldRuns + 1) {
            v = w[m];
        } else {
            uint64_t lo = 0, hi = 0;
            fold_run_bounds(m, kPartsFoldRuns, t, &lo, &hi);
            for (uint64_t j = lo; j < hi; ++j) v = (v ? G::mul(v, ktab[0]) : 0) ^ w[j];
            behind_pieces = m - hi;
            behind_bytes = parts_piece(addr, n, piece, m).len;
        }
    }
    v = fold_shift<G>(v, behind_pieces, ktab);
    return fold_shift<G>(v, behind_bytes, tab);
}

}  // namespace pcrc

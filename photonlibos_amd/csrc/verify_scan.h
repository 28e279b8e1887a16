// verify_scan.h -- stored CRCs checked on the device
// (photon_crc32c_verify_n / _verify_ptr_n and the CRC-64 forms, DESIGN.md
// §4.10), written once for the device kernels (verify_mark_kernel,
// verify_scan_kernel, verify_list_kernel in crc32c_kernels.h) and for the CPU
// replay of them (photon_crc_test_verify, tuning.h).
//
// Entry i is BAD when its computed word crc[i] differs from its expected
// word, the little-endian word at expected + i * stride or at
// expected_ptr[i]; an entry with a null pointer is not COMPARED. The entries
// are cut into tiles of `tile` entries (a power of two, 64 ... 65,536), a tile
// into rows of 64 consecutive entries: one row is one wavefront's step, its
// comparisons two 64-bit masks (bad, compared), bit l = entry row + l.
//
//   mark  a workgroup per tile: the rows' masks are counted into the tile's
//         three words of the workspace (verify_row_add): bad entries,
//         compared entries, the lowest bad index (~0: none).
//   scan  one workgroup: the tiles' bad counts become exclusive offsets, in
//         place, in chunks of kVerifyScanBlock tiles with a 64-bit carry
//         (verify_scan_step per tile, in tile order); the compared counts are
//         summed, the first bad index is the lowest of the tiles', and the
//         report is stored (verify_report_store).
//   list  a workgroup per tile with a bad entry and an offset below bad_cap:
//         the rows' masks again, entry row + l stored at offset + (bad
//         entries of the tile before the row) + verify_rank(bad, l) while
//         that is below bad_cap.
//
// Workspace: 3 * tiles words of 64 bits, [0, tiles) the bad counts / offsets,
// [tiles, 2 tiles) the compared counts, [2 tiles, 3 tiles) the first bad
// indices. Every word a call reads it has written before: the workspace needs
// no clearing and keeps nothing.
#pragma once
#include <stdint.h>

#include "gf2.h"

// as PCRC_HD, for the steps that take addresses apart (not constant expressions)
#ifdef __HIPCC__
#define PCRC_VHD __host__ __device__ inline
#else
#define PCRC_VHD inline
#endif

namespace pcrc {

constexpr uint32_t kVerifyMinTile = 64, kVerifyMaxTile = 65536;
constexpr uint32_t kVerifyBlock = 256;      // threads of a mark / list workgroup (fewer for tiles below 256)
constexpr uint32_t kVerifyScanBlock = 256;  // threads of the scan workgroup = tiles per chunk
constexpr uint32_t kVerifyMaxGrid = 2048;   // workgroups of mark / list / stamp; tiles beyond: a stride loop
constexpr uint64_t kVerifyMaxCount = 1ull << 40;  // entries of one call
constexpr uint64_t kVerifyNone = ~0ull;

PCRC_HD bool verify_tile_ok(uint64_t tile) {
    return tile >= kVerifyMinTile && tile <= kVerifyMaxTile && !(tile & (tile - 1));
}
PCRC_HD uint64_t verify_tiles(uint64_t count, uint32_t tile) { return (count + tile - 1) / tile; }
// ~0: more entries than one call takes
PCRC_HD uint64_t verify_work_words(uint64_t count, uint32_t tile) {
    return count > kVerifyMaxCount ? kVerifyNone : 3 * verify_tiles(count, tile);
}

// The little-endian word at any address: a word load where the address is a
// multiple of the width, byte loads elsewhere (never a misaligned word load).
template <typename T>
PCRC_VHD T verify_load(const void* p) {
    if (!((uintptr_t)p & (sizeof(T) - 1))) return *static_cast<const T*>(p);
    const uint8_t* b = static_cast<const uint8_t*>(p);
    T v = 0;
    for (unsigned k = 0; k < sizeof(T); ++k) v |= (T)b[k] << (8 * k);
    return v;
}
// The mirror for stamp: exactly sizeof(T) bytes written, nothing read.
template <typename T>
PCRC_VHD void verify_store(void* p, T v) {
    if (!((uintptr_t)p & (sizeof(T) - 1))) {
        *static_cast<T*>(p) = v;
        return;
    }
    uint8_t* b = static_cast<uint8_t*>(p);
    for (unsigned k = 0; k < sizeof(T); ++k) b[k] = (uint8_t)(v >> (8 * k));
}

// Where entry i's expected word lies: by stride, or by pointer (null = not compared).
PCRC_VHD const void* verify_expected_at(const void* expected, uint64_t stride, const void* const* expected_ptr,
                                       uint64_t i) {
    return expected_ptr ? expected_ptr[i] : static_cast<const void*>(static_cast<const char*>(expected) + i * stride);
}

// One entry: 0 = not compared, 1 = compared and equal, 3 = compared and bad.
template <typename T>
PCRC_VHD uint32_t verify_entry(const T* crc, const void* expected, uint64_t stride, const void* const* expected_ptr,
                              uint64_t i) {
    const void* p = verify_expected_at(expected, stride, expected_ptr, i);
    if (!p) return 0u;
    return crc[i] != verify_load<T>(p) ? 3u : 1u;
}

struct VerifyTile {
    uint64_t nbad, ncmp, first;
};
PCRC_HD VerifyTile verify_tile_none() { return VerifyTile{0, 0, kVerifyNone}; }

// A row of 64 entries from index `row` joins its tile (rows in index order).
PCRC_VHD void verify_row_add(VerifyTile* t, uint64_t row, uint64_t bad, uint64_t cmp) {
    t->nbad += (uint64_t)__builtin_popcountll(bad);
    t->ncmp += (uint64_t)__builtin_popcountll(cmp);
    if (bad && t->first == kVerifyNone) t->first = row + (uint64_t)__builtin_ctzll(bad);
}

// Bad entries of the row below lane l.
PCRC_HD uint32_t verify_rank(uint64_t bad, uint32_t l) {
    return (uint32_t)__builtin_popcountll(bad & ((1ull << l) - 1));
}

struct VerifyScan {
    uint64_t nbad, ncmp, first;  // bad entries before the tile at hand, compared entries so far, lowest bad index
};
PCRC_HD VerifyScan verify_scan_none() { return VerifyScan{0, 0, kVerifyNone}; }

// The scan over tile k (tiles in order): its bad count becomes its offset.
PCRC_VHD void verify_scan_step(VerifyScan* s, uint64_t* work, uint64_t tiles, uint64_t k) {
    const uint64_t n = work[k];
    work[k] = s->nbad;
    s->nbad += n;
    s->ncmp += work[tiles + k];
    const uint64_t f = work[2 * tiles + k];
    s->first = f < s->first ? f : s->first;
}

// photon_crc_verify_report's four words.
PCRC_VHD void verify_report_store(uint64_t* report, const VerifyScan& s, uint64_t bad_cap) {
    report[0] = s.nbad;
    report[1] = s.first;
    report[2] = s.nbad < bad_cap ? s.nbad : bad_cap;
    report[3] = s.ncmp;
}

// Does the list step walk tile k? (its offset is in work[k] after the scan)
PCRC_HD bool verify_tile_listed(const uint64_t* work, uint64_t tiles, uint64_t k, uint64_t bad_cap) {
    return work[2 * tiles + k] != kVerifyNone && work[k] < bad_cap;
}
// Where the list step starts in a listed tile from `lo`, walking `step` entries
// at a time: the step that holds the tile's first bad entry.
PCRC_HD uint64_t verify_list_start(uint64_t lo, uint64_t first, uint64_t step) {
    return lo + (first - lo) / step * step;
}

// The masks of the row of 64 entries from `row`, as a wavefront's __ballot gives them.
template <typename T>
inline void verify_row_masks(const T* crc, const void* expected, uint64_t stride, const void* const* expected_ptr,
                             uint64_t row, uint64_t end, uint64_t* bad, uint64_t* cmp) {
    *bad = *cmp = 0;
    for (uint32_t l = 0; l < 64 && row + l < end; ++l) {
        const uint32_t e = verify_entry<T>(crc, expected, stride, expected_ptr, row + l);
        *cmp |= (uint64_t)(e & 1u) << l;
        *bad |= (uint64_t)(e >> 1) << l;
    }
}

// The three steps in order over host arrays (the CPU replay of the kernels;
// the kernels take the masks by __ballot and the chunk's sums through LDS).
// work: verify_work_words(count, tile) words, uninitialised.
template <typename T>
inline void verify_replay(const T* crc, const void* expected, uint64_t stride, const void* const* expected_ptr,
                          uint64_t count, uint32_t tile, uint64_t bad_cap, uint64_t* work, uint64_t* report,
                          uint64_t* bad_idx) {
    const uint64_t tiles = verify_tiles(count, tile);
    for (uint64_t k = 0; k < tiles; ++k) {  // mark
        const uint64_t lo = k * tile, hi = count - lo < tile ? count : lo + tile;
        VerifyTile t = verify_tile_none();
        for (uint64_t row = lo; row < hi; row += 64) {
            uint64_t bad, cmp;
            verify_row_masks<T>(crc, expected, stride, expected_ptr, row, hi, &bad, &cmp);
            verify_row_add(&t, row, bad, cmp);
        }
        work[k] = t.nbad;
        work[tiles + k] = t.ncmp;
        work[2 * tiles + k] = t.first;
    }
    VerifyScan s = verify_scan_none();  // scan
    for (uint64_t c0 = 0; c0 < tiles; c0 += kVerifyScanBlock)
        for (uint64_t k = c0; k < tiles && k < c0 + kVerifyScanBlock; ++k) verify_scan_step(&s, work, tiles, k);
    verify_report_store(report, s, bad_cap);
    if (!bad_cap) return;
    for (uint64_t k = 0; k < tiles; ++k) {  // list
        if (!verify_tile_listed(work, tiles, k, bad_cap)) continue;
        const uint64_t lo = k * tile, hi = count - lo < tile ? count : lo + tile;
        uint64_t at = work[k];
        for (uint64_t row = verify_list_start(lo, work[2 * tiles + k], 64); row < hi && at < bad_cap; row += 64) {
            uint64_t bad, cmp;
            verify_row_masks<T>(crc, expected, stride, expected_ptr, row, hi, &bad, &cmp);
            for (uint32_t l = 0; l < 64; ++l)
                if ((bad >> l & 1) && at + verify_rank(bad, l) < bad_cap) bad_idx[at + verify_rank(bad, l)] = row + l;
            at += (uint64_t)__builtin_popcountll(bad);
        }
    }
}

}  // namespace pcrc

// parts_packed_plan.h -- the packed task space of the mixed-size parts calls
// (photon_crc32c_copy_parts_packed_n / photon_crc32c_batch_parts_packed_n and
// the CRC-64 forms), written once for the plan kernels, the
// piece kernels, the part fold kernels and the host
// (photon_crc_parts_packed_work_bytes, photon_crc_test_parts_packed_plan), as
// parts_plan.h is for the calls of §4.9. The cut of a part is parts_plan.h's,
// unchanged; what is new is how a task finds its part.
//
// count_i = parts_count(src_i, n_i, piece), n_i = min(len_i, max_part_bytes).
// first[i] = count_0 + ... + count_{i-1} (first[nparts] = T, the tasks of the
// call): task t in [first[i], first[i+1]) is piece t - first[i] of part i, and
// owner[t] = i. The host knows a bound on the SUM of the lengths only: a part
// has at most n_i / piece + 1 pieces (the merged head needs no slot, a short
// last piece needs one), so parts with sum n_i <= max_total_bytes have
//     T <= C = floor(max_total_bytes / piece) + nparts
// and C piece slots suffice. T > C is the call's overflow: the report says so
// and nothing else is written.
//
//   count  a workgroup per tile of kPackedTile parts: the tile's tasks and
//          bytes into its two words of the workspace.
//   scan   one workgroup: the tiles' task counts become exclusive offsets, in
//          place, in chunks of kPackedBlock tiles with a 64-bit carry; the
//          report and first[nparts] = T are stored.
//   first  a workgroup per tile: the counts again, thread u the kPackedRun
//          consecutive parts from u * kPackedRun, an exclusive sum over the
//          tile on top of the tile's offset, into first[].
//   owner  a thread per task t < min(T, C) (none when T > C): the last part
//          whose first[] is <= t, by binary search (packed_owner).
//
// Every sum saturates at ~0 (packed_add: min(the true sum, ~0), associative):
// lengths that add up beyond 2^64 give T = ~0 > C and not a small number.
//
// Workspace, in this order, every array 8-byte aligned (packed_layout):
//   first   nparts + 1 words of 64 bits
//   tiles   2 * ceil(nparts / 1024) words of 64 bits: tasks / offsets, bytes
//   crc     C words of the CRC's width w (4 or 8 bytes)
//   owner   C words of 32 bits
// Every word a call reads it has written before: no clearing, nothing kept.
//
// A value read from the plan never becomes an address by itself: owner[t] is
// clamped below nparts, the task bound to C (a kernel argument), and the
// piece comes from src[i] through parts_piece, which gives an empty piece
// behind the end of a part. A wrong plan word gives a wrong CRC, not an
// access outside the caller's buffers or the workspace.
#pragma once
#include <stdint.h>

#include "parts_plan.h"

// as PCRC_HD, for the steps that walk arrays (not constant expressions)
#ifndef PCRC_VHD
#ifdef __HIPCC__
#define PCRC_VHD __host__ __device__ inline
#else
#define PCRC_VHD inline
#endif
#endif

namespace pcrc {

constexpr uint32_t kPackedTile = 1024;  // parts of a plan tile
constexpr uint32_t kPackedBlock = 256;  // threads of a plan workgroup = tiles per chunk of the scan
constexpr uint32_t kPackedRun = kPackedTile / kPackedBlock;  // consecutive parts of one thread
constexpr uint32_t kPackedMaxGrid = 2048;         // workgroups of count / first / owner; beyond: a stride loop
constexpr uint64_t kPackedMaxSlots = 1ull << 40;  // C beyond this: -EINVAL
constexpr uint64_t kPackedMaxParts = 1ull << 31;  // nparts beyond this: -EINVAL (owner[] holds 32-bit words)

PCRC_HD uint64_t packed_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// C: the piece slots of a call.
PCRC_HD uint64_t packed_slots(uint64_t nparts, uint64_t max_total_bytes, uint64_t piece) {
    return packed_add(max_total_bytes / piece, nparts);
}
PCRC_HD uint64_t packed_tiles(uint64_t nparts) { return (nparts + kPackedTile - 1) / kPackedTile; }

// Byte offsets of the workspace's arrays and its size (nparts <= kPackedMaxParts, slots <= kPackedMaxSlots).
struct PackedLayout {
    uint64_t first, tiles, crc, owner, bytes;
};
PCRC_HD PackedLayout packed_layout(uint64_t nparts, uint64_t slots, uint64_t word) {
    PackedLayout l = {0, 0, 0, 0, 0};
    l.tiles = 8 * (nparts + 1);
    l.crc = l.tiles + 16 * packed_tiles(nparts);
    l.owner = l.crc + (slots * word + 7) / 8 * 8;
    l.bytes = l.owner + (slots * 4 + 7) / 8 * 8;
    return l;
}

// One part's tasks and bytes, and their sums.
struct PackedSum {
    uint64_t tasks, bytes;
};
PCRC_HD PackedSum packed_part(uint64_t addr, uint64_t len, uint64_t max_bytes, uint64_t piece) {
    const uint64_t n = len < max_bytes ? len : max_bytes;
    return PackedSum{parts_count(addr, n, piece), n};
}
PCRC_HD PackedSum packed_sum(PackedSum a, PackedSum b) {
    return PackedSum{packed_add(a.tasks, b.tasks), packed_add(a.bytes, b.bytes)};
}

// The tasks the piece kernel runs: all T, or none when they do not fit.
PCRC_HD uint64_t packed_bound(uint64_t tasks, uint64_t slots) { return tasks > slots ? 0 : tasks; }

// The report's four words.
PCRC_VHD void packed_report_store(uint64_t* report, PackedSum all, uint64_t slots) {
    report[0] = all.tasks > slots ? 1 : 0;
    report[1] = all.tasks;
    report[2] = all.bytes;
    report[3] = slots;
}

// The part of task t: the last i < nparts with first[i] <= t (first[0] = 0;
// parts without a piece share their first[] with the part behind them and are
// passed over). Reads first[1 .. nparts) only; the result is below nparts
// whatever first[] holds (nparts >= 1).
PCRC_VHD uint64_t packed_owner(const uint64_t* first, uint64_t nparts, uint64_t t) {
    uint64_t lo = 0, hi = nparts;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// owner[t] as an index of src[] / dst[] / first[].
PCRC_HD uint64_t packed_owner_clamp(uint32_t owner, uint64_t nparts) { return owner < nparts ? owner : nparts - 1; }

// Task t of a part of n (capped) bytes at addr whose first task is f: piece
// t - f, empty when the plan words do not fit each other (f > t, or a piece
// index whose offset would wrap) or the piece lies behind the end of the part.
PCRC_HD PartsPiece packed_piece(uint64_t addr, uint64_t n, uint64_t piece, uint64_t f, uint64_t t) {
    uint64_t lo = 0;
    if (f > t || __builtin_mul_overflow(t - f, piece, &lo)) return PartsPiece{0, 0};
    return parts_piece(addr, n, piece, t - f);
}

// The four steps in order over host arrays of (addr, len): the CPU replay of
// the kernels (which take the tile's sums by shuffles and through LDS). work:
// packed_layout(...).bytes bytes, uninitialised, 8-byte aligned.
inline void packed_replay(const uint64_t* addr, const uint64_t* len, uint64_t nparts, uint64_t max_bytes,
                          uint64_t piece, uint64_t slots, uint64_t word, uint8_t* work, uint64_t* report) {
    const PackedLayout l = packed_layout(nparts, slots, word);
    uint64_t* first = reinterpret_cast<uint64_t*>(work + l.first);
    uint64_t* tilew = reinterpret_cast<uint64_t*>(work + l.tiles);
    uint32_t* owner = reinterpret_cast<uint32_t*>(work + l.owner);
    const uint64_t tiles = packed_tiles(nparts);
    for (uint64_t k = 0; k < tiles; ++k) {  // count
        PackedSum s = {0, 0};
        for (uint64_t i = k * kPackedTile; i < nparts && i < (k + 1) * kPackedTile; ++i)
            s = packed_sum(s, packed_part(addr[i], len[i], max_bytes, piece));
        tilew[k] = s.tasks;
        tilew[tiles + k] = s.bytes;
    }
    PackedSum all = {0, 0};  // scan
    for (uint64_t k = 0; k < tiles; ++k) {
        const PackedSum s = {tilew[k], tilew[tiles + k]};
        tilew[k] = all.tasks;
        all = packed_sum(all, s);
    }
    packed_report_store(report, all, slots);
    first[nparts] = all.tasks;
    for (uint64_t k = 0; k < tiles; ++k) {  // first
        uint64_t at = tilew[k];
        for (uint64_t i = k * kPackedTile; i < nparts && i < (k + 1) * kPackedTile; ++i) {
            first[i] = at;
            at = packed_add(at, packed_part(addr[i], len[i], max_bytes, piece).tasks);
        }
    }
    const uint64_t bound = packed_bound(first[nparts], slots);  // owner
    for (uint64_t t = 0; t < bound; ++t) owner[t] = (uint32_t)packed_owner(first, nparts, t);
}

}  // namespace pcrc

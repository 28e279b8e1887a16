// iov_walk.h -- the two-cursor walk of copy + CRC between iovectors
// (photon_crc{32c,64ecma}_copy_msg_iov_n, _seg_n, _seg2_n, _window_n; DESIGN.md
// "The two-cursor walk, written once"), written once for the device kernels
// (the CRC-32C ones run it; the CRC-64 ones use IovCursor and keep copies of the
// rest, crc64_kernels.h) and for its CPU replay (tests/cpp/iov_walk_replay.cpp).
// No intrinsics here: whatever touches lanes, LDS or payload is the "unit" a
// kernel hands in (Unit32<G, U>; the replay's is memcpy + the CPU engines).
//
// Message m: source segments src[src_start[m] .. src_start[m+1]), destination
// segments dst[dst_start[m] .. dst_start[m+1]), at most size[m] bytes (no size
// array: no cap). Each step is a piece of n = min(left, src.rem, dst.rem) bytes
// through the unit; then the side(s) that ran out take their next segment:
//   - a zero-length segment on either side makes a zero-length piece (no loads,
//     no stores, the CRC unchanged), and only that side advances;
//   - both sides advance when their boundaries coincide;
//   - neither side advances when the cap ended the message.
//
// A unit gives T (the CRC's word), kGroups (lane groups per wavefront), gl and
// grp (the lane in its group, the group in its wavefront), first_wave() and
// nwaves() (the persistent grid's split), and reg = copy(s, d, left, n, reg):
// n bytes from s.p land at d.p and are chained into reg, and both cursors and
// `left` move by n (before or after the rows: the unit's choice).
#pragma once
#include <stdint.h>

#include "../../include/photon_crc/crc32c_gpu.h"

#ifdef __HIPCC__
#define PCRC_WALK __host__ __device__ __forceinline__
#else
#define PCRC_WALK inline
#endif
// Behind the parameter list of a lambda handed to the walk: every call between
// a kernel and its row loop is force-inlined, none left to the inliner.
#define PCRC_WALK_INLINE __attribute__((always_inline))

namespace pcrc {

// One side of the two-cursor walk: the current segment's unconsumed part
// [p, p + rem). PF: the NEXT segment's descriptor is loaded when the current
// one is taken -- before the rows of the piece(s) that consume it, as the
// message kernels prefetch theirs (the last one re-reads itself). Without PF
// (builds where its four registers per side would spill) the descriptor is
// loaded when it is needed, as crc64_gather_kernel loads its own.
template <bool PF>
struct IovCursor {
    const photon_crc_iovec* v;
    uint64_t i, end;           // the current segment and the message's last + 1
    const uint8_t* p;
    uint64_t rem;
    photon_crc_iovec nx[PF ? 1 : 0];
    PCRC_WALK void take(const photon_crc_iovec& c) {
        p = static_cast<const uint8_t*>(c.base);
        rem = c.len;
        if constexpr (PF) nx[0] = v[i + 1 < end ? i + 1 : i];
    }
    PCRC_WALK void begin(const photon_crc_iovec* iov, uint64_t s0, uint64_t s1) {
        v = iov;
        i = s0;
        end = s1;
        p = nullptr;
        rem = 0;
        if constexpr (PF) nx[0] = {nullptr, 0};
        if (s0 < s1) take(iov[s0]);
    }
    PCRC_WALK bool more() const { return i < end; }
    PCRC_WALK void next() {  // rem == 0: the next segment
        if (++i < end) {
            if constexpr (PF) take(nx[0]);
            else take(v[i]);
        }
    }
};

// One lane group per message, persistent grid and static split as the message
// kernels: f(m) for the group's message, which is not active when m >= nmsg
// (the groups of a wavefront stay together).
template <typename Unit, typename F>
PCRC_WALK void iov_walk_messages(const Unit& u, uint64_t nmsg, F f) {
    const uint64_t nwaves = u.nwaves();
    for (uint64_t wv = u.first_wave(); wv * Unit::kGroups < nmsg; wv += nwaves) f(wv * Unit::kGroups + u.grp);
}

// The set-up of message m: the cap, the seed (seed0, or seeds[m]) and both
// cursors. A group that is not active gets left = 0 and empty cursors: its
// walk has no piece and its cursors no segment.
template <typename A, typename T, bool PS, bool PD>
PCRC_WALK void iov_walk_begin(const A& args, uint64_t m, bool active, uint64_t& left, T& seed, IovCursor<PS>& s,
                              IovCursor<PD>& d) {
    seed = args.seed0;
    left = 0;
    s.begin(args.src, 0, 0);
    d.begin(args.dst, 0, 0);
    if (active) {
        left = args.size ? args.size[m] : ~0ull;
        if (args.seeds) seed = args.seeds[m];
        s.begin(args.src, args.src_start[m], args.src_start[m + 1]);
        d.begin(args.dst, args.dst_start[m], args.dst_start[m + 1]);
    }
}

struct IovNoHook {
    PCRC_WALK void operator()() const {}
};

// The piece loop. piece(n): the unit's copy (it moves the cursors and `left`).
// Behind a piece that did not use up the cap: before_next() (the one-side
// kernel closes a chosen-side segment there), then for each side whose segment
// ended its hook -- src_end(), dst_end(): s.i / d.i is still the segment that
// ended -- and that side's next(), the source side first.
template <bool PS, bool PD, typename Piece, typename Before = IovNoHook, typename SrcEnd = IovNoHook,
          typename DstEnd = IovNoHook>
PCRC_WALK void iov_walk_pieces(IovCursor<PS>& s, IovCursor<PD>& d, uint64_t& left, Piece piece,
                               Before before_next = Before(), SrcEnd src_end = SrcEnd(), DstEnd dst_end = DstEnd()) {
    while (left && s.more() && d.more()) {
        uint64_t n = s.rem < d.rem ? s.rem : d.rem;
        n = n < left ? n : left;
        piece(n);
        if (!left) break;
        before_next();
        if (!s.rem) {
            src_end();
            s.next();
        }
        if (!d.rem) {
            dst_end();
            d.next();
        }
    }
}

// The epilogue, by the first lane of an active group (`store`): out[m], and
// copied[m] = the cap less what is left of it.
template <typename A, typename T>
PCRC_WALK void iov_walk_finish(const A& args, uint64_t m, bool store, T crc, uint64_t left) {
    if (store) {
        args.out[m] = crc;
        // (the cap is read again: two registers less across the walk)
        if (args.copied) args.copied[m] = (args.size ? args.size[m] : ~0ull) - left;
    }
}

// The whole kernel body of _copy_msg_iov_n (SEG2 = false: the
// walk and nothing else) and of _copy_msg_iov_seg2_n (§4.13; SEG2: the running
// CRC -- chained from seed_m through the whole message, never reset -- stored at
// the entry of every segment a cursor leaves or ends in, for seg_unscan_kernel
// to turn into per-segment CRCs; no multiply here. A zero-length segment's
// entry receives the unchanged running value; the entries behind the segment
// in which the walk ended are not touched).
template <bool SEG2, typename Unit, typename A>
PCRC_WALK void iov_copy_messages(const A& args, const Unit& u) {
    iov_walk_messages(u, args.nmsg, [&](uint64_t m) PCRC_WALK_INLINE {
        const bool active = m < args.nmsg;
        typename Unit::T acc;
        uint64_t left;
        IovCursor<true> s, d;
        iov_walk_begin(args, m, active, left, acc, s, d);
        iov_walk_pieces(
            s, d, left, [&](uint64_t n) PCRC_WALK_INLINE { acc = u.copy(s, d, left, n, acc); }, IovNoHook(),
            [&]() PCRC_WALK_INLINE {  // the running CRC at the end of source segment s.i
                if constexpr (SEG2)
                    if (u.gl == 0) args.src_seg[s.i] = acc;
            },
            [&]() PCRC_WALK_INLINE {
                if constexpr (SEG2)
                    if (u.gl == 0) args.dst_seg[d.i] = acc;
            });
        if constexpr (SEG2) {
            // The segment each side's walk ended in (or before its first
            // byte); an inactive group's cursors are empty.
            if (u.gl == 0) {
                if (s.more()) args.src_seg[s.i] = acc;
                if (d.more()) args.dst_seg[d.i] = acc;
            }
        }
        iov_walk_finish(args, m, active && u.gl == 0, acc, left);
    });
}

}  // namespace pcrc

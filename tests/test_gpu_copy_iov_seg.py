"""Copy + CRC between iovectors with one CRC per segment of one side
(photon_crc32c_copy_msg_iov_seg_n, photon_crc64ecma_copy_msg_iov_seg_n).
Every CRC -- per message and per segment -- is checked bit-exactly against
the pinned oracle (tests/_oracle.py) over the host copy of the source bytes
that the piece walk below selects; every destination byte against that walk
(`_walk`: min(size, dst, src) per step, with the source and destination
segment of every piece -- a model of iovector.cpp:301-314 written here,
independent of the kernel). Every destination arena is pre-filled with 0xA5
and compared WHOLE; d_seg_out has 8 guard entries on each side, guards and
body are pre-filled with a canary that no test expects as a CRC, the guards
must survive and every body entry must be overwritten, the 0 entries
included. Every run also checks the fold identity: the oracle's combine of
the segment CRCs with the LANDED lengths from seed_m equals d_out. The case
generators assert that the destination ranges are disjoint from one another
and from the guards, and that they produce the number of cases they state."""
import os
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64
SEG_GUARD = 8
POOL = (1 << 20) + 4096
ROWS = {4: 4, 8: 4, 16: 2, 32: 4, 64: 4}  # default rows per step of each lane-group size
UNLIMITED = (1 << 64) - 1
SRC, DST = ck.SEG_OF_SRC, ck.SEG_OF_DST
SIDES = [pytest.param(SRC, id="src"), pytest.param(DST, id="dst")]
# A source segment that the call must never read: the walk ends before it.
NEVER = "never"
NEVER_ADDR = 0x00005EADBEEF0000
# PHOTON_FUZZ_ROUNDS=k multiplies the fuzz rounds (longer soak runs, new seeds).
SOAK = max(1, int(os.environ.get("PHOTON_FUZZ_ROUNDS", "1")))


def _seg_canary(crc64):
    return 0xA5A5A5A5A5A5A5A5 if crc64 else 0xA5A5A5A5


@pytest.fixture(scope="module")
def dev_pool():
    import torch
    assert torch.cuda.is_available()
    host = datagen.stream_bytes(0xC0B1A, POOL)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return torch, host, d


@pytest.fixture(autouse=True)
def _reset():
    yield
    ck.set_lanes_per_buffer(0)
    ck.set_batch_grid(0)


class Msg:
    """src: [(pool offset | None (null base) | NEVER, length)], dst: [(arena
    offset | None (null base), length)], size: the cap or None."""

    def __init__(self, src, dst, size=None, seed=0):
        self.src, self.dst, self.size, self.seed = list(src), list(dst), size, seed


class Layout:
    """Hands out destination ranges of one arena, in address order."""

    def __init__(self, start=GUARD):
        self.pos = start

    def put(self, n, like=None, delta=0, gap=0):
        """n bytes at the next free address + gap; with `like` (a source
        offset) moved up by 0..15 bytes so that (dst - like) % 16 == delta."""
        self.pos += gap
        if like is not None:
            self.pos += ((like + delta) - self.pos) % 16
        at = self.pos
        self.pos += n
        return at


def _walk(src, dst, size):
    """The piece walk: [(source offset, destination offset, n, source segment,
    destination segment)], n > 0."""
    pieces = []
    si = di = so = do = 0
    left = UNLIMITED if size is None else size
    while left and si < len(src) and di < len(dst):
        n = min(left, src[si][1] - so, dst[di][1] - do)
        if n:
            pieces.append((src[si][0] + so, dst[di][0] + do, n, si, di))
        left -= n
        so += n
        do += n
        if so == src[si][1]:
            si, so = si + 1, 0
        if do == dst[di][1]:
            di, do = di + 1, 0
    return pieces


def test_walk_model():
    # the model itself, on the cases of iovector.cpp:301-314 that matter (no GPU work)
    assert _walk([(0, 10)], [(100, 4), (200, 6)], None) == [(0, 100, 4, 0, 0), (4, 200, 6, 0, 1)]
    assert _walk([(0, 4), (50, 6)], [(100, 10)], None) == [(0, 100, 4, 0, 0), (50, 104, 6, 1, 0)]
    assert _walk([(0, 4), (50, 6)], [(100, 4), (200, 6)], None) == [(0, 100, 4, 0, 0), (50, 200, 6, 1, 1)]
    assert _walk([(0, 10)], [(100, 20)], 7) == [(0, 100, 7, 0, 0)]
    assert _walk([(None, 0), (0, 3), (None, 0)], [(None, 0), (None, 0), (9, 5)], None) == [(0, 9, 3, 1, 2)]
    assert _walk([(0, 10)], [], None) == [] and _walk([], [(0, 10)], None) == [] and _walk([(0, 1)], [(5, 1)], 0) == []
    # landed lengths per segment: a cap inside the second destination segment
    assert _landed(Msg([(0, 10)], [(100, 4), (200, 6), (300, 9)], 7), DST) == [4, 3, 0]
    assert _landed(Msg([(0, 4), (50, 6), (70, 1)], [(100, 7)], None), SRC) == [4, 3, 0]


def _landed(m, side):
    """Bytes of every segment of `side` that take part in the copy."""
    segs = m.dst if side == DST else m.src
    got = [0] * len(segs)
    for _, _, n, si, di in _walk(m.src, m.dst, m.size):
        got[di if side == DST else si] += n
    return got


def _check_disjoint(msgs, arena_size):
    rng = sorted((at, at + n) for m in msgs for at, n in m.dst if n)
    prev = GUARD
    for lo, hi in rng:
        assert lo >= prev, f"destination [{lo}, {hi}) overlaps its neighbour or the front guard"
        prev = hi
    assert prev <= arena_size - GUARD, "a destination reaches into the back guard"


def _dev64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _dev32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def _descriptors(msgs, side, base):
    rows, start = [], [0]
    for m in msgs:
        for at, n in getattr(m, side):
            if at is None:
                assert n == 0
                rows.append((0, 0))
            elif at is NEVER:
                rows.append((NEVER_ADDR, n))
            else:
                rows.append((base + at, n))
        start.append(len(rows))
    return np.asarray(rows or [(0, 0)], np.uint64).reshape(-1, 2), np.asarray(start, np.uint64), len(rows)


def _expect(oracle, host, msgs, arena_size, crc64, seed0, side):
    """The arena, the message CRCs, the copied counts, and per message the
    (CRC from seed 0, landed length) of every segment of `side`."""
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    want = np.full(arena_size, CANARY, np.uint8)
    crcs, copied, segs = [], [], []
    for m in msgs:
        pieces = _walk(m.src, m.dst, m.size)
        per = [[] for _ in (m.dst if side == DST else m.src)]
        for so, do, n, si, di in pieces:
            assert so is not NEVER and so is not None and do is not None
            want[do:do + n] = host[so:so + n]
            per[di if side == DST else si].append(host[so:so + n].tobytes())
        data = b"".join(host[so:so + n].tobytes() for so, _, n, _, _ in pieces)
        seed = m.seed if seed0 is None else seed0
        crcs.append(crc(data, seed))
        copied.append(len(data))
        segs.append([(crc(b"".join(p), 0), sum(len(x) for x in p)) for p in per])
        assert [n for _, n in segs[-1]] == _landed(m, side)
        assert all(c == 0 for c, n in segs[-1] if n == 0)
        assert all(c != _seg_canary(crc64) for c, _ in segs[-1])
    return want, crcs, copied, segs


def _combine(oracle, crc64, c1, c2, n):
    """crc_combine by the oracle. CRC-32C: its own combine. CRC-64/ECMA has
    none there; c1 * x^(8n) is crc(n zero bytes, c1) ^ crc(n zero bytes, 0)
    (the register starts at ~seed and the result is inverted, so the two
    differ by exactly the seed shifted by n bytes), and combine = that ^ c2."""
    if not crc64:
        assert n < 1 << 32
        return oracle.combine(c1, c2, n)
    z = bytes(n)
    return oracle.crc64ecma(z, c1) ^ oracle.crc64ecma(z, 0) ^ c2


def _launch(torch, msgs, src_base, arena, crc64, seed0, with_copied, side, stream=None):
    """One call; returns the device tensors that hold its results and inputs."""
    siov, sstart, nsrc = _descriptors(msgs, "src", src_base)
    diov, dstart, ndst = _descriptors(msgs, "dst", arena.data_ptr())
    nmsg = len(msgs)
    size = None
    if any(m.size is not None for m in msgs):
        size = _dev64(torch, [UNLIMITED if m.size is None else m.size for m in msgs])
    if seed0 is None:
        seeds = _dev64(torch, [m.seed for m in msgs]) if crc64 else _dev32(torch, [m.seed for m in msgs])
    else:
        seeds = None
    out = torch.full((nmsg,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
    copied = torch.full((nmsg,), -1, dtype=torch.int64, device="cuda") if with_copied else None
    nside = ndst if side == DST else nsrc
    seg = (_dev64 if crc64 else _dev32)(torch, [_seg_canary(crc64)] * (nside + 2 * SEG_GUARD))
    seg_body = seg.data_ptr() + SEG_GUARD * (8 if crc64 else 4)
    keep = (_dev64(torch, siov), _dev64(torch, sstart), _dev64(torch, diov), _dev64(torch, dstart), size, seeds,
            nsrc, ndst)

    def call(stream=stream):
        (ck.copy_msg64_iov_seg_n if crc64 else ck.copy_msg_iov_seg_n)(
            keep[0], keep[1], nsrc, keep[2], keep[3], ndst, nmsg, side, seg_body, out, size=size, seed=seed0 or 0,
            seeds=seeds, copied=copied, stream=stream)
    return call, out, copied, seg, keep


def _compare(oracle, msgs, out, copied, seg, arena_bytes, want, crcs, ncopied, segs, crc64, seed0, tag):
    got = out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    for k, m in enumerate(msgs):
        assert int(got[k]) == crcs[k], (tag, "crc of message", k, m.src, m.dst, m.size, hex(int(got[k])), hex(crcs[k]))
    if copied is not None:
        gc = copied.cpu().numpy().view(np.uint64)
        for k, m in enumerate(msgs):
            assert int(gc[k]) == ncopied[k], (tag, "copied of message", k, m.src, m.dst, m.size)
    gs = seg.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    canary = _seg_canary(crc64)
    nside = sum(len(s) for s in segs)
    assert gs.size == nside + 2 * SEG_GUARD
    assert all(int(v) == canary for v in gs[:SEG_GUARD]), (tag, "front guard of d_seg_out", gs[:SEG_GUARD])
    assert all(int(v) == canary for v in gs[SEG_GUARD + nside:]), (tag, "back guard of d_seg_out", gs[SEG_GUARD + nside:])
    at = SEG_GUARD
    for k, m in enumerate(msgs):
        acc = m.seed if seed0 is None else seed0
        for j, (c, n) in enumerate(segs[k]):
            g = int(gs[at])
            assert g != canary, (tag, "segment entry not written", k, j, m.src, m.dst, m.size)
            assert g == c, (tag, "segment crc", k, j, n, m.src, m.dst, m.size, hex(g), hex(c))
            acc = _combine(oracle, crc64, acc, g, n)
            at += 1
        assert acc == int(got[k]), (tag, "fold of the segment crcs with the landed lengths", k, hex(acc), hex(int(got[k])))
    bad = np.flatnonzero(arena_bytes != want)
    if bad.size:
        b = int(bad[0])
        near = [(k, at, n) for k, m in enumerate(msgs) for at, n in m.dst if n and at <= b + 16 and b < at + n + 16]
        raise AssertionError(f"{tag}: arena byte {b} is {arena_bytes[b]:#x}, want {want[b]:#x}; {bad.size} bytes "
                             f"differ; destinations near it (message, at, n): {near[:4]}")


def _run(torch, oracle, host, src_base, msgs, lanes, side, crc64=False, grid=0, seed0=None, with_copied=True):
    arena_size = max([GUARD] + [at + n for m in msgs for at, n in m.dst if n]) + GUARD
    _check_disjoint(msgs, arena_size)
    arena = torch.full((arena_size,), CANARY, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    want, crcs, ncopied, segs = _expect(oracle, host, msgs, arena_size, crc64, seed0, side)
    call, out, copied, seg, keep = _launch(torch, msgs, src_base, arena, crc64, seed0, with_copied, side)
    ck.set_lanes_per_buffer(lanes)
    ck.set_batch_grid(grid)
    call()
    torch.cuda.synchronize()
    arena_bytes = arena.cpu().numpy()
    _compare(oracle, msgs, out, copied, seg, arena_bytes, want, crcs, ncopied, segs, crc64, seed0,
             (lanes, crc64, grid, side))
    return out, copied, seg, arena, keep


def _seg_body(seg, crc64):
    a = seg.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    return a[SEG_GUARD:a.size - SEG_GUARD]


def _seed(rnd, crc64, k):
    return 0 if k % 5 == 0 else (1 << (64 if crc64 else 32)) - 1 if k % 5 == 1 else rnd.getrandbits(64 if crc64 else 32)


# ------------------------------------------------------------ boundary order
def _boundary_msgs(crc64):
    """src = [a, 200-a] into dst = [b, 200-b], a, b in 0, 20, .., 200: the
    source boundary before, on and after the destination's, empty first and
    last segments; destinations packed back to back at odd addresses."""
    rnd = random.Random(0xB0DA)
    edges = tuple(range(0, 201, 20))
    lay = Layout(GUARD + 1)  # odd: the packed segments share 16-byte blocks
    msgs = []
    for a in edges:
        for b in edges:
            k = len(msgs)
            s0 = 1024 * (k % 509) + 16 * (k % 7) + (0, 5, 15)[k % 3]
            s1 = s0 + 304 + (k % 11)
            d0 = lay.put(b, gap=(lay.pos + 1) % 2)  # every message starts at an odd address
            d1 = lay.put(200 - b)  # back to back
            msgs.append(Msg([(s0, a), (s1, 200 - a)], [(d0, b), (d1, 200 - b)], seed=_seed(rnd, crc64, k)))
    assert len(msgs) == 121
    assert all(m.dst[0][0] % 2 == 1 for m in msgs)
    assert sum(1 for m in msgs if m.src[0][1] == m.dst[0][1]) == 11  # the segment ends coincide
    return msgs


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
def test_boundary_order_4_lanes(dev_pool, oracle, crc64, side):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _boundary_msgs(crc64), 4, side, crc64)


# ------------------------------------------------------------ row boundaries
def _row_lengths(g):
    u = ROWS[g]
    lens = [k * 16 * g + dd for k in range(2 * u + 4) for dd in (-17, -16, -1, 0, 1, 15, 16, 17) if k * 16 * g + dd >= 0]
    assert len(lens) == 8 * (2 * u + 4) - 3  # k = 0 drops its three negative lengths
    return lens


def _scatter_msg(lens, delta, src_at):
    """One long source segment into destination segments of `lens`, every
    piece placed so that (dst - src) % 16 == delta."""
    lay = Layout()
    dst, pos = [], src_at
    for n in lens:
        dst.append((lay.put(n, like=pos, delta=delta), n))
        pos += n
    return Msg([(src_at, sum(lens))], dst, seed=0x12345678)


def _transposed_msg(lens, delta, dst_at):
    """Source segments of `lens` into one destination segment, every piece
    placed so that (dst - src) % 16 == delta."""
    src, spos, dpos = [], 0, dst_at
    for n in lens:
        spos += ((dpos - delta) - spos) % 16 + 16 * (len(src) % 3)
        src.append((spos, n))
        spos += n
        dpos += n
    assert spos <= POOL
    return Msg(src, [(dst_at, sum(lens))], seed=0x9ABCDEF0)


G_CRC = [(4, False), (8, False), (16, False), (32, False), (64, False), (8, True), (32, True)]


@pytest.mark.parametrize("delta", [0, 9])
@pytest.mark.parametrize("g,crc64", G_CRC)
def test_row_boundaries_scatter_dst_side_equals_batch_iov(dev_pool, oracle, g, crc64, delta):
    torch, host, d = dev_pool
    lens = _row_lengths(g)
    msg = _scatter_msg(lens, delta, 5)
    assert len(msg.dst) == len(lens) and len(_walk(msg.src, msg.dst, None)) == sum(1 for n in lens if n)
    out, copied, seg, arena, keep = _run(torch, oracle, host, d.data_ptr(), [msg], g, DST, crc64)
    # the destination blocks checksummed again where they landed: the same CRCs
    again = torch.full((len(lens),), -1, dtype=out.dtype, device="cuda")
    (ck.batch64_iov if crc64 else ck.batch_iov)(keep[2], len(lens), again)
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy().view(np.uint64 if crc64 else np.uint32), _seg_body(seg, crc64))


@pytest.mark.parametrize("delta", [0, 9])
@pytest.mark.parametrize("g,crc64", G_CRC)
def test_row_boundaries_transposed_src_side_equals_gather(dev_pool, oracle, g, crc64, delta):
    torch, host, d = dev_pool
    lens = _row_lengths(g)
    msg = _transposed_msg(lens, delta, GUARD + 3)
    assert len(msg.src) == len(lens)
    out, copied, seg, arena, keep = _run(torch, oracle, host, d.data_ptr(), [msg], g, SRC, crc64)
    # the same message through the gather: the same d_seg_out, d_out and bytes
    arena2 = torch.full((arena.numel(),), CANARY, dtype=torch.uint8, device="cuda")
    gout = torch.zeros_like(out)
    gseg = torch.full((len(lens),), -1, dtype=out.dtype, device="cuda")
    dst_ptrs = _dev64(torch, [arena2.data_ptr() + GUARD + 3])
    ck.set_lanes_per_buffer(g)
    (ck.gather64_msg_n if crc64 else ck.gather_msg_n)(keep[0], keep[1], 1, len(lens), dst_ptrs, gseg, gout,
                                                      seeds=keep[5])
    torch.cuda.synchronize()
    assert np.array_equal(gout.cpu().numpy(), out.cpu().numpy())
    assert np.array_equal(gseg.cpu().numpy().view(np.uint64 if crc64 else np.uint32), _seg_body(seg, crc64))
    assert np.array_equal(arena2.cpu().numpy(), arena.cpu().numpy())


# ------------------------------------------------- short sides and the cap
def _short_and_cap_msgs(crc64):
    rnd = random.Random(0x5CA9)
    lay = Layout(GUARD + 3)
    spos = [7]

    def src(*lens):
        segs = []
        for n in lens:
            if n is NEVER:
                segs.append((NEVER, 4096))
            else:
                segs.append((spos[0], n))
                spos[0] += n + 13
        return segs

    def dst(*lens, like=None):
        return [(lay.put(n, gap=(1 if i else 5), like=like if i == 0 else None), n) for i, n in enumerate(lens)]

    cases = []
    # sum(src) > sum(dst): the trailing source segments are never read, their entries are 0
    cases.append((src(300, 500, NEVER, NEVER), dst(100, 250, 450), None))
    cases.append((src(300, 500, NEVER), dst(700), None))          # the destination ends inside a source segment
    cases.append((src(5000, 3000, NEVER), dst(4096, 3904), None))  # on the source boundary, long pieces
    # sum(dst) > sum(src): the rest of the destination keeps its 0xA5, its segment a prefix CRC, later ones 0
    cases.append((src(100, 64), dst(50, 1000, 30, 40), None))
    cases.append((src(4097), dst(3000, 3000, 3000), None))
    # no source segments; no destination segments; neither
    cases.append((src(), dst(100), None))
    cases.append((src(100), dst(), None))
    cases.append((src(), dst(), None))
    # the cap: 0, mid-piece, on a source boundary, on a destination boundary, larger than both sums
    for size in (0, 1, 99, 100, 101, 120, 150, 151, 299, 300, 400, 599, 600, 601, 800, 10 ** 6, UNLIMITED):
        cases.append((src(100, 200, 300), dst(150, 250, 400), size))
    for size in (4095, 4096, 4097, 4999, 5000, 5001, 7999, 8000, 8192, 9000):
        s = src(5000, 3000)
        cases.append((s, dst(4096, 4096, like=s[0][0]), size))
    # the cap ends the message on a source boundary: the next descriptor is not followed
    cases.append((src(100, NEVER), dst(200), 100))
    cases.append((src(4096, NEVER), dst(3000, 3000), 4096))
    stated = 8 + 17 + 10 + 2
    assert len(cases) == stated
    msgs = [Msg(s, d_, size, _seed(rnd, crc64, k)) for k, (s, d_, size) in enumerate(cases)]
    assert spos[0] <= POOL
    empties = [m for m in msgs if not _walk(m.src, m.dst, m.size)]
    assert len(empties) == 4  # the seed comes back, every entry is 0
    for side in (SRC, DST):  # the cap on a boundary of this side, and a prefix in the ended-in segment
        assert sum(1 for m in msgs if m.size in (100, 300, 150, 400, 4096, 5000)) >= 6
        assert any(0 < n < seg[1] for m in msgs for n, seg in zip(_landed(m, side), m.dst if side == DST else m.src))
        assert any(n == 0 and seg[1] for m in msgs for n, seg in zip(_landed(m, side), m.dst if side == DST else m.src))
    return msgs


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("with_copied,seed0", [(True, None), (False, None), (True, 0xFEEDC0DE5EED0001)])
def test_short_sides_and_cap(dev_pool, oracle, crc64, lanes, with_copied, seed0, side):
    torch, host, d = dev_pool
    if seed0 is not None and not crc64:
        seed0 &= 0xFFFFFFFF
    _run(torch, oracle, host, d.data_ptr(), _short_and_cap_msgs(crc64), lanes, side, crc64, seed0=seed0,
         with_copied=with_copied)


# ------------------------------------------------- zero-length segment runs
def _zero_run_msgs(crc64):
    rnd = random.Random(0x2E80)
    lay = Layout(GUARD + 9)
    Z = (None, 0)
    msgs, spos = [], 11
    for a, b in ((50, 70), (3000, 5000)):
        s0, s1 = spos, spos + a + 29
        spos = s1 + b + 3
        S0, S1 = (s0, a), (s1, b)

        def D(n):
            return (lay.put(n, gap=1), n)
        shapes = [
            ([Z, Z, Z, S0, S1], [D(a + b)]),                    # leading, source
            ([S0, S1], [Z, Z, D(a + b)]),                        # leading, destination
            ([S0, S1, Z, Z], [D(a), D(b)]),                      # trailing, source
            ([S0, S1], [D(a), D(b), Z, Z, Z]),                   # trailing, destination
            ([S0, Z, Z, S1], [D(a + b)]),                        # between, source, mid-piece of the destination
            ([S0, S1], [D(a - 7), Z, Z, Z, D(b + 7)]),           # between, destination, mid-piece of the source
            ([S0, Z, Z, S1], [D(a), Z, Z, Z, D(b)]),             # both sides at the same stream position
            ([Z, S0, Z, S1, Z], [Z, D(a), Z, D(b), Z]),          # everywhere
            ([Z, Z], [D(10)]),                                   # only empty source segments
            ([S0], [Z, Z, Z]),                                   # only empty destination segments
        ]
        for s, d_ in shapes:
            msgs.append(Msg(s, d_, None, _seed(rnd, crc64, len(msgs))))
    assert len(msgs) == 20 and spos <= POOL
    return msgs


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("lanes", [4, 16, 64])
def test_zero_length_runs(dev_pool, oracle, crc64, lanes, side):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _zero_run_msgs(crc64), lanes, side, crc64)


# -------------------------------------------------------------------- rounds
def _round_msgs(g, crc64, side):
    """Three rounds of a one-workgroup grid. Chosen-side segment counts 0, 1,
    2, G-1, G, G+1, 2G+1 in turn; every fifth message a run of one length
    followed by a run of another; the first message of rounds 2 and 3 opens
    with the length that its lane group folded last in the round before."""
    gpw = 64 // g
    per_round = 16 * gpw
    nmsg = 2 * per_round + gpw + 1
    rnd = random.Random(0x5E6 + g + (1000 if side == DST else 0))
    counts = [0, 1, 2, g - 1, g, g + 1, 2 * g + 1]
    lens_from = [0, 1, 15, 16, 17, 63, 64, 65, 100, 300, 1000]
    lay = Layout(GUARD + 1)
    msgs, chosen_lens = [], []
    for k in range(nmsg):
        nc = counts[(k + 1) % 7]
        carried = k in (0, per_round, 2 * per_round) or k + per_round in (per_round, 2 * per_round)
        if k % 5 == 0 and nc >= 2:
            a = rnd.randrange(1, nc)
            cl = [rnd.choice(lens_from[1:])] * a + [rnd.choice(lens_from[1:])] * (nc - a)
        else:
            cl = [rnd.choice(lens_from[1:] if carried else lens_from) for _ in range(nc)]
        if k in (per_round, 2 * per_round):
            cl[0] = [n for n in chosen_lens[k - per_round] if n][-1]
        chosen_lens.append(cl)
        total = sum(cl)
        # the other side: one segment of exactly the sum (everything lands), or a few random ones
        if carried or k % 3 == 0:
            ol = [total]
        else:
            ol = [rnd.choice(lens_from) for _ in range(rnd.randrange(0, 4))]
        sl, dl = (ol, cl) if side == DST else (cl, ol)
        src = [(rnd.randrange(0, POOL - n), n) for n in sl]
        dst = [(lay.put(n, gap=rnd.choice((0, 0, 1, 5))), n) for n in dl]
        msgs.append(Msg(src, dst, None, _seed(rnd, crc64, k)))
    assert len(msgs) == {64: 34, 32: 67, 16: 133, 8: 265, 4: 529}[g]
    assert {len(c) for c in chosen_lens} == set(counts)
    for k in (per_round, 2 * per_round):  # the basis cache is carried across a round
        before = [n for n in _landed(msgs[k - per_round], side) if n]
        assert before and before[-1] == _landed(msgs[k], side)[0]
    assert sum(1 for k in range(0, nmsg, 5) if len(set(chosen_lens[k])) == 2) >= 1
    return msgs


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("g", [4, 8, 16, 32, 64])
def test_rounds_one_workgroup(dev_pool, oracle, g, crc64, side):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _round_msgs(g, crc64, side), g, side, crc64, grid=1)


# -------------------------------------------------------------- equal blocks
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("side", SIDES)
def test_equal_blocks(dev_pool, oracle, crc64, side):
    """8 x 8 KiB source segments into 16 x 4 KiB blocks with a CRC per block
    (dst side), and 16 x 4 KiB blocks into 8 x 8 KiB segments with a CRC per
    block (src side): one message per lane group of one full wave, 8 lanes."""
    torch, host, d = dev_pool
    big, small = [8192] * 8, [4096] * 16
    sl, dl = (big, small) if side == DST else (small, big)
    lay = Layout()
    msgs = []
    for k in range(8):
        base = 65536 * k
        order = [(5 * i + k) % len(sl) for i in range(len(sl))]  # the message's segments in permuted slots
        src = [(base + sl[0] * o, sl[0]) for o in order]
        dst = [(lay.put(n, like=0, delta=0, gap=16 * (i % 2)), n) for i, n in enumerate(dl)]
        msgs.append(Msg(src, dst, None, k * 0x01010101))
    assert len(msgs) == 8 and all(sum(n for _, n in m.src) == 65536 == sum(n for _, n in m.dst) for m in msgs)
    _run(torch, oracle, host, d.data_ptr(), msgs, 8, side, crc64)


# --------------------------------------------------------------- long pieces
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("delta", [0, 9])
@pytest.mark.parametrize("lanes", [32, 64])
def test_long_pieces(dev_pool, oracle, lanes, delta, crc64, side):
    torch, host, d = dev_pool
    n = (1 << 20) + 5
    so = 21
    lay = Layout()
    d0 = lay.put(3, like=so, delta=delta)
    d1 = lay.put(1 << 20, like=so + 3, delta=delta, gap=16)
    d2 = lay.put(2, gap=7)
    msg = Msg([(so, n)], [(d0, 3), (d1, 1 << 20), (d2, 2)], None, 0xA5A5A5A5)
    assert (d1 - (so + 3)) % 16 == delta and so + n <= POOL
    _run(torch, oracle, host, d.data_ptr(), [msg], lanes, side, crc64)


# ---------------------------------------------------------------------- fuzz
def _lengths(rnd, k):  # the length mix of tests/test_gpu_fuzz.py
    out = []
    for _ in range(k):
        r = rnd.random()
        out.append(rnd.randrange(0, 80) if r < 0.3 else rnd.randrange(80, 5000) if r < 0.8
                   else rnd.randrange(5000, 300000))
    return out


def _fuzz_msgs(rnd, crc64, nmsg):
    lay = Layout(GUARD + rnd.randrange(16))
    msgs = []
    for k in range(nmsg):
        src = [(rnd.randrange(0, POOL - n), n) if n or rnd.random() < 0.5 else (None, 0)
               for n in _lengths(rnd, rnd.randrange(0, 7))]
        dst = []
        for i, n in enumerate(_lengths(rnd, rnd.randrange(0, 7))):
            if n == 0 and rnd.random() < 0.5:
                dst.append((None, 0))
                continue
            like = rnd.choice([None, None, src[0][0] if src and src[0][0] is not None else None])
            dst.append((lay.put(n, like=like, delta=0, gap=rnd.choice((0, 0, 1, 7, 16, 33))), n))
        total = min(sum(n for _, n in src), sum(n for _, n in dst))
        r = rnd.random()
        size = None if r < 0.4 else rnd.randrange(0, total + 2) if r < 0.8 else total if r < 0.9 else total + 1000
        msgs.append(Msg(src, dst, size, 0 if rnd.random() < 0.3 else rnd.getrandbits(64 if crc64 else 32)))
    assert len(msgs) == nmsg
    return msgs


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("round_", range(3 * SOAK))
def test_fuzz(dev_pool, oracle, round_, crc64, side):
    torch, host, d = dev_pool
    rnd = random.Random(9000 + round_ + (500 if crc64 else 0) + (50 if side == DST else 0))
    ran = 0
    for i, lanes in enumerate((0, 4, 8, 16, 32, 64)):
        msgs = _fuzz_msgs(rnd, crc64, 40)
        _run(torch, oracle, host, d.data_ptr(), msgs, lanes, side, crc64, grid=(0, 2)[(i + round_) % 2],
             with_copied=rnd.random() < 0.8)
        ran += 1
    assert ran == 6


# ------------------------------------------------------------------ identity
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("crc64", [False, True])
def test_identity_with_copy_msg_iov_n(dev_pool, oracle, crc64, side):
    """d_out and d_copied are bit-equal to photon_crc*_copy_msg_iov_n's on the
    same arguments (the fold identity is part of every run, see _compare)."""
    torch, host, d = dev_pool
    rnd = random.Random(0x1DE7 + (500 if crc64 else 0))
    for lanes in (0, 8):
        msgs = _fuzz_msgs(rnd, crc64, 40)
        out, copied, seg, arena, keep = _run(torch, oracle, host, d.data_ptr(), msgs, lanes, side, crc64)
        # the arena sits at the same address: the same descriptors
        plain_out = torch.full_like(out, -1)
        plain_copied = torch.full_like(copied, -1)
        arena_before = arena.cpu().numpy()
        ck.set_lanes_per_buffer(lanes)
        (ck.copy_msg64_iov_n if crc64 else ck.copy_msg_iov_n)(keep[0], keep[1], keep[6], keep[2], keep[3], keep[7],
                                                              len(msgs), plain_out, size=keep[4], seeds=keep[5],
                                                              copied=plain_copied)
        torch.cuda.synchronize()
        assert np.array_equal(plain_out.cpu().numpy(), out.cpu().numpy())
        assert np.array_equal(plain_copied.cpu().numpy(), copied.cpu().numpy())
        assert np.array_equal(arena.cpu().numpy(), arena_before)


# ------------------------------------------------------------- graph capture
@pytest.mark.parametrize("crc64,side", [pytest.param(False, DST, id="crc32c-dst"), pytest.param(True, SRC, id="crc64-src")])
def test_graph_capture(oracle, crc64, side):
    # one call per graph, replayed over a refilled source, a re-canaried arena and a re-canaried d_seg_out
    import torch
    nbytes, count = 4096, 48
    d = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    lay = Layout(GUARD + 1)
    msgs = []
    for k in range(count):
        so = nbytes * k + (k % 16)
        cut = 1 + (k * 523) % 4000
        d0 = lay.put(cut, like=so, delta=0 if k % 2 == 0 else 3)
        d1 = lay.put(nbytes, gap=k % 3)
        msgs.append(Msg([(so, 1000), (so + 1000, nbytes - 1000 - 16)], [(d0, cut), (d1, nbytes)],
                        None if k % 4 else 3500, k + 1))
    arena_size = lay.pos + GUARD
    _check_disjoint(msgs, arena_size)
    arena = torch.full((arena_size,), CANARY, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC0B90)
    call, out, copied, seg, keep = _launch(torch, msgs, d.data_ptr(), arena, crc64, None, True, side)
    canary = seg.clone()
    call()  # first-call set-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(stream=torch.cuda.current_stream())
    for fill in (0xC0B91, 0xC0B92):
        ck.fill_splitmix(d, nbytes, nbytes, count, fill)
        arena.fill_(CANARY)
        out.fill_(-1)
        copied.fill_(-1)
        seg.copy_(canary)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = d.cpu().numpy()
        want, crcs, ncopied, segs = _expect(oracle, host, msgs, arena_size, crc64, None, side)
        _compare(oracle, msgs, out, copied, seg, arena.cpu().numpy(), want, crcs, ncopied, segs, crc64, None, hex(fill))

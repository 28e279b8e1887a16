"""The ranged read from checksummed blocks
(photon_crc32c_copy_msg_iov_window_n, photon_crc64ecma_copy_msg_iov_window_n):
every source segment read in full and checksummed, a window of the source
stream landed in the destination iovector. The rig is that of
tests/test_gpu_copy_iov_seg.py: a 1 MiB seeded pool, a destination arena
pre-filled with 0xA5 and compared WHOLE, 8 canary guard entries on each side
of d_src_seg_out with every body entry required to be overwritten, and a base
that must never be read (NEVER_ADDR) in zero-length segments only -- here
every non-empty source segment is read. Every CRC is checked bit-exactly
against the pinned oracle (tests/_oracle.py) over the host bytes that the
model below selects (`_window`: a = min(skip, L), k = min(size, D, L - a),
written here from the call's definition, independent of the kernel). Every run
also checks the identity: the oracle's combine of d_src_seg_out with the
segment lengths from seed 0 equals the oracle CRC of the whole source stream;
and that nothing is written behind the call's work words."""
import os
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_gpu_copy_iov_seg import (CANARY, GUARD, NEVER, NEVER_ADDR, POOL, ROWS, SEG_GUARD, UNLIMITED, Layout,
                                         _check_disjoint, _combine, _dev32, _dev64, _seg_canary)

pytestmark = pytest.mark.gpu

WORK_GUARD = 8
WORD_CANARY = 0xA5A5A5A5A5A5A5A5
LANES = [4, 8, 16, 32, 64]
EDGES = ("0", "1", "15", "16", "17", "63", "64", "len-1", "len")
# PHOTON_FUZZ_ROUNDS=k multiplies the fuzz rounds (longer soak runs, new seeds).
SOAK = max(1, int(os.environ.get("PHOTON_FUZZ_ROUNDS", "1")))


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
    """src: [(pool offset | None (null base) | NEVER, length)] (None and NEVER
    with length 0 only), dst: [(arena offset | None, length)], skip / size:
    the value or None (0 / unlimited)."""

    def __init__(self, src, dst, skip=None, size=None, seed=0):
        self.src, self.dst, self.skip, self.size, self.seed = list(src), list(dst), skip, size, seed
        assert all(n == 0 for at, n in self.src if at is None or at is NEVER)
        assert all(n == 0 for at, n in self.dst if at is None)


def _window(m):
    """(L, D, a, k) of a message."""
    L = sum(n for _, n in m.src)
    D = sum(n for _, n in m.dst)
    a = min(0 if m.skip is None else m.skip, L)
    k = min(UNLIMITED if m.size is None else m.size, D, L - a)
    return L, D, a, k


def _inside(m):
    """The window is not empty and both of its edges lie strictly inside source segments."""
    L, D, a, k = _window(m)
    ends, run = {0}, 0
    for _, n in m.src:
        run += n
        ends.add(run)
    return k > 0 and a not in ends and a + k not in ends


def test_window_model():
    # the model itself, on cases worked out by hand (no GPU work)
    assert _window(Msg([(0, 100), (200, 200)], [(0, 1000)])) == (300, 1000, 0, 300)
    assert _window(Msg([(0, 100), (200, 200)], [(0, 1000)], 150, 50)) == (300, 1000, 150, 50)
    assert _window(Msg([(0, 100), (200, 200)], [(0, 30), (40, 10)], 150, 50)) == (300, 40, 150, 40)
    assert _window(Msg([(0, 100)], [(0, 1000)], 100, 5)) == (100, 1000, 100, 0)
    assert _window(Msg([(0, 100)], [(0, 1000)], UNLIMITED, UNLIMITED)) == (100, 1000, 100, 0)
    assert _window(Msg([(0, 100)], [(0, 1000)], 99, UNLIMITED - 10)) == (100, 1000, 99, 1)
    assert _window(Msg([(0, 100)], [], 10)) == (100, 0, 10, 0)
    assert _inside(Msg([(0, 100), (200, 200)], [(0, 1000)], 50, 100))
    assert not _inside(Msg([(0, 100), (200, 200)], [(0, 1000)], 100, 100))
    assert not _inside(Msg([(0, 100), (200, 200)], [(0, 1000)], 50, 50))
    assert not _inside(Msg([(0, 100), (200, 200)], [(0, 1000)], 50, 0))


def _descriptors(segs_of, base):
    rows, start = [], [0]
    for segs in segs_of:
        for at, n in segs:
            rows.append((0, 0) if at is None else (NEVER_ADDR, 0) if at is NEVER else (base + at, n))
        start.append(len(rows))
    return np.asarray(rows or [(0, 0)], np.uint64).reshape(-1, 2), np.asarray(start, np.uint64), len(rows)


def _expect(oracle, host, msgs, arena_size, crc64, seed0):
    """The arena, the window CRCs, the copied counts, per message the (CRC
    from seed 0, length) of every WHOLE source segment, and the CRC from seed
    0 of every message's whole source stream."""
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    want = np.full(arena_size, CANARY, np.uint8)
    crcs, copied, segs, whole = [], [], [], []
    for m in msgs:
        stream = b"".join(host[at:at + n].tobytes() for at, n in m.src if n)
        L, D, a, k = _window(m)
        assert L == len(stream)
        w = stream[a:a + k]
        pos = 0
        for at, n in m.dst:
            take = min(n, k - pos)
            if take > 0:
                want[at:at + take] = np.frombuffer(w[pos:pos + take], np.uint8)
                pos += take
        assert pos == k
        crcs.append(crc(w, m.seed if seed0 is None else seed0))
        copied.append(k)
        segs.append([(crc(host[at:at + n].tobytes(), 0) if n else 0, n) for at, n in m.src])
        assert all(c != _seg_canary(crc64) for c, _ in segs[-1])
        whole.append(crc(stream, 0))
    return want, crcs, copied, segs, whole


class Call:
    """The device tensors of one call and the call itself."""

    def __init__(self, torch, msgs, src_base, arena, crc64, seed0, with_copied):
        self.crc64, self.nmsg = crc64, len(msgs)
        siov, sstart, self.nsrc = _descriptors([m.src for m in msgs], src_base)
        diov, dstart, self.ndst = _descriptors([m.dst for m in msgs], arena.data_ptr())
        self.siov, self.sstart, self.diov, self.dstart = (_dev64(torch, x) for x in (siov, sstart, diov, dstart))
        self.skip = self.size = self.seeds = None
        if any(m.skip is not None for m in msgs):
            self.skip = _dev64(torch, [0 if m.skip is None else m.skip for m in msgs])
        if any(m.size is not None for m in msgs):
            self.size = _dev64(torch, [UNLIMITED if m.size is None else m.size for m in msgs])
        if seed0 is None:
            self.seeds = (_dev64 if crc64 else _dev32)(torch, [m.seed for m in msgs])
        self.seed0 = seed0 or 0
        self.out = torch.full((self.nmsg,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
        self.copied = torch.full((self.nmsg,), -1, dtype=torch.int64, device="cuda") if with_copied else None
        self.seg = (_dev64 if crc64 else _dev32)(torch, [_seg_canary(crc64)] * (self.nsrc + 2 * SEG_GUARD))
        self.seg_body = self.seg.data_ptr() + SEG_GUARD * (8 if crc64 else 4)
        assert ck.window_work_bytes(self.nmsg) == 16 * self.nmsg
        self.work = _dev64(torch, [WORD_CANARY] * (2 * self.nmsg + WORK_GUARD))
        assert self.work.data_ptr() % 8 == 0

    def __call__(self, stream=None):
        (ck.copy_msg64_iov_window_n if self.crc64 else ck.copy_msg_iov_window_n)(
            self.siov, self.sstart, self.nsrc, self.diov, self.dstart, self.ndst, self.nmsg, self.seg_body, self.out,
            self.work, skip=self.skip, size=self.size, seed=self.seed0, seeds=self.seeds, copied=self.copied,
            stream=stream)


def _compare(oracle, msgs, c, arena_bytes, want, crcs, ncopied, segs, whole, seed0, tag):
    crc64 = c.crc64
    got = c.out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    for k, m in enumerate(msgs):
        assert int(got[k]) == crcs[k], (tag, "window crc of message", k, m.src, m.dst, m.skip, m.size,
                                        hex(int(got[k])), hex(crcs[k]))
    if c.copied is not None:
        gc = c.copied.cpu().numpy().view(np.uint64)
        for k, m in enumerate(msgs):
            assert int(gc[k]) == ncopied[k], (tag, "copied of message", k, m.src, m.dst, m.skip, m.size, int(gc[k]))
    gs = c.seg.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    canary = _seg_canary(crc64)
    nsrc = sum(len(s) for s in segs)
    assert gs.size == nsrc + 2 * SEG_GUARD
    assert all(int(v) == canary for v in gs[:SEG_GUARD]), (tag, "front guard of d_src_seg_out", gs[:SEG_GUARD])
    assert all(int(v) == canary for v in gs[SEG_GUARD + nsrc:]), (tag, "back guard of d_src_seg_out")
    at = SEG_GUARD
    for k, m in enumerate(msgs):
        acc = 0
        for j, (cj, n) in enumerate(segs[k]):
            g = int(gs[at])
            assert g != canary, (tag, "segment entry not written", k, j, m.src, m.dst, m.skip, m.size)
            assert g == cj, (tag, "segment crc", k, j, n, m.src, m.dst, m.skip, m.size, hex(g), hex(cj))
            acc = _combine(oracle, crc64, acc, g, n)
            at += 1
        assert acc == whole[k], (tag, "fold of the segment crcs from seed 0 against the whole stream", k)
    gw = c.work.cpu().numpy().view(np.uint64)
    assert all(int(v) == WORD_CANARY for v in gw[2 * len(msgs):]), (tag, "written behind the work words")
    bad = np.flatnonzero(arena_bytes != want)
    if bad.size:
        b = int(bad[0])
        near = [(k, at, n) for k, m in enumerate(msgs) for at, n in m.dst if n and at <= b + 16 and b < at + n + 16]
        raise AssertionError(f"{tag}: arena byte {b} is {arena_bytes[b]:#x}, want {want[b]:#x}; {bad.size} bytes "
                             f"differ; destinations near it (message, at, n): {near[:4]}")


def _arena_size(msgs):
    return max([GUARD] + [at + n for m in msgs for at, n in m.dst if n]) + GUARD


def _run(torch, oracle, host, src_base, msgs, lanes, crc64=False, grid=0, seed0=None, with_copied=True):
    arena_size = _arena_size(msgs)
    _check_disjoint(msgs, arena_size)
    arena = torch.full((arena_size,), CANARY, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    exp = _expect(oracle, host, msgs, arena_size, crc64, seed0)
    c = Call(torch, msgs, src_base, arena, crc64, seed0, with_copied)
    ck.set_lanes_per_buffer(lanes)
    ck.set_batch_grid(grid)
    c()
    torch.cuda.synchronize()
    _compare(oracle, msgs, c, arena.cpu().numpy(), *exp, seed0, (lanes, crc64, grid))
    return c, arena


def _seed(rnd, crc64, k):
    return 0 if k % 5 == 0 else (1 << (64 if crc64 else 32)) - 1 if k % 5 == 1 else rnd.getrandbits(64 if crc64 else 32)


class Pool:
    """Hands out source ranges of the pool, in address order, `gap` bytes apart."""

    def __init__(self, start=5):
        self.pos = start

    def take(self, n, gap=13):
        at = self.pos
        self.pos += n + gap
        assert self.pos <= POOL
        return at


def _edge(name, n):
    return n - 1 if name == "len-1" else n if name == "len" else int(name)


# ------------------------------------------------------------- window edges
def _edge_msgs(g, crc64, which):
    """Three source segments [300, n, 300]. which == "start": the window starts
    at every EDGES offset of the middle segment and ends 77 bytes into the
    last; "end": it starts 33 bytes into the first and ends at every EDGES
    offset of the middle one. n: 200 (every piece below one step) and three
    steps of the group + 37. Destinations co-aligned and 5 bytes off in turn."""
    rnd = random.Random(0xED6E + g)
    pool, lay, msgs = Pool(), Layout(GUARD + 1), []
    for n in (200, 3 * 16 * g * ROWS[g] + 37):
        assert n <= 16384
        for name in EDGES:
            e = _edge(name, n)
            s0, s1, s2 = pool.take(300), pool.take(n, gap=3), pool.take(300)
            if which == "start":
                a, b = 300 + e, 300 + n + 77
            else:
                a, b = 33, 300 + e
            k = b - a
            first = (s0 + a) if a < 300 else (s1 + a - 300) if a < 300 + n else s2 + (a - 300 - n)
            delta = 0 if len(msgs) % 2 == 0 else 5
            cut = 1 + (len(msgs) * 37) % max(1, k - 1) if k > 1 else k
            d0 = lay.put(cut, like=first, delta=delta, gap=1)
            d1 = lay.put(k - cut + 9)  # back to back; 9 bytes of it stay 0xA5
            msgs.append(Msg([(s0, 300), (s1, n), (s2, 300)], [(d0, cut), (d1, k - cut + 9)], a, k,
                            _seed(rnd, crc64, len(msgs))))
            assert _window(msgs[-1]) == (600 + n, k + 9, a, k) and k > 0
    assert len(msgs) == 18
    return msgs


@pytest.mark.parametrize("which", ["start", "end"])
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("g", LANES)
def test_window_edges(dev_pool, oracle, g, crc64, which):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _edge_msgs(g, crc64, which), g, crc64)


# ------------------------------------------------ alignment and piece sizes
def _align_msgs(g, crc64):
    """One source segment; a window of odd length inside it, followed by the
    non-window remainder of the same segment; the destination cuts the window
    into three back-to-back segments at odd addresses; every (dst - src) % 16.
    Window lengths from 1 byte (the tiny path below 64) to three steps of the
    group."""
    rnd = random.Random(0xA116 + g)
    step = 16 * g * ROWS[g]
    pool, lay, msgs = Pool(3), Layout(GUARD + 1), []
    wins = (1, 15, 63, 65, 255, step - 1, step + 17, 3 * step - 1)
    for delta in range(16):
        for i, k in enumerate(wins):
            if delta and i % 2 == (delta % 2):  # every delta with half of the lengths, delta 0 with all
                continue
            a = (7, 16, 64, 129)[(delta + i) % 4]
            n = a + k + (1, 40, 300)[i % 3]
            s = pool.take(n, gap=(delta + i) % 5)
            c1 = k // 3 | 1 if k > 3 else k
            c2 = (k - c1) // 2 if k > c1 else 0
            lens = [c1, c2, k - c1 - c2]
            dst, like = [], s + a
            for j, ln in enumerate(lens):
                # co-aligned per window piece where delta == 0 (a fresh 16-byte phase per segment would not be
                # back to back): the first segment sets the phase, the others follow it
                dst.append((lay.put(ln, like=like if j == 0 else None, delta=delta, gap=(1 if j == 0 else 0)), ln))
            msgs.append(Msg([(s, n)], dst, a, k, _seed(rnd, crc64, len(msgs))))
            assert (dst[0][0] - (s + a)) % 16 == delta and _window(msgs[-1]) == (n, k, a, k)
            assert dst[1][0] == dst[0][0] + c1 and dst[2][0] == dst[1][0] + c2  # back to back
    assert len(msgs) == 8 + 15 * 4
    assert {(m.dst[0][0] - (m.src[0][0] + m.skip)) % 16 for m in msgs} == set(range(16))
    assert any(m.dst[1][0] % 2 for m in msgs) and all(m.size % 2 == 1 for m in msgs)
    return msgs


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("g", LANES)
def test_alignment_and_piece_sizes(dev_pool, oracle, g, crc64):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _align_msgs(g, crc64), g, crc64)


# ------------------------------------- where the window lies, and empty ones
def _shape_msgs(crc64):
    rnd = random.Random(0x5A9E)
    pool, lay = Pool(7), Layout(GUARD + 3)
    Z, ZN = (None, 0), (NEVER, 0)

    def src(*lens):
        return [(Z, ZN)[i % 2] if n == 0 else (pool.take(n), n) for i, n in enumerate(lens)]

    def dst(*lens):
        return [Z if n == 0 else (lay.put(n, gap=(1 if i else 5)), n) for i, n in enumerate(lens)]

    L3 = (100, 5000, 300)
    cases = [
        # inside one segment, across three, the whole stream (with and without the arrays' values)
        (src(*L3), dst(4000), 150, 3000),
        (src(*L3), dst(6000), 50, 5200),
        (src(*L3), dst(5400), 0, 5400),
        (src(*L3), dst(5400), None, None),
        (src(*L3), dst(2000, 3400, 77), None, None),
        # on segment boundaries: starts on one, ends on one, both
        (src(*L3), dst(6000), 100, 700),
        (src(*L3), dst(6000), 33, 5067),
        (src(*L3), dst(6000), 100, 5000),
        # empty: skip == L, > L, ~0; size 0; no destination segments; only empty ones; no source; neither
        (src(*L3), dst(500), 5400, None),
        (src(*L3), dst(500), 5401, 10),
        (src(*L3), dst(500), UNLIMITED, UNLIMITED),
        (src(*L3), dst(500), 150, 0),
        (src(*L3), dst(), 150, 100),
        (src(*L3), dst(0, 0, 0), 150, 100),
        (src(), dst(500), 0, 100),
        (src(0, 0), dst(500), 0, 100),
        (src(), dst(), None, None),
        # skip + size past 2^64: the window is [skip, L)
        (src(*L3), dst(6000), 150, UNLIMITED - 10),
        (src(*L3), dst(6000), 5399, UNLIMITED),
        # size 1; larger than what is left; D smaller than the window: the source behind it is still checksummed
        (src(*L3), dst(500), 5399, 1),
        (src(*L3), dst(6000), 5000, 1000),
        (src(*L3), dst(700), 50, 3000),
        (src(*L3, 4096, 100), dst(30, 40), 99, None),
        (src(3000, 3000, 3000), dst(3000), 0, None),          # the destination ends on a source boundary
        # zero-length segments first, last and adjacent, on both sides
        (src(0, 0, 50, 70), dst(0, 0, 100), 10, 100),
        (src(50, 70, 0, 0), dst(100, 0, 0), 10, 200),
        (src(50, 0, 0, 70), dst(40, 0, 0, 60), 10, 100),
        (src(0, 3000, 0, 0, 5000, 0), dst(0, 2500, 0, 0, 3500, 0), 1000, 6000),
        (src(50, 0, 0, 70), dst(200), 50, 70),                # the window starts behind a run of empty segments
    ]
    assert len(cases) == 29
    msgs = [Msg(s, d_, skip, size, _seed(rnd, crc64, k)) for k, (s, d_, skip, size) in enumerate(cases)]
    empties = [m for m in msgs if _window(m)[3] == 0]
    assert len(empties) == 9
    assert sum(1 for m in msgs if _inside(m)) >= 6
    assert any(at is NEVER for m in msgs for at, _ in m.src)
    return msgs


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("with_copied,seed0", [(True, None), (False, None), (True, 0xFEEDC0DE5EED0001)])
def test_window_shapes_and_empty_windows(dev_pool, oracle, crc64, lanes, with_copied, seed0):
    """An empty window leaves the arena untouched (the whole arena is
    compared), d_out the seed and d_copied 0, and the segment CRCs those of
    the whole blocks (every run's comparison)."""
    torch, host, d = dev_pool
    if seed0 is not None and not crc64:
        seed0 &= 0xFFFFFFFF
    msgs = _shape_msgs(crc64)
    c, _ = _run(torch, oracle, host, d.data_ptr(), msgs, lanes, crc64, seed0=seed0, with_copied=with_copied)
    got = c.out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    for k, m in enumerate(msgs):
        if _window(m)[3] == 0:
            assert int(got[k]) == (m.seed if seed0 is None else seed0)


# -------------------------------------------------------------------- rounds
def _round_msgs(g, crc64):
    """Three rounds of a one-workgroup grid and a message count that is no
    multiple of the groups per wavefront."""
    gpw = 64 // g
    per_round = 16 * gpw
    nmsg = 2 * per_round + gpw + 1
    rnd = random.Random(0x7E6 + g)
    lay, msgs = Layout(GUARD + 1), []
    lens_from = [0, 1, 15, 16, 17, 63, 64, 65, 100, 300, 1000]
    for k in range(nmsg):
        sl = [rnd.choice(lens_from) for _ in range(rnd.randrange(1, 5))]
        L = sum(sl)
        a = rnd.randrange(0, L + 1)
        size = rnd.randrange(0, L - a + 2)
        src = [(rnd.randrange(0, POOL - n), n) if n else (NEVER, 0) for n in sl]
        dl = [size // 2, size - size // 2 + rnd.choice((0, 3))] if k % 3 else [max(0, size - 5)]
        dst = [(lay.put(n, gap=rnd.choice((0, 0, 1, 5))), n) for n in dl]
        msgs.append(Msg(src, dst, a, size, _seed(rnd, crc64, k)))
    assert len(msgs) == {64: 34, 32: 67, 16: 133, 8: 265, 4: 529}[g]
    assert gpw == 1 or len(msgs) % gpw  # the last wavefront has idle groups
    return msgs


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("g", LANES)
def test_rounds_one_workgroup(dev_pool, oracle, g, crc64):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _round_msgs(g, crc64), g, crc64, grid=1)


# --------------------------------------------------- the purpose, composed
@pytest.mark.parametrize("crc64", [False, True])
def test_ranged_read_then_verify_names_the_bad_block(oracle, crc64):
    """Blocks of 4 KiB payload + a stored CRC word each; a range that starts and
    ends inside blocks; one payload bit flipped in a block that is listed but
    lies outside the window. verify_n over d_src_seg_out with the trailer
    stride reports exactly that block; the window's bytes and CRC are right."""
    import torch
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    word = 8 if crc64 else 4
    payload, nblk = 4096, 6
    stride = payload + word
    host = datagen.stream_bytes(0xB10C, stride * nblk).copy()
    for b in range(nblk):  # stamp the trailers
        c = crc(host[b * stride:b * stride + payload].tobytes(), 0)
        host[b * stride + payload:(b + 1) * stride] = np.frombuffer(c.to_bytes(word, "little"), np.uint8)
    bad_block = 4
    host[bad_block * stride + 1234] ^= 0x10  # behind the window
    region = torch.from_numpy(host).cuda()
    a, k = payload + 100, 2 * payload + 500  # blocks 1..3; blocks 0, 4 and 5 are listed and outside
    dst_at = GUARD + 3
    msg = Msg([(b * stride, payload) for b in range(nblk)], [(dst_at, k)], a, k, 0x5EED)
    arena_size = _arena_size([msg])
    arena = torch.full((arena_size,), CANARY, dtype=torch.uint8, device="cuda")
    c = Call(torch, [msg], region.data_ptr(), arena, crc64, None, True)
    c()
    count = nblk
    work = torch.empty(ck.verify_work_bytes(count), dtype=torch.uint8, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    bad_idx = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    (ck.verify64_device if crc64 else ck.verify_device)(c.seg_body, region.data_ptr() + payload, stride, count, report,
                                                        bad_idx, 4, work)
    torch.cuda.synchronize()
    rep = report.cpu().numpy().view(np.uint64)
    assert [int(x) for x in rep] == [1, bad_block, 1, count]
    assert int(bad_idx.cpu().numpy().view(np.uint64)[0]) == bad_block
    _compare(oracle, [msg], c, arena.cpu().numpy(), *_expect(oracle, host, [msg], arena_size, crc64, None), None,
             "verify")
    stream = b"".join(host[b * stride:b * stride + payload].tobytes() for b in range(nblk))
    assert int(c.out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)[0]) == crc(stream[a:a + k], 0x5EED)
    assert bytes(arena.cpu().numpy()[dst_at:dst_at + k]) == stream[a:a + k]


# ------------------------------------------------------------- graph capture
def _capture_msgs(variant, nbytes, count):
    lay, msgs = Layout(GUARD + 1), []
    for k in range(count):
        so = nbytes * k + (k + variant) % 16
        n0 = 600 + 100 * variant + k
        n1 = nbytes - n0 - 16
        a = 1 + (k * 97 + 311 * variant) % (nbytes - 400)
        size = None if k % 4 == variant else 1 + (k * 523 + 7 * variant) % 3000
        cut = 1 + (k * 131 + variant) % 900
        d0 = lay.put(cut, like=so + a, delta=0 if (k + variant) % 2 == 0 else 3)
        d1 = lay.put(nbytes, gap=k % 3)
        msgs.append(Msg([(so, n0), (so + n0, n1)], [(d0, cut), (d1, nbytes)], a, size, k + 1 + variant))
    return msgs


@pytest.mark.parametrize("crc64", [False, True])
def test_graph_capture(oracle, crc64):
    # one call per graph, replayed twice; the descriptors, d_skip and d_size are rewritten on the device in between
    import torch
    nbytes, count = 4096, 48
    d = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    sets = [_capture_msgs(v, nbytes, count) for v in (0, 1, 2)]
    arena_size = max(_arena_size(ms) for ms in sets)
    for ms in sets:
        _check_disjoint(ms, arena_size)
    arena = torch.full((arena_size,), CANARY, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC0B90)
    c = Call(torch, sets[0], d.data_ptr(), arena, crc64, None, True)
    assert c.skip is not None and c.size is not None
    canary = c.seg.clone()
    c()  # first-call set-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c(stream=torch.cuda.current_stream())
    for fill, msgs in ((0xC0B91, sets[1]), (0xC0B92, sets[2])):
        ck.fill_splitmix(d, nbytes, nbytes, count, fill)
        other = Call(torch, msgs, d.data_ptr(), arena, crc64, None, True)
        assert (other.nsrc, other.ndst) == (c.nsrc, c.ndst)
        for mine, new in ((c.siov, other.siov), (c.diov, other.diov), (c.skip, other.skip), (c.size, other.size),
                          (c.seeds, other.seeds)):
            mine.copy_(new)
        arena.fill_(CANARY)
        c.out.fill_(-1)
        c.copied.fill_(-1)
        c.seg.copy_(canary)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = d.cpu().numpy()
        _compare(oracle, msgs, c, arena.cpu().numpy(), *_expect(oracle, host, msgs, arena_size, crc64, None), None,
                 hex(fill))


# ---------------------------------------------------------------------- fuzz
FUZZ_MSGS = 50


def _fuzz_lengths(rnd, k):
    out = []
    for _ in range(k):
        r = rnd.random()
        out.append(0 if r < 0.1 else rnd.randrange(1, 80) if r < 0.3 else rnd.randrange(80, 5000) if r < 0.85
                   else rnd.randrange(5000, 40000))
    return out


def _fuzz_msgs(rnd, crc64, nmsg=FUZZ_MSGS):
    lay, msgs = Layout(GUARD + rnd.randrange(16)), []
    for k in range(nmsg):
        sl = _fuzz_lengths(rnd, rnd.randrange(0, 7))
        src = [(rnd.randrange(0, POOL - n), n) if n else rnd.choice(((None, 0), (NEVER, 0))) for n in sl]
        L = sum(sl)
        r = rnd.random()
        if r < 0.7 and L >= 3:
            a = rnd.randrange(1, L - 1)
            size = rnd.randrange(1, L - a)
            room = size + rnd.choice((0, 0, 9))
        elif r < 0.85:
            a = rnd.choice((None, 0, L, L + 1, rnd.randrange(0, L + 1)))
            size = rnd.choice((None, 0, L, UNLIMITED - 3, rnd.randrange(0, L + 2)))
            room = rnd.randrange(0, L + 50)
        else:  # the destination ends the window
            a = rnd.randrange(0, L + 1)
            size = None
            room = rnd.randrange(0, max(1, L - a))
        dl = []
        while room:
            n = min(room, rnd.choice((1, 7, 64, 200, 3000, 40000)))
            dl.append(n)
            room -= n
            if rnd.random() < 0.15:
                dl.append(0)
        first = next((at for at, n in src if n), None)
        dst = []
        for n in dl:
            if n == 0:
                dst.append((None, 0))
                continue
            like = rnd.choice([None, None, first])
            dst.append((lay.put(n, like=like, delta=0, gap=rnd.choice((0, 0, 1, 7, 16, 33))), n))
        msgs.append(Msg(src, dst, a, size, 0 if rnd.random() < 0.3 else rnd.getrandbits(64 if crc64 else 32)))
    assert len(msgs) == nmsg
    return msgs


def _fuzz_rounds(round_, crc64):
    """The six calls of a round: [(lanes, grid, with_copied, messages)], 300
    messages, at least half of them with a non-empty window that starts and
    ends strictly inside segments."""
    rnd = random.Random(9700 + round_ + (500 if crc64 else 0))
    calls = []
    for i, lanes in enumerate((0, 4, 8, 16, 32, 64)):
        calls.append((lanes, (0, 2)[(i + round_) % 2], rnd.random() < 0.8, _fuzz_msgs(rnd, crc64)))
    every = [m for _, _, _, ms in calls for m in ms]
    assert len(every) == 6 * FUZZ_MSGS == 300
    assert 2 * sum(1 for m in every if _inside(m)) >= len(every)
    return calls


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("round_", range(SOAK))
def test_fuzz(dev_pool, oracle, round_, crc64):
    torch, host, d = dev_pool
    ran = 0
    for lanes, grid, with_copied, msgs in _fuzz_rounds(round_, crc64):
        _run(torch, oracle, host, d.data_ptr(), msgs, lanes, crc64, grid=grid, with_copied=with_copied)
        ran += 1
    assert ran == 6

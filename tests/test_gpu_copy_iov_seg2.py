"""Copy + CRC between iovectors with one CRC per segment of BOTH sides from
one read (photon_crc32c_copy_msg_iov_seg2_n, photon_crc64ecma_copy_msg_iov_seg2_n).
Ground rules as tests/test_gpu_copy_iov_seg.py, whose message model, piece
walk and case generators are used here: every CRC comes from the pinned oracle
over the host copy of the source, the pieces from the Python walk; every
destination arena is pre-filled with 0xA5 and compared WHOLE; BOTH segment
arrays have 8 guard entries on each side, guards and body pre-filled with a
canary, the guards must survive and every body entry must differ from the
canary and equal the model. Every run also checks, per side, that the oracle's
combine fold of that side's entries with the LANDED lengths from seed_m equals
d_out[m]. No never-mapped addresses here: the segments behind the end of a
copy point into the pool."""
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests import test_gpu_copy_iov_seg as one
from tests.test_gpu_copy_iov_seg import (CANARY, DST, GUARD, G_CRC, NEVER, POOL, SEG_GUARD, SOAK, SRC, UNLIMITED, Layout,
                                         Msg, _check_disjoint, _combine, _dev32, _dev64, _seg_canary)
from tests.test_seg_unscan_cpp import STEP_COUNTS

pytestmark = pytest.mark.gpu

NEVER_AT = 4096  # where in the pool a segment behind the end of the copy points


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


def _descriptors(msgs, side, base):
    rows, start = [], [0]
    for m in msgs:
        for at, n in getattr(m, side):
            if at is None:
                assert n == 0
                rows.append((0, 0))
            elif at is NEVER:
                assert side == "src" and NEVER_AT + n <= POOL
                rows.append((base + NEVER_AT, n))
            else:
                rows.append((base + at, n))
        start.append(len(rows))
    return np.asarray(rows or [(0, 0)], np.uint64).reshape(-1, 2), np.asarray(start, np.uint64), len(rows)


def _expect(oracle, host, msgs, arena_size, crc64, seed0):
    """The arena, the message CRCs, the copied counts, and per side and message
    the (CRC from seed 0, landed length) of every segment."""
    want, crcs, copied, ssegs = one._expect(oracle, host, msgs, arena_size, crc64, seed0, SRC)
    want2, crcs2, copied2, dsegs = one._expect(oracle, host, msgs, arena_size, crc64, seed0, DST)
    assert np.array_equal(want, want2) and crcs == crcs2 and copied == copied2
    return want, crcs, copied, {SRC: ssegs, DST: dsegs}


class Run:
    """The device tensors of one call: inputs, both segment arrays with their guards, outputs."""

    def __init__(self, torch, msgs, src_base, arena, crc64, seed0, with_copied):
        siov, sstart, self.nsrc = _descriptors(msgs, "src", src_base)
        diov, dstart, self.ndst = _descriptors(msgs, "dst", arena.data_ptr())
        self.nmsg, self.crc64, self.seed0 = len(msgs), crc64, seed0
        self.size = None
        if any(m.size is not None for m in msgs):
            self.size = _dev64(torch, [UNLIMITED if m.size is None else m.size for m in msgs])
        self.seeds = None
        if seed0 is None:
            self.seeds = (_dev64 if crc64 else _dev32)(torch, [m.seed for m in msgs])
        self.out = torch.full((self.nmsg,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
        self.copied = torch.full((self.nmsg,), -1, dtype=torch.int64, device="cuda") if with_copied else None
        word = 8 if crc64 else 4
        self.seg = {side: (_dev64 if crc64 else _dev32)(torch, [_seg_canary(crc64)] * (n + 2 * SEG_GUARD))
                    for side, n in ((SRC, self.nsrc), (DST, self.ndst))}
        self.body = {side: t.data_ptr() + SEG_GUARD * word for side, t in self.seg.items()}
        self.siov, self.sstart, self.diov, self.dstart = (_dev64(torch, a) for a in (siov, sstart, diov, dstart))

    def call(self, stream=None):
        (ck.copy_msg64_iov_seg2_n if self.crc64 else ck.copy_msg_iov_seg2_n)(
            self.siov, self.sstart, self.nsrc, self.diov, self.dstart, self.ndst, self.nmsg, self.body[SRC],
            self.body[DST], self.out, size=self.size, seed=self.seed0 or 0, seeds=self.seeds, copied=self.copied,
            stream=stream)

    def seg_body(self, side):
        a = self.seg[side].cpu().numpy().view(np.uint64 if self.crc64 else np.uint32)
        return a[SEG_GUARD:a.size - SEG_GUARD]


def _compare(oracle, msgs, r, arena_bytes, want, crcs, ncopied, segs, tag):
    crc64, seed0 = r.crc64, r.seed0
    got = r.out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    for k, m in enumerate(msgs):
        assert int(got[k]) == crcs[k], (tag, "crc of message", k, m.src, m.dst, m.size, hex(int(got[k])), hex(crcs[k]))
    if r.copied is not None:
        gc = r.copied.cpu().numpy().view(np.uint64)
        for k, m in enumerate(msgs):
            assert int(gc[k]) == ncopied[k], (tag, "copied of message", k, m.src, m.dst, m.size)
    canary = _seg_canary(crc64)
    for side, name in ((SRC, "d_src_seg_out"), (DST, "d_dst_seg_out")):
        gs = r.seg[side].cpu().numpy().view(np.uint64 if crc64 else np.uint32)
        nside = sum(len(s) for s in segs[side])
        assert gs.size == nside + 2 * SEG_GUARD
        assert all(int(v) == canary for v in gs[:SEG_GUARD]), (tag, "front guard of " + name, gs[:SEG_GUARD])
        assert all(int(v) == canary for v in gs[SEG_GUARD + nside:]), (tag, "back guard of " + name)
        at = SEG_GUARD
        for k, m in enumerate(msgs):
            acc = m.seed if seed0 is None else seed0
            for j, (c, n) in enumerate(segs[side][k]):
                g = int(gs[at])
                assert g != canary, (tag, name, "entry not written", k, j, m.src, m.dst, m.size)
                assert g == c, (tag, name, "segment crc", k, j, n, m.src, m.dst, m.size, hex(g), hex(c))
                acc = _combine(oracle, crc64, acc, g, n)
                at += 1
            assert acc == int(got[k]), (tag, name, "fold of the segment crcs with the landed lengths", k, hex(acc),
                                        hex(int(got[k])))
    bad = np.flatnonzero(arena_bytes != want)
    if bad.size:
        b = int(bad[0])
        raise AssertionError(f"{tag}: arena byte {b} is {arena_bytes[b]:#x}, want {want[b]:#x}; {bad.size} bytes differ")


def _run(torch, oracle, host, src_base, msgs, lanes, crc64=False, grid=0, seed0=None, with_copied=True):
    arena_size = max([GUARD] + [at + n for m in msgs for at, n in m.dst if n]) + GUARD
    _check_disjoint(msgs, arena_size)
    arena = torch.full((arena_size,), CANARY, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    want, crcs, ncopied, segs = _expect(oracle, host, msgs, arena_size, crc64, seed0)
    r = Run(torch, msgs, src_base, arena, crc64, seed0, with_copied)
    ck.set_lanes_per_buffer(lanes)
    ck.set_batch_grid(grid)
    r.call()
    torch.cuda.synchronize()
    _compare(oracle, msgs, r, arena.cpu().numpy(), want, crcs, ncopied, segs, (lanes, crc64, grid))
    return r, arena


# ------------------------------------------------------------ boundary order
@pytest.mark.parametrize("crc64", [False, True])
def test_boundary_order_4_lanes(dev_pool, oracle, crc64):
    torch, host, d = dev_pool
    msgs = one._boundary_msgs(crc64)  # 121 messages, destinations packed at odd addresses
    assert len(msgs) == 121
    _run(torch, oracle, host, d.data_ptr(), msgs, 4, crc64)


# ------------------------------------------------------------ row boundaries
@pytest.mark.parametrize("delta", [0, 9])
@pytest.mark.parametrize("g,crc64", G_CRC)
def test_row_boundaries_scatter(dev_pool, oracle, g, crc64, delta):
    torch, host, d = dev_pool
    lens = one._row_lengths(g)
    msg = one._scatter_msg(lens, delta, 5)
    assert len(msg.dst) == len(lens) and len(msg.src) == 1
    _run(torch, oracle, host, d.data_ptr(), [msg], g, crc64)


@pytest.mark.parametrize("delta", [0, 9])
@pytest.mark.parametrize("g,crc64", G_CRC)
def test_row_boundaries_transposed(dev_pool, oracle, g, crc64, delta):
    torch, host, d = dev_pool
    lens = one._row_lengths(g)
    msg = one._transposed_msg(lens, delta, GUARD + 3)
    assert len(msg.src) == len(lens) and len(msg.dst) == 1
    _run(torch, oracle, host, d.data_ptr(), [msg], g, crc64)


# ------------------------------------------------- short sides and the cap
def _short_and_cap_msgs(crc64, nonzero_seeds):
    """The one-side file's cases (caps inside a segment, on a source boundary,
    on a destination boundary; a shorter source, a shorter destination; empty
    sides; size 0) and caps on a boundary of BOTH sides."""
    msgs = one._short_and_cap_msgs(crc64)
    rnd = random.Random(0xB07E)
    lay = Layout(max(at + n for m in msgs for at, n in m.dst) + 3)
    spos = 300000
    for size in (99, 100, 101, 299, 300, 301, None):
        src, dst = [], []
        for n in (100, 200, 50):
            src.append((spos, n))
            spos += n + 13
            dst.append((lay.put(n, gap=1), n))
        msgs.append(Msg(src, dst, size, rnd.getrandbits(64 if crc64 else 32)))
    assert len(msgs) == 37 + 7 and spos <= POOL
    if nonzero_seeds:  # the first segment's difference uses the seed
        for m in msgs:
            m.seed = m.seed or 0x9E3779B97F4A7C15 & ((1 << (64 if crc64 else 32)) - 1)
        assert all(m.seed for m in msgs)
    both = [m for m in msgs if m.size in (100, 300) and [n for _, n in m.src] == [n for _, n in m.dst]]
    assert len(both) == 2
    return msgs


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("lanes", [4, 32])
@pytest.mark.parametrize("with_copied,seed0", [(True, None), (False, None), (True, 0xFEEDC0DE5EED0001)])
def test_short_sides_and_cap(dev_pool, oracle, crc64, lanes, with_copied, seed0):
    torch, host, d = dev_pool
    if seed0 is not None and not crc64:
        seed0 &= 0xFFFFFFFF
    _run(torch, oracle, host, d.data_ptr(), _short_and_cap_msgs(crc64, seed0 is None), lanes, crc64, seed0=seed0,
         with_copied=with_copied)


# ------------------------------------------------- zero-length segment runs
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("lanes", [4, 16, 64])
def test_zero_length_runs(dev_pool, oracle, crc64, lanes):
    torch, host, d = dev_pool
    msgs = one._zero_run_msgs(crc64)  # leading, between, on both sides at one stream position, trailing
    assert len(msgs) == 20
    _run(torch, oracle, host, d.data_ptr(), msgs, lanes, crc64)


# -------------------------------------------------------------------- rounds
def _round_msgs(g, crc64):
    """Three rounds of a one-workgroup grid. The sides' segment counts go
    through 0, 1, 2, 63, 64, 65, 129 (the un-scan step's width and its
    neighbours) at different paces, so they differ within a message; every
    fourth message has a cap."""
    gpw = 64 // g
    per_round = 16 * gpw
    nmsg = 2 * per_round + gpw + 1
    rnd = random.Random(0x5E62 + g)
    lens_from = [0, 1, 2, 3, 15, 16, 17, 40]
    lay = Layout(GUARD + 1)
    msgs = []
    for k in range(nmsg):
        ns, nd = STEP_COUNTS[k % 7], STEP_COUNTS[(3 * k + 2) % 7]
        sl = [rnd.choice(lens_from) for _ in range(ns)]
        dl = [rnd.choice(lens_from) for _ in range(nd)]
        if k % 3 == 0 and ns and nd:  # everything lands: the last segment takes up the difference
            a, b = sum(sl), sum(dl)
            if a < b:
                sl[-1] += b - a
            else:
                dl[-1] += a - b
        total = min(sum(sl), sum(dl))
        src = [(rnd.randrange(0, POOL - n), n) for n in sl]
        dst = [(lay.put(n, gap=rnd.choice((0, 0, 1, 5))), n) for n in dl]
        msgs.append(Msg(src, dst, rnd.randrange(0, total + 2) if k % 4 == 3 else None,
                        one._seed(rnd, crc64, k)))
    assert len(msgs) == {64: 34, 32: 67, 16: 133, 8: 265, 4: 529}[g]
    pairs = {(len(m.src), len(m.dst)) for m in msgs}
    assert {a for a, _ in pairs} == set(STEP_COUNTS) == {b for _, b in pairs}
    assert sum(1 for a, b in pairs if a != b) >= 6
    return msgs


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("g", [4, 8, 16, 32, 64])
def test_rounds_one_workgroup(dev_pool, oracle, g, crc64):
    torch, host, d = dev_pool
    _run(torch, oracle, host, d.data_ptr(), _round_msgs(g, crc64), g, crc64, grid=1)


# -------------------------------------------------------------- equal blocks
@pytest.mark.parametrize("crc64", [False, True])
def test_equal_blocks(dev_pool, oracle, crc64):
    """8 x 8 KiB source segments in permuted slots into 16 x 4 KiB blocks, a
    CRC for each of the 24: one message per lane group of one full wave, 8 lanes."""
    torch, host, d = dev_pool
    lay = Layout()
    msgs = []
    for k in range(8):
        order = [(5 * i + k) % 8 for i in range(8)]
        src = [(65536 * k + 8192 * o, 8192) for o in order]
        dst = [(lay.put(4096, like=0, delta=0, gap=16 * (i % 2)), 4096) for i in range(16)]
        msgs.append(Msg(src, dst, None, k * 0x01010101))
    _run(torch, oracle, host, d.data_ptr(), msgs, 8, crc64)


# --------------------------------------------------------------- long pieces
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("lanes", [32, 64])
def test_long_pieces(dev_pool, oracle, lanes, reverse, crc64):
    torch, host, d = dev_pool
    n = (1 << 20) + 5
    so = 21
    lay = Layout()
    if reverse:  # [3, 1 MiB, 2] into one segment of 1 MiB + 5
        msg = Msg([(so, 3), (so + 3 + 16, 1 << 20), (7, 2)], [(lay.put(n, like=so, delta=9), n)], None, 0xA5A5A5A5)
    else:
        d0 = lay.put(3, like=so, delta=0)
        d1 = lay.put(1 << 20, like=so + 3, delta=0, gap=16)
        d2 = lay.put(2, gap=7)
        msg = Msg([(so, n)], [(d0, 3), (d1, 1 << 20), (d2, 2)], None, 0xA5A5A5A5)
    assert so + 3 + 16 + (1 << 20) <= POOL and so + n <= POOL
    _run(torch, oracle, host, d.data_ptr(), [msg], lanes, crc64)


# --------------------------------------------------------------- equivalence
@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("round_", range(3 * SOAK))
def test_fuzz_equals_the_one_side_calls(dev_pool, oracle, round_, crc64):
    """On fuzz messages: d_src_seg_out bit-equal to the src-side _seg_n call's
    d_seg_out, d_dst_seg_out to the dst-side call's, d_out / d_copied to
    copy_msg_iov_n's, on the same inputs."""
    torch, host, d = dev_pool
    rnd = random.Random(9700 + round_ + (500 if crc64 else 0))
    ran = 0
    for i, lanes in enumerate((0, 4, 8, 16, 32, 64)):
        msgs = one._fuzz_msgs(rnd, crc64, 40)
        grid = (0, 2)[(i + round_) % 2]
        r, arena = _run(torch, oracle, host, d.data_ptr(), msgs, lanes, crc64, grid=grid)
        arena_before = arena.cpu().numpy()
        for side in (SRC, DST):  # the arena sits at the same address: the same descriptors
            seg = torch.full(((r.ndst if side == DST else r.nsrc) + 1,), -1, dtype=r.out.dtype, device="cuda")
            out = torch.full_like(r.out, -1)
            copied = torch.full_like(r.copied, -1)
            (ck.copy_msg64_iov_seg_n if crc64 else ck.copy_msg_iov_seg_n)(
                r.siov, r.sstart, r.nsrc, r.diov, r.dstart, r.ndst, r.nmsg, side, seg, out, size=r.size,
                seeds=r.seeds, copied=copied)
            torch.cuda.synchronize()
            assert np.array_equal(seg.cpu().numpy()[:-1].view(np.uint64 if crc64 else np.uint32), r.seg_body(side))
            assert np.array_equal(out.cpu().numpy(), r.out.cpu().numpy())
            assert np.array_equal(copied.cpu().numpy(), r.copied.cpu().numpy())
        out = torch.full_like(r.out, -1)
        copied = torch.full_like(r.copied, -1)
        (ck.copy_msg64_iov_n if crc64 else ck.copy_msg_iov_n)(r.siov, r.sstart, r.nsrc, r.diov, r.dstart, r.ndst,
                                                              r.nmsg, out, size=r.size, seeds=r.seeds, copied=copied)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), r.out.cpu().numpy())
        assert np.array_equal(copied.cpu().numpy(), r.copied.cpu().numpy())
        assert np.array_equal(arena.cpu().numpy(), arena_before)
        ran += 1
    assert ran == 6


# ------------------------------------------------------------- graph capture
@pytest.mark.parametrize("crc64", [False, True])
def test_graph_capture(oracle, crc64):
    # both launches in one graph, replayed over a refilled source, a re-canaried arena and re-canaried seg arrays
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
    r = Run(torch, msgs, d.data_ptr(), arena, crc64, None, True)
    canary = {side: t.clone() for side, t in r.seg.items()}
    r.call()  # first-call set-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r.call(stream=torch.cuda.current_stream())
    for fill in (0xC0B91, 0xC0B92):
        ck.fill_splitmix(d, nbytes, nbytes, count, fill)
        arena.fill_(CANARY)
        r.out.fill_(-1)
        r.copied.fill_(-1)
        for side in (SRC, DST):
            r.seg[side].copy_(canary[side])
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = d.cpu().numpy()
        want, crcs, ncopied, segs = _expect(oracle, host, msgs, arena_size, crc64, None)
        _compare(oracle, msgs, r, arena.cpu().numpy(), want, crcs, ncopied, segs, hex(fill))

"""Copy + CRC-64/ECMA in one pass (photon_crc64ecma_copy_batch_strided / _iov,
photon_crc64ecma_gather_msg_n), by the method of tests/test_gpu_copy_crc.py:
every CRC bit-exact against the pinned oracle (tests/_oracle.py crc64ecma) over
the HOST copy of the source with per-unit 64-bit seeds, and every destination
arena pre-filled with 0xA5 and compared WHOLE against a numpy image built from
host slices -- guards, gaps and neighbours included -- so a store that strays
by one byte, or a block that is never stored, fails. The case generators are
plain numpy / random code and assert that the destination ranges are disjoint
from one another and from the guards.

The CRC-64 generic kernel takes 2 rows per step at every lane-group size, its
head touches lanes 0 and 1 (source offsets 9..15 put the init into block 1),
and its tiny buffers (< 64 B) and tails run on the group's first lane."""
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_gpu_copy_crc import CANARY, GUARD, _arena, _i64

pytestmark = pytest.mark.gpu

POOL = 1 << 20
GS = [4, 8, 16, 32, 64]
U = 2          # rows per step of the CRC-64 generic kernel (PCRC64_U)
K_WAVES = 16   # wavefronts of a workgroup: one pass of a 1-workgroup grid
ONES = (1 << 64) - 1


@pytest.fixture(scope="module")
def dev_pool():
    import torch
    assert torch.cuda.is_available()
    host = datagen.stream_bytes(0xC641, POOL)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return torch, host, d


@pytest.fixture(autouse=True)
def _reset():
    yield
    ck.set_lanes_per_buffer(0)
    ck.set_batch_grid(0)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _out64(torch, n, fill=0):
    return torch.full((n,), fill, dtype=torch.int64, device="cuda")


def _seeds(rnd, n):
    """0, all-ones and random, in turn."""
    return [(0, ONES, rnd.getrandbits(64))[k % 3] for k in range(n)]


def three_rounds(g):
    """Units that give a 1-workgroup grid three rounds: two full passes, then
    two wavefronts, the last with one active group."""
    gpw = 64 // g
    return 2 * K_WAVES * gpw + gpw + 1


# ------------------------------------------------------------ host-side cases

def _assert_disjoint(ranges, size):
    end = GUARD
    for at, n in sorted(ranges):
        assert at >= end, (at, n, end)
        end = at + n
    assert end <= size - GUARD, (end, size)


def _first_diff(got, want, what):
    bad = np.flatnonzero(got != want)
    if bad.size:
        b = int(bad[0])
        raise AssertionError(f"{what}: arena byte {b} is {got[b]:#x}, want {want[b]:#x}; {bad.size} bytes differ")


def _place(cases):
    """cases: (source offset, length, (dst - src) mod 16). Destinations packed
    with only the 0..15 bytes of padding that the wanted alignment needs."""
    pos, places = GUARD, []
    for so, n, delta in cases:
        pos += ((so + delta) - pos) % 16
        places.append(pos)
        pos += n
    size = pos + GUARD
    _assert_disjoint([(at, c[1]) for at, c in zip(places, cases)], size)
    return places, size


def _iov_image(host, cases, places, size):
    want = np.full(size, CANARY, np.uint8)
    for (so, n, _), at in zip(cases, places):
        want[at:at + n] = host[so:so + n]
    return want


def _run_iov(torch, oracle, host, src, cases, lanes, what=""):
    places, size = _place(cases)
    want = _iov_image(host, cases, places, size)
    arena = _arena(torch, size)
    seeds = _seeds(random.Random(len(cases) * 131 + lanes), len(cases))
    iov = np.zeros((len(cases), 2), np.uint64)
    iov[:, 0] = np.uint64(src.data_ptr()) + np.asarray([c[0] for c in cases], np.uint64)
    iov[:, 1] = np.asarray([c[1] for c in cases], np.uint64)
    d_iov = _i64(torch, iov)
    out = _out64(torch, len(cases))
    ck.set_lanes_per_buffer(lanes)
    ck.copy_batch64_iov(d_iov, _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(places, np.uint64)),
                        len(cases), out, seeds=_i64(torch, seeds))
    torch.cuda.synchronize()
    got = _u64(out)
    for k, ((so, n, delta), s) in enumerate(zip(cases, seeds)):
        ref = oracle.crc64ecma(host[so:so + n], s)
        assert int(got[k]) == ref, f"{what} lanes {lanes}: crc of case {k} {(so, n, delta)} seed {s:#x} is " \
                              f"{int(got[k]):#x}, want {ref:#x}"
    _first_diff(arena.cpu().numpy(), want, f"{what} lanes {lanes}")
    return d_iov, seeds, got


def _row_cases(g, deltas):
    cases = []
    for k in range(2 * U + 4):
        for dd in (-17, -16, -1, 0, 1, 15, 16, 17):
            n = k * 16 * g + dd
            if n < 0:
                continue
            for j, so in enumerate((0, 7, 13)):
                # sources spread over the pool (they may overlap: read only)
                cases.append((4096 * (len(cases) % 61) + 16 * j + so, n, deltas[len(cases) % len(deltas)]))
    return cases


# ---------------------------------------------------------------- buffers

def test_length_sweep_4_lanes(dev_pool, oracle):
    # tiny buffers, heads (the init in block 0, across blocks 0 and 1, in block
    # 1), tails, the lead row, the first step and the loop entry (a row is 64 B)
    torch, host, d = dev_pool
    cases = [(1024 * (n % 97) + 16 * (n % 5) + so, n, 0) for n in range(401) for so in (0, 1, 7, 8, 9, 15)]
    _run_iov(torch, oracle, host, d, cases, 4)


@pytest.mark.parametrize("g", GS)
def test_row_boundaries(dev_pool, oracle, g):
    torch, host, d = dev_pool
    _run_iov(torch, oracle, host, d, _row_cases(g, (0,)), g)


@pytest.mark.parametrize("g", GS)
def test_not_co_aligned(dev_pool, oracle, g):
    torch, host, d = dev_pool
    _run_iov(torch, oracle, host, d, _row_cases(g, (1, 4, 8, 13)), g)


@pytest.mark.parametrize("nbytes,src_stride,dst_stride", [
    (4096, 4096, 4096), (4096, 4112, 4099), (65536, 65536, 65536 + 16), (1000, 1003, 1000)])
def test_strided(oracle, nbytes, src_stride, dst_stride):
    # the first and third shapes take the init at the end (shift_init); the
    # first is where the read-only call picks the full-row kernel
    import torch
    count = 257  # the last wavefront is partly inactive
    host = datagen.stream_bytes(0xC642 + nbytes, (count - 1) * src_stride + nbytes)
    d = torch.from_numpy(host.copy()).cuda()
    dst_len = (count - 1) * dst_stride + nbytes
    size = GUARD + dst_len + GUARD
    _assert_disjoint([(GUARD + i * dst_stride, nbytes) for i in range(count)], size)
    want = np.full(size, CANARY, np.uint8)
    for i in range(count):
        want[GUARD + i * dst_stride:GUARD + i * dst_stride + nbytes] = host[i * src_stride:i * src_stride + nbytes]
    seeds = _seeds(random.Random(nbytes), count)
    seed0 = 0xFEDCBA9876543210
    refs = {True: np.asarray([oracle.crc64ecma(host[i * src_stride:i * src_stride + nbytes], seeds[i])
                              for i in range(count)], np.uint64),
            False: oracle.crc64ecma_strided(host, src_stride, nbytes, count, seed0)}
    for use_seeds in (True, False):
        d_seeds = _i64(torch, seeds) if use_seeds else None
        arena = _arena(torch, size)
        out = _out64(torch, count)
        ck.copy_batch64_strided(d, src_stride, arena.data_ptr() + GUARD, dst_stride, nbytes, count, out,
                                seed=seed0, seeds=d_seeds)
        plain = _out64(torch, count)
        ck.batch64_strided(d, src_stride, nbytes, count, plain, seed=seed0, seeds=d_seeds)
        torch.cuda.synchronize()
        got = _u64(out)
        for i in np.flatnonzero(got != refs[use_seeds])[:1]:
            raise AssertionError(f"seeds {use_seeds}: crc of buffer {i} is {int(got[i]):#x}, "
                                 f"want {int(refs[use_seeds][i]):#x}")
        assert np.array_equal(got, _u64(plain)), use_seeds
        _first_diff(arena.cpu().numpy(), want, f"seeds {use_seeds}")
    assert np.array_equal(d.cpu().numpy(), host)  # the source is only read


# ------------------------------------------ three rounds of the persistent loop

def round_cases(g):
    """Three rounds of buffers: the lengths' cycle moves on by one per round
    and the alignments' by one per eight buffers, so a wavefront position
    meets other lengths in each round and every length of 64 bytes or more
    meets both a co-aligned and a not-co-aligned destination."""
    gpw = 64 // g
    lens = [0, 1, 63, 64, 16 * g - 1, 16 * g * U + 17, 16 * g * (2 * U + 1) + 5, 16 * g * (3 * U + 2)]
    cases = []
    for k in range(three_rounds(g)):
        li = (k + k // (K_WAVES * gpw)) % 8
        so = 4096 * (k % 61) + 16 * (k % 5) + (0, 5, 15)[k % 3]
        cases.append((so, lens[li], (0, 0, 0, 7)[(li + k // 8) % 4]))
    return cases


@pytest.mark.parametrize("g", GS)
def test_buffer_rounds(dev_pool, oracle, g):
    torch, host, d = dev_pool
    ck.set_batch_grid(1)
    _run_iov(torch, oracle, host, d, round_cases(g), g, "one workgroup,")


@pytest.mark.parametrize("form", ["co_aligned", "not_co_aligned"])
@pytest.mark.parametrize("g", GS)
def test_strided_rounds(dev_pool, oracle, g, form):
    # an aligned source and no seed array: the init enters at the end (shift_init)
    torch, host, d = dev_pool
    nbytes, count = 16 * g * (2 * U + 1), three_rounds(g)
    src_stride = nbytes + 16
    dst_stride = nbytes + 3 if form == "not_co_aligned" else src_stride
    size = GUARD + (count - 1) * dst_stride + nbytes + GUARD
    _assert_disjoint([(GUARD + i * dst_stride, nbytes) for i in range(count)], size)
    want = np.full(size, CANARY, np.uint8)
    for i in range(count):
        want[GUARD + i * dst_stride:GUARD + i * dst_stride + nbytes] = host[i * src_stride:i * src_stride + nbytes]
    arena = _arena(torch, size)
    out = _out64(torch, count)
    ck.set_lanes_per_buffer(g)
    ck.set_batch_grid(1)
    ck.copy_batch64_strided(d, src_stride, arena.data_ptr() + GUARD, dst_stride, nbytes, count, out, seed=ONES)
    torch.cuda.synchronize()
    ref = oracle.crc64ecma_strided(host, src_stride, nbytes, count, ONES)
    got = _u64(out)
    for i in np.flatnonzero(got != ref)[:1]:
        raise AssertionError(f"lanes {g}, {form}: crc of buffer {i} is {int(got[i]):#x}, want {int(ref[i]):#x}")
    _first_diff(arena.cpu().numpy(), want, f"lanes {g}, {form}, buffers of {nbytes} B every {dst_stride}")


# ------------------------------------------------------------------- gather

def gather_layout(rnd, pool, msgs):
    """msgs: per message the list of its segments' lengths. Sources at random
    pool offsets, destinations packed back to back with no padding."""
    iov, start, dst_off = [], [0], []
    pos = GUARD
    for segs in msgs:
        dst_off.append(pos)
        for n in segs:
            iov.append((rnd.randrange(0, pool - n), n))
            pos += n
        start.append(len(iov))
    size = pos + GUARD
    _assert_disjoint([(at, sum(segs)) for at, segs in zip(dst_off, msgs)], size)
    return {"msgs": msgs, "iov": np.asarray(iov, np.uint64).reshape(-1, 2), "start": np.asarray(start, np.uint64),
            "dst_off": dst_off, "size": size}


def gather_expect(oracle, host, lay, seeds):
    """From the host copy: the arena's image, crc64ecma(seg, 0) per segment and
    crc64ecma chained over each message's segments from its seed."""
    want = np.full(lay["size"], CANARY, np.uint8)
    at = GUARD
    seg_crc = np.zeros(lay["iov"].shape[0], np.uint64)
    for k, (o, n) in enumerate(lay["iov"].tolist()):
        want[at:at + n] = host[o:o + n]
        at += n
        seg_crc[k] = oracle.crc64ecma(host[o:o + n], 0)
    chained = np.zeros(len(lay["msgs"]), np.uint64)
    for m in range(len(lay["msgs"])):
        c = seeds[m]
        for o, n in lay["iov"][int(lay["start"][m]):int(lay["start"][m + 1])].tolist():
            c = oracle.crc64ecma(host[o:o + n], c)
        chained[m] = c
    return want, seg_crc, chained


def _run_gather(torch, lay, expect, src_ptr, with_seg, seeds, what, against_plain=True):
    want, seg_crc, chained = expect
    nmsg, nseg = len(lay["msgs"]), lay["iov"].shape[0]
    arena = _arena(torch, lay["size"])
    dev_iov = lay["iov"].copy()
    dev_iov[:, 0] += np.uint64(src_ptr)
    d_iov = _i64(torch, dev_iov) if nseg else None
    d_start, d_seeds = _i64(torch, lay["start"]), _i64(torch, seeds)
    out = _out64(torch, nmsg)
    seg = _out64(torch, nseg + 2, -1) if with_seg else None
    ck.gather64_msg_n(d_iov, d_start, nmsg, nseg,
                      _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(lay["dst_off"], np.uint64)), seg, out,
                      seeds=d_seeds)
    torch.cuda.synchronize()
    got = _u64(out)
    for m in np.flatnonzero(got != chained)[:1]:
        raise AssertionError(f"{what}: message {m} {lay['msgs'][m]} is {int(got[m]):#x}, want {int(chained[m]):#x}")
    if with_seg:
        gseg = _u64(seg)
        for k in np.flatnonzero(gseg[:nseg] != seg_crc)[:1]:
            m = int(np.searchsorted(lay["start"], k, side="right")) - 1
            raise AssertionError(f"{what}: segment {k} (number {k - int(lay['start'][m])} of message {m}, "
                                 f"{len(lay['msgs'][m])} segments) is {int(gseg[k]):#x}, want {int(seg_crc[k]):#x}")
        assert (gseg[nseg:] == np.uint64(ONES)).all(), what  # nothing stored past the last segment's CRC
    _first_diff(arena.cpu().numpy(), want, what)
    if against_plain and nseg:
        pout = _out64(torch, nmsg)
        pseg = _out64(torch, nseg, -1) if with_seg else None
        ck.batch64_msg_n(d_iov, d_start, nmsg, nseg, pseg, pout, seeds=d_seeds)
        torch.cuda.synchronize()
        assert np.array_equal(_u64(pout), got), what
        if with_seg:
            assert np.array_equal(_u64(pseg), _u64(seg)[:nseg]), what


def round_msgs(g):
    """Three rounds of messages of 0, 1, 2, G-1, G, G+1 and 2G+1 segments; the
    lengths run from 0 through tiny (< 64), one row and several steps."""
    rnd = random.Random(0x6A64 + g)
    counts = [0, 1, 2, g - 1, g, g + 1, 2 * g + 1]
    lens = [0, 1, 15, 16, 17, 63, 64, 100, 16 * g, 16 * g * (U + 1) + 9, 16 * g * (3 * U + 1) + 16, 4097]
    msgs = [[rnd.choice(lens) for _ in range(counts[(m + 1) % 7])] for m in range(three_rounds(g))]
    assert {len(s) for s in msgs} >= set(counts)
    return msgs


def _segment_places(lay):
    at, out = GUARD, []
    for n in lay["iov"][:, 1].tolist():
        out.append(at)
        at += n
    return out


@pytest.fixture(scope="module")
def round_gathers(dev_pool, oracle):
    torch, host, d = dev_pool
    made = {}

    def get(g):
        if g not in made:
            rnd = random.Random(0x6A65 + g)
            lay = gather_layout(rnd, POOL, round_msgs(g))
            seeds = _seeds(rnd, len(lay["msgs"]))
            made[g] = lay, seeds, gather_expect(oracle, host, lay, seeds)
        return made[g]
    return get


@pytest.mark.parametrize("with_seg", [False, True])
@pytest.mark.parametrize("g", GS)
def test_gather_rounds(dev_pool, round_gathers, g, with_seg):
    """Chained (the register broadcast from the first lane into the next
    segment's head) and with segment CRCs (+ the fold kernel); messages packed
    back to back in one arena; three rounds on one workgroup, then the full
    grid; both against the read-only call on the same descriptors."""
    torch, host, d = dev_pool
    lay, seeds, expect = round_gathers(g)
    co = [(at - o) % 16 == 0 for (o, n), at in zip(lay["iov"].tolist(), _segment_places(lay)) if n >= 64]
    assert any(co) and not all(co)  # the decision is per segment
    ck.set_lanes_per_buffer(g)
    for cap in (1, 0):
        ck.set_batch_grid(cap)
        _run_gather(torch, lay, expect, d.data_ptr(), with_seg, seeds,
                    f"lanes {g}, segment CRCs {with_seg}, grid cap {cap}", against_plain=cap == 1)


@pytest.mark.parametrize("with_seg", [False, True])
def test_gather_co_aligned_parts(dev_pool, oracle, with_seg):
    # an object's parts: every segment co-aligned with its place (one read),
    # default lanes; the object CRC and the parts' CRCs
    torch, host, d = dev_pool
    rnd = random.Random(0x6A66)
    msgs = [[16 * rnd.randrange(4, 600) for _ in range(rnd.randrange(1, 7))] + [rnd.randrange(0, 5000)]
            for _ in range(40)]
    lay = gather_layout(rnd, POOL, msgs)
    for k, (at, n) in enumerate(zip(_segment_places(lay), lay["iov"][:, 1].tolist())):
        o = 16 * rnd.randrange(0, (POOL - n) // 16 - 1) + at % 16  # the destination's alignment
        assert (at - o) % 16 == 0 and o + n <= POOL
        lay["iov"][k, 0] = o
    seeds = _seeds(rnd, len(msgs))
    _run_gather(torch, lay, gather_expect(oracle, host, lay, seeds), d.data_ptr(), with_seg, seeds,
                f"co-aligned parts, segment CRCs {with_seg}")


@pytest.mark.parametrize("with_seg", [False, True])
def test_gather_only_empty_messages(with_seg):
    import torch
    arena = _arena(torch, 256)
    nmsg = 7
    seeds = [0, 1, 2, ONES, 0xDEADBEEFCAFEF00D, 5, 6]
    d_dst = _i64(torch, np.full(nmsg, arena.data_ptr() + GUARD, np.uint64))
    d_start = _i64(torch, np.zeros(nmsg + 1, np.uint64))
    seg = _out64(torch, 4, -1) if with_seg else None
    for use_seeds in (True, False):
        out = _out64(torch, nmsg)
        ck.gather64_msg_n(None, d_start, nmsg, 0, d_dst, seg, out, seed=0xABCD0123456789EF,
                          seeds=_i64(torch, seeds) if use_seeds else None)
        torch.cuda.synchronize()
        assert _u64(out).tolist() == (seeds if use_seeds else [0xABCD0123456789EF] * nmsg)
    if with_seg:
        assert (_u64(seg) == np.uint64(ONES)).all()
    assert bool((arena.cpu().numpy() == CANARY).all())


def test_zero_length_buffers():
    # a zero-length buffer writes nothing and returns the seed
    import torch
    arena = _arena(torch, 256)
    seeds = [0, 1, ONES, 0x123456789ABCDEF0, 7]
    for use_seeds in (False, True):
        out = _out64(torch, 5)
        ck.copy_batch64_strided(None, 64, None, 64, 0, 5, out, seed=0xC0FFEE0000C0FFEE,
                                seeds=_i64(torch, seeds) if use_seeds else None)
        torch.cuda.synchronize()
        assert _u64(out).tolist() == (seeds if use_seeds else [0xC0FFEE0000C0FFEE] * 5)
    iov = np.zeros((5, 2), np.uint64)
    out = _out64(torch, 5)
    ck.copy_batch64_iov(_i64(torch, iov), _i64(torch, np.full(5, arena.data_ptr() + GUARD, np.uint64)), 5, out,
                        seeds=_i64(torch, seeds))
    torch.cuda.synchronize()
    assert _u64(out).tolist() == seeds
    assert bool((arena.cpu().numpy() == CANARY).all())


# ------------------------------------------------- other memory, long, capture

@pytest.fixture(scope="module")
def pinned_pool():
    import torch
    host = datagen.stream_bytes(0xC647, POOL)
    src = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    src.numpy()[:] = host
    assert src.data_ptr() % 16 == 0
    return torch, host, src


def test_iov_from_pinned_host(pinned_pool, oracle):
    # the kernel reads pinned host memory in place, at every alignment
    torch, host, src = pinned_pool
    lens = [1, 63, 64, 4097, 70001]
    cases = [(80000 * k + (0, 3, 15)[k % 3], lens[k % 5], (0, 11)[k // 5 % 2]) for k in range(12)]
    assert {(n, delta) for _, n, delta in cases} >= {(n, dl) for n in lens[2:] for dl in (0, 11)}
    _run_iov(torch, oracle, host, src, cases, 0, "pinned source,")
    assert np.array_equal(src.numpy(), host)


@pytest.mark.parametrize("with_seg", [False, True])
def test_gather_from_pinned_host(pinned_pool, oracle, with_seg):
    torch, host, src = pinned_pool
    rnd = random.Random(0xC648)
    msgs = [[rnd.choice([0, 1, 63, 64, 100, 4097, 20000]) for _ in range(rnd.randrange(0, 6))] for _ in range(16)]
    lay = gather_layout(rnd, host.size, msgs)
    seeds = _seeds(rnd, len(msgs))
    _run_gather(torch, lay, gather_expect(oracle, host, lay, seeds), src.data_ptr(), with_seg, seeds,
                f"pinned source, segment CRCs {with_seg}")
    assert np.array_equal(src.numpy(), host)


def test_source_untouched_and_plain_calls_unchanged(dev_pool, oracle):
    torch, host, d = dev_pool
    cases = [(3000 * k + (k % 16), n, k % 2 * 5) for k, n in enumerate([0, 1, 63, 64, 65, 1000, 4096, 4097, 70000])]
    d_iov, seeds, got = _run_iov(torch, oracle, host, d, cases, 0)
    assert np.array_equal(d.cpu().numpy(), host)
    out = _out64(torch, len(cases))
    ck.batch64_iov(d_iov, len(cases), out, seeds=_i64(torch, seeds))
    torch.cuda.synchronize()
    assert np.array_equal(_u64(out), got)


@pytest.mark.parametrize("g", [32, 64])
def test_long_buffer(oracle, g):
    # thousands of rows per lane: the rolling-reload loop with its stores, and
    # the separate copy of a long buffer that is not co-aligned
    import torch
    n = (1 << 20) + 5
    host = datagen.stream_bytes(0xC649, n + 16)
    d = torch.from_numpy(host.copy()).cuda()
    _run_iov(torch, oracle, host, d, [(3, n, 0), (3, n, 9)], g, "long buffer,")


def _splitmix_source(torch, nbytes, count):
    d = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 16 == 0
    return d


def test_graph_capture_iov(oracle):
    # one branch: a single copy_batch64_iov captured on the capture stream
    import torch
    nbytes, count = 4096, 40
    d = _splitmix_source(torch, nbytes, count)
    lens = [0, 1, 63, 64, 1000, 4097, 9000]
    cases = [(nbytes * k // 2 + (0, 5, 15)[k % 3], lens[k % 7], (0, 6)[k // 7 % 2]) for k in range(count)]
    places, size = _place(cases)
    seeds = _seeds(random.Random(0xC64A), count)
    iov = np.zeros((count, 2), np.uint64)
    iov[:, 0] = np.uint64(d.data_ptr()) + np.asarray([c[0] for c in cases], np.uint64)
    iov[:, 1] = np.asarray([c[1] for c in cases], np.uint64)
    d_iov, d_seeds = _i64(torch, iov), _i64(torch, seeds)
    arena = _arena(torch, size)
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(places, np.uint64))
    out = _out64(torch, count)
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC64B0)
    ck.copy_batch64_iov(d_iov, d_dst, count, out, seeds=d_seeds)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ck.copy_batch64_iov(d_iov, d_dst, count, out, seeds=d_seeds, stream=torch.cuda.current_stream())
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC64B1)  # replayed once over a refilled source
    arena.fill_(CANARY)
    out.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    host = d.cpu().numpy()
    got = _u64(out)
    for k, ((so, n, _), s) in enumerate(zip(cases, seeds)):
        assert int(got[k]) == oracle.crc64ecma(host[so:so + n], s), k
    _first_diff(arena.cpu().numpy(), _iov_image(host, cases, places, size), "replay")


def test_graph_capture_gather(oracle):
    # one branch: a single gather64_msg_n with segment CRCs (the gather kernel, then the fold)
    import torch
    nbytes, count = 4096, 40
    d = _splitmix_source(torch, nbytes, count)
    rnd = random.Random(0xC64C)
    msgs = [[rnd.choice([0, 1, 16, 63, 64, 100, 4097, 6000]) for _ in range(rnd.choice([0, 1, 2, 3, 9, 17]))]
            for _ in range(48)]
    lay = gather_layout(rnd, nbytes * count, msgs)
    nmsg, nseg = len(msgs), lay["iov"].shape[0]
    seeds = _seeds(rnd, nmsg)
    dev_iov = lay["iov"].copy()
    dev_iov[:, 0] += np.uint64(d.data_ptr())
    d_iov, d_start, d_seeds = _i64(torch, dev_iov), _i64(torch, lay["start"]), _i64(torch, seeds)
    arena = _arena(torch, lay["size"])
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(lay["dst_off"], np.uint64))
    out = _out64(torch, nmsg)
    seg = _out64(torch, nseg, -1)
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC64D0)
    ck.gather64_msg_n(d_iov, d_start, nmsg, nseg, d_dst, seg, out, seeds=d_seeds)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ck.gather64_msg_n(d_iov, d_start, nmsg, nseg, d_dst, seg, out, seeds=d_seeds,
                          stream=torch.cuda.current_stream())
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC64D1)  # replayed once over a refilled source
    arena.fill_(CANARY)
    out.zero_()
    seg.fill_(-1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    host = d.cpu().numpy()
    want, seg_crc, chained = gather_expect(oracle, host, lay, seeds)
    assert np.array_equal(_u64(out), chained)
    assert np.array_equal(_u64(seg), seg_crc)
    _first_diff(arena.cpu().numpy(), want, "replay")

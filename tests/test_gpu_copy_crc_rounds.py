"""Copy + CRC-32C where tests/test_gpu_copy_crc.py does not reach: several
rounds of every copying kernel's persistent loop (the grid capped at one
workgroup), every lane-group size of the buffer and of both message builds,
long rows, pinned host memory on either side, the contract's edges, graph
capture of the iovec and gather calls, and randomised cases.

The rule of that file holds here: every CRC is bit-exact against the pinned
oracle (tests/_oracle.py) over the HOST copy of the source, and every
destination arena is pre-filled with 0xA5 and compared WHOLE against a numpy
image built from host slices -- guards, gaps and neighbours included. The case
generators are plain numpy / random code (no device), and each asserts that
its destination ranges are disjoint from one another and from the guards."""
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_gpu_copy_crc import CANARY, GUARD, ROWS, _arena, _i32, _i64, _run_iov, _u32
from tests.test_gpu_fuzz import SOAK, _lengths

pytestmark = pytest.mark.gpu

POOL = 4 << 20
GS = [4, 8, 16, 32, 64]
K_WAVES = 16  # wavefronts of a workgroup (kWaves): one pass of a 1-workgroup grid


@pytest.fixture(scope="module")
def dev_pool():
    import torch
    assert torch.cuda.is_available()
    host = datagen.stream_bytes(0xC0C1, POOL)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return torch, host, d


@pytest.fixture(autouse=True)
def _reset():
    yield
    ck.set_lanes_per_buffer(0)
    ck.set_batch_grid(0)


def three_rounds(g):
    """Units (buffers or messages) that give a 1-workgroup grid three rounds:
    two full passes, then two wavefronts, the last with one active group."""
    gpw = 64 // g
    return 2 * K_WAVES * gpw + gpw + 1


# ------------------------------------------------------------ host-side cases

def _assert_disjoint(ranges, size):
    """ranges: (start, length) of every destination in the arena of `size` bytes."""
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


def _place(cases, gaps=None):
    """cases: (source offset, length, (dst - src) mod 16); gaps: free bytes in
    front of each destination (plus the 0..15 that the alignment needs).
    Returns the destinations' arena offsets and the arena's size."""
    pos, places = GUARD, []
    for k, (so, n, delta) in enumerate(cases):
        pos += gaps[k] if gaps else 0
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


def _buffer_crcs(oracle, host, offs, lens, seeds, seed0):
    """CRC of host[o:o+n] per buffer, seeded per buffer or with seed0 (one C call)."""
    iov = np.zeros((len(lens), 2), np.uint64)
    iov[:, 0] = np.uint64(host.ctypes.data) + np.asarray(offs, np.uint64)
    iov[:, 1] = np.asarray(lens, np.uint64)
    return oracle.msg_chain(iov, np.arange(len(lens) + 1, dtype=np.uint64), seeds=seeds, seed0=seed0)


def round_cases(g):
    """Group A: three rounds of buffers. The lengths' cycle moves on by one
    per round and the alignments' by one per eight buffers, so a wavefront
    position meets other lengths in each round and every length of 64 bytes
    or more meets both a co-aligned and a not-co-aligned destination."""
    u, gpw = ROWS[g], 64 // g
    lens = [0, 1, 63, 64, 16 * g - 1, 16 * g * u + 17, 16 * g * (2 * u + 1) + 5, 16 * g * (3 * u + 2)]
    cases = []
    for k in range(three_rounds(g)):
        li = (k + k // (K_WAVES * gpw)) % 8
        so = 4096 * (k % 61) + 16 * (k % 5) + (0, 5, 15)[k % 3]
        cases.append((so, lens[li], (0, 0, 0, 7)[(li + k // 8) % 4]))
    return cases


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


def gather_expect(oracle, host, lay):
    """The arena's image and the segments' seed-0 CRCs, from the host copy."""
    want = np.full(lay["size"], CANARY, np.uint8)
    at = GUARD
    for o, n in lay["iov"].tolist():
        want[at:at + n] = host[o:o + n]
        at += n
    host_iov = lay["iov"].copy()
    host_iov[:, 0] += np.uint64(host.ctypes.data)
    return want, host_iov, oracle.crc32c_iov(host_iov)


def round_msgs(g):
    """Group C: three rounds of messages (see the module's test_gather_rounds)."""
    rnd = random.Random(0x6A70 + g)
    u, gpw = ROWS[g], 64 // g
    per = K_WAVES * gpw  # messages of one pass: message m + per runs on the lane group of message m
    counts = [0, 1, 2, g - 1, g, g + 1, 2 * g + 1]
    lens = [0, 1, 15, 16, 17, 63, 64, 100, 16 * g, 16 * g * (u + 1) + 9, 4097]
    msgs = []
    for m in range(three_rounds(g)):
        # the first message of a later round (and every third after it) starts
        # with the length its lane group folded last in the round before
        prev = msgs[m - per] if m >= per and (m - per) % 3 == 0 else None
        carry = prev[-1] if prev else None
        if m % 5 == 4:
            # equal lengths, then another: the fold basis is built, hit, rebuilt
            k = rnd.choice([c for c in counts if c >= 3])
            n = carry if carry is not None else rnd.choice(lens[1:])
            segs = [n] * (k - 1) + [rnd.choice([x for x in lens if x != n])]
        else:
            segs = [rnd.choice(lens) for _ in range(counts[(m + 1) % 7])]
            if segs and carry is not None:
                segs[0] = carry
        msgs.append(segs)
    assert msgs[0] and msgs[per] and msgs[per][0] == msgs[0][-1]
    assert {len(s) for s in msgs} >= set(counts)
    return msgs


def fuzz_iov_case(rnd):
    lens = _lengths(rnd, 100)
    cases = [(rnd.randrange(0, POOL - n), n, 0 if rnd.random() < 0.5 else rnd.randrange(16)) for n in lens]
    gaps = [rnd.randrange(41) for _ in lens]
    seeds = [rnd.getrandbits(32) if rnd.random() < 0.7 else 0 for _ in lens]
    return cases, gaps, seeds


def fuzz_strided_case(rnd):
    aligned = rnd.random() < 0.5
    nbytes = rnd.choice([4096, 8192, 65536, 16 * 64 * 4]) if aligned else rnd.randrange(1, 70000)
    stride = nbytes if aligned else nbytes + rnd.randrange(0, 64)
    count = max(1, min(rnd.randrange(1, 300), (POOL - 64) // stride))
    base = 0 if aligned else rnd.randrange(0, 16)
    dst_stride, dst_base = nbytes + rnd.randrange(0, 64), rnd.randrange(0, 16)
    if rnd.random() < 0.25:  # co-aligned throughout
        dst_stride, dst_base = stride, base
    seeds = [rnd.getrandbits(32) for _ in range(count)] if rnd.random() < 0.3 else None
    size = GUARD + dst_base + (count - 1) * dst_stride + nbytes + GUARD
    _assert_disjoint([(GUARD + dst_base + i * dst_stride, nbytes) for i in range(count)], size)
    return nbytes, stride, count, base, dst_stride, dst_base, seeds, size


def fuzz_gather_msgs(rnd):
    return [[min(n, 40000) for n in _lengths(rnd, rnd.choice([0, 1, 2, 5, 12]))]
            for _ in range(rnd.randrange(1, 301))]


# ------------------------------------------------------------------- runners

def _run_copy_iov(torch, oracle, host, src_ptr, cases, gaps, seeds, seed, what):
    places, size = _place(cases, gaps)
    want = _iov_image(host, cases, places, size)
    arena = _arena(torch, size)
    iov = np.zeros((len(cases), 2), np.uint64)
    iov[:, 0] = np.uint64(src_ptr) + np.asarray([c[0] for c in cases], np.uint64)
    iov[:, 1] = np.asarray([c[1] for c in cases], np.uint64)
    out = torch.zeros(len(cases), dtype=torch.int32, device="cuda")
    ck.copy_batch_iov(_i64(torch, iov), _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(places, np.uint64)),
                      len(cases), out, seed=seed, seeds=None if seeds is None else _i32(torch, seeds))
    torch.cuda.synchronize()
    ref = _buffer_crcs(oracle, host, [c[0] for c in cases], [c[1] for c in cases], seeds, seed)
    got = _u32(out)
    for k in np.flatnonzero(got != ref)[:1]:
        raise AssertionError(f"{what}: crc {k} of {cases[k]} is {got[k]:#x}, want {ref[k]:#x}")
    _first_diff(arena.cpu().numpy(), want, what)


def _run_gather(torch, oracle, lay, expect, src_ptr, with_seg, seeds, seed, what, arena=None):
    want, host_iov, seg_crc = expect
    nmsg, nseg = len(lay["msgs"]), lay["iov"].shape[0]
    arena = _arena(torch, lay["size"]) if arena is None else arena
    dev_iov = lay["iov"].copy()
    dev_iov[:, 0] += np.uint64(src_ptr)
    out = torch.zeros(nmsg, dtype=torch.int32, device="cuda")
    seg = torch.full((nseg + 2,), -1, dtype=torch.int32, device="cuda") if with_seg else None
    ck.gather_msg_n(_i64(torch, dev_iov) if nseg else None, _i64(torch, lay["start"]), nmsg, nseg,
                    _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(lay["dst_off"], np.uint64)), seg, out,
                    seed=seed, seeds=None if seeds is None else _i32(torch, seeds))
    torch.cuda.synchronize()
    ref = oracle.msg_chain(host_iov, lay["start"], seeds=seeds, seed0=seed)
    got = _u32(out)
    for m in np.flatnonzero(got != ref)[:1]:
        raise AssertionError(f"{what}: message {m} {lay['msgs'][m]} is {got[m]:#x}, want {ref[m]:#x}")
    if with_seg:
        got = _u32(seg)
        for k in np.flatnonzero(got[:nseg] != seg_crc)[:1]:
            m = int(np.searchsorted(lay["start"], k, side="right")) - 1
            raise AssertionError(f"{what}: segment {k} (number {k - int(lay['start'][m])} of message {m}, "
                                 f"{len(lay['msgs'][m])} segments) is {got[k]:#x}, want {seg_crc[k]:#x}")
        assert (got[nseg:] == 0xFFFFFFFF).all(), what  # nothing stored past the last segment's CRC
    _first_diff(arena.cpu().numpy(), want, what)


# ------------------------------------------------------------ A: buffer rounds

@pytest.mark.parametrize("g", GS)
def test_buffer_rounds(dev_pool, oracle, g):
    torch, host, d = dev_pool
    ck.set_batch_grid(1)
    _run_iov(torch, oracle, host, d, round_cases(g), g)


# ----------------------------------------------------------- B: strided rounds

@pytest.mark.parametrize("form", ["co_aligned", "not_co_aligned", "seeds"])
@pytest.mark.parametrize("g", GS)
def test_strided_rounds(dev_pool, oracle, g, form):
    # an aligned source and no seed array: the seed enters through the shift at
    # the end (shift_init); at 32 and 64 lanes this is the loop whose first
    # buffer is preloaded across the table barrier and every later one inside
    torch, host, d = dev_pool
    nbytes, count = 16 * g * (2 * ROWS[g] + 1), three_rounds(g)
    src_stride = nbytes + 16
    dst_stride = nbytes + 3 if form == "not_co_aligned" else src_stride
    size = GUARD + (count - 1) * dst_stride + nbytes + GUARD
    _assert_disjoint([(GUARD + i * dst_stride, nbytes) for i in range(count)], size)
    want = np.full(size, CANARY, np.uint8)
    for i in range(count):
        want[GUARD + i * dst_stride:GUARD + i * dst_stride + nbytes] = host[i * src_stride:i * src_stride + nbytes]
    rnd = random.Random(g)
    seeds = [rnd.getrandbits(32) if i % 4 else 0 for i in range(count)] if form == "seeds" else None
    arena = _arena(torch, size)
    out = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck.set_lanes_per_buffer(g)
    ck.set_batch_grid(1)
    ck.copy_batch_strided(d, src_stride, arena.data_ptr() + GUARD, dst_stride, nbytes, count, out,
                          seed=0xFFFFFFFF, seeds=None if seeds is None else _i32(torch, seeds))
    torch.cuda.synchronize()
    ref = _buffer_crcs(oracle, host, [i * src_stride for i in range(count)], [nbytes] * count, seeds, 0xFFFFFFFF)
    got = _u32(out)
    for i in np.flatnonzero(got != ref)[:1]:
        raise AssertionError(f"lanes {g}, {form}: crc of buffer {i} is {got[i]:#x}, want {ref[i]:#x}")
    _first_diff(arena.cpu().numpy(), want, f"lanes {g}, {form}, buffers of {nbytes} B every {dst_stride}")


# ------------------------------------------------------------ C: gather rounds

@pytest.fixture(scope="module")
def round_gathers(dev_pool, oracle):
    torch, host, d = dev_pool
    made = {}

    def get(g):
        if g not in made:
            lay = gather_layout(random.Random(0x6A71 + g), POOL, round_msgs(g))
            made[g] = lay, gather_expect(oracle, host, lay)
        return made[g]
    return get


@pytest.mark.parametrize("with_seg", [False, True])
@pytest.mark.parametrize("g", GS)
def test_gather_rounds(dev_pool, oracle, round_gathers, g, with_seg):
    """Messages of 0, 1, 2, G-1, G, G+1 and 2G+1 segments (the coalesced
    segment-CRC store fires zero, one and several times per message), every
    fifth a run of equal lengths and then another (the fold-basis cache hit and
    rebuilt), the first message of a later round opening with the length its
    lane group saw last; three rounds on one workgroup, then the full grid."""
    torch, host, d = dev_pool
    lay, expect = round_gathers(g)
    co = [(at - o) % 16 == 0 for (o, n), at in zip(lay["iov"].tolist(), _segment_places(lay)) if n >= 64]
    assert any(co) and not all(co)
    assert max(len(s) for s in lay["msgs"]) > 2 * g
    rnd = random.Random(g)
    seeds = [rnd.getrandbits(32) for _ in lay["msgs"]]
    ck.set_lanes_per_buffer(g)
    for cap in (1, 0):
        ck.set_batch_grid(cap)
        _run_gather(torch, oracle, lay, expect, d.data_ptr(), with_seg, seeds, 0,
                    f"lanes {g}, segment CRCs {with_seg}, grid cap {cap}")


def _segment_places(lay):
    at, out = GUARD, []
    for n in lay["iov"][:, 1].tolist():
        out.append(at)
        at += n
    return out


# ---------------------------------------------------------------- E: long rows

@pytest.mark.parametrize("g", [32, 64])
def test_long_rows(dev_pool, oracle, g):
    # thousands of rows per lane: the row loop with its stores, and the
    # separate copy of a long not-co-aligned buffer
    torch, host, d = dev_pool
    cases = [(3, (1 << 20) + 5, 0), (0, 3 << 20, 0), (3, (1 << 20) + 5, 9), (0, 3 << 20, 9)]
    _run_iov(torch, oracle, host, d, cases, g)


# -------------------------------------------------------------------- F: fuzz

FUZZ_LANES = [0, 4, 8, 16, 32, 64]


@pytest.mark.parametrize("round_", range(3 * SOAK))
def test_fuzz_copy_iov(dev_pool, oracle, round_):
    torch, host, d = dev_pool
    rnd = random.Random(11000 + round_)
    ck.set_batch_grid(2 * (round_ % 2))
    for e, lanes in enumerate(FUZZ_LANES):
        cases, gaps, seeds = fuzz_iov_case(rnd)
        seed = rnd.getrandbits(32)
        ck.set_lanes_per_buffer(lanes)
        _run_copy_iov(torch, oracle, host, d.data_ptr(), cases, gaps, None if e % 2 else seeds, seed,
                      f"round {round_}, lanes {lanes}")


@pytest.mark.parametrize("round_", range(3 * SOAK))
def test_fuzz_copy_strided(dev_pool, oracle, round_):
    torch, host, d = dev_pool
    rnd = random.Random(12000 + round_)
    ck.set_batch_grid(2 * (round_ % 2))
    for lanes in FUZZ_LANES:
        nbytes, stride, count, base, dst_stride, dst_base, seeds, size = fuzz_strided_case(rnd)
        seed = rnd.getrandbits(32)
        what = f"round {round_}, lanes {lanes}, {count} x {nbytes} B every {stride} from {base} to every " \
               f"{dst_stride} from {dst_base}"
        want = np.full(size, CANARY, np.uint8)
        for i in range(count):
            at = GUARD + dst_base + i * dst_stride
            want[at:at + nbytes] = host[base + i * stride:base + i * stride + nbytes]
        arena = _arena(torch, size)
        out = torch.zeros(count, dtype=torch.int32, device="cuda")
        ck.set_lanes_per_buffer(lanes)
        ck.copy_batch_strided(d.data_ptr() + base, stride, arena.data_ptr() + GUARD + dst_base, dst_stride, nbytes,
                              count, out, seed=seed, seeds=None if seeds is None else _i32(torch, seeds))
        torch.cuda.synchronize()
        ref = _buffer_crcs(oracle, host, [base + i * stride for i in range(count)], [nbytes] * count, seeds, seed)
        got = _u32(out)
        for i in np.flatnonzero(got != ref)[:1]:
            raise AssertionError(f"{what}: crc of buffer {i} is {got[i]:#x}, want {ref[i]:#x}")
        _first_diff(arena.cpu().numpy(), want, what)


@pytest.mark.parametrize("round_", range(3 * SOAK))
def test_fuzz_gather(dev_pool, oracle, round_):
    torch, host, d = dev_pool
    rnd = random.Random(13000 + round_)
    ck.set_batch_grid(2 * (round_ % 2))
    for lanes in FUZZ_LANES:
        lay = gather_layout(rnd, POOL, fuzz_gather_msgs(rnd))
        with_seg = rnd.random() < 0.5
        seeds = [rnd.getrandbits(32) for _ in lay["msgs"]] if round_ % 2 == 0 else None
        seed = rnd.getrandbits(32)
        ck.set_lanes_per_buffer(lanes)
        _run_gather(torch, oracle, lay, gather_expect(oracle, host, lay), d.data_ptr(), with_seg, seeds, seed,
                    f"round {round_}, lanes {lanes}, segment CRCs {with_seg}")


# ------------------------------------------------------------ G: other memory

@pytest.fixture(scope="module")
def pinned_pool():
    import torch
    host = datagen.stream_bytes(0xC0C7, 1 << 20)
    src = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    src.numpy()[:] = host
    assert src.data_ptr() % 16 == 0
    return torch, host, src


@pytest.mark.parametrize("lanes", [0, 8])
def test_iov_from_pinned_host(pinned_pool, oracle, lanes):
    # the kernel reads pinned host memory in place, at every alignment
    torch, host, src = pinned_pool
    lens = [1, 63, 64, 4097, 70001]
    cases = [(80000 * k + (0, 3, 15)[k % 3], lens[k % 5], (0, 11)[k // 5 % 2]) for k in range(12)]
    assert {(n, delta) for _, n, delta in cases} >= {(n, dl) for n in lens[2:] for dl in (0, 11)}
    _run_iov(torch, oracle, host, src, cases, lanes)


@pytest.mark.parametrize("with_seg", [False, True])
def test_gather_from_pinned_host(pinned_pool, oracle, with_seg):
    torch, host, src = pinned_pool
    rnd = random.Random(0xC0C8)
    msgs = [[rnd.choice([0, 1, 63, 64, 100, 4097, 20000]) for _ in range(rnd.randrange(0, 6))] for _ in range(16)]
    lay = gather_layout(rnd, host.size, msgs)
    seeds = [rnd.getrandbits(32) for _ in msgs]
    _run_gather(torch, oracle, lay, gather_expect(oracle, host, lay), src.data_ptr(), with_seg, seeds, 0,
                f"pinned source, segment CRCs {with_seg}")


@pytest.mark.parametrize("nbytes,dst_stride", [(4096, 4096), (1000, 1003)])
def test_strided_into_pinned_host(dev_pool, oracle, nbytes, dst_stride):
    # the destination only has to be device-accessible: stores over the link
    torch, host, d = dev_pool
    count = 33
    size = GUARD + (count - 1) * dst_stride + nbytes + GUARD
    arena = torch.empty(size, dtype=torch.uint8, pin_memory=True)
    assert arena.data_ptr() % 16 == 0
    arena.numpy()[:] = CANARY
    want = np.full(size, CANARY, np.uint8)
    for i in range(count):
        want[GUARD + i * dst_stride:GUARD + i * dst_stride + nbytes] = host[i * nbytes:(i + 1) * nbytes]
    out = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck.copy_batch_strided(d, nbytes, arena.data_ptr() + GUARD, dst_stride, nbytes, count, out, seed=9)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), oracle.crc32c_strided(host, nbytes, nbytes, count, 9))
    _first_diff(arena.numpy(), want, f"pinned destination, {nbytes} B every {dst_stride}")


# ---------------------------------------------------------- H: contract edges

def _untouched(arena):
    return bool((arena.cpu().numpy() == CANARY).all())


def test_strided_zero_bytes_null_pointers():
    import torch
    arena = _arena(torch, 256)
    seeds = [0, 1, 0xFFFFFFFF, 0x12345678, 7]
    for use_seeds in (False, True):
        out = torch.zeros(5, dtype=torch.int32, device="cuda")
        ck.copy_batch_strided(None, 64, None, 64, 0, 5, out, seed=0xC0FFEE,
                              seeds=_i32(torch, seeds) if use_seeds else None)
        torch.cuda.synchronize()
        assert _u32(out).tolist() == (seeds if use_seeds else [0xC0FFEE] * 5)
    assert _untouched(arena)


@pytest.mark.parametrize("with_seg", [False, True])
def test_gather_only_empty_messages(with_seg):
    import torch
    arena = _arena(torch, 256)
    nmsg = 7
    seeds = [0, 1, 2, 0xFFFFFFFF, 0xDEADBEEF, 5, 6]
    d_dst = _i64(torch, np.full(nmsg, arena.data_ptr() + GUARD, np.uint64))
    d_start = _i64(torch, np.zeros(nmsg + 1, np.uint64))
    seg = torch.full((4,), -1, dtype=torch.int32, device="cuda") if with_seg else None
    for use_seeds in (True, False):
        out = torch.zeros(nmsg, dtype=torch.int32, device="cuda")
        ck.gather_msg_n(None, d_start, nmsg, 0, d_dst, seg, out, seed=0xABCD,
                        seeds=_i32(torch, seeds) if use_seeds else None)
        torch.cuda.synchronize()
        assert _u32(out).tolist() == (seeds if use_seeds else [0xABCD] * nmsg)
    if with_seg:
        assert (_u32(seg) == 0xFFFFFFFF).all()
    assert _untouched(arena)


def test_iov_all_lengths_zero(dev_pool):
    torch, host, d = dev_pool
    arena = _arena(torch, 1024)
    count = 37
    iov = np.zeros((count, 2), np.uint64)
    iov[:, 0] = [0 if k % 3 == 0 else d.data_ptr() + 17 * k for k in range(count)]  # null or any address
    d_dst = _i64(torch, np.asarray([arena.data_ptr() + GUARD + 5 * k for k in range(count)], np.uint64))
    seeds = [(0x9E3779B9 * k) & 0xFFFFFFFF for k in range(count)]
    for use_seeds in (True, False):
        out = torch.zeros(count, dtype=torch.int32, device="cuda")
        ck.copy_batch_iov(_i64(torch, iov), d_dst, count, out, seed=0x51, seeds=_i32(torch, seeds) if use_seeds else None)
        torch.cuda.synchronize()
        assert _u32(out).tolist() == (seeds if use_seeds else [0x51] * count)
    assert _untouched(arena)


# ------------------------------------------------------------ I: graph capture

def _splitmix_source(torch, nbytes, count):
    d = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 16 == 0
    return d


def test_graph_capture_iov(oracle):
    # one branch: a single copy_batch_iov captured on the capture stream
    import torch
    nbytes, count = 4096, 40
    d = _splitmix_source(torch, nbytes, count)
    lens = [0, 1, 63, 64, 1000, 4097, 9000]
    cases = [(nbytes * k // 2 + (0, 5, 15)[k % 3], lens[k % 7], (0, 6)[k // 7 % 2]) for k in range(count)]
    places, size = _place(cases)
    seeds = [(0x85EBCA6B * (k + 1)) & 0xFFFFFFFF if k % 3 else 0 for k in range(count)]
    iov = np.zeros((count, 2), np.uint64)
    iov[:, 0] = np.uint64(d.data_ptr()) + np.asarray([c[0] for c in cases], np.uint64)
    iov[:, 1] = np.asarray([c[1] for c in cases], np.uint64)
    d_iov, d_seeds = _i64(torch, iov), _i32(torch, seeds)
    arena = _arena(torch, size)
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(places, np.uint64))
    out = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC0C90)
    ck.copy_batch_iov(d_iov, d_dst, count, out, seeds=d_seeds)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ck.copy_batch_iov(d_iov, d_dst, count, out, seeds=d_seeds, stream=torch.cuda.current_stream())
    for fill in (0xC0C91, 0xC0C92):
        ck.fill_splitmix(d, nbytes, nbytes, count, fill)
        arena.fill_(CANARY)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = d.cpu().numpy()
        ref = _buffer_crcs(oracle, host, [c[0] for c in cases], [c[1] for c in cases], seeds, 0)
        assert np.array_equal(_u32(out), ref), hex(fill)
        _first_diff(arena.cpu().numpy(), _iov_image(host, cases, places, size), hex(fill))


def test_graph_capture_gather(oracle):
    # one branch: a single gather_msg_n with segment CRCs
    import torch
    nbytes, count = 4096, 40
    d = _splitmix_source(torch, nbytes, count)
    rnd = random.Random(0xC0CA)
    msgs = [[rnd.choice([0, 1, 16, 63, 64, 100, 4097, 6000]) for _ in range(rnd.choice([0, 1, 2, 3, 9, 17]))]
            for _ in range(48)]
    lay = gather_layout(rnd, nbytes * count, msgs)
    nmsg, nseg = len(msgs), lay["iov"].shape[0]
    seeds = [rnd.getrandbits(32) for _ in msgs]
    dev_iov = lay["iov"].copy()
    dev_iov[:, 0] += np.uint64(d.data_ptr())
    d_iov, d_start, d_seeds = _i64(torch, dev_iov), _i64(torch, lay["start"]), _i32(torch, seeds)
    arena = _arena(torch, lay["size"])
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(lay["dst_off"], np.uint64))
    out = torch.zeros(nmsg, dtype=torch.int32, device="cuda")
    seg = torch.full((nseg,), -1, dtype=torch.int32, device="cuda")
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC0CB0)
    ck.gather_msg_n(d_iov, d_start, nmsg, nseg, d_dst, seg, out, seeds=d_seeds)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ck.gather_msg_n(d_iov, d_start, nmsg, nseg, d_dst, seg, out, seeds=d_seeds,
                        stream=torch.cuda.current_stream())
    for fill in (0xC0CB1, 0xC0CB2):
        ck.fill_splitmix(d, nbytes, nbytes, count, fill)
        arena.fill_(CANARY)
        out.zero_()
        seg.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = d.cpu().numpy()
        want, host_iov, seg_crc = gather_expect(oracle, host, lay)
        assert np.array_equal(_u32(out), oracle.msg_chain(host_iov, lay["start"], seeds=seeds)), hex(fill)
        assert np.array_equal(_u32(seg), seg_crc), hex(fill)
        _first_diff(arena.cpu().numpy(), want, hex(fill))

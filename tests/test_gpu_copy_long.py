"""Copy + CRC of one long buffer over the whole device
(photon_crc32c_copy_extend_device, photon_crc64ecma_copy_extend_device,
DESIGN.md §4.7), by the method of tests/test_gpu_copy_crc.py: every CRC
bit-exact against the pinned oracle over the HOST copy of the source, every
destination arena pre-filled with 0xA5 with at least 64 guard bytes on each
side and compared WHOLE, and the source compared afterwards.

The shapes are those of tests/test_copy_long_abi.py PLAN_SHAPES, which
asserts (without a GPU) that each reaches the state of the cut it is there
for: the head slot alone, a merged head, empty leading slots, a last chunk
under 64 bytes, two and three rounds, 32- and 64-lane groups, more than one
workgroup, every workgroup factor. A source "at offset off" starts off bytes
after a 4 KiB boundary, which is what the cut is anchored at."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_copy_long_abi import MIB, PLAN_SHAPES
from tests.test_gpu_copy_crc import CANARY, GUARD
from tests.test_gpu_copy_crc64 import _first_diff

pytestmark = pytest.mark.gpu

SEEDS = {False: (0, 0x9E3779B1), True: (0, 0xFEDCBA9876543210)}
CRCS = [False, True]
IDS = ["crc32c", "crc64"]
POOL = 36 * MIB


@pytest.fixture(scope="module")
def pool():
    """One host payload; a source of n bytes is its first n bytes, wherever it is placed."""
    import torch
    assert torch.cuda.is_available()
    return torch, datagen.stream_bytes(0xC0A7, POOL)


@pytest.fixture(scope="module")
def want_crc(oracle):
    """The oracle's CRC of a host array, computed once per (payload, seed, CRC)."""
    made = {}

    def get(key, host, seed, crc64):
        k = (key, host.size, seed, crc64)
        if k not in made:
            made[k] = oracle.crc64ecma(host, seed) if crc64 else oracle.crc32c(host, seed)
        return made[k]
    return get


def _source(torch, host, off, pinned=False):
    """A copy of host that starts off bytes after a 4 KiB boundary: (tensor, index of its first byte)."""
    t = torch.empty(host.size + 2 * 4096, dtype=torch.uint8, pin_memory=True) if pinned else \
        torch.empty(host.size + 2 * 4096, dtype=torch.uint8, device="cuda")
    o = (-t.data_ptr()) % 4096 + off
    t[o:o + host.size] = torch.from_numpy(host)
    assert (t.data_ptr() + o) % 4096 == off % 4096
    return t, o


def _dest(torch, n, src_ptr, delta, pinned=False):
    """An arena of 0xA5 and the index at which (dst - src) % 16 == delta, guards on both sides."""
    size = GUARD + 16 + n + GUARD
    a = torch.empty(size, dtype=torch.uint8, pin_memory=True) if pinned else \
        torch.empty(size, dtype=torch.uint8, device="cuda")
    a.fill_(CANARY)
    at = GUARD + (src_ptr + delta - (a.data_ptr() + GUARD)) % 16
    assert (a.data_ptr() + at - src_ptr) % 16 == delta and at >= GUARD and at + n + GUARD <= size
    return a, at


def _out(torch, crc64):
    return torch.full((1,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")


def _value(out):
    a = out.cpu().numpy()
    return int(a.view(np.uint64 if a.dtype == np.int64 else np.uint32)[0])


def _call(crc64, src, dst, n, seed, out, stream=None):
    if crc64:
        ck.copy_extend64_device(src, dst, n, out, seed=seed, stream=stream)
    else:
        ck.copy_extend_device(src, dst, n, seed, out, stream=stream)


def _image(host, n, at, size):
    want = np.full(size, CANARY, np.uint8)
    want[at:at + n] = host[:n]
    return want


def _check_one(torch, want_crc, key, host, src, so, delta, seed, crc64, what, pinned_dst=False):
    """One call from src[so:so + n] to a fresh arena: CRC, arena and source."""
    n = host.size
    arena, at = _dest(torch, n, src.data_ptr() + so, delta, pinned_dst)
    out = _out(torch, crc64)
    _call(crc64, src.data_ptr() + so, arena.data_ptr() + at, n, seed, out)
    torch.cuda.synchronize()
    ref = want_crc(key, host, seed, crc64)
    got = _value(out)
    print(f"{what}: crc {got:#x}, want {ref:#x}")
    assert got == ref, f"{what}: crc is {got:#x}, want {ref:#x}"
    _first_diff(arena.cpu().numpy(), _image(host, n, at, arena.numel()), what)
    assert np.array_equal(src[so:so + n].cpu().numpy(), host), f"{what}: the source changed"


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
@pytest.mark.parametrize("row", range(len(PLAN_SHAPES)))
def test_plan_shapes(pool, want_crc, row, crc64):
    torch, payload = pool
    off, n, lanes, rounds, _ = PLAN_SHAPES[row]
    host = payload[:n]
    src, so = _source(torch, host, off)
    # the 36 MiB rows: one destination alignment each (host oracle and compare time)
    deltas = (0, 9) if n < 36 * MIB - 100000 else (0,) if n == 36 * MIB else (9,)
    ck.set_long_shape(lanes, rounds)
    try:
        for delta in deltas:
            for seed in SEEDS[crc64]:
                _check_one(torch, want_crc, "pool", host, src, so, delta, seed, crc64,
                           f"row {row} {PLAN_SHAPES[row][:4]} delta {delta} seed {seed:#x}")
    finally:
        ck.set_long_shape(0, 0)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_small_sizes(pool, want_crc, crc64):
    torch, payload = pool
    seed = SEEDS[crc64][1]
    for off in (0, 5):
        src, so = _source(torch, payload[:4097], off)
        for n in (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097):
            for delta in (0, 9):
                _check_one(torch, want_crc, "pool", payload[:n], src, so, delta, seed, crc64,
                           f"{n} bytes at offset {off}, delta {delta}")
    # no bytes and no buffers: the seed, and nothing else is touched
    arena = torch.full((256,), CANARY, dtype=torch.uint8, device="cuda")
    for s in SEEDS[crc64]:
        out = _out(torch, crc64)
        _call(crc64, None, None, 0, s, out)
        torch.cuda.synchronize()
        assert _value(out) == s
    assert bool((arena == CANARY).all())


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_matches_extend_device(pool, want_crc, crc64):
    torch, payload = pool
    n = 7 * MIB + 13
    host = payload[:n]
    src, so = _source(torch, host, 5)
    seed = SEEDS[crc64][1]
    _check_one(torch, want_crc, "pool", host, src, so, 0, seed, crc64, "7 MiB + 13 at offset 5")
    plain = _out(torch, crc64)
    if crc64:
        ck.extend64_device(src.data_ptr() + so, n, plain, seed=seed)
    else:
        ck.extend_device(src.data_ptr() + so, n, seed, plain)
    torch.cuda.synchronize()
    assert _value(plain) == want_crc("pool", host, seed, crc64)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_parts_back_to_back(pool, oracle, crc64):
    """An object from three large parts: one call per part with seed 0 on one
    stream, landed back to back at an odd address (the joins share 16-byte
    blocks); the object's CRC is the combine fold of the part CRCs."""
    torch, _ = pool
    lens = [MIB + 3, 65539, 2 * MIB + 1]
    hosts = [datagen.stream_bytes(0xC0B0 + k, n) for k, n in enumerate(lens)]
    srcs = [_source(torch, h, (7, 0, 4090)[k]) for k, h in enumerate(hosts)]
    total = sum(lens)
    arena = torch.full((GUARD + 16 + total + GUARD,), CANARY, dtype=torch.uint8, device="cuda")
    at = GUARD + 3
    assert (arena.data_ptr() + at) % 2 == 1
    assert all((at + sum(lens[:k])) % 16 for k in (1, 2))  # a join inside a 16-byte block
    outs = [_out(torch, crc64) for _ in lens]
    st = torch.cuda.Stream()
    pos = at
    torch.cuda.synchronize()
    for (src, so), n, out in zip(srcs, lens, outs):
        _call(crc64, src.data_ptr() + so, arena.data_ptr() + pos, n, 0, out, stream=st)
        pos += n
    torch.cuda.synchronize()
    whole = np.concatenate(hosts)
    want = np.full(arena.numel(), CANARY, np.uint8)
    want[at:at + total] = whole
    _first_diff(arena.cpu().numpy(), want, "three parts")
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    parts = [_value(o) for o in outs]
    assert parts == [crc(h, 0) for h in hosts]
    acc = parts[0]
    for c, n in zip(parts[1:], lens[1:]):
        acc = ck.crc64ecma_combine(acc, c, n) if crc64 else ck.crc32c_combine(acc, c, n)
    assert acc == crc(whole, 0)
    for (src, so), h in zip(srcs, hosts):
        assert np.array_equal(src[so:so + h.size].cpu().numpy(), h)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_pinned_host_source(pool, want_crc, crc64):
    # the kernel reads pinned host memory in place; one case lands in pinned host memory too
    torch, payload = pool
    host = payload[:MIB + 5]
    seed = SEEDS[crc64][1]
    for off, delta, pinned_dst in ((0, 0, False), (3, 9, False), (3, 0, True)):
        src, so = _source(torch, host, off, pinned=True)
        _check_one(torch, want_crc, "pool", host, src, so, delta, seed, crc64,
                   f"pinned source at offset {off}, delta {delta}, pinned destination {pinned_dst}", pinned_dst)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_streams(pool, want_crc, crc64):
    # four streams at once, each with its own buffers and its own reduce state
    torch, payload = pool
    jobs = []
    for k in range(4):
        host = payload[k * 1000:k * 1000 + 3 * MIB + k]
        src, so = _source(torch, host, (0, 1, 15, 4095)[k])
        arena, at = _dest(torch, host.size, src.data_ptr() + so, (0, 9, 0, 5)[k])
        jobs.append((host, src, so, arena, at, _out(torch, crc64), torch.cuda.Stream()))
    torch.cuda.synchronize()
    for rep in range(3):
        for k, (host, src, so, arena, at, out, st) in enumerate(jobs):
            _call(crc64, src.data_ptr() + so, arena.data_ptr() + at, host.size, SEEDS[crc64][1] + k, out, stream=st)
    torch.cuda.synchronize()
    for k, (host, src, so, arena, at, out, st) in enumerate(jobs):
        assert _value(out) == want_crc(("stream", k), host, SEEDS[crc64][1] + k, crc64), k
        _first_diff(arena.cpu().numpy(), _image(host, host.size, at, arena.numel()), f"stream {k}")
        assert np.array_equal(src[so:so + host.size].cpu().numpy(), host)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_graph_capture(pool, oracle, crc64):
    # one call of more than one workgroup captured; the second replay runs over a refilled source
    torch, _ = pool
    n = 1000013
    src = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
    so = (-src.data_ptr()) % 4096 + 1
    arena, at = _dest(torch, n, src.data_ptr() + so, 0)
    out = _out(torch, crc64)
    seed = SEEDS[crc64][1]
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0xC0C0)
    _call(crc64, src.data_ptr() + so, arena.data_ptr() + at, n, seed, out)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(crc64, src.data_ptr() + so, arena.data_ptr() + at, n, seed, out, stream=torch.cuda.current_stream())
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    for rep in range(2):
        ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0xC0C1 + rep)
        arena.fill_(CANARY)
        out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = src.cpu().numpy()[so:so + n]
        assert _value(out) == crc(host, seed), rep
        _first_diff(arena.cpu().numpy(), _image(host, n, at, arena.numel()), f"replay {rep}")


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_1gib_reference_shape(pool, crc64):
    """The reference's perf shape (1 GiB at buf+1) to dbuf+1: the CRC equals
    extend_device's over the source (pinned at this shape by
    tests/test_gpu_fullsize.py), the bytes by a comparison on the device."""
    torch, _ = pool
    n = 1 << 30
    src = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
    arena = torch.empty(4096 + n + 4096, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 4096 == 0 and arena.data_ptr() % 4096 == 0
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0xC0D0 + crc64)
    arena.fill_(CANARY)
    at = 4096 + 1
    out, plain = _out(torch, crc64), _out(torch, crc64)
    seed = SEEDS[crc64][1]
    _call(crc64, src.data_ptr() + 1, arena.data_ptr() + at, n, seed, out)
    if crc64:
        ck.extend64_device(src.data_ptr() + 1, n, plain, seed=seed)
    else:
        ck.extend_device(src.data_ptr() + 1, n, seed, plain)
    torch.cuda.synchronize()
    assert _value(out) == _value(plain)
    assert torch.equal(arena[at:at + n], src[1:1 + n])
    assert bool((arena[at - GUARD:at] == CANARY).all()) and bool((arena[at + n:at + n + GUARD] == CANARY).all())
    del src, arena

"""Copy + CRC-32C in one pass (photon_crc32c_copy_batch_strided / _iov,
photon_crc32c_gather_msg_n): every CRC bit-exact against the pinned oracle
(tests/_oracle.py), every destination byte against numpy slices of the host
copy of the source, and every destination arena compared WHOLE -- 0xA5
canaries in the guards, the gaps and the neighbours included -- so a store
that strays by one byte fails."""
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen

pytestmark = pytest.mark.gpu

CANARY = 0xA5
GUARD = 64
POOL = 1 << 20
ROWS = {4: 4, 8: 4, 16: 2, 32: 4, 64: 4}  # default rows per step of each lane-group size


@pytest.fixture(scope="module")
def dev_pool():
    import torch
    assert torch.cuda.is_available()
    host = datagen.stream_bytes(0xC0B1, POOL)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return torch, host, d


@pytest.fixture(autouse=True)
def _reset():
    yield
    ck.set_lanes_per_buffer(0)


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _i32(torch, a):
    return torch.from_numpy(np.asarray(a, np.uint32).view(np.int32)).cuda()


def _i64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _arena(torch, nbytes):
    a = torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda")
    assert a.data_ptr() % 16 == 0
    return a


def _run_iov(torch, oracle, host, d, cases, lanes):
    """cases: (source offset in the pool, length, (dst - src) mod 16). The
    destinations follow one another with only the 0..15 bytes of padding that
    the wanted alignment needs; per-buffer seeds."""
    rnd = random.Random(len(cases) * 131 + lanes)
    pos, places = GUARD, []
    for so, n, delta in cases:
        pos += ((so + delta) - pos) % 16
        places.append(pos)
        pos += n
    arena = _arena(torch, pos + GUARD)
    want = np.full(pos + GUARD, CANARY, np.uint8)
    seeds = [rnd.getrandbits(32) if k % 3 else 0 for k in range(len(cases))]
    for (so, n, _), at in zip(cases, places):
        want[at:at + n] = host[so:so + n]
    iov = np.zeros((len(cases), 2), np.uint64)
    iov[:, 0] = np.uint64(d.data_ptr()) + np.asarray([c[0] for c in cases], np.uint64)
    iov[:, 1] = np.asarray([c[1] for c in cases], np.uint64)
    d_iov = _i64(torch, iov)
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(places, np.uint64))
    out = torch.zeros(len(cases), dtype=torch.int32, device="cuda")
    ck.set_lanes_per_buffer(lanes)
    ck.copy_batch_iov(d_iov, d_dst, len(cases), out, seeds=_i32(torch, seeds))
    torch.cuda.synchronize()
    got = _u32(out)
    for k, ((so, n, delta), s) in enumerate(zip(cases, seeds)):
        assert got[k] == oracle.crc32c(host[so:so + n], s), (lanes, so, n, delta)
    got_arena = arena.cpu().numpy()
    bad = np.flatnonzero(got_arena != want)
    if bad.size:
        b = int(bad[0])
        k = max(i for i, at in enumerate(places) if at <= b) if b >= places[0] else -1
        raise AssertionError(f"lanes {lanes}: arena byte {b} is {got_arena[b]:#x}, want {want[b]:#x}; "
                             f"{bad.size} bytes differ; nearest case {cases[k] if k >= 0 else None} at {places[k]}")
    return d_iov, seeds, got


def _row_cases(g, deltas):
    u = ROWS[g]
    cases = []
    for k in range(2 * u + 4):
        for dd in (-17, -16, -1, 0, 1, 15, 16, 17):
            n = k * 16 * g + dd
            if n < 0:
                continue
            for j, so in enumerate((0, 5, 15)):
                # sources spread over the pool (they may overlap: read only)
                cases.append((4096 * (len(cases) % 61) + 16 * j + so, n, deltas[len(cases) % len(deltas)]))
    return cases


def test_length_sweep_4_lanes(dev_pool, oracle):
    # tiny buffers, heads, tails, the first step and the loop entry (a row is 64 B)
    torch, host, d = dev_pool
    cases = [(1024 * (n % 97) + 16 * (n % 5) + so, n, 0) for n in range(401) for so in (0, 1, 7, 15)]
    _run_iov(torch, oracle, host, d, cases, 4)


@pytest.mark.parametrize("g", [4, 8, 16, 32, 64])
def test_row_boundaries(dev_pool, oracle, g):
    # preload only, one step, the loop edge, remainder rows, the partial last
    # row -- each with and without a head and a tail
    torch, host, d = dev_pool
    _run_iov(torch, oracle, host, d, _row_cases(g, (0,)), g)


@pytest.mark.parametrize("g", [4, 8, 16, 32, 64])
def test_not_co_aligned(dev_pool, oracle, g):
    torch, host, d = dev_pool
    _run_iov(torch, oracle, host, d, _row_cases(g, (1, 4, 8, 13)), g)


@pytest.mark.parametrize("nbytes,src_stride,dst_stride", [
    (4096, 4096, 4096), (4096, 4112, 4099), (65536, 65536, 65536 + 16), (1000, 1003, 1000)])
def test_strided(oracle, nbytes, src_stride, dst_stride):
    import torch
    count = 257  # the last wavefront is partly inactive
    src_len = (count - 1) * src_stride + nbytes
    host = datagen.stream_bytes(0xC0B2 + nbytes, src_len)
    d = torch.from_numpy(host.copy()).cuda()
    dst_len = (count - 1) * dst_stride + nbytes
    want = np.full(GUARD + dst_len + GUARD, CANARY, np.uint8)
    for i in range(count):
        want[GUARD + i * dst_stride:GUARD + i * dst_stride + nbytes] = host[i * src_stride:i * src_stride + nbytes]
    rnd = random.Random(nbytes)
    seeds = [rnd.getrandbits(32) for _ in range(count)]
    for use_seeds in (True, False):
        arena = _arena(torch, GUARD + dst_len + GUARD)
        out = torch.zeros(count, dtype=torch.int32, device="cuda")
        ck.copy_batch_strided(d, src_stride, arena.data_ptr() + GUARD, dst_stride, nbytes, count, out,
                              seed=0xFFFFFFFF, seeds=_i32(torch, seeds) if use_seeds else None)
        torch.cuda.synchronize()
        got = _u32(out)
        for i in range(count):
            s = seeds[i] if use_seeds else 0xFFFFFFFF
            assert got[i] == oracle.crc32c(host[i * src_stride:i * src_stride + nbytes], s), (use_seeds, i)
        assert np.array_equal(arena.cpu().numpy(), want), use_seeds


@pytest.fixture(scope="module")
def gather_case(dev_pool):
    torch, host, d = dev_pool
    rnd = random.Random(0x6A7)
    lens_from = [0, 1, 15, 16, 17, 63, 64, 100, 4096, 4097, 6000]
    msgs = []
    for m in range(64):
        if m == 7:
            msgs.append([])  # an empty message
        elif m == 11:
            msgs.append([0, 0, 0])  # only empty segments
        else:
            msgs.append([rnd.choice(lens_from) for _ in range(rnd.randrange(1, 10))])
    iov, start, dst_off, parts = [], [0], [], []
    pos = GUARD
    for segs in msgs:
        dst_off.append(pos)  # packed back to back: tails and heads share 16-byte blocks
        for n in segs:
            o = rnd.randrange(0, POOL - n)
            iov.append((o, n))
            parts.append(host[o:o + n])
            pos += n
        start.append(len(iov))
    want = np.full(pos + GUARD, CANARY, np.uint8)
    at = GUARD
    for p in parts:
        want[at:at + p.size] = p
        at += p.size
    seeds = [rnd.getrandbits(32) for _ in msgs]
    return msgs, np.asarray(iov, np.uint64), np.asarray(start, np.uint64), dst_off, parts, want, seeds


@pytest.mark.parametrize("lanes", [0, 4, 16])
@pytest.mark.parametrize("with_seg", [False, True])
def test_gather(dev_pool, oracle, gather_case, lanes, with_seg):
    torch, host, d = dev_pool
    msgs, iov, start, dst_off, parts, want, seeds = gather_case
    nmsg, nseg = len(msgs), len(iov)
    arena = _arena(torch, want.size)
    dev_iov = iov.copy()
    dev_iov[:, 0] += np.uint64(d.data_ptr())
    host_iov = iov.copy()
    host_iov[:, 0] += np.uint64(host.ctypes.data)
    out = torch.zeros(nmsg, dtype=torch.int32, device="cuda")
    seg = torch.full((nseg,), -1, dtype=torch.int32, device="cuda") if with_seg else None
    ck.set_lanes_per_buffer(lanes)
    ck.gather_msg_n(_i64(torch, dev_iov), _i64(torch, start), nmsg, nseg,
                    _i64(torch, np.uint64(arena.data_ptr()) + np.asarray(dst_off, np.uint64)), seg, out,
                    seeds=_i32(torch, seeds))
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), oracle.msg_chain(host_iov, start, seeds=seeds))
    if with_seg:
        got = _u32(seg)
        for k, p in enumerate(parts):
            assert got[k] == oracle.crc32c(p, 0), k
    got_arena = arena.cpu().numpy()
    at = GUARD
    for m, segs in enumerate(msgs):  # each destination = the concatenation of its segments
        n = sum(segs)
        assert np.array_equal(got_arena[at:at + n], want[at:at + n]), (lanes, m)
        at += n
    assert np.array_equal(got_arena, want)


def test_pinned_host_source(oracle):
    # the kernel reads pinned host memory over the link in place
    import torch
    nbytes, count = 65536, 33
    src = torch.empty(nbytes * count, dtype=torch.uint8, pin_memory=True)
    host = datagen.stream_bytes(0xC0B6, nbytes * count)
    src.numpy()[:] = host
    arena = _arena(torch, GUARD + nbytes * count + GUARD)
    out = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck.copy_batch_strided(src, nbytes, arena.data_ptr() + GUARD, nbytes, nbytes, count, out, seed=5)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), oracle.crc32c_strided(host, nbytes, nbytes, count, 5))
    want = np.full(arena.numel(), CANARY, np.uint8)
    want[GUARD:GUARD + host.size] = host
    assert np.array_equal(arena.cpu().numpy(), want)


def test_source_untouched_and_plain_calls_unchanged(dev_pool, oracle):
    torch, host, d = dev_pool
    cases = [(3000 * k + (k % 16), n, k % 2 * 5) for k, n in enumerate([0, 1, 63, 64, 65, 1000, 4096, 4097, 70000])]
    d_iov, seeds, got = _run_iov(torch, oracle, host, d, cases, 0)
    assert np.array_equal(d.cpu().numpy(), host)
    out = torch.zeros(len(cases), dtype=torch.int32, device="cuda")
    ck.batch_iov(d_iov, len(cases), out, seeds=_i32(torch, seeds))
    torch.cuda.synchronize()
    assert np.array_equal(_u32(out), got)


def test_graph_capture(oracle):
    # one branch: a single copy_batch_strided captured on a side stream
    import torch
    nbytes, count = 4096, 64
    d = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    arena = _arena(torch, GUARD + nbytes * count + GUARD)
    out = torch.zeros(count, dtype=torch.int32, device="cuda")
    ck.fill_splitmix(d, nbytes, nbytes, count, 0xC0B80)
    ck.copy_batch_strided(d, nbytes, arena.data_ptr() + GUARD, nbytes, nbytes, count, out)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ck.copy_batch_strided(d, nbytes, arena.data_ptr() + GUARD, nbytes, nbytes, count, out, seed=3,
                              stream=torch.cuda.current_stream())
    for fill in (0xC0B81, 0xC0B82):
        ck.fill_splitmix(d, nbytes, nbytes, count, fill)
        arena.fill_(CANARY)
        out.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = d.cpu().numpy()
        assert np.array_equal(_u32(out), oracle.crc32c_strided(host, nbytes, nbytes, count, 3)), hex(fill)
        want = np.full(arena.numel(), CANARY, np.uint8)
        want[GUARD:GUARD + host.size] = host
        assert np.array_equal(arena.cpu().numpy(), want), hex(fill)

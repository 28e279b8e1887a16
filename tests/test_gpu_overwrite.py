"""Overwrite + CRC delta on the device (photon_crc32c_overwrite_batch_* /
photon_crc64ecma_overwrite_batch_*) and the patch of stored CRCs by the deltas
(photon_crc32c_patch_n / photon_crc64ecma_patch_n), DESIGN.md §4.14.

Expected values come from the pinned oracle (tests/_oracle.py) over host
copies, never from another call of this library: delta = crc(old, s) ^
crc(new, s), patched block and object CRCs = the oracle's CRC of the modified
bytes. The destination arena holds known pseudo-random old bytes
(datagen.stream_bytes with a second seed) and is compared WHOLE afterwards:
written ranges equal the source, every other byte -- guards, gaps and
neighbours -- the old content. The sizes are the geometry's edges (lane-group
rows, 16-byte blocks, the 64-byte tiny rule, grid rounds), not a workload's."""
import random

import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_gpu_copy_crc import GUARD, _i64
from tests.test_gpu_copy_crc64 import _assert_disjoint, _first_diff, _place
from tests.test_patch_abi import DT, fuzz_cases, large_tail_case, replay

pytestmark = pytest.mark.gpu

POOL = 1 << 20
GS = [4, 8, 16, 32, 64]
U = 2                  # rows per step of every overwrite build (overwrite_rows)
SEED = 0xDEADBEEF      # any common seed gives the same delta
OLD_SEED = 0x0DD5EED
WIDTHS = [False, True]
IDS = ["crc32c", "crc64"]


@pytest.fixture(scope="module")
def dev_pool():
    import torch
    assert torch.cuda.is_available()
    host = datagen.stream_bytes(0x0F7E1, POOL)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return torch, host, d


@pytest.fixture(autouse=True)
def _reset():
    yield
    ck.set_lanes_per_buffer(0)
    ck.set_batch_grid(0)


def crc_of(oracle, c64):
    return oracle.crc64ecma if c64 else oracle.crc32c


def words(t, c64):
    return t.cpu().numpy().view(DT[c64])


def out_words(torch, n, c64, fill=0x5A):
    """n delta / CRC words on the device, pre-filled so that a word never written shows."""
    return torch.full((n * (8 if c64 else 4),), fill, dtype=torch.uint8, device="cuda")


def dev_words(torch, a, c64):
    return torch.from_numpy(np.ascontiguousarray(a, DT[c64]).view(np.uint8).copy()).cuda()


def old_bytes(size):
    return datagen.stream_bytes(OLD_SEED + size, size)


def expect(oracle, host, writes, old, c64):
    """writes: (source offset, length, arena offset). The oracle's deltas and the arena afterwards."""
    crc = crc_of(oracle, c64)
    want = old.copy()
    deltas = np.zeros(len(writes), DT[c64])
    for k, (so, n, at) in enumerate(writes):
        deltas[k] = crc(old[at:at + n], SEED) ^ crc(host[so:so + n], SEED)
        want[at:at + n] = host[so:so + n]
    return deltas, want


def check(got, want_deltas, arena, want_arena, writes, what):
    bad = np.flatnonzero(got != want_deltas)
    if bad.size:
        k = int(bad[0])
        raise AssertionError(f"{what}: delta of write {k} {writes[k]} is {int(got[k]):#x}, want "
                             f"{int(want_deltas[k]):#x}; {bad.size} of {len(writes)} differ")
    _first_diff(arena.cpu().numpy(), want_arena, what)


def run_iov(torch, oracle, host, src, writes, size, lanes, c64, what="", old=None):
    _assert_disjoint([(at, n) for _, n, at in writes], size)
    old = old_bytes(size) if old is None else old
    want_deltas, want_arena = expect(oracle, host, writes, old, c64)
    arena = torch.from_numpy(old.copy()).cuda()
    assert arena.data_ptr() % 16 == 0
    iov = np.zeros((len(writes), 2), np.uint64)
    iov[:, 0] = np.uint64(src.data_ptr()) + np.asarray([w[0] for w in writes], np.uint64)
    iov[:, 1] = np.asarray([w[1] for w in writes], np.uint64)
    dst = np.uint64(arena.data_ptr()) + np.asarray([w[2] for w in writes], np.uint64)
    delta = out_words(torch, len(writes), c64)
    ck.set_lanes_per_buffer(lanes)
    (ck.overwrite_batch64_iov if c64 else ck.overwrite_batch_iov)(_i64(torch, iov), _i64(torch, dst), len(writes),
                                                                  delta)
    torch.cuda.synchronize()
    check(words(delta, c64), want_deltas, arena, want_arena, writes, f"{IDS[c64]} {what} lanes {lanes}")
    return arena, want_arena


def placed(cases):
    """cases (source offset, length, (dst - src) % 16) -> writes, packed as tests/test_gpu_copy_crc64.py packs."""
    places, size = _place(cases)
    return [(so, n, at) for (so, n, _), at in zip(cases, places)], size


# ------------------------------------------------------------------ geometry

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_length_sweep_every_alignment(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    cases = []
    for n in range(401):
        for delta in range(16):
            so = 1024 * (len(cases) % 997) + (7 * n + delta) % 16   # co-aligned (delta 0) at every source offset
            cases.append((so, n, delta))
    writes, size = placed(cases)
    run_iov(torch, oracle, host, d, writes, size, 4, c64, "length sweep")


def row_cases(g, deltas):
    cases = []
    for k in range(2 * U + 4):
        for i, dd in enumerate((-17, -16, -1, 0, 1, 15, 16, 17)):
            n = k * 16 * g + dd
            if n < 0:
                continue
            for j, so in enumerate((0, 5, 15)):
                cases.append((4096 * (len(cases) % 61) + 16 * j + so, n, deltas[(3 * i + j + k) % len(deltas)]))
    return cases


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("deltas", [(0,), (1, 7, 8, 15)], ids=["coaligned", "misaligned"])
def test_rows_of_every_lane_group(dev_pool, oracle, g, deltas, c64):
    torch, host, d = dev_pool
    cases = row_cases(g, deltas)
    if len(deltas) > 1:
        assert {c[2] for c in cases if c[1] >= 64} == set(deltas)
    writes, size = placed(cases)
    run_iov(torch, oracle, host, d, writes, size, g, c64, "rows")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", [4, 8])
def test_packed_back_to_back(dev_pool, oracle, g, c64):
    # no padding between destinations: a tail and the next head share a 16-byte block
    torch, host, d = dev_pool
    rnd = random.Random(0xBAC + g)
    writes, pos = [], GUARD + 1
    for k in range(200):
        n = rnd.randrange(1, 301)
        so = 16 * rnd.randrange(0, 60000) + (pos % 16 if k % 4 else rnd.randrange(16))  # 3 of 4 co-aligned
        writes.append((so, n, pos))
        pos += n
    assert sum((at - so) % 16 == 0 for so, _, at in writes) >= 150
    assert any(at % 16 and (at - so) % 16 == 0 for so, _, at in writes)
    run_iov(torch, oracle, host, d, writes, pos + GUARD, g, c64, "packed")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_old_equals_new(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    cases = [(3000 * k + k % 16, n, (0, 0, 9)[k % 3]) for k, n in
             enumerate([0, 1, 63, 64, 65, 1000, 4096, 4097, 20000])]
    writes, size = placed(cases)
    _, old = expect(oracle, host, writes, old_bytes(size), c64)  # the source bytes already in place
    arena, want = run_iov(torch, oracle, host, d, writes, size, 0, c64, "old == new", old=old)
    assert np.array_equal(want, old)


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_single_flipped_bit(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    cases, flips = [], []
    for n in (1, 63, 64, 65, 1000, 4097):
        for where in (0, n // 2, n - 1):
            cases.append((5000 * len(cases) + len(cases) % 16, n, (0, 0, 5)[len(cases) % 3]))
            flips.append(where)
    writes, size = placed(cases)
    _, old = expect(oracle, host, writes, old_bytes(size), c64)
    for k, ((_, _, at), where) in enumerate(zip(writes, flips)):
        old[at + where] ^= 1 << (k % 8)
    crc = crc_of(oracle, c64)
    one_bit = [crc(bytes(w) + bytes([1 << (k % 8)]) + bytes(c[1] - 1 - w), 0) ^ crc(bytes(c[1]), 0)
               for k, (c, w) in enumerate(zip(cases, flips))]
    want_deltas, _ = expect(oracle, host, writes, old, c64)
    assert [int(x) for x in want_deltas] == one_bit  # the delta of one bit depends on its place alone
    run_iov(torch, oracle, host, d, writes, size, 0, c64, "flipped bit", old=old)


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("nbytes,src_stride,gap", [(100, 116, 0), (100, 4096, 0), (4096, 4096, 0), (1000, 1008, 37),
                                                   (0, 64, 16), (63, 64, 1), (8192, 8192 + 16, 48)])
def test_strided(dev_pool, oracle, nbytes, src_stride, gap, c64):
    torch, host, d = dev_pool
    count = 40
    dst_stride = nbytes + gap  # gap 0: packed
    writes = [(5 + k * src_stride, nbytes, GUARD + 5 + k * dst_stride) for k in range(count)]
    size = GUARD + 5 + count * dst_stride + GUARD
    old = old_bytes(size)
    want_deltas, want_arena = expect(oracle, host, writes, old, c64)
    arena = torch.from_numpy(old.copy()).cuda()
    delta = out_words(torch, count, c64)
    fn = ck.overwrite_batch64_strided if c64 else ck.overwrite_batch_strided
    fn(d.data_ptr() + 5, src_stride, arena.data_ptr() + GUARD + 5, dst_stride, nbytes, count, delta)
    torch.cuda.synchronize()
    check(words(delta, c64), want_deltas, arena, want_arena, writes, f"{IDS[c64]} strided {nbytes} B")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_pinned_host_source_and_sources_untouched(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    src = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    src.numpy()[:] = host
    assert src.data_ptr() % 16 == 0
    lens = [1, 63, 64, 4097, 70001]
    cases = [(80000 * k + (0, 3, 15)[k % 3], lens[k % 5], (0, 11)[k // 5 % 2]) for k in range(12)]
    writes, size = placed(cases)
    run_iov(torch, oracle, host, src, writes, size, 0, c64, "pinned source")
    assert np.array_equal(src.numpy(), host)
    run_iov(torch, oracle, host, d, writes, size, 0, c64, "device source")
    assert np.array_equal(d.cpu().numpy(), host)


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g,count,lo,hi", [(4, 1300, 0, 200), (32, 200, 2 * 16 * 32 - 40, 2 * 16 * 32 + 40)])
def test_several_grid_rounds(dev_pool, oracle, g, count, lo, hi, c64):
    torch, host, d = dev_pool
    rnd = random.Random(0x6F1D + g)
    cases = [(rnd.randrange(0, POOL - 2048), rnd.randrange(lo, hi + 1), 0 if k % 3 else rnd.randrange(16))
             for k in range(count)]
    writes, size = placed(cases)
    ck.set_batch_grid(2)
    assert count > 2 * 2 * 16 * (64 // g)  # more than two rounds of a 2-workgroup grid
    run_iov(torch, oracle, host, d, writes, size, g, c64, "grid rounds")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_graph_capture_two_replays(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    lens = [0, 1, 63, 64, 1000, 4097, 9000]
    cases = [(2048 * k + (0, 5, 15)[k % 3], lens[k % 7], (0, 6)[k // 7 % 2]) for k in range(40)]
    writes, size = placed(cases)
    old = old_bytes(size)
    want_deltas, want_arena = expect(oracle, host, writes, old, c64)
    d_old = torch.from_numpy(old.copy()).cuda()
    arena = d_old.clone()
    iov = np.zeros((len(writes), 2), np.uint64)
    iov[:, 0] = np.uint64(d.data_ptr()) + np.asarray([w[0] for w in writes], np.uint64)
    iov[:, 1] = np.asarray([w[1] for w in writes], np.uint64)
    d_iov = _i64(torch, iov)
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray([w[2] for w in writes], np.uint64))
    delta = out_words(torch, len(writes), c64)
    fn = ck.overwrite_batch64_iov if c64 else ck.overwrite_batch_iov
    fn(d_iov, d_dst, len(writes), delta)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn(d_iov, d_dst, len(writes), delta, stream=torch.cuda.current_stream())
    arena.copy_(d_old)
    delta.fill_(0x5A)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    check(words(delta, c64), want_deltas, arena, want_arena, writes, "first replay")
    delta.fill_(0x5A)
    g.replay()  # the bytes written over themselves
    torch.cuda.synchronize()
    check(words(delta, c64), np.zeros(len(writes), DT[c64]), arena, want_arena, writes, "second replay")


# ---------------------------------------------------------------- end to end

def e2e_writes(rnd, nblocks, bs):
    """48 non-overlapping writes (arena offsets from 0) as per-block pieces in address order: 46 inside
    quarter-block slots (every fifth ends on its slot's end, the first ones on a block's end) and one over
    two whole blocks, cut into two."""
    two = rnd.randrange(0, nblocks - 1)
    q = bs // 4
    slots = [(b, s) for b in range(nblocks) if b not in (two, two + 1) for s in range(4)]
    rnd.shuffle(slots)
    chosen = [(b, 3) for b in sorted({b for b, _ in slots})[:6]]  # six that can end on a block's end
    chosen += [s for s in slots if s not in chosen][:46 - len(chosen)]
    pieces = [(two * bs, bs), ((two + 1) * bs, bs)]
    for k, (b, s) in enumerate(chosen):
        lo, hi = b * bs + s * q, b * bs + (s + 1) * q
        a = rnd.randrange(lo, hi)
        e = hi if k % 5 == 0 or k < 6 else rnd.randrange(a + 1, hi + 1)
        pieces.append((a, e - a))
    pieces.sort()
    assert len(pieces) == 48 and sum((a + n) % bs == 0 for a, n in pieces) >= 8
    return pieces


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("nblocks,bs", [(64, 4096), (16, 65536)])
def test_end_to_end_blocks_and_object(dev_pool, oracle, nblocks, bs, c64):
    torch, host, d = dev_pool
    rnd = random.Random(0xE2E + nblocks)
    crc = crc_of(oracle, c64)
    total = nblocks * bs
    pieces = e2e_writes(rnd, nblocks, bs)
    # sources anywhere in the pool: most co-aligned with their destination, every fourth not
    writes = []
    for k, (a, n) in enumerate(pieces):
        so = 16 * rnd.randrange(0, (POOL - n) // 16 - 1) + ((GUARD + a) % 16 if k % 4 else rnd.randrange(16))
        writes.append((so, n, GUARD + a))
    size = total + 2 * GUARD
    old = old_bytes(size)
    want_deltas, want_arena = expect(oracle, host, writes, old, c64)
    blocks = lambda img: np.array([crc(img[GUARD + k * bs:GUARD + (k + 1) * bs], SEED) for k in range(nblocks)],
                                  DT[c64])
    obj = lambda img: np.array([crc(img[GUARD:GUARD + total], SEED)], DT[c64])

    n = len(writes)
    ends = np.array([a + m for a, m in pieces], np.uint64)
    blk = np.array([a // bs for a, _ in pieces])
    block_tail = (blk.astype(np.uint64) + np.uint64(1)) * np.uint64(bs) - ends
    object_tail = np.uint64(total) - ends
    block_start = np.searchsorted(blk, np.arange(nblocks + 1)).astype(np.uint64)
    assert np.count_nonzero(block_tail == 0) >= 8

    arena = torch.from_numpy(old.copy()).cuda()
    iov = np.zeros((n, 2), np.uint64)
    iov[:, 0] = np.uint64(d.data_ptr()) + np.asarray([w[0] for w in writes], np.uint64)
    iov[:, 1] = np.asarray([w[1] for w in writes], np.uint64)
    d_dst = _i64(torch, np.uint64(arena.data_ptr()) + np.asarray([w[2] for w in writes], np.uint64))
    delta = out_words(torch, n, c64)
    stored = dev_words(torch, blocks(old), c64)       # patched in place
    patched = out_words(torch, nblocks, c64)          # and into a second array
    obj_word = dev_words(torch, obj(old), c64)
    overwrite = ck.overwrite_batch64_iov if c64 else ck.overwrite_batch_iov
    patch = ck.patch64_device if c64 else ck.patch_device
    # overwrite -> patch (blocks) -> patch (object), one stream, no synchronisation in between
    overwrite(_i64(torch, iov), d_dst, n, delta)
    patch(delta, _i64(torch, block_tail), n, _i64(torch, block_start), nblocks, stored, patched)
    patch(delta, _i64(torch, block_tail), n, _i64(torch, block_start), nblocks, stored, stored)
    patch(delta, _i64(torch, object_tail), n, _i64(torch, [0, n]), 1, obj_word, obj_word)
    # freshly computed block CRCs against the patched words
    fresh = out_words(torch, nblocks, c64)
    (ck.batch64_strided if c64 else ck.batch_strided)(arena.data_ptr() + GUARD, bs, bs, nblocks, fresh, seed=SEED)
    report = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    work = torch.empty(max(int(ck.verify_work_bytes(nblocks)), 8), dtype=torch.uint8, device="cuda")
    (ck.verify64_device if c64 else ck.verify_device)(fresh, patched, 8 if c64 else 4, nblocks, report, None, 0, work)
    torch.cuda.synchronize()
    check(words(delta, c64), want_deltas, arena, want_arena, writes, "end to end")
    assert np.array_equal(words(patched, c64), blocks(want_arena))
    assert np.array_equal(words(stored, c64), blocks(want_arena))
    assert np.array_equal(words(obj_word, c64), obj(want_arena))
    rep = report.cpu().numpy().view(np.uint64)
    assert int(rep[0]) == 0 and int(rep[3]) == nblocks, rep


# -------------------------------------------------- patch_n against its replay

def device_patch(torch, c64, delta, tail, start, ntgt, crc_in, in_place=False):
    d_in = dev_words(torch, crc_in, c64)
    d_out = d_in if in_place else out_words(torch, ntgt, c64)
    (ck.patch64_device if c64 else ck.patch_device)(
        dev_words(torch, delta, c64) if len(delta) else None, _i64(torch, tail) if len(tail) else None, len(tail),
        None if start is None else _i64(torch, start), ntgt, d_in, d_out)
    return d_out


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_patch_device_equals_cpu_replay(oracle, c64):
    import torch
    runs = []
    for i, c in enumerate(fuzz_cases(oracle)):
        obj_start = np.array([0, len(c.pieces)], np.uint64)
        runs.append((c.delta[c64], c.block_tail, c.block_start, c.nblocks, c.block_old[c64], c.block_new[c64]))
        runs.append((c.delta[c64], c.object_tail, obj_start, 1, c.object_old[c64], c.object_new[c64]))
        if c.pieces:
            idx = [k for k, _, _ in c.pieces]
            runs.append((c.delta[c64], c.block_tail, None, len(idx), c.block_old[c64][idx], c.alone[c64]))
    deltas, tails, start, crc_in, want = large_tail_case(c64)
    runs.append((deltas, tails, start, 3, crc_in, want))
    outs = [device_patch(torch, c64, dl, tl, st, nt, ci, in_place=bool(k & 1))
            for k, (dl, tl, st, nt, ci, _) in enumerate(runs)]
    torch.cuda.synchronize()
    for k, ((dl, tl, st, nt, ci, want), out) in enumerate(zip(runs, outs)):
        got = words(out, c64)
        assert np.array_equal(got, replay(c64, dl, tl, st, nt, ci, 64)), k
        assert np.array_equal(got, want), k  # and the oracle's words (the multiply of test_patch_abi for the big tails)

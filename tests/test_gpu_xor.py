"""Stripe parity + CRC on the device (photon_crc32c_xor_batch_* /
photon_crc64ecma_xor_batch_*) and the expected parity word from stored block
CRCs (photon_crc32c_xor_expect_n / photon_crc64ecma_xor_expect_n), DESIGN.md
§4.16.

Expected values come from the pinned oracle (tests/_oracle.py) over host
copies, never from another call of this library: P = np.bitwise_xor.reduce of
the stripe's blocks, want = oracle.crc(P, seed). The parity arena holds known
pseudo-random old bytes and is compared WHOLE afterwards: parity ranges equal
P, every other byte -- guards, gaps and neighbours -- the old content; the
sources are compared untouched. The sizes are the geometry's edges (lane-group
rows, 16-byte blocks, the 64-byte tiny rule, chunks of sources, grid rounds),
not a workload's."""
import ctypes
import random

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_gpu_copy_crc import GUARD, _i64
from tests.test_gpu_copy_crc64 import _assert_disjoint, _first_diff
from tests.test_patch_abi import DT
from tests.test_xor_expect_abi import fuzz_cases, large_length_case, replay

pytestmark = pytest.mark.gpu

POOL = 1 << 20
GS = [4, 8, 16, 32, 64]
OLD_SEED = 0x0A71D
WIDTHS = [False, True]
IDS = ["crc32c", "crc64"]
IN_PLACE = "parity"  # a source that is the stripe's own parity range


def geometry():
    L = _native.lib()
    f, u, u64, m = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.photon_crc_xor_geometry(ctypes.addressof(f), ctypes.addressof(u), ctypes.addressof(u64),
                                     ctypes.addressof(m)) == 0
    return f.value, u.value, u64.value, m.value


@pytest.fixture(scope="module")
def dev_pool():
    import torch
    assert torch.cuda.is_available()
    host = datagen.stream_bytes(0x57A1E, POOL)
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
    """n CRC words on the device, pre-filled so that a word never written shows."""
    return torch.full((max(n, 1) * (8 if c64 else 4),), fill, dtype=torch.uint8, device="cuda")


def dev_words(torch, a, c64):
    return torch.from_numpy(np.ascontiguousarray(a, DT[c64]).view(np.uint8).copy()).cuda()


def old_bytes(size):
    return datagen.stream_bytes(OLD_SEED + size, size)


def seed_of(k, c64):
    s = (0x9E3779B97F4A7C15 * (k + 1)) & 0xFFFFFFFFFFFFFFFF
    return s if c64 else s >> 32


class Stripe:
    """srcs: pool offsets, None (a NULL source) or IN_PLACE; n bytes; res = the parity's address
    modulo 16, or `at` = its arena offset outright."""

    def __init__(self, srcs, n, res=0, at=None):
        self.srcs, self.n, self.res, self.at = list(srcs), n, res, at


def place(stripes):
    pos = GUARD
    for st in stripes:
        if st.at is None:
            pos += (st.res - pos) % 16
            st.at = pos
        assert st.at >= pos
        pos = st.at + st.n
    size = pos + GUARD
    _assert_disjoint([(st.at, st.n) for st in stripes], size)
    return size


def parity_of(host, old, st):
    p = np.zeros(st.n, np.uint8)
    for so in st.srcs:
        if so is None:
            continue
        p ^= old[st.at:st.at + st.n] if so is IN_PLACE else host[so:so + st.n]
    return p


def expect(oracle, host, old, stripes, seeds, c64):
    crc = crc_of(oracle, c64)
    want = old.copy()
    crcs = np.zeros(len(stripes), DT[c64])
    for i, st in enumerate(stripes):
        p = parity_of(host, old, st)
        crcs[i] = crc(p, int(seeds[i]))
        want[st.at:st.at + st.n] = p
    return crcs, want


def check(got, want_crcs, arena, want_arena, stripes, what):
    bad = np.flatnonzero(got != want_crcs)
    if bad.size:
        i = int(bad[0])
        st = stripes[i]
        raise AssertionError(f"{what}: CRC of stripe {i} (n {st.n}, at {st.at}, sources {st.srcs[:6]}) is "
                             f"{int(got[i]):#x}, want {int(want_crcs[i]):#x}; {bad.size} of {len(stripes)} differ")
    _first_diff(arena.cpu().numpy(), want_arena, what)


def ptr_args(torch, src, arena, stripes, k):
    ptrs = np.zeros((len(stripes), k), np.uint64)
    for i, st in enumerate(stripes):
        assert len(st.srcs) <= k
        for j, so in enumerate(st.srcs):
            if so is IN_PLACE:
                ptrs[i, j] = arena.data_ptr() + st.at
            elif so is not None:
                ptrs[i, j] = src.data_ptr() + so
    iov = np.zeros((len(stripes), 2), np.uint64)
    iov[:, 0] = np.uint64(arena.data_ptr()) + np.asarray([st.at for st in stripes], np.uint64)
    iov[:, 1] = np.asarray([st.n for st in stripes], np.uint64)
    return _i64(torch, ptrs), _i64(torch, iov)


def run_ptr(torch, oracle, host, src, stripes, k, lanes, c64, what="", one_seed=False):
    """One _ptr call over the stripes (each padded with NULL sources up to k), checked against the oracle."""
    size = place(stripes)
    old = old_bytes(size)
    n = len(stripes)
    seeds = np.array([seed_of(0 if one_seed else i, c64) for i in range(n)], DT[c64])
    want_crcs, want_arena = expect(oracle, host, old, stripes, seeds, c64)
    arena = torch.from_numpy(old.copy()).cuda()
    assert arena.data_ptr() % 16 == 0
    d_ptrs, d_iov = ptr_args(torch, src, arena, stripes, k)
    out = out_words(torch, n, c64)
    ck.set_lanes_per_buffer(lanes)
    fn = ck.xor_batch64_ptr if c64 else ck.xor_batch_ptr
    if one_seed:
        fn(d_ptrs, k, d_iov, n, out, seed=int(seeds[0]))
    else:
        fn(d_ptrs, k, d_iov, n, out, seeds=dev_words(torch, seeds, c64))
    torch.cuda.synchronize()
    check(words(out, c64)[:n], want_crcs, arena, want_arena, stripes, f"{IDS[c64]} {what} k {k} lanes {lanes}")
    return arena, want_arena


def sources(rnd, k, n, res, off=None):
    """k pool offsets congruent to res modulo 16 (off: {index: bytes off that residue})."""
    out = []
    for j in range(k):
        r = (res + (off or {}).get(j, 0)) % 16
        out.append(16 * rnd.randrange(0, (POOL - n) // 16 - 2) + r)
    return out


# ------------------------------------------------------------------ geometry

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_length_sweep_every_residue(dev_pool, oracle, k, c64):
    torch, host, d = dev_pool
    rnd = random.Random(0x5EE + k)
    stripes = [Stripe(sources(rnd, k, n, res), n, res) for n in range(401) for res in range(16)]
    run_ptr(torch, oracle, host, d, stripes, k, 4, c64, "length sweep")
    assert np.array_equal(d.cpu().numpy(), host)  # sources untouched


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", GS)
def test_rows_of_every_lane_group(dev_pool, oracle, g, c64):
    torch, host, d = dev_pool
    rnd = random.Random(0x0F0 + g)
    stripes = []
    for j in range(8):
        for i, dd in enumerate((0, 1, 15, 16 * g - 1)):
            n = j * 16 * g + dd
            stripes.append(Stripe(sources(rnd, 3, n, (5 * j + 3 * i) % 16), n, (5 * j + 3 * i) % 16))
    run_ptr(torch, oracle, host, d, stripes, 3, g, c64, "rows")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_source_counts_around_the_chunk(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    f, _, _, most = geometry()
    assert most == 64
    for k in sorted({1, 2, max(f - 1, 1), f, f + 1, 2 * f + 1, 17, 64}):
        for g in GS:
            rnd = random.Random(0xC0C + 64 * k + g)
            stripes = [Stripe(sources(rnd, k, n, res), n, res) for n, res in ((4096, 0), (4096, 9), (4096 + 33, 3))]
            run_ptr(torch, oracle, host, d, stripes, k, g, c64, "source counts")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", GS)
def test_one_source_not_coaligned(dev_pool, oracle, g, c64):
    # the slow route from 64 bytes on; below, byte by byte as every tiny stripe
    torch, host, d = dev_pool
    rnd = random.Random(0xA11 + g)
    stripes = []
    for n in (63, 64, 65, 4099):
        for i, by in enumerate((1, 7, 8, 15)):
            res = (3 * i + n) % 16
            stripes.append(Stripe(sources(rnd, 3, n, res, {i % 3: by}), n, res))
    stripes.append(Stripe(sources(rnd, 3, 4099, 4, {0: 5, 1: 9, 2: 13}), 4099, 4))  # the parity alone at its residue
    run_ptr(torch, oracle, host, d, stripes, 3, g, c64, "not co-aligned")
    assert np.array_equal(d.cpu().numpy(), host)


# -------------------------------------------------------------- NULL sources

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", [4, 16, 64])
def test_null_sources(dev_pool, oracle, g, c64):
    torch, host, d = dev_pool
    f = geometry()[0]
    k = f + 2  # NULLs in the first chunk and behind it
    rnd = random.Random(0x0011 + g)
    stripes = []
    # different n_s side by side: the lane groups of one wavefront diverge
    for i, n in enumerate((0, 1, 63, 64, 65, 1000, 4096, 4097, 300, 17, 5000, 64)):
        res = (7 * i) % 16
        src = sources(rnd, k, n, res)
        for hole in ((0,), (k // 2,), (k - 1,), (0, k - 1), tuple(range(k)), (1, 2, 3), ())[i % 7]:
            src[hole] = None
        stripes.append(Stripe(src, n, res))
    for n in (0, 10, 64, 4100):  # every source NULL: n zero bytes
        stripes.append(Stripe([None] * k, n, n % 16))
    assert any(all(s is None for s in st.srcs) and st.n >= 64 for st in stripes)
    run_ptr(torch, oracle, host, d, stripes, k, g, c64, "NULL sources")
    # a stripe shorter than k sources: the call pads with NULLs
    short = [Stripe(sources(rnd, j, 2000 + j, j), 2000 + j, j) for j in range(1, k)]
    run_ptr(torch, oracle, host, d, short, k, g, c64, "short stripes", one_seed=True)


# ------------------------------------------------------------------ in place

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", GS)
def test_in_place_accumulate(dev_pool, oracle, g, c64):
    torch, host, d = dev_pool
    f = geometry()[0]
    rnd = random.Random(0x19AC + g)
    stripes = []
    for k in (1, 2, 3, f + 2):
        for where in sorted({0, k // 2, k - 1}):
            for n in (1, 63, 64, 16 * g * 5 + 7, 4096):
                res = (n + where) % 16
                src = sources(rnd, k, n, res)
                src[where] = IN_PLACE
                stripes.append((k, Stripe(src, n, res)))
    # and on the slow route: another source off the parity's residue
    src = sources(rnd, 3, 4099, 6, {2: 3})
    src[0] = IN_PLACE
    stripes.append((3, Stripe(src, 4099, 6)))
    for k in sorted({k for k, _ in stripes}):
        run_ptr(torch, oracle, host, d, [st for kk, st in stripes if kk == k], k, g, c64, "in place")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_raid5_small_write(dev_pool, oracle, c64):
    # P' = P ^ D_old ^ D_new with k = 3 leaves the parity of the stripe with D_new in place of D_old
    torch, host, d = dev_pool
    crc = crc_of(oracle, c64)
    rnd = random.Random(0x5A1D)
    n, count = 4096, 24
    stripes, others, news = [], [], []
    for i in range(count):
        res = (5 * i) % 16
        old_d, new_d, other = sources(rnd, 3, n, res)
        stripes.append(Stripe([IN_PLACE, old_d, new_d], n, res))
        others.append(other)
        news.append(new_d)
    size = place(stripes)
    arena_old = old_bytes(size)
    for st, other in zip(stripes, others):  # the parity as it stands: D_old ^ the stripe's other data
        arena_old[st.at:st.at + n] = host[st.srcs[1]:st.srcs[1] + n] ^ host[other:other + n]
    seeds = np.array([seed_of(i, c64) for i in range(count)], DT[c64])
    want_crcs, want_arena = expect(oracle, host, arena_old, stripes, seeds, c64)
    for i, (st, other, new_d) in enumerate(zip(stripes, others, news)):
        p = host[new_d:new_d + n] ^ host[other:other + n]
        assert np.array_equal(want_arena[st.at:st.at + n], p)
        assert int(want_crcs[i]) == crc(p, int(seeds[i]))
    arena = torch.from_numpy(arena_old.copy()).cuda()
    d_ptrs, d_iov = ptr_args(torch, d, arena, stripes, 3)
    out = out_words(torch, count, c64)
    (ck.xor_batch64_ptr if c64 else ck.xor_batch_ptr)(d_ptrs, 3, d_iov, count, out, seeds=dev_words(torch, seeds, c64))
    torch.cuda.synchronize()
    check(words(out, c64), want_crcs, arena, want_arena, stripes, "small write")


# ----------------------------------------------------- packing, hosts, forms

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g", [4, 8])
def test_parities_packed_back_to_back(dev_pool, oracle, g, c64):
    # no padding between parities: a tail and the next head share a 16-byte block
    torch, host, d = dev_pool
    rnd = random.Random(0xBAC + g)
    stripes, pos = [], GUARD + 1
    for i in range(200):
        n = rnd.randrange(1, 301)
        src = sources(rnd, 3, n, pos % 16, None if i % 4 else {rnd.randrange(3): rnd.randrange(1, 16)})
        if i % 5 == 0:
            src[i % 3] = IN_PLACE
        stripes.append(Stripe(src, n, at=pos))
        pos += n
    assert any(st.at % 16 for st in stripes)
    run_ptr(torch, oracle, host, d, stripes, 3, g, c64, "packed")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_pinned_host_source(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    src = torch.empty(host.size, dtype=torch.uint8, pin_memory=True)
    src.numpy()[:] = host
    assert src.data_ptr() % 16 == 0
    rnd = random.Random(0x917)
    stripes = [Stripe(sources(rnd, 3, n, res, off), n, res)
               for n, res, off in ((1, 0, None), (63, 5, None), (64, 15, None), (4097, 3, None), (70001, 8, None),
                                   (4097, 2, {1: 11}))]
    run_ptr(torch, oracle, host, src, stripes, 3, 0, c64, "pinned source")
    assert np.array_equal(src.numpy(), host)


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("nbytes,k,block_gap,stripe_gap,dst_gap",
                         [(100, 4, 0, 0, 0), (4096, 4, 0, 0, 0), (4096, 8, 0, 0, 0), (1000, 3, 8, 40, 37),
                          (0, 2, 16, 16, 16), (63, 5, 1, 3, 1), (8192, 2, 16, 48, 48), (4099, 9, 13, 0, 0)])
def test_strided(dev_pool, oracle, nbytes, k, block_gap, stripe_gap, dst_gap, c64):
    torch, host, d = dev_pool
    count = 20
    block_stride = nbytes + block_gap           # gap 0: packed
    stripe_stride = k * block_stride + stripe_gap
    dst_stride = nbytes + dst_gap
    base = 5
    stripes = [Stripe([base + s * stripe_stride + i * block_stride for i in range(k)], nbytes,
                      at=GUARD + 5 + s * dst_stride) for s in range(count)]
    size = place(stripes)
    old = old_bytes(size)
    seeds = np.array([seed_of(i, c64) for i in range(count)], DT[c64])
    want_crcs, want_arena = expect(oracle, host, old, stripes, seeds, c64)
    arena = torch.from_numpy(old.copy()).cuda()
    out = out_words(torch, count, c64)
    fn = ck.xor_batch64_strided if c64 else ck.xor_batch_strided
    fn(d.data_ptr() + base, stripe_stride, block_stride, k, arena.data_ptr() + GUARD + 5, dst_stride, nbytes, count,
       out, seeds=dev_words(torch, seeds, c64))
    torch.cuda.synchronize()
    check(words(out, c64), want_crcs, arena, want_arena, stripes, f"{IDS[c64]} strided {nbytes} B k {k}")
    assert np.array_equal(d.cpu().numpy(), host)


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("g,count,lo,hi", [(4, 1300, 0, 200), (32, 200, 2 * 16 * 32 - 40, 2 * 16 * 32 + 40)])
def test_several_grid_rounds(dev_pool, oracle, g, count, lo, hi, c64):
    torch, host, d = dev_pool
    rnd = random.Random(0x6F1D + g)
    stripes = []
    for i in range(count):
        n, res = rnd.randrange(lo, hi + 1), rnd.randrange(16)
        src = sources(rnd, 3, n, res, None if i % 3 else {i % 2: 1 + i % 15})
        if i % 7 == 0:
            src[1] = None
        stripes.append(Stripe(src, n, res))
    ck.set_batch_grid(2)
    assert count > 2 * 2 * 16 * (64 // g)  # more than two rounds of a 2-workgroup grid
    run_ptr(torch, oracle, host, d, stripes, 3, g, c64, "grid rounds")


@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_graph_capture_two_replays(dev_pool, oracle, c64):
    torch, host, d = dev_pool
    rnd = random.Random(0x6A4)
    k, lens = 5, [0, 1, 63, 64, 1000, 4097, 9000]
    stripes = []
    for i in range(40):
        n, res = lens[i % 7], (3 * i) % 16
        stripes.append(Stripe(sources(rnd, k, n, res, None if i % 5 else {2: 6}), n, res))
    size = place(stripes)
    old = old_bytes(size)
    count = len(stripes)
    seeds = np.array([seed_of(i, c64) for i in range(count)], DT[c64])
    want_crcs, want_arena = expect(oracle, host, old, stripes, seeds, c64)
    d_old = torch.from_numpy(old.copy()).cuda()
    arena = d_old.clone()
    d_ptrs, d_iov = ptr_args(torch, d, arena, stripes, k)
    d_seeds = dev_words(torch, seeds, c64)
    out = out_words(torch, count, c64)
    # the expected words of the same stripes from the oracle's block CRCs (one seed: a stored CRC has one)
    crc = crc_of(oracle, c64)
    stored = np.array([crc(host[so:so + st.n], int(seeds[0])) for st in stripes for so in st.srcs], DT[c64])
    d_stored = dev_words(torch, stored, c64)
    d_lens = _i64(torch, [st.n for st in stripes])
    want = out_words(torch, count, c64)
    want_words = np.array([crc(parity_of(host, old, st), int(seeds[0])) for st in stripes], DT[c64])
    fn = ck.xor_batch64_ptr if c64 else ck.xor_batch_ptr
    ex = ck.xor_expect64_device if c64 else ck.xor_expect_device
    fn(d_ptrs, k, d_iov, count, out, seeds=d_seeds)  # first-call set-up
    ex(d_stored, stored.size, None, k, d_lens, 0, count, want, seed=int(seeds[0]))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn(d_ptrs, k, d_iov, count, out, seeds=d_seeds, stream=torch.cuda.current_stream())
        ex(d_stored, stored.size, None, k, d_lens, 0, count, want, seed=int(seeds[0]),
           stream=torch.cuda.current_stream())
    for rep in ("first replay", "second replay"):  # the second one writes the same parities again
        arena.copy_(d_old)
        out.fill_(0x5A)
        want.fill_(0x5A)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(words(out, c64), want_crcs, arena, want_arena, stripes, rep)
        assert np.array_equal(words(want, c64), want_words), rep


# ------------------------------------------- xor_expect_n against its replay

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
def test_expect_device_equals_cpu_replay(oracle, c64):
    import torch
    runs = []
    for c in fuzz_cases(oracle):
        runs.append((c.crcs[c64], c.start, 0, c.lens, 0, len(c.m), c.seed[c64], c.want[c64]))
        if c.k:
            runs.append((c.crcs[c64], None, c.k, c.lens, 0, len(c.m), c.seed[c64], c.want[c64]))
    wd, start, lens, seed, want = large_length_case(c64)
    runs.append((wd, start, 0, lens, 0, len(lens), seed, want))
    runs.append((wd[:8], None, 2, None, (1 << 40) + 12345, 4, seed, None))
    outs = []
    fn = ck.xor_expect64_device if c64 else ck.xor_expect_device
    for crcs, st, k, ln, nbytes, count, sd, _ in runs:
        out = out_words(torch, count, c64)
        fn(dev_words(torch, crcs, c64) if len(crcs) else None, len(crcs), None if st is None else _i64(torch, st), k,
           None if ln is None else _i64(torch, ln), nbytes, count, out, seed=sd)
        outs.append(out)
    torch.cuda.synchronize()
    for i, ((crcs, st, k, ln, nbytes, count, sd, want), out) in enumerate(zip(runs, outs)):
        got = words(out, c64)[:count]
        assert np.array_equal(got, replay(c64, crcs, st, k, ln, nbytes, count, sd)), i
        if want is not None:  # and the oracle's words (the multiply of test_patch_abi for the big lengths)
            assert np.array_equal(got, want), i


# ---------------------------------------------------------------- end to end

@pytest.mark.parametrize("c64", WIDTHS, ids=IDS)
@pytest.mark.parametrize("count,k,bs", [(16, 4, 4096), (4, 8, 65536)])
def test_end_to_end_encode_detect_rebuild(dev_pool, oracle, count, k, bs, c64):
    torch, host, d = dev_pool
    crc = crc_of(oracle, c64)
    seed = seed_of(7, c64)
    wb = 8 if c64 else 4
    h_data = datagen.stream_bytes(0xE2E0 + count, count * k * bs)   # count stripes of k blocks, packed
    data = torch.from_numpy(h_data.copy()).cuda()
    parity = torch.from_numpy(old_bytes(count * bs + 2 * GUARD)).cuda()
    h_blocks = h_data.reshape(count, k, bs)
    h_parity = np.bitwise_xor.reduce(h_blocks, axis=1)
    stored = np.array([crc(b, seed) for s in h_blocks for b in s], DT[c64])   # the store's block CRCs
    d_stored = dev_words(torch, stored, c64)
    verify = ck.verify64_device if c64 else ck.verify_device
    xor_strided = ck.xor_batch64_strided if c64 else ck.xor_batch_strided
    ex = ck.xor_expect64_device if c64 else ck.xor_expect_device
    work = torch.empty(max(int(ck.verify_work_bytes(count)), 8), dtype=torch.uint8, device="cuda")

    def encode_and_verify():
        out, want = out_words(torch, count, c64), out_words(torch, count, c64)
        report = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        bad = torch.full((count,), -1, dtype=torch.int64, device="cuda")
        # encode -> expected words -> verify: one stream, no synchronisation in between
        xor_strided(data, k * bs, bs, k, parity.data_ptr() + GUARD, bs, bs, count, out, seed=seed)
        ex(d_stored, stored.size, None, k, None, bs, count, want, seed=seed)
        verify(out, want, wb, count, report, bad, count, work)
        torch.cuda.synchronize()
        rep = report.cpu().numpy().view(np.uint64)
        return out, int(rep[0]), bad.cpu().numpy()

    out, nbad, _ = encode_and_verify()
    want_parity = np.array([crc(p, seed) for p in h_parity], DT[c64])
    assert np.array_equal(words(out, c64), want_parity)
    got = parity.cpu().numpy()
    want_arena = old_bytes(count * bs + 2 * GUARD)
    want_arena[GUARD:GUARD + count * bs] = h_parity.reshape(-1)
    _first_diff(got, want_arena, "encode")
    assert nbad == 0

    # stamp_n: the parity words into trailers behind a copy of each parity block
    trailers = torch.full((count * (bs + wb),), 0x33, dtype=torch.uint8, device="cuda")
    (ck.stamp64_device if c64 else ck.stamp_device)(out, count, trailers.data_ptr() + bs, bs + wb)
    torch.cuda.synchronize()
    tr = trailers.cpu().numpy().reshape(count, bs + wb)
    assert np.all(tr[:, :bs] == 0x33)
    assert np.array_equal(tr[:, bs:].copy().view(DT[c64]).reshape(-1), want_parity)

    # one bit flipped in one source of one stripe: verify lists exactly that stripe
    hit, blk = count // 2 + 1, k - 2
    at = (hit * k + blk) * bs + bs // 3
    data[at] ^= 0x10
    _, nbad, bad = encode_and_verify()
    assert nbad == 1 and int(bad[0]) == hit, (nbad, bad[:4])
    data[at] ^= 0x10

    # rebuild block `blk` of every stripe: survivors + parity into a scratch block
    encode_and_verify()
    scratch = torch.from_numpy(old_bytes(count * bs + 2 * GUARD)).cuda()
    ptrs = np.zeros((count, k), np.uint64)
    for s in range(count):
        survivors = [data.data_ptr() + (s * k + i) * bs for i in range(k) if i != blk]
        ptrs[s] = survivors + [parity.data_ptr() + GUARD + s * bs]
    iov = np.zeros((count, 2), np.uint64)
    iov[:, 0] = np.uint64(scratch.data_ptr() + GUARD) + np.arange(count, dtype=np.uint64) * np.uint64(bs)
    iov[:, 1] = bs
    out = out_words(torch, count, c64)
    report = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    lost = dev_words(torch, stored.reshape(count, k)[:, blk], c64)   # the lost blocks' stored words
    (ck.xor_batch64_ptr if c64 else ck.xor_batch_ptr)(_i64(torch, ptrs), k, _i64(torch, iov), count, out, seed=seed)
    verify(out, lost, wb, count, report, None, 0, work)
    torch.cuda.synchronize()
    want_arena = old_bytes(count * bs + 2 * GUARD)
    want_arena[GUARD:GUARD + count * bs] = h_blocks[:, blk, :].reshape(-1)
    _first_diff(scratch.cpu().numpy(), want_arena, "rebuild")
    rep = report.cpu().numpy().view(np.uint64)
    assert int(rep[0]) == 0 and int(rep[3]) == count, rep
    assert np.array_equal(data.cpu().numpy(), h_data)

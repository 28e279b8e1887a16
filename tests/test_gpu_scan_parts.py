"""Running CRCs of objects over their parts on the device
(photon_crc32c_scan_parts_n, photon_crc64ecma_scan_parts_n),
on the GPU, at tile 64 and at the default tile. Expected values: the pinned
oracle chained part by part over real bytes (run[s] = crc(part s, run[s - 1])
from the object's seed), and the bit-serial GF(2) chain of
tests/test_fold_parts_abi.py for pairs no buffer stands behind. Every output
array is pre-filled with 0xA5 bytes with 8 guard words on each side and
compared WHOLE (d_end untouched where it is not passed), the workspace is
exactly the bytes the call asks for with 64 guard bytes behind it, and the
inputs are compared afterwards."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_fold_parts_abi import BIG_LENS, CRCS, IDS, SEEDS, synthetic_pairs
from tests.test_gpu_fold_parts import Out, _dev, _same, many_objects  # noqa: F401 (many_objects: a fixture)
from tests.test_scan_parts_abi import (A5, Case, fixed_batch, geometry, gf_chain, real_cases, wdt, wrapped_ends)

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
WORK_GUARD = 64
TILE_IDS = ["tile 64", "default tile"]


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(params=[64, 0], ids=TILE_IDS)
def tile(request):
    ck.set_scan_tile(request.param)
    try:
        yield request.param
    finally:
        ck.set_scan_tile(0)


class Work:
    """A workspace of exactly the bytes the call asks for, full of 0xA5 (it needs no clearing), and 64
    guard bytes behind it."""

    def __init__(self, torch, nparts):
        self.need = ck.scan_work_bytes(nparts)
        self.t = torch.full((self.need + WORK_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        self.ptr = self.t.data_ptr()

    def check(self, what):
        assert bool((self.t[self.need:] == 0xA5).all()), f"{what}: written beyond work_bytes"


def _ptr(t):
    return t if t is None or isinstance(t, int) else t.data_ptr()


def _scan(c64, dc, dl, ds, nobj, nparts, run, work, seed=0, seeds=None, end=None, stream=None):
    f = ck.scan_parts64_device if c64 else ck.scan_parts_device
    f(_ptr(dc), _ptr(dl), _ptr(ds), nobj, nparts, run.ptr, work.ptr, work.need, seed=seed, seeds=_ptr(seeds),
      end=None if end is None else end.ptr, stream=stream)


class Dev:
    """The inputs of one call on the device."""

    def __init__(self, torch, c64, crcs, lens, start=None, seeds=None):
        self.c64, self.nparts = c64, len(lens)
        self.nobj = 1 if start is None else len(start) - 1
        self.host = [np.asarray(crcs, wdt(c64)), np.asarray(lens, np.uint64),
                     None if start is None else np.asarray(start, np.uint64),
                     None if seeds is None else np.asarray(seeds, wdt(c64))]
        self.dc, self.dl, self.ds, self.dseeds = (None if a is None else _dev(torch, a) for a in self.host)

    def run(self, torch, want, want_end, what, seed=0, per_object=False, with_end=True):
        run, end, work = Out(torch, self.nparts, wdt(self.c64)), Out(torch, self.nparts, np.uint64), \
            Work(torch, self.nparts)
        _scan(self.c64, self.dc, self.dl, self.ds, self.nobj, self.nparts, run, work, seed=seed,
              seeds=self.dseeds if per_object else None, end=end if with_end else None)
        torch.cuda.synchronize()
        run.check(want, what)
        end.check(want_end if with_end else [A5] * self.nparts, what + " (end)")
        work.check(what)
        return run, end

    def unchanged(self, what):
        for t, a in zip((self.dc, self.dl, self.ds, self.dseeds), self.host):
            if a is not None:
                _same(t, a, what)


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_real_parts(torch_dev, oracle, tile, c64):
    """Every object of real_shapes alone, both seeds, with and without d_end, with and without d_obj_start."""
    for k, case in enumerate(real_cases(oracle)):
        dev = Dev(torch_dev, c64, case.crc[c64], case.len, case.start if k % 2 else None)
        for seed in SEEDS[c64]:
            for with_end in (True, False):
                dev.run(torch_dev, case.want0[c64, seed], case.end, f"{case.name}, seed {seed:#x}", seed=seed,
                        with_end=with_end)
        dev.unchanged(case.name)


@pytest.fixture(scope="module")
def batch(oracle):
    return fixed_batch(oracle)


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_batch(torch_dev, batch, tile, c64):
    """The boundary cases of the CPU fuzz as one batch: empty objects first, in the middle and last."""
    dev = Dev(torch_dev, c64, batch.crc[c64], batch.len, batch.start, batch.seeds[c64])
    dev.run(torch_dev, batch.want[c64], batch.end, "batch, per-object seeds", seed=0x55, per_object=True)
    for seed in SEEDS[c64]:
        dev.run(torch_dev, batch.want0[c64, seed], batch.end, f"batch, seed {seed:#x}", seed=seed, with_end=False)
    dev.unchanged("batch")


@pytest.fixture(scope="module")
def many_case(oracle, many_objects):  # noqa: F811
    """many_objects of tests/test_gpu_fold_parts.py (4,099 objects of 0..33 parts of 0..40 bytes) with the
    oracle's running words from the same per-object seeds."""
    nobj, start, lens, totals, made = many_objects
    case = Case(oracle, "4,099 objects", start, lens, 0x0B1EC7, seeds={c64: made[c64][1] for c64 in CRCS})
    for c64 in CRCS:
        assert np.array_equal(case.crc[c64], made[c64][0])  # the same bytes
        for m, a, b in case.objects():
            if b > a:
                assert int(case.want[c64][b - 1]) == made[c64][2][m] and int(case.end[b - 1]) == totals[m]
    return case


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_many_objects(torch_dev, many_case, tile, c64):
    dev = Dev(torch_dev, c64, many_case.crc[c64], many_case.len, many_case.start, many_case.seeds[c64])
    dev.run(torch_dev, many_case.want[c64], many_case.end, "4,099 objects", per_object=True)
    dev.unchanged("4,099 objects")


@pytest.fixture(scope="module")
def big_object(oracle):
    """One object of tile_min * (grid_cap + 1) + 5 parts of 0..40 bytes, so that the reduce and apply steps'
    stride loops run at tile 64; its first tile_min * (chunk_tiles + 1) + 1 parts are the object whose carry
    crosses one chunk. Part CRCs and the oracle's running words from SEEDS[c64][1]."""
    _, chunk, cap = geometry()
    sizes = (64 * (chunk + 1) + 1, 64 * (cap + 1) + 5)
    lens = np.random.default_rng(0xB160B).integers(0, 41, sizes[1]).astype(np.uint64)
    lens[1000:1300] = 24  # a long run of equal lengths
    data = datagen.stream_bytes(0xB160B, int(lens.sum()))
    cuts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    made = {}
    for c64 in CRCS:
        crc = oracle.crc64ecma if c64 else oracle.crc32c
        parts, want, acc = np.zeros(lens.size, wdt(c64)), np.zeros(lens.size, wdt(c64)), SEEDS[c64][1]
        for s in range(lens.size):
            piece = data[cuts[s]:cuts[s + 1]]
            parts[s] = crc(piece, 0)
            acc = want[s] = crc(piece, acc)
        assert int(want[-1]) == crc(data, SEEDS[c64][1])
        made[c64] = (parts, want)
    return sizes, lens, cuts[1:].astype(np.uint64), made


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_one_big_object(torch_dev, big_object, tile, c64):
    sizes, lens, ends, made = big_object
    parts, want = made[c64]
    assert sizes[0] > 64 * geometry()[1] and sizes[1] > 64 * geometry()[2]
    for n in sizes:
        dev = Dev(torch_dev, c64, parts[:n], lens[:n])
        dev.run(torch_dev, want[:n], ends[:n], f"one object of {n} parts", seed=SEEDS[c64][1])
        dev.unchanged(f"one object of {n} parts")


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_synthetic_lengths(torch_dev, tile, c64):
    count = 150
    crcs, lens = synthetic_pairs(c64, count)
    assert all(n in lens for n in BIG_LENS)
    for start in ([0, count], [0, 20, 20, 65, count]):
        nobj = len(start) - 1
        seeds = np.array([SEEDS[c64][1] ^ (m * 0x01010101) for m in range(nobj)], wdt(c64))
        dev = Dev(torch_dev, c64, crcs, lens, start, seeds)
        ends = wrapped_ends(lens, start)
        for seed in SEEDS[c64]:
            dev.run(torch_dev, gf_chain(crcs, lens, start, [seed] * nobj, c64), ends,
                    f"lengths of 4 GiB and more, {nobj} objects, seed {seed:#x}", seed=seed)
        dev.run(torch_dev, gf_chain(crcs, lens, start, seeds, c64), ends, f"{nobj} objects, per-object seeds",
                per_object=True, with_end=False)
        dev.unchanged("synthetic")


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_agrees_with_fold(torch_dev, batch, many_case, tile, c64):
    """fold_parts_n on the same device arrays: its d_out = the last entries, its d_total = d_end there."""
    torch = torch_dev
    for case in (batch, many_case):
        dev = Dev(torch, c64, case.crc[c64], case.len, case.start, case.seeds[c64])
        run, end = dev.run(torch, case.want[c64], case.end, case.name, per_object=True)
        out, tot = Out(torch, case.nobj, wdt(c64)), Out(torch, case.nobj, np.uint64)
        (ck.fold_parts64_device if c64 else ck.fold_parts_device)(
            dev.dc, dev.dl, dev.ds, case.nobj, case.nparts, out.ptr, seeds=dev.dseeds, total=tot.ptr)
        torch.cuda.synchronize()
        got_run = run.t.cpu().numpy().view(wdt(c64))[8:-8]
        got_end = end.t.cpu().numpy().view(np.uint64)[8:-8]
        assert any(b == a for m, a, b in case.objects())  # there are empty objects: the fold gives their seed, the scan writes nothing
        out.check([int(got_run[b - 1]) if b > a else int(case.seeds[c64][m]) for m, a, b in case.objects()],
                  case.name + ": fold")
        tot.check([int(got_end[b - 1]) if b > a else 0 for m, a, b in case.objects()], case.name + ": fold totals")


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_object_path(torch_dev, oracle, tile, c64):
    """copy_parts_n of two objects of 12 parts of 64 KiB + 3 .. 1 MiB + 1 into one arena at an odd address,
    the scan, verify_n against the oracle's running words: one stream, nothing in between. Then with one source
    byte of part 7 flipped: entries 7..11 are bad, the second object stays clean."""
    torch = torch_dev
    crc = oracle.crc64ecma if c64 else oracle.crc32c
    w = 8 if c64 else 4
    sizes = [64 * KIB + 3 + k * ((MIB + 1 - 64 * KIB - 3) // 11) for k in range(11)] + [MIB + 1]
    lens = np.array(sizes * 2, np.uint64)
    nparts, total = 24, int(lens.sum())
    host = datagen.stream_bytes(0x0B1EC8, total)
    cuts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    seeds = np.array([SEEDS[c64][1], 0x1234567], wdt(c64))
    start = np.array([0, 12, 24], np.uint64)
    expected = np.zeros(nparts, wdt(c64))
    for m in range(2):
        acc = int(seeds[m])
        for s in range(12 * m, 12 * m + 12):
            acc = expected[s] = crc(host[cuts[s]:cuts[s + 1]], acc)
    src = torch.from_numpy(host).cuda()
    arena = torch.full((64 + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    at = 64 - 1 - (arena.data_ptr() + 64) % 2
    assert (arena.data_ptr() + at) % 2 == 1
    iov = np.array([[src.data_ptr() + int(cuts[s]), int(lens[s])] for s in range(nparts)], np.uint64)
    d_iov = torch.from_numpy(iov.view(np.int64)).cuda()
    d_dst = torch.from_numpy((arena.data_ptr() + at + cuts[:-1]).astype(np.int64)).cuda()
    d_len = torch.from_numpy(lens.view(np.int64)).pin_memory()     # read in place from pinned host memory
    d_start = torch.from_numpy(start.view(np.int64)).pin_memory()
    d_seeds, d_exp = _dev(torch, seeds), _dev(torch, expected)
    cap = MIB + 1
    pwork = torch.empty(ck.parts_work_bytes(nparts, cap, crc64=c64), dtype=torch.uint8, device="cuda")
    vwork = torch.full((ck.verify_work_bytes(nparts),), 0xA5, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    for flipped in (False, True):
        if flipped:
            src[int(cuts[7]) + 4099] ^= 0x10
        arena.fill_(0xA5)
        parts, run, end = Out(torch, nparts, wdt(c64)), Out(torch, nparts, wdt(c64)), Out(torch, nparts, np.uint64)
        rep, lst, work = Out(torch, 4, np.uint64), Out(torch, nparts, np.uint64), Work(torch, nparts)
        torch.cuda.synchronize()
        (ck.copy_parts64_device if c64 else ck.copy_parts_device)(d_iov, d_dst, nparts, cap, parts.ptr, pwork,
                                                                   stream=st)
        _scan(c64, parts.ptr, d_len, d_start, 2, nparts, run, work, seeds=d_seeds, end=end, stream=st)
        (ck.verify64_device if c64 else ck.verify_device)(run.ptr, d_exp, w, nparts, rep.ptr, lst.ptr, nparts,
                                                          vwork, stream=st)
        torch.cuda.synchronize()
        now = src.cpu().numpy()
        assert np.array_equal(arena.cpu().numpy()[at:at + total], now)
        parts.check([crc(now[cuts[s]:cuts[s + 1]], 0) for s in range(nparts)], "part CRCs")
        end.check([int(cuts[s + 1] - cuts[12 * (s // 12)]) for s in range(nparts)], "positions")
        work.check("object path")
        if not flipped:
            run.check(expected, "running CRCs")
            rep.check([0, (1 << 64) - 1, 0, nparts], "report")  # first_bad = ~0: none
            lst.check([A5] * nparts, "index list")
        else:
            got = run.t.cpu().numpy().view(wdt(c64))[8:-8]
            assert np.array_equal(got[:7], expected[:7]) and np.array_equal(got[12:], expected[12:])
            rep.check([5, 7, 5, nparts], "report, part 7 flipped")
            lst.check([7, 8, 9, 10, 11] + [A5] * (nparts - 5), "index list, part 7 flipped")
    _same(d_exp, expected, "expected words")
    assert list(d_len.numpy().view(np.uint64)) == list(lens) and list(d_start.numpy()) == [0, 12, 24]


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_streams(torch_dev, oracle, tile, c64):
    """Four streams, three calls each, every stream with its own outputs and workspace."""
    torch = torch_dev
    seed = SEEDS[c64][1]
    jobs = []
    for case in [c for c in real_cases(oracle) if c.nparts in (65, 257, 1000, 10007)]:
        jobs.append((case, Dev(torch, c64, case.crc[c64], case.len), Out(torch, case.nparts, wdt(c64)),
                     Out(torch, case.nparts, np.uint64), Work(torch, case.nparts), torch.cuda.Stream()))
    assert len(jobs) == 4
    torch.cuda.synchronize()
    for rep in range(3):
        for case, dev, run, end, work, st in jobs:
            _scan(c64, dev.dc, dev.dl, None, 1, case.nparts, run, work, seed=seed, end=end, stream=st)
    torch.cuda.synchronize()
    for case, dev, run, end, work, st in jobs:
        run.check(case.want0[c64, seed], case.name)
        end.check(case.end, case.name)
        work.check(case.name)
        dev.unchanged(case.name)


def test_graph_capture(torch_dev, oracle, tile):
    """A captured copy_extend64_device + scan pair, replayed twice over refilled sources: 130 parts already
    landed and the one the copy lands (three tiles of 64, so all three launches are captured at tile 64)."""
    torch = torch_dev
    n, nfirst = 1000013, 130
    flens = np.random.default_rng(0x6A9F).integers(1, 41, nfirst).astype(np.uint64)
    first = datagen.stream_bytes(0x6A9F, int(flens.sum()))
    fcuts = np.concatenate(([0], np.cumsum(flens))).astype(np.int64)
    crcs = np.array([oracle.crc64ecma(first[fcuts[s]:fcuts[s + 1]], 0) for s in range(nfirst)] + [0], np.uint64)
    lens = np.concatenate((flens, [n])).astype(np.uint64)
    nparts = nfirst + 1
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dc, dl = _dev(torch, crcs), _dev(torch, lens)
    last = dc.data_ptr() + 8 * nfirst  # written by the copy
    run, end, work = Out(torch, nparts, np.uint64), Out(torch, nparts, np.uint64), Work(torch, nparts)
    seed = SEEDS[True][1]
    ck.fill_splitmix(src, n, n, 1, 0x6A90)
    ck.copy_extend64_device(src.data_ptr(), dst.data_ptr() + 64, n, last)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream()
        ck.copy_extend64_device(src.data_ptr(), dst.data_ptr() + 64, n, last, stream=st)
        _scan(True, dc, dl, None, 1, nparts, run, work, seed=seed, end=end, stream=st)
    want, acc = [], seed
    for s in range(nfirst):
        acc = oracle.crc64ecma(first[fcuts[s]:fcuts[s + 1]], acc)
        want.append(acc)
    for rep in range(2):
        ck.fill_splitmix(src, n, n, 1, 0x6A91 + rep)
        dst.fill_(0xA5)
        run.refill()
        end.refill()
        work.t.fill_(0xA5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = src.cpu().numpy()
        assert np.array_equal(dst.cpu().numpy()[64:64 + n], host), rep
        run.check(want + [oracle.crc64ecma(host, acc)], f"replay {rep}")
        end.check(np.cumsum(lens), f"replay {rep} (end)")
        work.check(f"replay {rep}")
    _same(dl, lens, "graph")

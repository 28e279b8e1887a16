"""Fold of part CRCs into object CRCs on the device (photon_crc32c_fold_parts_n,
photon_crc64ecma_fold_parts_n), the CRC-64 series calls and their routing
(DESIGN.md §4.8), on the GPU. Expected values: the pinned oracle over real
bytes, and the bit-serial GF(2) reference of tests/test_fold_parts_abi.py
(pinned to the oracle there) for pairs no buffer stands behind. Every output
array is pre-filled with 0xA5 bytes with 8 guard words on each side and
compared WHOLE; the inputs are compared afterwards."""
import ctypes

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_fold_parts_abi import (BIG_LENS, CRCS, IDS, SEEDS, Shape, gf_fold, real_shapes, synthetic_pairs)

pytestmark = pytest.mark.gpu

GUARDW = 8
MIB = 1 << 20


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def shapes(oracle):
    return real_shapes(oracle)


def _wdt(crc64):
    return np.uint64 if crc64 else np.uint32


def _dev(torch, arr):
    """A host array of unsigned words on the device (as bytes: torch has no unsigned words)."""
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda() if arr.size else \
        torch.empty(16, dtype=torch.uint8, device="cuda")


def _same(t, arr, what):
    arr = np.ascontiguousarray(arr)
    if arr.size:
        assert np.array_equal(t.cpu().numpy(), arr.view(np.uint8).reshape(-1)), f"{what}: the input changed"


class Out:
    """n output words of `dtype` between two guards of 8 words, everything 0xA5."""

    def __init__(self, torch, n, dtype, pinned=False):
        self.n, self.dtype, self.w = n, np.dtype(dtype), np.dtype(dtype).itemsize
        size = (n + 2 * GUARDW) * self.w
        self.t = torch.empty(size, dtype=torch.uint8, pin_memory=True) if pinned else \
            torch.empty(size, dtype=torch.uint8, device="cuda")
        self.t.fill_(0xA5)
        self.ptr = self.t.data_ptr() + GUARDW * self.w

    def refill(self):
        self.t.fill_(0xA5)

    def check(self, want, what):
        """The whole array: the guards untouched, the n words equal to want."""
        got = self.t.cpu().numpy().view(self.dtype)
        full = np.full(self.n + 2 * GUARDW, 0xA5A5A5A5A5A5A5A5 & ((1 << (8 * self.w)) - 1), self.dtype)
        full[GUARDW:GUARDW + self.n] = np.asarray(want, self.dtype)
        bad = np.nonzero(got != full)[0]
        assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {int(bad[0]) - GUARDW}: "
                               f"{int(got[bad[0]]):#x}, want {int(full[bad[0]]):#x}")


def _fold(crc64, crcs, lens, start, nobj, nparts, out, seed=0, seeds=None, total=None, stream=None):
    f = ck.fold_parts64_device if crc64 else ck.fold_parts_device
    f(crcs, lens, start, nobj, nparts, out, seed=seed, seeds=seeds, total=total, stream=stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _one_object(torch, crc64, crcs, lens, seed, want, want_total, what, with_total=True):
    n = len(lens)
    dc, dl = _dev(torch, np.asarray(crcs, _wdt(crc64))), _dev(torch, np.asarray(lens, np.uint64))
    out, tot = Out(torch, 1, _wdt(crc64)), Out(torch, 1, np.uint64)
    _fold(crc64, _ptr(dc) if n else None, _ptr(dl) if n else None, None, 1, n, out.ptr, seed=seed,
          total=tot.ptr if with_total else None)
    torch.cuda.synchronize()
    out.check([want], what)
    tot.check([want_total] if with_total else [0xA5A5A5A5A5A5A5A5], what + " (total)")
    _same(dc, np.asarray(crcs, _wdt(crc64)), what)
    _same(dl, np.asarray(lens, np.uint64), what)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_real_parts(torch_dev, shapes, crc64):
    torch = torch_dev
    s0, s1 = SEEDS[crc64]
    for sh in shapes:
        _one_object(torch, crc64, sh.crc[crc64], sh.len, s0, sh.want[crc64, s0], sh.total, sh.name)
        _one_object(torch, crc64, sh.crc[crc64], sh.len, s1, sh.want[crc64, s1], sh.total, sh.name + ", seeded",
                    with_total=False)
    # all of them as one batch; empty objects first, in the middle and last
    empty = next(sh for sh in shapes if sh.len.size == 0)
    objs = [empty] + list(shapes[:6]) + [empty] + list(shapes[6:]) + [empty]
    nobj = len(objs)
    crcs = np.concatenate([o.crc[crc64] for o in objs])
    lens = np.concatenate([o.len for o in objs])
    start = np.concatenate(([0], np.cumsum([o.len.size for o in objs]))).astype(np.uint64)
    seeds = np.array([(s1, s0, s1)[m % 3] for m in range(nobj)], _wdt(crc64))
    dc, dl, ds, dseeds = (_dev(torch, a) for a in (crcs, lens, start, seeds))
    totals = [o.total for o in objs]
    for what, seed, dsd, with_total in (("per-object seeds", 0, dseeds, True),
                                        ("seed0", s1, None, False),
                                        ("seed 0", 0, None, True)):
        out, tot = Out(torch, nobj, _wdt(crc64)), Out(torch, nobj, np.uint64)
        _fold(crc64, _ptr(dc), _ptr(dl), _ptr(ds), nobj, lens.size, out.ptr, seed=seed, seeds=_ptr(dsd),
              total=tot.ptr if with_total else None)
        torch.cuda.synchronize()
        want = [o.want[crc64, int(seeds[m]) if dsd is not None else seed] for m, o in enumerate(objs)]
        assert want[0] == (int(seeds[0]) if dsd is not None else seed)  # an empty object gives its seed
        out.check(want, "batch, " + what)
        tot.check(totals if with_total else [0xA5A5A5A5A5A5A5A5] * nobj, "batch totals, " + what)
    for t, a in ((dc, crcs), (dl, lens), (ds, start), (dseeds, seeds)):
        _same(t, a, "batch")


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_synthetic_lengths(torch_dev, crc64):
    crcs, lens = synthetic_pairs(crc64)
    assert all(n in lens for n in BIG_LENS)
    total = int(lens.astype(object).sum()) % (1 << 64)
    for seed in SEEDS[crc64]:
        _one_object(torch_dev, crc64, crcs, lens, seed, gf_fold(crcs, lens, seed, crc64), total,
                    f"lengths of 4 GiB and more, seed {seed:#x}")
    # two objects of them, and one part of 4 GiB + 5 alone
    cut = 20
    dc, dl = _dev(torch_dev, crcs), _dev(torch_dev, lens)
    ds = _dev(torch_dev, np.array([0, cut, cut, lens.size], np.uint64))
    out = Out(torch_dev, 3, _wdt(crc64))
    seed = SEEDS[crc64][1]
    _fold(crc64, _ptr(dc), _ptr(dl), _ptr(ds), 3, lens.size, out.ptr, seed=seed)
    torch_dev.cuda.synchronize()
    out.check([gf_fold(crcs[:cut], lens[:cut], seed, crc64), seed, gf_fold(crcs[cut:], lens[cut:], seed, crc64)],
              "three objects")
    _one_object(torch_dev, crc64, crcs[:1], lens[5:6], seed, gf_fold(crcs[:1], lens[5:6], seed, crc64),
                BIG_LENS[2], "one part of 4 GiB + 5")


@pytest.fixture(scope="module")
def many_parts(oracle):
    return Shape(oracle, 70001, "mixed", 200)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_many_parts(torch_dev, many_parts, crc64):
    # more parts than threads of any workgroup: every thread folds a run of 69 (the last ones fewer)
    sh = many_parts
    for seed in SEEDS[crc64]:
        _one_object(torch_dev, crc64, sh.crc[crc64], sh.len, seed, sh.want[crc64, seed], sh.total,
                    f"{sh.name}, seed {seed:#x}")


@pytest.fixture(scope="module")
def many_objects(oracle):
    """4,099 objects of 0..33 parts of 0..40 bytes over one byte stream: the
    part CRCs and, per object and CRC, the oracle's CRC from the object's seed."""
    rng = np.random.default_rng(0x0B1EC7)
    nobj = 4099
    counts = rng.integers(0, 34, nobj)
    counts[:34] = np.arange(34)
    start = np.concatenate(([0], np.cumsum(counts))).astype(np.uint64)
    lens = rng.integers(0, 41, int(start[-1])).astype(np.uint64)
    data = datagen.stream_bytes(0x0B1EC7, int(lens.sum()))
    cuts = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    made = {}
    for c64 in CRCS:
        crc = oracle.crc64ecma if c64 else oracle.crc32c
        parts = np.array([crc(data[cuts[s]:cuts[s + 1]], 0) for s in range(lens.size)], _wdt(c64))
        seeds = rng.integers(0, 1 << 32, nobj, dtype=np.uint64).astype(_wdt(c64)) * _wdt(c64)(3)
        want = [crc(data[cuts[int(start[m])]:cuts[int(start[m + 1])]], int(seeds[m])) for m in range(nobj)]
        made[c64] = (parts, seeds, want)
    totals = [int(cuts[int(start[m + 1])] - cuts[int(start[m])]) for m in range(nobj)]
    return nobj, start, lens, totals, made


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_many_objects(torch_dev, many_objects, crc64):
    torch = torch_dev
    nobj, start, lens, totals, made = many_objects
    parts, seeds, want = made[crc64]
    dc, dl, ds, dseeds = (_dev(torch, a) for a in (parts, lens, start, seeds))
    out, tot = Out(torch, nobj, _wdt(crc64)), Out(torch, nobj, np.uint64)
    _fold(crc64, _ptr(dc), _ptr(dl), _ptr(ds), nobj, lens.size, out.ptr, seeds=_ptr(dseeds), total=tot.ptr)
    torch.cuda.synchronize()
    out.check(want, "4,099 objects")
    tot.check(totals, "4,099 objects (totals)")
    # a sample folded one call each: the same words
    w = np.dtype(_wdt(crc64)).itemsize
    sample = list(range(0, 34, 3)) + list(range(4099 - 52, 4099))
    assert len(sample) == 64
    single = Out(torch, len(sample), _wdt(crc64))
    for k, m in enumerate(sample):
        a, b = int(start[m]), int(start[m + 1])
        _fold(crc64, dc.data_ptr() + a * w if b > a else None, dl.data_ptr() + a * 8 if b > a else None, None, 1,
              b - a, single.ptr + k * w, seed=int(seeds[m]))
    torch.cuda.synchronize()
    single.check([want[m] for m in sample], "one call per object")
    for t, a in ((dc, parts), (dl, lens), (ds, start), (dseeds, seeds)):
        _same(t, a, "4,099 objects")


def _copy_extend(crc64, src, dst, n, out, stream):
    if crc64:
        ck.copy_extend64_device(src, dst, n, out, seed=0, stream=stream)
    else:
        ck.copy_extend_device(src, dst, n, 0, out, stream=stream)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_after_copy_extend(torch_dev, oracle, crc64):
    """The object path: one copy + CRC call per part (seed 0) into one
    destination at an odd address, then ONE fold on the same stream with
    nothing in between; the lengths are read from pinned host memory."""
    torch = torch_dev
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    lens = [MIB + 3, 65539, 2 * MIB + 1]
    hosts = [datagen.stream_bytes(0xF0B0 + k, n) for k, n in enumerate(lens)]
    srcs = [torch.from_numpy(h).cuda() for h in hosts]
    total = sum(lens)
    arena = torch.full((64 + total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    at = 64 - 1 - (arena.data_ptr() + 64) % 2
    assert (arena.data_ptr() + at) % 2 == 1 and at >= 62
    w = 8 if crc64 else 4
    dlen = torch.from_numpy(np.array(lens, np.int64)).pin_memory()
    whole = np.concatenate(hosts)
    st = torch.cuda.Stream()
    for seed in SEEDS[crc64]:
        arena.fill_(0xA5)
        parts, out, tot = Out(torch, 3, _wdt(crc64)), Out(torch, 1, _wdt(crc64)), Out(torch, 1, np.uint64)
        torch.cuda.synchronize()
        pos = at
        for k, (src, n) in enumerate(zip(srcs, lens)):
            _copy_extend(crc64, src.data_ptr(), arena.data_ptr() + pos, n, parts.ptr + k * w, st)
            pos += n
        _fold(crc64, parts.ptr, dlen.data_ptr(), None, 1, 3, out.ptr, seed=seed, total=tot.ptr, stream=st)
        torch.cuda.synchronize()
        got = arena.cpu().numpy()
        assert np.array_equal(got[at:at + total], whole)
        assert (got[:at] == 0xA5).all() and (got[at + total:] == 0xA5).all()
        parts.check([crc(h, 0) for h in hosts], "part CRCs")
        out.check([crc(got[at:at + total], seed)], f"object CRC, seed {seed:#x}")
        tot.check([total], "object bytes")
        assert list(dlen.numpy()) == lens
    for src, h in zip(srcs, hosts):
        assert np.array_equal(src.cpu().numpy(), h)


def test_series64(torch_dev, oracle):
    torch = torch_dev
    # series: one pool of 1,000 parts of 65,539 bytes + 5, filled on the device
    pool_n = 65539 * 1000 + 5
    pool = torch.empty(pool_n, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(pool, pool_n, pool_n, 1, 0x5E71E5)
    torch.cuda.synchronize()
    host = pool.cpu().numpy()
    for off in (0, 5):
        for ps in (0, 1, 7, 8, 510, 4096, 65539):
            for n in (1, 10, 1000):
                out = Out(torch, n, np.uint64)
                ck.series64_device(pool.data_ptr() + off, ps, n, out.ptr)
                torch.cuda.synchronize()
                want = oracle.crc64ecma_strided(host[off:], ps, ps, n, 0)
                out.check(want, f"series64 of {n} parts of {ps} bytes at offset {off}")
    untouched = Out(torch, 4, np.uint64)
    ck.series64_device(pool.data_ptr(), 8, 0, untouched.ptr)  # n_parts == 0: nothing is touched
    ck.series64_device(None, 0, 4, untouched.ptr)             # part_size == 0: zeros, nothing is read
    torch.cuda.synchronize()
    untouched.check([0, 0, 0, 0], "series64 of empty parts")
    assert np.array_equal(pool.cpu().numpy(), host)
    # combine_series: against the host drop-in, and against the oracle over the bytes
    rng = np.random.default_rng(0xC0B1)
    for ps in (0, 1, 510):
        for n in (0, 1, 2, 16, 17, 4096, 100003):
            if ps:
                crcs = oracle.crc64ecma_strided(host, ps, ps, n, 0)
            else:
                crcs = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
            want = ck.crc64ecma_combine_series([int(c) for c in crcs], ps)
            if ps:
                assert want == oracle.crc64ecma(host[:ps * n], 0), (ps, n)
            dc = _dev(torch, crcs)
            res = Out(torch, 1, np.uint64)
            ck.combine_series64_device(_ptr(dc) if n else None, ps, n, res.ptr)
            torch.cuda.synchronize()
            res.check([want], f"combine_series64 of {n} parts of {ps} bytes")
            _same(dc, crcs, "combine_series64")
    # leading CRCs of 0 (combine64's crc1 == 0 shortcut agrees with the formula)
    crcs = rng.integers(0, 1 << 63, 300, dtype=np.uint64)
    crcs[:37] = 0
    dc, res = _dev(torch, crcs), Out(torch, 1, np.uint64)
    ck.combine_series64_device(dc, 77, 300, res.ptr)
    torch.cuda.synchronize()
    res.check([ck.crc64ecma_combine_series([int(c) for c in crcs], 77)], "leading zero CRCs")


def _slots():
    L = _native.lib()
    return L.auto["crc64ecma_series_auto"].value, L.auto["crc64ecma_combine_series_auto"].value


def test_routed(torch_dev, oracle, capfd):
    torch = torch_dev
    ps, n = 510, 4099
    d = torch.empty(ps * n + 5, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(d, d.numel(), d.numel(), 1, 0x2007ED)
    torch.cuda.synchronize()
    host = d.cpu().numpy()[5:]
    want = ck.crc64ecma_series(host, ps, n)          # the host engines on the host copy
    want_all = ck.crc64ecma_combine_series(want, ps)
    assert want == list(oracle.crc64ecma_strided(host, ps, ps, n, 0)) and want_all == oracle.crc64ecma(host, 0)
    old = _slots()
    fb0 = ck.dispatch_fallbacks()
    ck.set_device_dispatch(True)
    failed = False
    try:
        assert _slots() != old and old[0] not in _slots() and old[1] not in _slots()
        for inject in (0, 1):
            out_d, out_h = Out(torch, n, np.uint64), np.full(n + 2, 0xA5A5A5A5A5A5A5A5, np.uint64)
            ck.inject_failures(inject)
            ck.crc64ecma_series_at(d.data_ptr() + 5, ps, n, out_d.ptr)        # parts on the device
            out_d.check(want, f"routed series, parts on the device, {inject} failures")
            ck.inject_failures(inject)
            ck.crc64ecma_series_at(d.data_ptr() + 5, ps, n, out_h.ctypes.data + 8)  # parts on the host
            assert list(out_h[1:-1]) == want and out_h[0] == out_h[-1] == 0xA5A5A5A5A5A5A5A5
            ck.inject_failures(inject)
            assert ck.crc64ecma_combine_series_at(out_d.ptr, ps, n) == want_all
            assert ck.dispatch_fallbacks() == fb0 + 3 * inject
            failed = failed or bool(inject)
        # host pointers go to the saved host engine
        hbuf = np.ascontiguousarray(host[:ps * 7])
        hout = np.zeros(7, np.uint64)
        ck.crc64ecma_series_at(hbuf.ctypes.data, ps, 7, hout.ctypes.data)
        assert list(hout) == want[:7]
        assert ck.crc64ecma_combine_series_at(hout.ctypes.data, ps, 7) == oracle.crc64ecma(hbuf, 0)
        assert ck.dispatch_fallbacks() == fb0 + 3
    finally:
        ck.inject_failures(0)
        if failed:
            with pytest.raises(ck.CrcError) as e:  # -EIO once: the sticky flag of the failed calls
                ck.set_device_dispatch(False)
            assert e.value.code == -5
        else:
            ck.set_device_dispatch(False)
    ck.set_device_dispatch(True)
    ck.set_device_dispatch(False)  # and clean the second time
    assert _slots() == old
    assert capfd.readouterr().err.count("recomputing on the host") == 3
    assert np.array_equal(d.cpu().numpy()[5:], host)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_streams(torch_dev, shapes, crc64):
    # four streams, three launches each, every stream with its own outputs
    torch = torch_dev
    jobs = []
    for k, sh in enumerate([s for s in shapes if s.len.size in (65, 257, 1000, 10007)]):
        jobs.append((sh, _dev(torch, sh.crc[crc64]), _dev(torch, sh.len), Out(torch, 1, _wdt(crc64)),
                     Out(torch, 1, np.uint64), torch.cuda.Stream()))
    assert len(jobs) == 4
    seed = SEEDS[crc64][1]
    torch.cuda.synchronize()
    for rep in range(3):
        for sh, dc, dl, out, tot, st in jobs:
            _fold(crc64, _ptr(dc), _ptr(dl), None, 1, sh.len.size, out.ptr, seed=seed, total=tot.ptr, stream=st)
    torch.cuda.synchronize()
    for sh, dc, dl, out, tot, st in jobs:
        out.check([sh.want[crc64, seed]], sh.name)
        tot.check([sh.total], sh.name)
        _same(dc, sh.crc[crc64], sh.name)
        _same(dl, sh.len, sh.name)


def test_graph_capture(torch_dev, oracle):
    """A captured copy_extend64_device + fold pair, replayed twice over refilled sources."""
    torch = torch_dev
    n, prefix = 1000013, 4097
    src = torch.empty(n, dtype=torch.uint8, device="cuda")
    dst = torch.full((64 + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    first = datagen.stream_bytes(0x6A9F, prefix)                 # the object's first part, already landed
    crcs = np.array([oracle.crc64ecma(first, 0), 0], np.uint64)  # [1] is written by the copy
    lens = np.array([prefix, n], np.uint64)
    dc, dl = _dev(torch, crcs), _dev(torch, lens)
    out, tot = Out(torch, 1, np.uint64), Out(torch, 1, np.uint64)
    seed = SEEDS[True][1]
    ck.fill_splitmix(src, n, n, 1, 0x6A90)
    ck.copy_extend64_device(src.data_ptr(), dst.data_ptr() + 64, n, dc.data_ptr() + 8)  # first-call set-up
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream()
        ck.copy_extend64_device(src.data_ptr(), dst.data_ptr() + 64, n, dc.data_ptr() + 8, stream=st)
        ck.fold_parts64_device(dc.data_ptr(), dl.data_ptr(), None, 1, 2, out.ptr, seed=seed, total=tot.ptr, stream=st)
    for rep in range(2):
        ck.fill_splitmix(src, n, n, 1, 0x6A91 + rep)
        dst.fill_(0xA5)
        out.refill()
        tot.refill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = src.cpu().numpy()
        assert np.array_equal(dst.cpu().numpy()[64:64 + n], host), rep
        out.check([oracle.crc64ecma(np.concatenate((first, host)), seed)], f"replay {rep}")
        tot.check([prefix + n], f"replay {rep} (total)")
    _same(dl, lens, "graph")

"""Stored CRCs checked on the device (photon_crc32c_verify_n / _verify_ptr_n /
_stamp_n / _stamp_ptr_n and the CRC-64 forms), on the GPU.
Expected values: the numpy reference of tests/test_verify_abi.py
(np.nonzero(crc != expected)) over its counts, bad patterns, caps and
layouts, and the pinned oracle over real bytes for the end-to-end trailer
layouts. Every output array is pre-filled with 0xA5 bytes with 8 guard words
on each side and compared WHOLE; the inputs are compared afterwards."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_verify_abi import (A5, CRCS, DEFAULT_TILE, IDS, LAYOUTS, NONE, PATTERNS, Layout, caps, layout_counts,
                                   make_case, want_report, wdt, width)

pytestmark = pytest.mark.gpu

GUARDW = 8


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture
def tile_setter():
    yield ck.set_verify_tile
    ck.set_verify_tile(0)


def _dev(torch, arr):
    """A host array on the device, as bytes (torch has no unsigned words)."""
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


def _same(t, arr, what):
    assert np.array_equal(t.cpu().numpy(), np.ascontiguousarray(arr).view(np.uint8).reshape(-1)), \
        f"{what}: the input changed"


class Out:
    """n output words of 64 bits between two guards of 8 words, everything 0xA5."""

    def __init__(self, torch, n, pinned=False):
        self.n = n
        size = (n + 2 * GUARDW) * 8
        self.t = torch.empty(size, dtype=torch.uint8, pin_memory=True) if pinned else \
            torch.empty(size, dtype=torch.uint8, device="cuda")
        self.t.fill_(0xA5)
        self.ptr = self.t.data_ptr() + GUARDW * 8

    def refill(self):
        self.t.fill_(0xA5)

    def check(self, want, what):
        """The whole array: the guards untouched, the first len(want) words equal to want, the rest 0xA5."""
        got = self.t.cpu().numpy().view(np.uint64)
        full = np.full(self.n + 2 * GUARDW, A5, np.uint64)
        full[GUARDW:GUARDW + len(want)] = np.asarray(want, np.uint64)
        bad = np.nonzero(got != full)[0]
        assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {int(bad[0]) - GUARDW}: "
                               f"{int(got[bad[0]]):#x}, want {int(full[bad[0]]):#x}")


def _work(torch, count):
    """A workspace of exactly the bytes the call asks for, full of 0xA5: it needs no clearing."""
    return torch.full((ck.verify_work_bytes(count),), 0xA5, dtype=torch.uint8, device="cuda")


def _verify(c64, d_crc, lay, d_buf, d_ptrs, count, rep, lst, cap, work, stream=None):
    if lay.stride is None:
        (ck.verify64_ptr_device if c64 else ck.verify_ptr_device)(
            d_crc, d_ptrs, count, rep.ptr, lst.ptr if cap else None, cap, work, stream=stream)
    else:
        (ck.verify64_device if c64 else ck.verify_device)(
            d_crc, d_buf.data_ptr() + int(lay.off[0]), lay.stride, count, rep.ptr, lst.ptr if cap else None, cap,
            work, stream=stream)


class Case:
    """One case of tests/test_verify_abi.py on the device."""

    def __init__(self, torch, c64, layout, count, pattern, tile):
        probe = Layout(layout, c64, count, 0)
        self.d_buf = torch.empty(probe.size + 1, dtype=torch.uint8, device="cuda")
        self.crc, exp, self.lay, self.ref = make_case(c64, layout, count, pattern, tile, self.d_buf.data_ptr())
        self.image = np.full(probe.size + 1, 0xA5, np.uint8)
        self.image[:self.lay.size] = self.lay.image(exp)
        self.d_buf.copy_(torch.from_numpy(self.image))
        self.d_crc = _dev(torch, self.crc)
        self.ptrs = self.lay.pointers(self.d_buf.data_ptr()) if self.lay.stride is None else None
        self.d_ptrs = _dev(torch, self.ptrs) if self.ptrs is not None else None
        self.c64, self.count = c64, count
        self.what = f"{count} entries, {pattern}, {layout}"

    def run(self, rep, lst, cap, work, stream=None):
        _verify(self.c64, self.d_crc, self.lay, self.d_buf, self.d_ptrs, self.count, rep, lst, cap, work, stream)

    def check(self, rep, lst, cap, what=""):
        rep.check(want_report(self.ref, cap, self.lay), f"{self.what}, cap {cap}{what}: report")
        lst.check(self.ref[:cap], f"{self.what}, cap {cap}{what}: list")

    def inputs_unchanged(self):
        _same(self.d_crc, self.crc, self.what)
        _same(self.d_buf, self.image, self.what)
        if self.ptrs is not None:
            _same(self.d_ptrs, self.ptrs, self.what)


@pytest.mark.parametrize("tile", [64, 0], ids=["tile 64", "default tile"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_parity(torch_dev, tile_setter, c64, layout, tile):
    """verify_n / verify_ptr_n against the numpy reference, report and list in device memory. 131,281
    entries at tile 64 are 2,052 tiles, more than twice the scan's chunk: the scan loops."""
    torch = torch_dev
    tile_setter(tile)
    rep = Out(torch, 4)
    ran = 0
    for count in layout_counts(layout):
        work = _work(torch, count)
        for pattern in PATTERNS:
            case = Case(torch, c64, layout, count, pattern, tile or DEFAULT_TILE)
            assert (case.ref.size > 0) == (pattern != "none")
            for cap in caps(int(case.ref.size)):
                lst = Out(torch, cap + 8)
                rep.refill()
                case.run(rep, lst, cap, work)
                torch.cuda.synchronize()
                case.check(rep, lst, cap, f", tile {tile}")
                ran += 1
            case.inputs_unchanged()
    assert ran > 100


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_pinned_outputs(torch_dev, tile_setter, c64):
    """Report and list in pinned host memory: read after the sync with no copy."""
    torch = torch_dev
    tile_setter(64)
    for layout, count, pattern in (("dense", 131281, "random"), ("pointers", 4097, "tile edges"),
                                   ("odd stride", 4097, "run of 130"), ("component", 65, "none")):
        case = Case(torch, c64, layout, count, pattern, 64)
        work = _work(torch, count)
        for cap in caps(int(case.ref.size)):
            rep, lst = Out(torch, 4, pinned=True), Out(torch, cap + 8, pinned=True)
            case.run(rep, lst, cap, work)
            torch.cuda.synchronize()
            case.check(rep, lst, cap, " (pinned)")
        case.inputs_unchanged()


# ------------------------------------------------ end to end: in-band trailers
def _corrupt(torch, region, offsets):
    idx = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    region[idx] = region[idx] ^ 0xFF


@pytest.mark.parametrize("nbytes,stride", [(4096, 8192), (4093, 4101)], ids=["4096 at 8192", "4093 at 4101"])
@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_zerocopy_layout(torch_dev, oracle, c64, nbytes, stride):
    """copy_batch_strided + stamp_n lands payload + trailer (zerocopy-server's layout); batch_strided +
    verify_n on one stream, nothing in between, finds the three buffers corrupted afterwards. With 4,093
    bytes at stride 4,101 every trailer is misaligned and (CRC-64) the next payload starts right behind it."""
    torch = torch_dev
    count, w, seed = 257, width(c64), 0x2E80C0
    assert nbytes + w <= stride
    src_stride = nbytes + 3
    src = torch.empty(count * src_stride, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, src_stride, nbytes, count, seed)
    region = torch.full((64 + count * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dst = region.data_ptr() + 64
    crcs = torch.zeros(count * w, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    (ck.copy_batch64_strided if c64 else ck.copy_batch_strided)(src, src_stride, dst, stride, nbytes, count, crcs,
                                                                stream=st)
    (ck.stamp64_device if c64 else ck.stamp_device)(crcs, count, dst + nbytes, stride, stream=st)
    torch.cuda.synchronize()
    crc = oracle.crc64ecma if c64 else oracle.crc32c
    want = np.full(region.numel(), 0xA5, np.uint8)
    for i in range(count):
        payload = datagen.stream_bytes(seed + i, nbytes)
        at = 64 + i * stride
        want[at:at + nbytes] = payload
        want[at + nbytes:at + nbytes + w] = np.frombuffer(int(crc(payload, 0)).to_bytes(w, "little"), np.uint8)
    got = region.cpu().numpy()
    diff = np.nonzero(got != want)[0]
    assert diff.size == 0, f"{diff.size} bytes differ, first at {int(diff[0]) - 64}"
    # one byte flipped in buffers 0, 128 and 256, then CRC and verify with no sync between
    _corrupt(torch, region, [64 + 0 * stride, 64 + 128 * stride + nbytes // 2, 64 + 256 * stride + nbytes - 1])
    again = torch.zeros(count * w, dtype=torch.uint8, device="cuda")
    work = _work(torch, count)
    rep, lst = Out(torch, 4), Out(torch, 8 + 8)
    before = region.cpu().numpy()
    torch.cuda.synchronize()
    (ck.batch64_strided if c64 else ck.batch_strided)(dst, stride, nbytes, count, again, stream=st)
    (ck.verify64_device if c64 else ck.verify_device)(again, dst + nbytes, stride, count, rep.ptr, lst.ptr, 8, work,
                                                      stream=st)
    torch.cuda.synchronize()
    rep.check([3, 0, 3, 257], "report")
    lst.check([0, 128, 256], "list")
    assert np.array_equal(region.cpu().numpy(), before)


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_iov_trailers(torch_dev, oracle, c64):
    """batch_iov + stamp_ptr_n / verify_ptr_n: entries of 0 .. 65,539 bytes with the trailer behind each;
    the empty entries have a null pointer: not stamped, not compared."""
    torch = torch_dev
    w = width(c64)
    lens = [0, 1, 17, 4095, 65539] * 7 + [17, 0, 1]
    count = len(lens)
    offs, pos, live_no = [], 64, 0
    for n in lens:
        if n:  # the live entries' trailers at every alignment of 8 in turn (the region is 8-byte aligned)
            pos += (live_no - (pos + n)) % 8
            live_no += 1
        offs.append(pos)
        pos += n + w if n else 0
    host = np.full(pos + 64, 0xA5, np.uint8)
    for k, (o, n) in enumerate(zip(offs, lens)):
        host[o:o + n] = datagen.stream_bytes(0x10F + k, n)
    region = torch.from_numpy(host.copy()).cuda()
    base = region.data_ptr()
    iov = np.array([[base + o, n] for o, n in zip(offs, lens)], np.uint64)
    ptrs = np.array([base + o + n if n else 0 for o, n in zip(offs, lens)], np.uint64)
    assert base % 8 == 0 and len({int(p) % 8 for p in ptrs if p}) == 8
    d_iov, d_ptrs = _dev(torch, iov), _dev(torch, ptrs)
    crcs = torch.zeros(count * w, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    batch = ck.batch64_iov if c64 else ck.batch_iov
    batch(d_iov, count, crcs, stream=st)
    (ck.stamp64_ptr_device if c64 else ck.stamp_ptr_device)(crcs, count, d_ptrs, stream=st)
    torch.cuda.synchronize()
    crc = oracle.crc64ecma if c64 else oracle.crc32c
    want = host.copy()
    for o, n in zip(offs, lens):
        if n:
            want[o + n:o + n + w] = np.frombuffer(int(crc(host[o:o + n], 0)).to_bytes(w, "little"), np.uint8)
    assert np.array_equal(region.cpu().numpy(), want)
    live = [k for k, n in enumerate(lens) if n]
    hit = [live[0], live[len(live) // 2], live[-1]]
    _corrupt(torch, region, [offs[k] + lens[k] // 2 for k in hit])
    before = region.cpu().numpy()
    again = torch.zeros(count * w, dtype=torch.uint8, device="cuda")
    work = _work(torch, count)
    rep, lst = Out(torch, 4), Out(torch, count)
    torch.cuda.synchronize()
    batch(d_iov, count, again, stream=st)
    (ck.verify64_ptr_device if c64 else ck.verify_ptr_device)(again, d_ptrs, count, rep.ptr, lst.ptr, count, work,
                                                              stream=st)
    torch.cuda.synchronize()
    rep.check([3, hit[0], 3, len(live)], "report")
    lst.check(hit, "list")
    assert np.array_equal(region.cpu().numpy(), before)
    _same(d_iov, iov, "iov")
    _same(d_ptrs, ptrs, "pointers")


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_stamp_writes_exactly_the_word(torch_dev, c64):
    """Single entries at each of the 8 byte alignments, sentinel bytes on both sides."""
    torch = torch_dev
    w = width(c64)
    word = 0x8899AABBCCDDEEFF if c64 else 0xCCDDEEFF
    d_crc = _dev(torch, np.array([word], wdt(c64)))
    for a in range(8):
        for form in ("stride", "pointer"):
            t = torch.full((64,), 0xA5, dtype=torch.uint8, device="cuda")
            at = 16 + a
            assert (t.data_ptr() + at) % 8 == a
            if form == "stride":
                (ck.stamp64_device if c64 else ck.stamp_device)(d_crc, 1, t.data_ptr() + at, 0)
            else:
                d_ptr = _dev(torch, np.array([t.data_ptr() + at], np.uint64))
                (ck.stamp64_ptr_device if c64 else ck.stamp_ptr_device)(d_crc, 1, d_ptr)
            torch.cuda.synchronize()
            want = np.full(64, 0xA5, np.uint8)
            want[at:at + w] = np.frombuffer(word.to_bytes(w, "little"), np.uint8)
            assert np.array_equal(t.cpu().numpy(), want), (a, form)
    # a run of entries at an odd stride, every third pointer null
    count, stride = 1000, w + 3
    crc = (np.arange(count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(wdt(c64))
    d_crc = _dev(torch, crc)
    le = crc.astype(np.dtype(wdt(c64)).newbyteorder("<")).view(np.uint8).reshape(-1, w)
    for form in ("stride", "pointer"):
        t = torch.full((32 + count * stride + 32,), 0xA5, dtype=torch.uint8, device="cuda")
        want = np.full(t.numel(), 0xA5, np.uint8)
        off = 33 + np.arange(count) * stride
        if form == "stride":
            (ck.stamp64_device if c64 else ck.stamp_device)(d_crc, count, t.data_ptr() + 33, stride)
            keep = np.ones(count, bool)
        else:
            keep = np.arange(count) % 3 != 1
            ptrs = np.where(keep, t.data_ptr() + off, 0).astype(np.uint64)
            d_ptrs = _dev(torch, ptrs)
            (ck.stamp64_ptr_device if c64 else ck.stamp_ptr_device)(d_crc, count, d_ptrs)
        torch.cuda.synchronize()
        want[off[keep][:, None] + np.arange(w)] = le[keep]
        assert np.array_equal(t.cpu().numpy(), want), form
    _same(d_crc, crc, "stamp")


def test_graph_capture(torch_dev, oracle):
    """A captured batch_strided + verify_n pair, replayed three times with a different buffer corrupted
    before each of the first two and none before the third."""
    torch = torch_dev
    count, nbytes, stride, seed = 257, 4096, 8192, 0x6A9F
    region = torch.full((count * stride,), 0xA5, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(region, stride, nbytes, count, seed)
    crcs = torch.zeros(count * 4, dtype=torch.uint8, device="cuda")
    ck.batch_strided(region, stride, nbytes, count, crcs)  # first-call set-up, and the CRCs to store
    ck.stamp_device(crcs, count, region.data_ptr() + nbytes, stride)
    torch.cuda.synchronize()
    assert int.from_bytes(bytes(region[nbytes:nbytes + 4].cpu().numpy()), "little") == \
        oracle.crc32c(datagen.stream_bytes(seed, nbytes), 0)
    work = _work(torch, count)
    rep, lst = Out(torch, 4), Out(torch, 8)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        st = torch.cuda.current_stream()
        ck.batch_strided(region, stride, nbytes, count, crcs, stream=st)
        ck.verify_device(crcs, region.data_ptr() + nbytes, stride, count, rep.ptr, lst.ptr, 8, work, stream=st)
    last = None
    for rep_no, hit in enumerate((77, 200, None)):
        if last is not None:
            _corrupt(torch, region, [last * stride + 5])  # restore the one before
        if hit is not None:
            _corrupt(torch, region, [hit * stride + 5])
        last = hit
        rep.refill()
        lst.refill()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        rep.check([1, hit, 1, count] if hit is not None else [0, NONE, 0, count], f"replay {rep_no}: report")
        lst.check([hit] if hit is not None else [], f"replay {rep_no}: list")


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_streams(torch_dev, tile_setter, c64):
    """Two calls on two streams with distinct outputs and workspaces."""
    torch = torch_dev
    tile_setter(64)
    jobs = []
    for layout, count, pattern in (("dense", 131281, "one per 64"), ("pointers", 3 * 4096 + 5, "random")):
        case = Case(torch, c64, layout, count, pattern, 64)
        cap = int(case.ref.size)
        jobs.append((case, cap, Out(torch, 4), Out(torch, cap + 8), _work(torch, count), torch.cuda.Stream()))
    torch.cuda.synchronize()
    for _ in range(3):
        for case, cap, rep, lst, work, st in jobs:
            case.run(rep, lst, cap, work, stream=st)
    torch.cuda.synchronize()
    for case, cap, rep, lst, work, st in jobs:
        case.check(rep, lst, cap, " (two streams)")
        case.inputs_unchanged()


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_failure_injection(torch_dev, c64):
    """photon_crc_test_fail_next(1): each new call returns -EIO and leaves its outputs at 0xA5."""
    torch = torch_dev
    count = 300
    dense = Case(torch, c64, "dense", count, "all", DEFAULT_TILE)
    ptr = Case(torch, c64, "pointers", count, "all", DEFAULT_TILE)
    work = _work(torch, count)
    for case in (dense, ptr):
        rep, lst = Out(torch, 4), Out(torch, count)
        ck.inject_failures(1)
        with pytest.raises(ck.CrcError) as e:
            case.run(rep, lst, count, work)
        assert e.value.code == -5 and "injected" in str(e.value)
        torch.cuda.synchronize()
        rep.check([], "report after an injected failure")
        lst.check([], "list after an injected failure")
        assert (work.cpu().numpy() == 0xA5).all()
        case.run(rep, lst, count, work)  # and the next call runs
        torch.cuda.synchronize()
        case.check(rep, lst, count, " (after the failure)")
        work.fill_(0xA5)
    target = Out(torch, count * 2)
    d_ptrs = _dev(torch, (target.ptr + 16 * np.arange(count)).astype(np.uint64))
    for call in (lambda: (ck.stamp64_device if c64 else ck.stamp_device)(dense.d_crc, count, target.ptr, 16),
                 lambda: (ck.stamp64_ptr_device if c64 else ck.stamp_ptr_device)(dense.d_crc, count, d_ptrs)):
        ck.inject_failures(1)
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code == -5
        torch.cuda.synchronize()
        target.check([], "stamp after an injected failure")

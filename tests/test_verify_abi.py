"""Stored CRCs checked on the device (photon_crc32c_verify_n / _verify_ptr_n /
_stamp_n / _stamp_ptr_n and the CRC-64 forms), without a
GPU: exported, declared, argument checks, a loud failure where there is no
device, the tile setter, and the CPU replay of the kernels' mark, scan and
list steps (photon_crc_test_verify, tuning.h) against a numpy reference
(np.nonzero(crc != expected)). CPU only.

The counts, bad patterns, caps and expected-word layouts made here are shared
with tests/test_gpu_verify.py."""
import ctypes
import os

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = {"photon_crc32c_verify_n": 10, "photon_crc64ecma_verify_n": 10,
         "photon_crc32c_verify_ptr_n": 9, "photon_crc64ecma_verify_ptr_n": 9,
         "photon_crc32c_stamp_n": 5, "photon_crc64ecma_stamp_n": 5,
         "photon_crc32c_stamp_ptr_n": 4, "photon_crc64ecma_stamp_ptr_n": 4}
HOOKS = ["photon_crc_set_verify_tile", "photon_crc_test_verify", "photon_crc_util_verify_on_host"]
WRAPPERS = ["verify_device", "verify64_device", "verify_ptr_device", "verify64_ptr_device",
            "stamp_device", "stamp64_device", "stamp_ptr_device", "stamp64_ptr_device",
            "verify_work_bytes", "set_verify_tile", "VerifyReport"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
CRCS = [False, True]
IDS = ["crc32c", "crc64"]
NONE = (1 << 64) - 1
A5 = 0xA5A5A5A5A5A5A5A5

# ------------------------------------------------------------------ cases
COUNTS = [1, 2, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, 131281]
TILES = [64, 256, 4096]
DEFAULT_TILE = 1024
PATTERNS = ["none", "all", "first", "last", "tile edges", "one per 64", "run of 130", "random"]
LAYOUTS = ["dense", "component", "odd stride", "pointers"]
ODD_STRIDE = 4099
ODD_MAX_COUNT = 12293  # the odd-stride layout: 4,099 bytes per entry


def width(c64):
    return 8 if c64 else 4


def wdt(c64):
    return np.uint64 if c64 else np.uint32


def bad_set(pattern, count, tile):
    """The indices pattern makes bad among `count` entries in tiles of `tile`, ascending. Every pattern
    but 'none' gives at least one for every count >= 1."""
    if pattern == "none":
        idx = []
    elif pattern == "all":
        idx = range(count)
    elif pattern == "first":
        idx = [0]
    elif pattern == "last":
        idx = [count - 1]
    elif pattern == "tile edges":  # the first and the last entry of every tile
        idx = [i for lo in range(0, count, tile) for i in (lo, min(lo + tile, count) - 1)]
    elif pattern == "one per 64":  # at a lane that rotates from row to row
        idx = [i for g in range((count + 63) // 64) for i in (64 * g + (5 * g) % 64,) if i < count]
    elif pattern == "run of 130":  # dense, across the first tile border where there is one
        lo = max(0, min(tile, count) - 65)
        idx = range(lo, min(lo + 130, count))
    else:  # p = 0.01, and one index so that no count gives an empty set
        assert pattern == "random"
        rng = np.random.default_rng(0xBAD + count)
        idx = set(np.nonzero(rng.random(count) < 0.01)[0].tolist()) | {count // 2}
    return np.array(sorted(set(idx)), np.int64)


def words(c64, count, bad):
    """Computed words (random, a fixed seed) and expected words: the computed ones with ONE bit flipped
    in the bad entries, the bit moving over the whole width, so a bad entry never compares equal."""
    rng = np.random.default_rng(0xC0FFEE + count + c64)
    crc = rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, count, dtype=np.uint64)
    crc = crc.astype(wdt(c64)) if c64 else (crc >> np.uint64(32)).astype(np.uint32)
    exp = crc.copy()
    bits = 8 * width(c64)
    flip = (np.ones(bad.size, np.uint64) << ((bad.astype(np.uint64) * np.uint64(7)) % np.uint64(bits))).astype(wdt(c64))
    assert (flip != 0).all()
    exp[bad] ^= flip
    return crc, exp


def caps(nbad):
    return sorted({c for c in (0, 1, nbad - 1, nbad, nbad + 8) if c >= 0})


class Layout:
    """Where the expected words lie, as byte offsets into one buffer: size = its bytes, off[i] = entry
    i's offset from the buffer's start given the address the buffer got; stride (None for the pointer
    form); null[i] = entry i has a null pointer (the pointer form: every 7th)."""

    def __init__(self, name, c64, count, addr):
        w = width(c64)
        i = np.arange(count, dtype=np.int64)
        self.name, self.c64, self.count, self.w = name, c64, count, w
        self.null = np.zeros(count, bool)
        if name == "dense":
            self.stride, self.off = w, 16 + i * w
        elif name == "component":  # CRC32C_Component {u32 crc, u32 size} / CRC64ECMA_Component {u64 crc, u64 size}
            self.stride, self.off = 2 * w, 16 + i * 2 * w
        elif name == "odd stride":  # from an odd address
            assert count <= ODD_MAX_COUNT
            self.stride, self.off = ODD_STRIDE, 16 + (addr + 1) % 2 + i * ODD_STRIDE
            assert (addr + int(self.off[0])) % 2 == 1
        else:
            assert name == "pointers"  # every alignment of 8; every 7th pointer null
            self.stride, self.off = None, 16 + i * 16 + i % 8
            self.null = i % 7 == 5
        self.size = int(self.off[-1]) + w + 16

    def image(self, exp):
        """The buffer's bytes: 0xA5 but the expected words, little-endian."""
        buf = np.full(self.size, 0xA5, np.uint8)
        le = np.ascontiguousarray(exp, wdt(self.c64)).astype(np.dtype(wdt(self.c64)).newbyteorder("<"))
        buf[self.off[:, None] + np.arange(self.w)] = le.view(np.uint8).reshape(-1, self.w)
        return buf

    def pointers(self, addr):
        p = (addr + self.off).astype(np.uint64)
        p[self.null] = 0
        return p


def make_case(c64, layout, count, pattern, tile, addr):
    """One case: the computed words, the layout and its image, the reference. addr = the address
    the expected-word buffer will have. In the pointer form the entries with a
    null pointer carry a MISMATCHING word: they must be skipped, not found equal."""
    bad = bad_set(pattern, count, tile)
    lay = Layout(layout, c64, count, addr)
    if lay.null.any():
        crc, exp = words(c64, count, np.union1d(bad, np.nonzero(lay.null)[0]))
    else:
        crc, exp = words(c64, count, bad)
    ref = np.nonzero((crc != exp) & ~lay.null)[0]
    assert np.array_equal(ref, bad[~lay.null[bad]] if bad.size else bad)
    return crc, exp, lay, ref


def want_report(ref, cap, lay):
    return [int(ref.size), int(ref[0]) if ref.size else NONE, min(int(ref.size), cap), int((~lay.null).sum())]


def layout_counts(layout):
    return [c for c in COUNTS if layout != "odd stride" or c <= ODD_MAX_COUNT]


# ------------------------------------------------------------------- tests
def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    inc = os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc")
    header = open(os.path.join(inc, "crc32c_gpu.h")).read()
    tuning = open(os.path.join(inc, "tuning.h")).read()
    for n, nargs in NAMES.items():
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == nargs, n
        assert f"int {n}(" in header, n
    assert "photon_crc_verify_work_bytes" in exported
    assert "uint64_t photon_crc_verify_work_bytes(uint64_t count);" in header
    assert "} photon_crc_verify_report;" in header
    for n in HOOKS:
        assert n in exported, n
        assert f"int {n}(" in tuning, n
    assert len(L.photon_crc_test_verify.argtypes) == 10
    assert ctypes.sizeof(ck.VerifyReport) == 32
    assert [f[0] for f in ck.VerifyReport._fields_] == ["nbad", "first_bad", "nlisted", "count"]


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


C, E, R, B, W, D = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000  # never dereferenced
BIG = 1 << 30


def _einval(call, *texts):
    with pytest.raises(ck.CrcError) as e:
        call()
    assert e.value.code == -22, str(e.value)
    for t in texts:
        assert t in str(e.value), str(e.value)


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_null_arguments_are_einval(c64):
    v = ck.verify64_device if c64 else ck.verify_device
    vp = ck.verify64_ptr_device if c64 else ck.verify_ptr_device
    s = ck.stamp64_device if c64 else ck.stamp_device
    sp = ck.stamp64_ptr_device if c64 else ck.stamp_ptr_device
    for call in (lambda: v(None, E, 8, 100, R, B, 4, W, BIG),
                 lambda: v(C, None, 8, 100, R, B, 4, W, BIG),
                 lambda: v(C, E, 8, 100, None, B, 4, W, BIG),
                 lambda: v(C, E, 8, 100, R, B, 4, None, BIG),
                 lambda: v(C, E, 8, 100, R, None, 1, W, BIG),
                 lambda: v(C, E, 8, 1, R, None, 0, None, 0),
                 lambda: vp(None, E, 100, R, B, 4, W, BIG),
                 lambda: vp(C, None, 100, R, B, 4, W, BIG),
                 lambda: vp(C, E, 100, None, B, 4, W, BIG),
                 lambda: vp(C, E, 100, R, B, 4, None, BIG),
                 lambda: vp(C, E, 100, R, None, 100, W, BIG),
                 lambda: s(None, 100, D, 8),
                 lambda: s(C, 100, None, 8),
                 lambda: sp(None, 100, D),
                 lambda: sp(C, 100, None)):
        _einval(call, "null")


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_stride_rules(c64):
    w = width(c64)
    v = ck.verify64_device if c64 else ck.verify_device
    s = ck.stamp64_device if c64 else ck.stamp_device
    for stride in (0, 1, w - 1):
        _einval(lambda: v(C, E, stride, 2, R, B, 4, W, BIG), "stride", str(w))
        _einval(lambda: s(C, 2, D, stride), "stride", str(w))
    if NO_GPU:  # a stride below the width is allowed for ONE entry, the width for any count: past the checks
        for call in (lambda: v(C, E, 0, 1, R, B, 4, W, BIG), lambda: v(C, E, w, 2, R, B, 4, W, BIG),
                     lambda: s(C, 1, D, 0), lambda: s(C, 2, D, w)):
            with pytest.raises(ck.CrcError) as e:
                call()
            assert e.value.code < 0 and e.value.code != -22, str(e.value)


@pytest.fixture
def tile_setter():
    yield ck.set_verify_tile
    ck.set_verify_tile(0)


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_workspace_rules(tile_setter, c64):
    v = ck.verify64_device if c64 else ck.verify_device
    vp = ck.verify64_ptr_device if c64 else ck.verify_ptr_device
    for tile in (64, 4096, 0):
        tile_setter(tile)
        for count in (1, 64, 65, 4097, 131281):
            need = ck.verify_work_bytes(count)
            assert need == 24 * ((count + (tile or DEFAULT_TILE) - 1) // (tile or DEFAULT_TILE)), (tile, count)
            for call in (lambda: v(C, E, 8, count, R, B, 4, W, need - 1),
                         lambda: vp(C, E, count, R, None, 0, W, need - 1)):
                _einval(call, str(need - 1), str(need))
    assert ck.verify_work_bytes(0) == 0
    assert ck.verify_work_bytes(1 << 40) == 24 << 30
    assert ck.verify_work_bytes((1 << 40) + 1) == NONE
    _einval(lambda: v(C, E, 8, (1 << 40) + 1, R, B, 4, W, NONE), "too many")
    _einval(lambda: vp(C, E, (1 << 40) + 1, R, B, 4, W, NONE), "too many")
    _einval(lambda: v(C, E, 8, 100, R, B, 4, W + 4, BIG), "aligned")


def test_count_zero_touches_nothing():
    for call in (lambda: ck.verify_device(None, None, 0, 0, None, None, 7, None, 0),
                 lambda: ck.verify64_device(C, E, 8, 0, R, B, 4, W, 0),
                 lambda: ck.verify_ptr_device(None, None, 0, None, None, 7, None, 0),
                 lambda: ck.verify64_ptr_device(C, E, 0, R, B, 4, W, 0),
                 lambda: ck.stamp_device(None, 0, None, 0),
                 lambda: ck.stamp64_device(C, 0, D, 0),
                 lambda: ck.stamp_ptr_device(None, 0, None),
                 lambda: ck.stamp64_ptr_device(C, 0, D)):
        call()  # returns 0: no CrcError


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for call in (lambda: ck.verify_device(C, E, 4, 100, R, B, 4, W, BIG),
                 lambda: ck.verify_device(C, E, 8192, 100, R, None, 0, W, BIG),
                 lambda: ck.verify64_device(C, E + 1, 4101, 100, R, B, 100, W, BIG),
                 lambda: ck.verify_ptr_device(C, E, 100, R, B, 4, W, BIG),
                 lambda: ck.verify64_ptr_device(C, E, 100, R, None, 0, W, BIG),
                 lambda: ck.stamp_device(C, 100, D + 1, 4101),
                 lambda: ck.stamp64_device(C, 100, D, 8),
                 lambda: ck.stamp_ptr_device(C, 100, D),
                 lambda: ck.stamp64_ptr_device(C, 100, D)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code < 0


def test_tile_setter(tile_setter):
    for bad in (1, 32, 63, 96, 4095, 4097, 65537, 1 << 17, 1 << 31):
        _einval(lambda: tile_setter(bad), "power of two")
    for good in (64, 128, 4096, 65536, 0):
        tile_setter(good)
    L = _native.lib()
    one = ctypes.c_uint64(0)
    rep = (ctypes.c_uint64 * 4)()
    for tile in (0, 32, 96, 1 << 17):  # the replay takes the same tiles
        assert L.photon_crc_test_verify(0, ctypes.addressof(one), ctypes.addressof(one), 4, None, 1, tile, 0, rep,
                                        None) == -22
    assert L.photon_crc_test_verify(0, ctypes.addressof(one), ctypes.addressof(one), 4, None, 0, 64, 0, rep,
                                    None) == -22


def replay(c64, crc, lay, buf, count, tile, cap):
    """photon_crc_test_verify over host arrays: the report's words and the index list WHOLE, cap + 8
    words that were 0xA5 before."""
    rep = np.full(4, A5, np.uint64)
    lst = np.full(cap + 8, A5, np.uint64)
    ptrs = lay.pointers(buf.ctypes.data) if lay.stride is None else None
    rc = _native.lib().photon_crc_test_verify(int(c64), crc.ctypes.data,
                                              None if ptrs is not None else buf.ctypes.data + int(lay.off[0]),
                                              lay.stride or 0, None if ptrs is None else ptrs.ctypes.data, count,
                                              tile, cap, rep.ctypes.data, lst.ctypes.data if cap else None)
    assert rc == 0, _native.lib().photon_crc_last_error()
    return [int(x) for x in rep], lst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_replay(c64, layout):
    ran = 0
    for count in layout_counts(layout):
        probe = Layout(layout, c64, count, 0)
        buf = np.empty(probe.size + 1, np.uint8)  # + 1: the same size whatever the address's parity
        for tile in TILES:
            for pattern in PATTERNS:
                crc, exp, lay, ref = make_case(c64, layout, count, pattern, tile, buf.ctypes.data)
                assert (ref.size > 0) == (pattern != "none"), (count, pattern)
                buf[:lay.size] = lay.image(exp)
                crc0, buf0 = crc.copy(), buf[:lay.size].copy()
                for cap in caps(int(ref.size)):
                    rep, lst = replay(c64, crc, lay, buf, count, tile, cap)
                    what = f"{count} entries, {pattern}, tile {tile}, cap {cap}"
                    assert rep == want_report(ref, cap, lay), what
                    assert np.array_equal(lst[:rep[2]], ref[:cap].astype(np.uint64)), what
                    assert (lst[rep[2]:] == A5).all(), what + ": written beyond nlisted"
                    ran += 1
                assert np.array_equal(crc, crc0) and np.array_equal(buf[:lay.size], buf0)
    assert ran > 300


def test_patterns_cover_the_scan():
    # the shapes the GPU test relies on: every pattern but 'none' is non-empty for every count, 131,281
    # entries at tile 64 are more than twice a scan chunk of tiles, the run of 130 crosses a tile border
    for count in COUNTS:
        for tile in TILES:
            for pattern in PATTERNS[1:]:
                assert bad_set(pattern, count, tile).size > 0, (count, tile, pattern)
    assert (131281 + 63) // 64 == 2052
    run = bad_set("run of 130", 4097, 256)
    assert run.size == 130 and run[0] < 256 <= run[-1]
    for c64 in CRCS:
        for pattern in PATTERNS[1:]:
            _, _, lay, ref = make_case(c64, "pointers", 4097, pattern, 64, 0x1000)
            assert lay.null.sum() == 585 and ref.size > 0

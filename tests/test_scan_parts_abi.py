"""Running CRCs of objects over their parts on the device
(photon_crc32c_scan_parts_n, photon_crc64ecma_scan_parts_n),
without a GPU: exported, declared, argument checks, the workspace and tile
rules, a loud failure where there is no device, and the CPU replay of the
kernels' three steps (photon_crc_test_scan_parts, tuning.h) against the
pinned oracle chained part by part over real bytes, and against the
bit-serial GF(2) chain of tests/test_fold_parts_abi.py over synthetic pairs
with lengths of 4 GiB and more. Every output array of the replay is
pre-filled with 0xA5 bytes with 8 guard words on each side and compared
WHOLE. CPU only.

The cases, part CRCs and expected values made here are shared with
tests/test_gpu_scan_parts.py and tests/test_scan_parts_cpp.py."""
import ctypes
import os

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_fold_parts_abi import (BIG_LENS, CRCS, IDS, SEEDS, gf_mul, gf_xpow8, real_shapes, synthetic_pairs)
from tests.test_fold_parts_abi import replay as fold_replay

NAMES = {"photon_crc32c_scan_parts_n": 12, "photon_crc64ecma_scan_parts_n": 12}
TUNING = {"photon_crc_scan_work_bytes": 1, "photon_crc_set_scan_tile": 1, "photon_crc_test_scan_geometry": 1,
          "photon_crc_test_scan_parts": 12, "photon_crc_util_scan_on_host": 11}
WRAPPERS = ["scan_work_bytes", "set_scan_tile", "scan_parts_device", "scan_parts64_device"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
A5 = 0xA5A5A5A5A5A5A5A5
NONE = (1 << 64) - 1
DEFAULT_TILE = 1024
GUARDW = 8
TILES = [64, 256, 65536]
THREADS = [1, 7, 64, 256]
WORK_WORDS = 4  # 64-bit words of workspace per tile


def wdt(c64):
    return np.uint64 if c64 else np.uint32


def a5(dtype):
    return A5 & ((1 << (8 * np.dtype(dtype).itemsize)) - 1)


# ------------------------------------------------------------ expected values
class Case:
    """Objects over real bytes: obj_start (nobj + 1), the parts' lengths, per
    CRC the oracle's part CRCs (seed 0), per-object seeds, and the oracle's
    running words from the per-object seeds (want) and from each seed of
    SEEDS (want0[c64, seed]): run[s] = crc(part s, run[s - 1]), the object's
    seed before its first part. end = the bytes of the object through part s."""

    def __init__(self, oracle, name, start, lens, data_seed, seeds=None, rng=None):
        self.name = name
        self.start = np.asarray(start, np.uint64)
        self.len = np.asarray(lens, np.uint64)
        self.nobj, self.nparts = self.start.size - 1, self.len.size
        assert self.start[0] == 0 and self.start[-1] == self.nparts and (np.diff(self.start.astype(np.int64)) >= 0).all()
        data = datagen.stream_bytes(data_seed, int(self.len.sum()))
        cuts = np.concatenate(([0], np.cumsum(self.len))).astype(np.int64)
        pieces = [data[cuts[s]:cuts[s + 1]] for s in range(self.nparts)]
        rng = rng or np.random.default_rng(data_seed)
        self.crc, self.seeds, self.want, self.want0 = {}, {}, {}, {}
        for c64 in CRCS:
            crc = oracle.crc64ecma if c64 else oracle.crc32c
            self.crc[c64] = np.array([crc(p, 0) for p in pieces], wdt(c64))
            self.seeds[c64] = (rng.integers(0, 1 << 32, self.nobj, dtype=np.uint64).astype(wdt(c64)) * wdt(c64)(3)
                               if seeds is None else np.asarray(seeds[c64], wdt(c64)))
            self.want[c64] = self._chain(crc, pieces, [int(x) for x in self.seeds[c64]], c64)
            for seed in SEEDS[c64]:
                self.want0[c64, seed] = self._chain(crc, pieces, [seed] * self.nobj, c64)
        self.end = np.zeros(self.nparts, np.uint64)
        for m in range(self.nobj):
            a, b = int(self.start[m]), int(self.start[m + 1])
            self.end[a:b] = np.cumsum(self.len[a:b])

    def _chain(self, crc, pieces, seeds, c64):
        out = np.zeros(self.nparts, wdt(c64))
        for m in range(self.nobj):
            acc = seeds[m]
            for s in range(int(self.start[m]), int(self.start[m + 1])):
                acc = out[s] = crc(pieces[s], acc)
        return out

    def objects(self):
        return [(m, int(self.start[m]), int(self.start[m + 1])) for m in range(self.nobj)]


_REAL = []


def real_cases(oracle):
    """Every object of real_shapes alone. Made once per process; nothing changes them afterwards."""
    if not _REAL:
        for k, sh in enumerate(real_shapes(oracle)):
            c = Case.__new__(Case)
            c.name, c.len, c.nobj, c.nparts = sh.name, sh.len, 1, sh.len.size
            c.start = np.array([0, sh.len.size], np.uint64)
            cuts = np.concatenate(([0], np.cumsum(sh.len))).astype(np.int64)
            pieces = [sh.data[cuts[s]:cuts[s + 1]] for s in range(c.nparts)]
            c.crc, c.want0, c.shape = sh.crc, {}, sh
            for c64 in CRCS:
                for seed in SEEDS[c64]:
                    c.want0[c64, seed] = c._chain(oracle.crc64ecma if c64 else oracle.crc32c, pieces, [seed], c64)
                    if c.nparts:  # the chain ends at the oracle's CRC of the whole buffer
                        assert int(c.want0[c64, seed][-1]) == sh.want[c64, seed]
            c.end = np.cumsum(sh.len).astype(np.uint64)
            _REAL.append(c)
    return _REAL


def small_lengths(rng, n):
    """n lengths of 0..40 bytes with runs of equal lengths and of empty parts."""
    out = rng.integers(0, 41, n).astype(np.uint64)
    i = 0
    while i < n:
        if rng.random() < 0.2:
            run = int(rng.integers(2, 7))
            out[i:i + run] = 0 if rng.random() < 0.3 else out[i]
            i += run
        i += 1
    return out


FUZZ_KINDS = ["random", "tile borders", "one tile exactly", "three tiles, no border inside", "40 objects in a tile",
              "runs of empty objects"]
FUZZ_CASES = 300


def fuzz_start(kind, rng):
    """obj_start of one fuzz case at tile 64: (nparts, the boundaries as a sorted multiset)."""
    if kind == "random":
        nparts = int(rng.integers(1, 201))
        cuts = sorted(int(x) for x in rng.integers(0, nparts + 1, int(rng.integers(0, 12))))
    elif kind == "tile borders":
        nparts = int(rng.integers(129, 201))
        cuts = sorted([63, 64, 65, 127, 128] + [int(x) for x in rng.integers(0, nparts + 1, int(rng.integers(0, 5)))])
    elif kind == "one tile exactly":
        nparts = int(rng.integers(128, 201))
        cuts = sorted([64, 128] + [int(x) for x in rng.integers(0, 64, int(rng.integers(0, 4)))] +
                      [int(x) for x in rng.integers(128, nparts + 1, int(rng.integers(0, 4)))])
    elif kind == "three tiles, no border inside":
        nparts = 200
        a, b = (0, 192) if rng.random() < 0.3 else (int(rng.integers(0, 64)), int(rng.integers(129, 201)))
        cuts = sorted([a, b] + [int(x) for x in rng.integers(0, a + 1, int(rng.integers(0, 3)))] +
                      [int(x) for x in rng.integers(b, 201, int(rng.integers(0, 3)))])
    elif kind == "40 objects in a tile":
        nparts = int(rng.integers(128, 201))
        cuts = sorted([64, 128] + [int(x) for x in rng.integers(64, 129, 39)])
    else:  # runs of empty objects: first, in the middle and last
        nparts = int(rng.integers(1, 201))
        at = [0, nparts] + [int(x) for x in rng.integers(0, nparts + 1, 3)]
        cuts = sorted(x for x in at for _ in range(int(rng.integers(1, 5))))
    return nparts, cuts


def fuzz_case(oracle, i):
    rng = np.random.default_rng(0x5CA9 + i)
    kind = FUZZ_KINDS[i % len(FUZZ_KINDS)]
    nparts, cuts = fuzz_start(kind, rng)
    start = [0] + cuts + [nparts]
    return Case(oracle, f"fuzz {i} ({kind}): start {start}", start, small_lengths(rng, nparts), 0x5CA900 + i, rng=rng)


_FUZZ = []


def fuzz_cases(oracle):
    if not _FUZZ:
        _FUZZ.extend(fuzz_case(oracle, i) for i in range(FUZZ_CASES))
    return _FUZZ


def fixed_batch(oracle):
    """The boundary cases of the fuzz as one batch of 600 parts at tile 64: empty objects first, in the middle
    and last, borders at 63, 64, 65, 127 and 128, an object of exactly one tile [192, 256), one over three
    tiles and more with no border inside [261, 459), 40 objects inside the tile [512, 576)."""
    inner = sorted(np.random.default_rng(0xBA7C).integers(513, 576, 39).tolist())
    start = [0, 0, 0, 63, 64, 65, 127, 128, 128, 128, 192, 256, 261, 459, 512] + inner + [576, 600, 600, 600]
    assert len([1 for a, b in zip(start[13:], start[14:]) if 512 <= a and b <= 576]) == 40
    return Case(oracle, "fixed batch", start, small_lengths(np.random.default_rng(0xBA7D), 600), 0xBA7C00)


_XPOW = {}


def gf_chain(crcs, lens, start, seeds, c64):
    """The bit-serial definition: run[s] over every object, from seeds[m]."""
    out = np.zeros(len(crcs), wdt(c64))
    for m in range(len(start) - 1):
        acc = int(seeds[m])
        for s in range(int(start[m]), int(start[m + 1])):
            n = int(lens[s])
            if (n, c64) not in _XPOW:
                _XPOW[n, c64] = gf_xpow8(n, c64)
            acc = gf_mul(acc, _XPOW[n, c64], c64) ^ int(crcs[s])
            out[s] = acc
    return out


def wrapped_ends(lens, start):
    out = np.zeros(len(lens), np.uint64)
    for m in range(len(start) - 1):
        acc = 0
        for s in range(int(start[m]), int(start[m + 1])):
            acc = (acc + int(lens[s])) % (1 << 64)
            out[s] = acc
    return out


# ------------------------------------------------------------------ the replay
def replay(c64, crcs, lens, start, nparts, seed0, seeds, tile, nt, with_end=True):
    """photon_crc_test_scan_parts over host arrays: run[] and end[] WHOLE with their guards (end left at 0xA5
    when it is not passed)."""
    crcs = np.ascontiguousarray(crcs, wdt(c64))
    lens = np.ascontiguousarray(lens, np.uint64)
    start = None if start is None else np.ascontiguousarray(start, np.uint64)
    seeds = None if seeds is None else np.ascontiguousarray(seeds, wdt(c64))
    run = np.full(nparts + 2 * GUARDW, a5(wdt(c64)), wdt(c64))
    end = np.full(nparts + 2 * GUARDW, A5, np.uint64)
    before = [None if a is None else a.copy() for a in (crcs, lens, start, seeds)]
    rc = _native.lib().photon_crc_test_scan_parts(
        int(c64), crcs.ctypes.data, lens.ctypes.data, None if start is None else start.ctypes.data,
        1 if start is None else start.size - 1, nparts, seed0, None if seeds is None else seeds.ctypes.data, tile, nt,
        run.ctypes.data + GUARDW * run.itemsize, end.ctypes.data + GUARDW * 8 if with_end else None)
    assert rc == 0, _native.lib().photon_crc_last_error()
    for a, b in zip((crcs, lens, start, seeds), before):
        assert a is None or np.array_equal(a, b), "the replay changed an input"
    return run, end


def guarded(want, dtype, n=None):
    """want between two guards of 8 words of 0xA5; None: n words of 0xA5 (nothing written)."""
    n = len(want) if want is not None else n
    full = np.full(n + 2 * GUARDW, a5(dtype), dtype)
    if want is not None:
        full[GUARDW:GUARDW + n] = np.asarray(want, dtype)
    return full


# ------------------------------------------------------------------- tests
def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    inc = os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc")
    header, tuning = open(os.path.join(inc, "crc32c_gpu.h")).read(), open(os.path.join(inc, "tuning.h")).read()
    for n, nargs in NAMES.items():
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == nargs, n
        assert f"int {n}(" in header, n
    assert "uint64_t photon_crc_scan_work_bytes(" in header
    assert header.index("photon_crc64ecma_fold_parts_n(") < header.index("photon_crc32c_scan_parts_n(")
    for n, nargs in TUNING.items():
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == nargs, n
        assert f" {n}(" in (header if n == "photon_crc_scan_work_bytes" else tuning), n


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


C, N, S, R, E, W, SD = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000  # never dereferenced
BIG = 1 << 30


def _einval(call, *texts):
    with pytest.raises(ck.CrcError) as e:
        call()
    assert e.value.code == -22, str(e.value)
    for t in texts:
        assert t in str(e.value), str(e.value)


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_null_arguments_are_einval(c64):
    f = ck.scan_parts64_device if c64 else ck.scan_parts_device
    for call in (lambda: f(None, N, S, 2, 8, R, W, BIG),
                 lambda: f(C, None, S, 2, 8, R, W, BIG, end=E),
                 lambda: f(C, N, S, 2, 8, None, W, BIG),
                 lambda: f(C, N, S, 2, 8, R, None, BIG),
                 lambda: f(C, N, S, 2, 8, R, None, 0, seeds=SD),
                 lambda: f(C, N, None, 1, 8, None, W, BIG, seed=5),
                 lambda: f(C, N, None, 2, 8, R, W, BIG),
                 lambda: f(C, N, None, 1 << 32, 8, R, W, BIG, end=E)):
        _einval(call, "null")


@pytest.fixture
def tile_setter():
    yield ck.set_scan_tile
    ck.set_scan_tile(0)


def geometry():
    out = (ctypes.c_uint64 * 3)()
    _native.lib().photon_crc_test_scan_geometry(out)
    return [int(x) for x in out]


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_workspace_rules(tile_setter, c64):
    f = ck.scan_parts64_device if c64 else ck.scan_parts_device
    for tile in (64, 4096, 0):
        tile_setter(tile)
        assert geometry()[0] == (tile or DEFAULT_TILE)
        for nparts in (1, 64, 65, 4097, 131281):
            need = ck.scan_work_bytes(nparts)
            t = tile or DEFAULT_TILE
            assert need == 8 * WORK_WORDS * ((nparts + t - 1) // t), (tile, nparts)
            _einval(lambda: f(C, N, S, 2, nparts, R, W, need - 1), str(need - 1), str(need))
            _einval(lambda: f(C, N, None, 1, nparts, R, W, need - 1, end=E), str(need - 1), str(need))
    assert ck.scan_work_bytes(0) == 0
    assert ck.scan_work_bytes(1 << 40) == 8 * WORK_WORDS << 30
    assert ck.scan_work_bytes((1 << 40) + 1) == NONE
    _einval(lambda: f(C, N, S, 2, (1 << 40) + 1, R, W, NONE), "too many", str((1 << 40) + 1), str(1 << 40))
    _einval(lambda: f(C, N, S, 2, 100, R, W + 4, BIG), "aligned")


def test_geometry():
    tile, chunk, cap = geometry()
    assert tile == DEFAULT_TILE and chunk >= 2 and cap >= 2
    # the sizes of the GPU test's big objects stay quick: about 16 Ki and 131 Ki parts
    assert 64 * (chunk + 1) + 1 <= 1 << 15 and 64 * (cap + 1) + 5 <= 1 << 18


def test_nothing_to_do_touches_nothing():
    for call in (lambda: ck.scan_parts_device(None, None, None, 0, 0, None, None, 0),
                 lambda: ck.scan_parts_device(C, N, S, 0, 8, R, W, 0, end=E),      # no objects
                 lambda: ck.scan_parts64_device(C, N, S, 3, 0, R, W, 0, end=E),    # no parts
                 lambda: ck.scan_parts64_device(None, None, None, 1, 0, None, None, 0),
                 lambda: ck.scan_parts_device(None, None, None, 5, 0, None, None, 0)):
        call()  # returns 0: no CrcError
    one = np.zeros(4, np.uint64)
    for c64 in CRCS:  # the replay too
        run, end = replay(c64, one[:0], one[:0], one[:3], 0, 7, None, 64, 64)
        assert (run == a5(wdt(c64))).all() and (end == A5).all()


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for call in (lambda: ck.scan_parts_device(C, N, S, 2, 8, R, W, BIG),
                 lambda: ck.scan_parts_device(C, N, None, 1, 8, R, W, BIG, seed=1, end=E),
                 lambda: ck.scan_parts64_device(C, N, S, 2, 8, R, W, BIG, seeds=SD),
                 lambda: ck.scan_parts64_device(C, N, None, 1, 100000, R, W, BIG, end=E)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code < 0 and e.value.code != -22, str(e.value)


def test_tile_setter(tile_setter):
    for bad in (1, 32, 63, 96, 4095, 4097, 65537, 1 << 17, 1 << 31):
        _einval(lambda: tile_setter(bad), "power of two")
    for good in (64, 128, 4096, 65536, 0):
        tile_setter(good)
    L = _native.lib()
    one = np.zeros(2, np.uint64)
    for tile in (0, 32, 96, 1 << 17):  # the replay takes the same tiles
        assert L.photon_crc_test_scan_parts(0, one.ctypes.data, one.ctypes.data, None, 1, 1, 0, None, tile, 64,
                                            one.ctypes.data, None) == -22
    assert L.photon_crc_test_scan_parts(0, one.ctypes.data, one.ctypes.data, None, 1, 1, 0, None, 64, 0,
                                        one.ctypes.data, None) == -22
    assert L.photon_crc_test_scan_parts(0, one.ctypes.data, one.ctypes.data, None, 2, 1, 0, None, 64, 64,
                                        one.ctypes.data, None) == -22


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_replay_real_parts(oracle, c64):
    for case in real_cases(oracle):
        for k, seed in enumerate(SEEDS[c64]):
            for tile in TILES:
                for nt in THREADS:
                    start = None if (tile + nt + k) % 2 else case.start  # a null obj_start: one object
                    run, end = replay(c64, case.crc[c64], case.len, start, case.nparts, seed, None, tile, nt,
                                      with_end=bool(k))
                    what = f"{case.name}, seed {seed:#x}, tile {tile}, {nt} threads"
                    assert np.array_equal(run, guarded(case.want0[c64, seed], wdt(c64))), what
                    assert np.array_equal(end, guarded(case.end if k else None, np.uint64, case.nparts)), what


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_replay_synthetic_lengths(c64):
    for count, tiles in ((41, (64, 65536)), (150, (64, 256))):  # 150 parts: three tiles of 64
        crcs, lens = synthetic_pairs(c64, count)
        assert all(n in lens for n in BIG_LENS)
        for start in ([0, count], [0, 20, 20, 65 if count > 65 else 30, count]):
            nobj = len(start) - 1
            ends = wrapped_ends(lens, start)
            for seed in SEEDS[c64]:
                seeds = np.array([seed ^ (m * 0x01010101) for m in range(nobj)], wdt(c64))
                want0 = gf_chain(crcs, lens, start, [seed] * nobj, c64)
                want = gf_chain(crcs, lens, start, seeds, c64)
                for tile in tiles:
                    for nt in THREADS:
                        what = f"{count} pairs, {nobj} objects, seed {seed:#x}, tile {tile}, {nt} threads"
                        run, end = replay(c64, crcs, lens, start, count, seed, None, tile, nt)
                        assert np.array_equal(run, guarded(want0, wdt(c64))), what
                        assert np.array_equal(end, guarded(ends, np.uint64)), what
                        run, _ = replay(c64, crcs, lens, start, count, 0x77, seeds, tile, nt, with_end=False)
                        assert np.array_equal(run, guarded(want, wdt(c64))), what + ", per-object seeds"
    # one part of 4 GiB + 5 after a seed: one step, not two
    for seed in SEEDS[c64]:
        run, end = replay(c64, crcs[:1], lens[5:6], None, 1, seed, None, 64, 64)
        assert int(run[GUARDW]) == gf_mul(seed, gf_xpow8(BIG_LENS[2], c64), c64) ^ int(crcs[0])
        assert int(end[GUARDW]) == BIG_LENS[2]


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_replay_boundary_fuzz(oracle, c64):
    cases = fuzz_cases(oracle)
    assert len(cases) == 300 and all(c.nparts <= 200 for c in cases)
    seen = set()
    for i, case in enumerate(cases):
        nt = THREADS[i % 4] if i % 5 else 3
        per_object = bool(i % 2)
        seed0 = SEEDS[c64][(i // 2) % 2]
        run, end = replay(c64, case.crc[c64], case.len, case.start, case.nparts, seed0,
                          case.seeds[c64] if per_object else None, 64, nt, with_end=i % 3 != 2)
        want = case.want[c64] if per_object else case.want0[c64, seed0]
        assert np.array_equal(run, guarded(want, wdt(c64))), f"{case.name}, {nt} threads"
        assert np.array_equal(end, guarded(case.end if i % 3 != 2 else None, np.uint64, case.nparts)), case.name
        seen.update(int(x) for x in case.start)
    assert {63, 64, 65, 127, 128} <= seen


def test_fuzz_covers_the_borders(oracle):
    cases = fuzz_cases(oracle)
    objs = [(a, b) for c in cases for _, a, b in c.objects()]
    assert (64, 128) in objs                                  # an object of exactly one tile
    assert any(a < 64 and b > 128 for a, b in objs)           # three tiles, no border inside
    assert (0, 192) in objs
    assert any(sum(1 for _, a, b in c.objects() if 64 <= a and b <= 128) >= 40 for c in cases)
    assert any(c.start[1] == 0 for c in cases) and any(c.start[-2] == c.nparts for c in cases)  # empty first / last
    fixed = fixed_batch(oracle)
    assert (192, 256) in [(a, b) for _, a, b in fixed.objects()] and fixed.nparts == 600


@pytest.mark.parametrize("c64", CRCS, ids=IDS)
def test_last_entry_is_the_fold(oracle, c64):
    """The last entry of every non-empty object = photon_crc_test_fold_parts on the same pairs."""
    ran = 0
    for case in fuzz_cases(oracle)[::7] + [fixed_batch(oracle)]:
        run, end = replay(c64, case.crc[c64], case.len, case.start, case.nparts, 0, case.seeds[c64], 64, 64)
        for m, a, b in case.objects():
            if b > a:
                got, total = fold_replay(c64, case.crc[c64][a:b], case.len[a:b], int(case.seeds[c64][m]), 64)
                assert (got, total) == (int(run[GUARDW + b - 1]), int(end[GUARDW + b - 1])), (case.name, m)
                ran += 1
    for case in real_cases(oracle):
        seed = SEEDS[c64][1]
        if case.nparts:
            run, end = replay(c64, case.crc[c64], case.len, None, case.nparts, seed, None, 256, 256)
            got, total = fold_replay(c64, case.crc[c64], case.len, seed, 256)
            assert (got, total) == (int(run[GUARDW + case.nparts - 1]), int(end[GUARDW + case.nparts - 1])), case.name
            ran += 1
    crcs, lens = synthetic_pairs(c64)
    run, end = replay(c64, crcs, lens, None, lens.size, 5, None, 64, 7)
    assert fold_replay(c64, crcs, lens, 5, 7) == (int(run[GUARDW + lens.size - 1]), int(end[GUARDW + lens.size - 1]))
    assert ran > 100

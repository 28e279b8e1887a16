"""Fold of part CRCs into object CRCs on the device
(photon_crc32c_fold_parts_n, photon_crc64ecma_fold_parts_n) and the CRC-64
series calls (photon_crc64ecma_series_device,
photon_crc64ecma_combine_series_device), without a GPU:
exported, declared, argument checks, a loud failure where there is no device,
and the CPU replay of the fold kernels' per-thread and combine steps
(photon_crc_test_fold_parts, tuning.h) against the pinned oracle over real
bytes and against a bit-serial GF(2) reference (in this file, itself pinned
to the oracle) over synthetic pairs with lengths of 4 GiB and more. CPU only.

The shapes, part CRCs and expected values made here are shared with
tests/test_gpu_fold_parts.py."""
import ctypes
import os

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen

NAMES = {"photon_crc64ecma_series_device": 5, "photon_crc64ecma_combine_series_device": 5,
         "photon_crc32c_fold_parts_n": 10, "photon_crc64ecma_fold_parts_n": 10}
WRAPPERS = ["series64_device", "combine_series64_device", "fold_parts_device", "fold_parts64_device",
            "crc64ecma_series_at", "crc64ecma_combine_series_at"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
SEEDS = {False: (0, 0x9E3779B1), True: (0, 0xFEDCBA9876543210)}
CRCS = [False, True]
IDS = ["crc32c", "crc64"]

# ----------------------------------------------------------------- shapes
PART_COUNTS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 10007]
PART_LENS = [0, 1, 7, 8, 15, 16, 17, 4095, 4096, 65539]
THREADS = [1, 64, 256, 1024, 7]  # 7 divides none of the counts above but 0 and 63


def part_lengths(count, kind, rng):
    """The lengths of one object's parts: 'mixed' = drawn from PART_LENS (the
    large ones rarely, to bound the bytes), with runs of equal lengths;
    'zero' = every part empty."""
    if kind == "zero":
        return np.zeros(count, np.uint64)
    small = np.array(PART_LENS[:7], np.uint64)
    out = np.empty(count, np.uint64)
    i = 0
    while i < count:
        r = rng.random()
        n = PART_LENS[7 + int(rng.integers(3))] if r < 0.02 else int(small[rng.integers(7)])
        run = int(rng.integers(1, 9)) if rng.random() < 0.3 else 1  # a run of equal lengths
        out[i:i + run] = n
        i += run
    if count >= 3:  # every large length at least once, also first and last
        out[0], out[count // 2], out[count - 1] = PART_LENS[9], PART_LENS[7], PART_LENS[8]
    return out


class Shape:
    """One object over real bytes: lengths, the bytes, the oracle's part CRCs
    (seed 0) and whole-buffer CRCs (every seed of SEEDS), for both CRCs."""

    def __init__(self, oracle, count, kind, k):
        rng = np.random.default_rng(0xF01D + 97 * k)
        self.name = f"{count} parts ({kind})"
        self.len = part_lengths(count, kind, rng)
        self.data = datagen.stream_bytes(0xF01D00 + k, int(self.len.sum()))
        cuts = np.concatenate(([0], np.cumsum(self.len))).astype(np.int64)
        self.crc = {False: np.zeros(count, np.uint32), True: np.zeros(count, np.uint64)}
        for s in range(count):
            piece = self.data[cuts[s]:cuts[s + 1]]
            self.crc[False][s] = oracle.crc32c(piece, 0)
            self.crc[True][s] = oracle.crc64ecma(piece, 0)
        self.want = {(c64, seed): (oracle.crc64ecma if c64 else oracle.crc32c)(self.data, seed)
                     for c64 in CRCS for seed in SEEDS[c64]}
        self.total = int(self.len.sum())


_SHAPES = []


def real_shapes(oracle):
    """Made once per process; nothing changes them afterwards."""
    if not _SHAPES:
        for k, count in enumerate(PART_COUNTS):
            _SHAPES.append(Shape(oracle, count, "mixed", k))
        _SHAPES.append(Shape(oracle, 300, "zero", 100))
    return _SHAPES


@pytest.fixture(scope="module")
def shapes(oracle):
    return real_shapes(oracle)


# ------------------------------------------------- bit-serial GF(2) reference
# Reflected representation (bit W-1 = x^0): the definition of the fold with
# nothing shared with the library. POLY = the reflected polynomials of
# CRC-32C and CRC-64/ECMA.
POLY = {False: (32, 0x82F63B78), True: (64, 0xC96C5795D7870F42)}


def gf_mul(a, b, c64):
    w, poly = POLY[c64]
    r = 0
    for i in range(w - 1, -1, -1):  # b's coefficient of x^(w-1-i), from x^0 up: a, a*x, a*x^2 ...
        if (b >> i) & 1:
            r ^= a
        a = (a >> 1) ^ (poly if a & 1 else 0)
    return r


def gf_xpow8(n, c64):
    """x^(8n) by square and multiply."""
    w, _ = POLY[c64]
    result, base, e = 1 << (w - 1), 1 << (w - 2), 8 * n
    while e:
        if e & 1:
            result = gf_mul(result, base, c64)
        base = gf_mul(base, base, c64)
        e >>= 1
    return result


def gf_fold(crcs, lens, seed, c64):
    acc, known = seed, {}
    for c, n in zip(crcs, lens):
        n = int(n)
        if n not in known:
            known[n] = gf_xpow8(n, c64)
        acc = gf_mul(acc, known[n], c64) ^ int(c)
    return acc


def replay(c64, crcs, lens, seed, threads):
    crcs = np.ascontiguousarray(crcs, np.uint64 if c64 else np.uint32)
    lens = np.ascontiguousarray(lens, np.uint64)
    res, tot = ctypes.c_uint64(0xA5A5), ctypes.c_uint64(0xA5A5)
    rc = _native.lib().photon_crc_test_fold_parts(int(c64), crcs.ctypes.data, lens.ctypes.data, crcs.size, seed,
                                                  threads, ctypes.addressof(res), ctypes.addressof(tot))
    assert rc == 0, _native.lib().photon_crc_last_error()
    return res.value, tot.value


BIG_LENS = [(1 << 32) - 1, 1 << 32, (1 << 32) + 5, (1 << 40) + 3]


def synthetic_pairs(c64, count=41):
    """Random CRC words with lengths of 4 GiB and more among small ones."""
    rng = np.random.default_rng(0x5EED + c64)
    crcs = rng.integers(0, 1 << 63, count, dtype=np.uint64) * 2 + rng.integers(0, 2, count, dtype=np.uint64)
    if not c64:
        crcs = (crcs >> np.uint64(32)).astype(np.uint32)
    lens = np.array([BIG_LENS[i % 4] if i % 3 == 0 else int(rng.integers(0, 70000)) for i in range(count)],
                    np.uint64)
    lens[5] = lens[6] = lens[7] = BIG_LENS[2]  # a run of equal large lengths
    crcs[9] = 0
    return crcs, lens


# ------------------------------------------------------------------- tests
def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    inc = os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc")
    header = open(os.path.join(inc, "crc32c_gpu.h")).read()
    for n, nargs in NAMES.items():
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == nargs, n
        assert f"int {n}(" in header, n
    assert "photon_crc_test_fold_parts" in exported
    assert "int photon_crc_test_fold_parts(" in open(os.path.join(inc, "tuning.h")).read()


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


B, P, C, N, S, O, T = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000  # never dereferenced


def test_null_arguments_are_einval():
    L = _native.lib()

    def bad(rc, what):
        assert rc == -22, what
        assert b"null" in L.photon_crc_last_error(), what

    bad(L.photon_crc64ecma_series_device(B, 8, 4, None, None), "series: d_crc_parts")
    bad(L.photon_crc64ecma_series_device(None, 8, 4, P, None), "series: d_buffer with part_size > 0")
    bad(L.photon_crc64ecma_series_device(B, 0, 4, None, None), "series: d_crc_parts, part_size 0")
    bad(L.photon_crc64ecma_combine_series_device(C, 8, 4, None, None), "combine_series: d_result")
    bad(L.photon_crc64ecma_combine_series_device(C, 8, 0, None, None), "combine_series: d_result, no parts")
    bad(L.photon_crc64ecma_combine_series_device(None, 8, 4, O, None), "combine_series: d_crc")
    for name in ("photon_crc32c_fold_parts_n", "photon_crc64ecma_fold_parts_n"):
        f = getattr(L, name)
        bad(f(C, N, S, 2, 8, 0, None, None, T, None), f"{name}: d_out")
        bad(f(None, N, S, 2, 8, 0, None, O, T, None), f"{name}: d_crc with parts")
        bad(f(C, None, S, 2, 8, 0, None, O, None, None), f"{name}: d_len with parts")
        bad(f(None, None, None, 1, 8, 0, None, O, None, None), f"{name}: d_crc, one object")
        bad(f(C, N, None, 2, 8, 0, None, O, None, None), f"{name}: null d_obj_start, nobj 2")
        bad(f(None, None, None, 3, 0, 0, None, O, None, None), f"{name}: null d_obj_start, nobj 3, no parts")
        bad(f(None, None, S, 1, 0, 0, None, None, None, None), f"{name}: d_out, no parts")
        assert f(None, None, None, 0, 0, 0, None, None, None, None) == 0  # nobj == 0: nothing is touched
        assert f(C, N, S, 0, 8, 5, S, None, None, None) == 0
    assert L.photon_crc64ecma_series_device(None, 8, 0, None, None) == 0  # n_parts == 0
    assert L.photon_crc_test_fold_parts(0, None, None, 3, 0, 64, ctypes.addressof(ctypes.c_uint64()), None) == -22
    assert L.photon_crc_test_fold_parts(0, None, None, 0, 0, 0, ctypes.addressof(ctypes.c_uint64()), None) == -22


def test_wrappers_raise():
    for call in (lambda: ck.series64_device(B, 8, 4, None),
                 lambda: ck.series64_device(None, 8, 4, P),
                 lambda: ck.combine_series64_device(C, 8, 4, None),
                 lambda: ck.combine_series64_device(None, 8, 4, O),
                 lambda: ck.fold_parts_device(C, N, S, 2, 8, None),
                 lambda: ck.fold_parts_device(C, N, None, 2, 8, O),
                 lambda: ck.fold_parts_device(None, N, None, 1, 8, O, seed=5),
                 lambda: ck.fold_parts64_device(C, N, S, 2, 8, None, total=T),
                 lambda: ck.fold_parts64_device(C, N, None, 0x100000000, 8, O),
                 lambda: ck.fold_parts64_device(C, None, None, 1, 8, O, seeds=S)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code == -22 and "null" in str(e.value)


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for call in (lambda: ck.series64_device(B, 8, 4, P),
                 lambda: ck.series64_device(None, 0, 4, P),
                 lambda: ck.combine_series64_device(C, 8, 4, O),
                 lambda: ck.combine_series64_device(None, 8, 0, O),
                 lambda: ck.fold_parts_device(C, N, S, 2, 8, O),
                 lambda: ck.fold_parts_device(C, N, None, 1, 8, O, seed=1, total=T),
                 lambda: ck.fold_parts64_device(C, N, S, 2, 8, O, seeds=S),
                 lambda: ck.fold_parts64_device(None, None, None, 1, 0, O)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code < 0


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_replay_real_parts(shapes, crc64):
    for sh in shapes:
        for seed in SEEDS[crc64]:
            for nt in THREADS:
                got, total = replay(crc64, sh.crc[crc64], sh.len, seed, nt)
                assert got == sh.want[crc64, seed], f"{sh.name}, seed {seed:#x}, {nt} threads: {got:#x}"
                assert total == sh.total, (sh.name, nt)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_reference_matches_oracle(shapes, crc64):
    # the bit-serial reference is the definition the synthetic cases are held to: pin it to the oracle
    for sh in shapes:
        if sh.len.size <= 1000:
            for seed in SEEDS[crc64]:
                assert gf_fold(sh.crc[crc64], sh.len, seed, crc64) == sh.want[crc64, seed], sh.name


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_replay_synthetic_lengths(crc64):
    crcs, lens = synthetic_pairs(crc64)
    assert all(n in lens for n in BIG_LENS)
    for seed in SEEDS[crc64]:
        want = gf_fold(crcs, lens, seed, crc64)
        for nt in THREADS:
            got, total = replay(crc64, crcs, lens, seed, nt)
            assert got == want, f"seed {seed:#x}, {nt} threads: {got:#x}, want {want:#x}"
            assert total == int(lens.astype(object).sum()) % (1 << 64)
    # one part of 4 GiB + 5 after a seed: one step, not two
    for seed in SEEDS[crc64]:
        got, _ = replay(crc64, crcs[:1], lens[5:6], seed, 64)
        assert got == gf_mul(seed, gf_xpow8(BIG_LENS[2], crc64), crc64) ^ int(crcs[0])

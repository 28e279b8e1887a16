"""photon_crc32c_xor_expect_n / photon_crc64ecma_xor_expect_n through the CPU
replay of the kernel (photon_crc_test_xor_expect,
photonlibos_amd/csrc/xor_expect.h), both CRCs: random stripes of 0..9 blocks of
0..5,000 bytes with random seeds, compared with the oracle's CRC of the XOR of
the blocks; the grouped and the uniform-k form; d_grp_start arrays that break
their rules; and lengths of 2^32 and beyond against the bit-serial GF(2)
multiply of tests/test_patch_abi.py. CPU only."""
import functools

import numpy as np
import pytest

from photonlibos_amd import _native
from tests.test_patch_abi import BITS, DT, shifted

BIG_LENS = (1 << 32, (1 << 32) + 1, (1 << 40) + 12345)


def crc_of(oracle, c64):
    return oracle.crc64ecma if c64 else oracle.crc32c


class Case:
    """Stripes of m_s blocks of n_s bytes under one seed: the stored CRCs of the
    blocks (the oracle's, from the seed), grouped, and the oracle's CRC of each
    stripe's XOR (n_s zero bytes for an empty stripe)."""

    def __init__(self, oracle, rng, nstripes, uniform_k=None):
        self.seed = {False: int(rng.integers(0, 1 << 32)), True: int(rng.integers(0, 1 << 63)) * 2 + 1}
        self.k = uniform_k
        self.m = [uniform_k if uniform_k else int(rng.integers(0, 10)) for _ in range(nstripes)]
        # every eighth stripe is empty or one byte: the ends of 0..5,000
        self.lens = np.array([int(rng.integers(0, 2)) if rng.integers(0, 8) == 0 else int(rng.integers(0, 5001))
                              for _ in range(nstripes)], np.uint64)
        self.start = np.concatenate([[0], np.cumsum(self.m)]).astype(np.uint64)
        self.crcs = {False: [], True: []}
        self.want = {False: [], True: []}
        for m, n in zip(self.m, self.lens):
            n = int(n)
            blocks = rng.integers(0, 256, (m, n), dtype=np.uint8)
            parity = np.bitwise_xor.reduce(blocks, axis=0) if m else np.zeros(n, np.uint8)
            for c64 in (False, True):
                crc, s = crc_of(oracle, c64), self.seed[c64]
                self.crcs[c64] += [crc(b, s) for b in blocks]
                self.want[c64].append(crc(parity, s))
        for c64 in (False, True):
            self.crcs[c64] = np.array(self.crcs[c64], DT[c64])
            self.want[c64] = np.array(self.want[c64], DT[c64])


@functools.lru_cache(maxsize=None)
def _fuzz_cases(oracle):
    rng = np.random.default_rng(0x0E7A5)
    cases = [Case(oracle, rng, int(rng.integers(1, 25))) for _ in range(30)]
    cases += [Case(oracle, rng, int(rng.integers(1, 12)), uniform_k=k) for k in (1, 2, 3, 4, 5, 8, 9)]
    return tuple(cases)


def fuzz_cases(oracle):
    """The cases shared by test_xor_expect_cpp.py and test_gpu_xor.py, computed once."""
    return _fuzz_cases(oracle)


def replay(c64, crcs, start, k, lens, nbytes, count, seed):
    L = _native.lib()
    crcs = np.ascontiguousarray(crcs, DT[c64])
    want = np.full(count, 0xA5, DT[c64])
    start = None if start is None else np.ascontiguousarray(start, np.uint64)
    lens = None if lens is None else np.ascontiguousarray(lens, np.uint64)
    rc = L.photon_crc_test_xor_expect(int(c64), crcs.ctypes.data if crcs.size else None, crcs.size,
                                      None if start is None else start.ctypes.data, k,
                                      None if lens is None else lens.ctypes.data, nbytes, count, seed,
                                      want.ctypes.data)
    assert rc == 0, L.photon_crc_last_error()
    return want


def test_fuzz_has_the_cases_it_names(oracle):
    cases = fuzz_cases(oracle)
    sizes = {m for c in cases for m in c.m}
    assert sizes == set(range(10))                                   # m = 0..9, even and odd
    assert any(n == 0 for c in cases for n in c.lens)
    assert any(c.k for c in cases) and any(not c.k for c in cases)


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_expected_word_is_the_oracles_crc_of_the_xor(oracle, c64):
    for i, c in enumerate(fuzz_cases(oracle)):
        n = len(c.m)
        got = replay(c64, c.crcs[c64], c.start, 0, c.lens, 0, n, c.seed[c64])
        assert np.array_equal(got, c.want[c64]), (i, "grouped")
        if c.k:  # the same stripes without d_grp_start
            got = replay(c64, c.crcs[c64], None, c.k, c.lens, 0, n, c.seed[c64])
            assert np.array_equal(got, c.want[c64]), (i, "uniform k")


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_one_length_for_every_stripe(oracle, c64):
    rng = np.random.default_rng(0x1E4)
    crc, seed = crc_of(oracle, c64), 0x5EED5EED
    for k, n in ((4, 4096), (3, 17), (2, 0), (5, 100)):
        blocks = rng.integers(0, 256, (6, k, n), dtype=np.uint8)
        crcs = [crc(b, seed) for s in blocks for b in s]
        want = np.array([crc(np.bitwise_xor.reduce(s, axis=0), seed) for s in blocks], DT[c64])
        assert np.array_equal(replay(c64, crcs, None, k, None, n, 6, seed), want), (k, n)


def bad_starts(start, ncrc):
    """d_grp_start arrays that break the rules: reversed, not from 0, far beyond ncrc, all equal."""
    start = np.asarray(start, np.uint64)
    huge = start * np.uint64(1000)
    huge[-1] = np.uint64(~0 & 0x7FFFFFFFFFFFFFFF)
    return [start[::-1].copy(), start + np.uint64(5), huge, np.full(start.size, ncrc // 2, np.uint64)]


def clamped(crcs, start, lens, seed, c64, zeros):
    """What the definition gives for any d_grp_start: both ends clamped into [0, ncrc]."""
    out = []
    for s in range(len(start) - 1):
        b = min(int(start[s + 1]), len(crcs))
        a = min(int(start[s]), b)
        x = 0
        for w in crcs[a:b]:
            x ^= int(w)
        if (b - a) % 2 == 0:
            x ^= zeros(int(lens[s]), seed)
        out.append(x)
    return np.array(out, DT[c64])


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_group_starts_that_break_the_rules_are_clamped(oracle, c64):
    crc = crc_of(oracle, c64)
    zeros = lambda n, seed: crc(bytes(n), seed)
    for i, c in enumerate(fuzz_cases(oracle)[:12]):
        n = len(c.m)
        # exactly-sized arrays: numpy's own bounds are not checked by the library, so the
        # values are compared with the definition (a read outside the array would change them
        # or fault; tests/test_xor_expect_cpp.py runs the same under a sanitizer)
        for j, st in enumerate(bad_starts(c.start, c.crcs[c64].size)):
            got = replay(c64, c.crcs[c64], st, 0, c.lens, 0, n, c.seed[c64])
            assert np.array_equal(got, clamped(c.crcs[c64], st, c.lens, c.seed[c64], c64, zeros)), (i, j)
    # the uniform-k form with fewer words than count * k
    c = fuzz_cases(oracle)[-1]
    short = c.crcs[c64][:c.k + 1]
    start = np.arange(len(c.m) + 1, dtype=np.uint64) * np.uint64(c.k)
    got = replay(c64, short, None, c.k, c.lens, 0, len(c.m), c.seed[c64])
    assert np.array_equal(got, clamped(short, start, c.lens, c.seed[c64], c64, zeros))


def zeros_word(n, seed, c64):
    """crc_extend(n zero bytes, seed) by the bit-serial multiply of tests/test_patch_abi.py."""
    mask = (1 << BITS[c64]) - 1
    inv = mask if c64 else 0
    return shifted(seed ^ inv, n, c64) ^ inv


def large_length_case(c64):
    """Synthetic words at the big lengths, groups of 0..4 words, with the expected words."""
    mask = (1 << BITS[c64]) - 1
    seed = 0xC0FFEE1234567895 & mask
    lens = list(BIG_LENS) + [0, 1, (1 << 32) - 1, 1 << 50, BIG_LENS[2]]
    sizes = [2, 0, 4, 1, 3, 2, 0, 2]
    words = [(0x9E3779B97F4A7C15 * (k + 1)) & mask for k in range(sum(sizes))]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    want = []
    for s, m in enumerate(sizes):
        x = 0
        for w in words[int(start[s]):int(start[s + 1])]:
            x ^= w
        if m % 2 == 0:
            x ^= zeros_word(lens[s], seed, c64)
        want.append(x)
    return np.array(words, DT[c64]), start, np.array(lens, np.uint64), seed, np.array(want, DT[c64])


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_zero_run_word_is_pinned_to_the_oracle(oracle, c64):
    crc = crc_of(oracle, c64)
    mask = (1 << BITS[c64]) - 1
    for n in (0, 1, 17, 100, 4096, 65536):
        for seed in (0, 1, 0xDEADBEEF12345678 & mask, mask):
            assert crc(bytes(n), seed) == zeros_word(n, seed, c64), (n, seed)


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_large_lengths(c64):
    words, start, lens, seed, want = large_length_case(c64)
    assert np.array_equal(replay(c64, words, start, 0, lens, 0, len(lens), seed), want)
    # one length for every stripe, uniform k = 2: every group is even
    for n in BIG_LENS:
        z = zeros_word(n, seed, c64)
        w = np.array([int(words[2 * s]) ^ int(words[2 * s + 1]) ^ z for s in range(4)], DT[c64])
        assert np.array_equal(replay(c64, words[:8], None, 2, None, n, 4, seed), w), n

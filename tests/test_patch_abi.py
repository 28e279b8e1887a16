"""photon_crc32c_patch_n / photon_crc64ecma_patch_n through the CPU replay of
the kernel (photon_crc_test_patch, photonlibos_amd/csrc/patch_crc.h), both
CRCs: random objects of blocks with non-overlapping sub-range writes, patched
per block and per object and compared with the oracle's CRC of the modified
bytes; and tails of 2^32 and beyond against a bit-serial GF(2) multiply
written here and pinned to the oracle first. CPU only."""
import functools

import numpy as np
import pytest

from photonlibos_amd import _native

SEED = {False: 0xDEADBEEF, True: 0x0123456789ABCDEF}
DT = {False: np.uint32, True: np.uint64}
THREADS = (1, 3, 64, 256)
BIG_TAILS = (1 << 32, (1 << 32) + 1, (1 << 40) + 12345, 1 << 63)


def crc_of(oracle, c64):
    return oracle.crc64ecma if c64 else oracle.crc32c


class Case:
    """An object of blocks, old and new bytes, and the writes cut at block ends
    into pieces (block, start, end), in address order."""

    def __init__(self, oracle, rng, nblocks, max_block, nwrites):
        self.sizes = rng.integers(1, max_block + 1, nblocks)
        self.ends = np.cumsum(self.sizes)
        self.total = int(self.ends[-1])
        self.old = rng.integers(0, 256, self.total, dtype=np.uint8)
        self.new = self.old.copy()
        # nwrites non-overlapping ranges from 2 * nwrites sorted cut points; some
        # end on a block's end (tail 0), some are empty, one may cover whole blocks
        cuts = np.sort(rng.integers(0, self.total + 1, 2 * nwrites))
        ranges = []
        for a, b in zip(cuts[0::2], cuts[1::2]):
            a, b = int(a), int(b)
            if rng.integers(0, 4) == 0 and b > a:  # move the end to the end of the block that holds byte b - 1
                b = int(self.ends[np.searchsorted(self.ends, b - 1, side="right")])
            ranges.append((a, b))
        # (a range moved into the next one: the next one starts behind it)
        self.pieces = []
        last = 0
        for a, b in ranges:
            a = max(a, last)
            b = max(a, b)
            last = b
            self.new[a:b] = rng.integers(0, 256, b - a, dtype=np.uint8)
            if a == b:
                blk = min(int(np.searchsorted(self.ends, a, side="right")), nblocks - 1)
                self.pieces.append((blk, a, b))
            while a < b:
                blk = int(np.searchsorted(self.ends, a, side="right"))
                e = min(b, int(self.ends[blk]))
                self.pieces.append((blk, a, e))
                a = e
        self.nblocks = nblocks
        self.starts = np.concatenate([[0], self.ends[:-1]])
        self.block_start = np.searchsorted([p[0] for p in self.pieces], np.arange(nblocks + 1)).astype(np.uint64)
        self.block_tail = np.array([int(self.ends[k]) - e for k, _, e in self.pieces], np.uint64)
        self.object_tail = np.array([self.total - e for _, _, e in self.pieces], np.uint64)
        self.delta, self.block_old, self.block_new, self.object_old, self.object_new, self.alone = {}, {}, {}, {}, {}, {}
        for c64 in (False, True):
            crc, s = crc_of(oracle, c64), SEED[c64]
            self.delta[c64] = np.array([crc(self.old[a:e], s) ^ crc(self.new[a:e], s) for _, a, e in self.pieces],
                                       DT[c64])
            blocks = lambda data: np.array([crc(data[a:e], s) for a, e in zip(self.starts, self.ends)], DT[c64])
            self.block_old[c64], self.block_new[c64] = blocks(self.old), blocks(self.new)
            self.object_old[c64] = np.array([crc(self.old, s)], DT[c64])
            self.object_new[c64] = np.array([crc(self.new, s)], DT[c64])
            # piece i applied alone to its block (a null tgt_start: write i patches word i)
            alone = []
            for k, a, e in self.pieces:
                blk = self.old[self.starts[k]:self.ends[k]].copy()
                blk[a - self.starts[k]:e - self.starts[k]] = self.new[a:e]
                alone.append(crc(blk, s))
            self.alone[c64] = np.array(alone, DT[c64])


@functools.lru_cache(maxsize=None)
def _fuzz_cases(oracle):
    rng = np.random.default_rng(0x9A7C4)
    cases = [Case(oracle, rng, int(rng.integers(1, 41)), int(rng.integers(1, 5001)), int(rng.integers(0, 13)))
             for _ in range(40)]
    cases.append(Case(oracle, rng, 1, 1, 3))       # one block of one byte
    cases.append(Case(oracle, rng, 40, 16, 12))    # writes spanning many whole blocks
    cases.append(Case(oracle, rng, 7, 5000, 0))    # no write: every group is empty
    return tuple(cases)


def fuzz_cases(oracle):
    """The cases shared by test_patch_cpp.py and test_gpu_overwrite.py, computed once."""
    return _fuzz_cases(oracle)


def replay(c64, delta, tail, tgt_start, ntgt, crc_in, nthreads, in_place=False):
    L = _native.lib()
    delta, tail = np.ascontiguousarray(delta, DT[c64]), np.ascontiguousarray(tail, np.uint64)
    out = np.array(crc_in, DT[c64]) if in_place else np.full(ntgt, 0xA5, DT[c64])
    src = out if in_place else np.ascontiguousarray(crc_in, DT[c64])
    start = None if tgt_start is None else np.ascontiguousarray(tgt_start, np.uint64)
    rc = L.photon_crc_test_patch(int(c64), delta.ctypes.data, tail.ctypes.data, delta.size,
                                 None if start is None else start.ctypes.data, ntgt, src.ctypes.data,
                                 out.ctypes.data, nthreads)
    assert rc == 0, L.photon_crc_last_error()
    return out


def test_fuzz_has_the_cases_it_names(oracle):
    cases = fuzz_cases(oracle)
    pieces = [p for c in cases for p in c.pieces]
    assert any(t == 0 for c in cases for t in c.block_tail)                       # a write ends at a block's end
    assert any(a == c.starts[k] and e == c.ends[k] for c in cases for k, a, e in c.pieces)  # a whole block
    assert any(a == e for _, a, e in pieces)                                      # an empty write
    assert any(np.any(np.diff(c.block_start.astype(np.int64)) == 0) for c in cases)  # an empty group
    assert any(not c.pieces for c in cases)


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_patch_blocks_and_objects_match_the_oracle(oracle, c64):
    for i, c in enumerate(fuzz_cases(oracle)):
        nt = THREADS[i % len(THREADS)]
        in_place = bool(i & 1)
        got = replay(c64, c.delta[c64], c.block_tail, c.block_start, c.nblocks, c.block_old[c64], nt, in_place)
        assert np.array_equal(got, c.block_new[c64]), (i, "blocks")
        start = np.array([0, len(c.pieces)], np.uint64)
        got = replay(c64, c.delta[c64], c.object_tail, start, 1, c.object_old[c64], nt, not in_place)
        assert np.array_equal(got, c.object_new[c64]), (i, "object")
        if c.pieces:  # a null tgt_start: write i patches word i
            words = c.block_old[c64][[k for k, _, _ in c.pieces]]
            got = replay(c64, c.delta[c64], c.block_tail, None, len(c.pieces), words, nt, in_place)
            assert np.array_equal(got, c.alone[c64]), (i, "null tgt_start")


# ---- tails of 2^32 and more: a bit-serial multiply of this file's own
POLY = {False: 0x82F63B78, True: 0xC96C5795D7870F42}
BITS = {False: 32, True: 64}


def gf_mul(a, b, c64):
    """a * b mod P, reflected: bit (w - 1 - j) is the coefficient of x^j."""
    r = 0
    for _ in range(BITS[c64]):
        r = (r >> 1) ^ (POLY[c64] if r & 1 else 0) ^ (a if b & 1 else 0)
        b >>= 1
    return r


def gf_xpow(n, c64):
    result, base = 1 << (BITS[c64] - 1), 1 << (BITS[c64] - 2)
    while n:
        if n & 1:
            result = gf_mul(result, base, c64)
        base = gf_mul(base, base, c64)
        n >>= 1
    return result


def shifted(delta, tail, c64):
    return gf_mul(delta, gf_xpow(8 * tail, c64), c64)


def large_tail_case(c64):
    """Synthetic deltas at the big tails (and 0 and 1 beside them), three targets, with the expected words."""
    mask = (1 << BITS[c64]) - 1
    deltas = [(0x9E3779B97F4A7C15 * (k + 1)) & mask for k in range(len(BIG_TAILS) + 3)] + [0]
    tails = list(BIG_TAILS) + [0, 1, (1 << 32) - 1, 1 << 50]
    start = [0, 3, 3, len(deltas)]
    crc_in = [0x1111111111111111 & mask, 0x2222222222222222 & mask, 0]
    want = list(crc_in)
    for t in range(3):
        for i in range(start[t], start[t + 1]):
            want[t] ^= shifted(deltas[i], tails[i], c64)
    return (np.array(deltas, DT[c64]), np.array(tails, np.uint64), np.array(start, np.uint64),
            np.array(crc_in, DT[c64]), np.array(want, DT[c64]))


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_multiply_is_pinned_to_the_oracle(oracle, c64):
    mask = (1 << BITS[c64]) - 1
    for n in (0, 1, 2, 15, 16, 17, 100, 4096, 65535, 65536):
        for reg in (1, 0x80000000, 0xDEADBEEF12345678 & mask, mask):
            want = shifted(reg, n, c64)
            zeros = bytes(n)
            if c64:  # crc64ecma_extend inverts the register on the way in and out
                assert oracle.crc64ecma(zeros, reg ^ mask) ^ mask == want, (n, reg)
            else:
                assert oracle.crc32c(zeros, reg) == want, (n, reg)


@pytest.mark.parametrize("c64", [False, True], ids=["crc32c", "crc64"])
def test_large_tails(c64):
    deltas, tails, start, crc_in, want = large_tail_case(c64)
    for nt in THREADS:
        assert np.array_equal(replay(c64, deltas, tails, start, 3, crc_in, nt), want), nt
    # one write per word
    alone = np.array([shifted(int(d), int(t), c64) for d, t in zip(deltas, tails)], DT[c64])
    got = replay(c64, deltas, tails, None, deltas.size, np.zeros(deltas.size, DT[c64]), 64, in_place=True)
    assert np.array_equal(got, alone)

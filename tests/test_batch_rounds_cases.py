"""The case generators of tests/test_gpu_batch_rounds.py, checked without a
device: the arithmetic the GPU tests rely on -- three rounds of every grid,
every length class and message shape in each full round, other work for a
wavefront position in each round, both states of the fold-basis cache, all
source ranges inside the pool, every case within the memory budget.

A round here is one pass of the grid: pass_waves() wavefronts of 64 / g lane
groups. Rounds one and two are full; round three has 64 / g + 1 units (two at
64 lanes), fewer than there are classes, so "every class" is asserted for the
full rounds and the third round's shape is asserted on its own."""
import numpy as np
import pytest

from tests.test_gpu_batch_rounds import (AUTO_NBYTES, BUDGET, GS, K_WAVES, LONG_EVERY, POOL, SHORT_COUNTS, batch_lens,
                                         full_row_auto_shape, full_row_shape, fused_msgs, generic64_shape, iov_cases,
                                         msg_lens, pass_waves, shape_index, strided_cases, two_kernel_msgs, units)

CUS = [64, 256, 304]


def _grid_rounds(count, g, cus, capped):
    """batch_grid() of crc32c_device.hip and the rounds of its persistent loop:
    (rounds, wavefronts of the last round, active groups of the last wavefront)."""
    gpw = 64 // g
    waves = -(-count // gpw)
    grid = min(-(-waves // K_WAVES), cus)
    if capped:
        grid = min(grid, 1)
    nwaves = grid * K_WAVES
    assert nwaves == pass_waves(cus, capped)
    rounds = -(-waves // nwaves)
    return rounds, waves - (rounds - 1) * nwaves, count - (waves - 1) * gpw


@pytest.mark.parametrize("capped", [True, False])
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("cus", CUS)
def test_units_give_three_rounds(cus, g, capped):
    count = units(cus, g, capped)
    assert _grid_rounds(count, g, cus, capped) == (3, 2, 1)
    # one unit fewer ends on a full wavefront, one pass fewer is two rounds
    assert _grid_rounds(count - 1, g, cus, capped) == (3, 1, 64 // g)
    assert _grid_rounds(count - (64 // g) - 1, g, cus, capped)[0] == 2


def test_unit_counts_of_a_256_cu_device():
    assert units(256, 64, False) == 8194 and units(256, 4, False) == 131089
    assert units(256, 64, True) == 34 and units(256, 4, True) == 529


def _classes_per_round(cls, per, k):
    """Every class in each full round, and another class for a place in the next round."""
    for rnd in (0, 1):
        assert set(cls[rnd * per:(rnd + 1) * per].tolist()) == set(range(k)), rnd
    assert (cls[:per] != cls[per:2 * per]).all()
    tail = cls[2 * per:]
    assert (tail != cls[:tail.size]).all() and (tail != cls[per:per + tail.size]).all()


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("cus", CUS)
def test_shape_index_moves_on_every_round(cus, g):
    for capped, k in ((True, 8), (False, len(SHORT_COUNTS))):
        per = pass_waves(cus, capped) * (64 // g)
        _classes_per_round(shape_index(units(cus, g, capped), per, k), per, k)


@pytest.mark.parametrize("u", [2, 4, 8])
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("cus", CUS)
def test_plain_batch_cases(cus, g, u):
    table = batch_lens(g, u)
    assert len(set(table)) == (7 if g == 4 else 8)  # at 4 lanes 16 g - 1 is 63 again
    offs, lens, cls = iov_cases(cus, g, u)
    per = K_WAVES * (64 // g)
    assert lens.size == units(cus, g, True) and (lens == np.asarray(table)[cls]).all()
    _classes_per_round(cls, per, 8)
    assert (offs >= 0).all() and (offs + lens <= POOL).all()
    for c in range(3, 8):  # every length of 64 bytes or more at every alignment
        assert set((offs[cls == c] % 16).tolist()) == {0, 5, 15}, c
    forms = strided_cases(cus, g, u)
    assert sorted({f[2] for f in forms}) == sorted({64, 2 * 16 * g * u, 3 * 16 * g * u + 48, 5000})
    for base, stride, nbytes, count, seeded in forms:
        assert count == units(cus, g, True) and stride >= nbytes
        assert base + (count - 1) * stride + nbytes <= POOL
        if seeded:
            assert base % 16 and stride % 2 == 1
        else:  # what batch_strided<> asks of the shift_init path
            assert base % 16 == 0 and stride % 16 == 0 and nbytes >= 64
    assert {f[2] for f in forms if f[4]} == {f[2] for f in forms if not f[4]}


@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("cus", CUS)
def test_two_kernel_message_cases(cus, g):
    lay = two_kernel_msgs(cus, g)
    start = lay["start"].astype(np.int64)
    assert start[0] == 0 and start[-1] == lay["lens"].size == units(cus, g, True)
    cnt = np.diff(start)
    assert cnt.min() == 0 and cnt.max() == 5 and set(cnt.tolist()) == set(range(6))
    assert cnt[-1] == 0
    assert (lay["offs"] + lay["lens"] <= POOL).all()


def _has_rebuild_pattern(lens):
    """a, a, b, a somewhere in the message: the basis built, hit, rebuilt and rebuilt again."""
    x = np.asarray(lens)
    return bool(((x[:-3] == x[1:-2]) & (x[2:-1] != x[:-3]) & (x[3:] == x[:-3])).any())


@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("g", GS)
@pytest.mark.parametrize("cus", CUS)
def test_fused_message_cases(cus, g, r):
    table = msg_lens(g, r)
    assert len(set(table)) == 8
    lay = fused_msgs(cus, g, r)
    cnt, per, lens = lay["cnt"], lay["per"], lay["lens"]
    start = lay["start"].astype(np.int64)
    nmsg = cnt.size
    assert nmsg == units(cus, g, False) and per == pass_waves(cus, False) * (64 // g)
    assert (np.diff(start) == cnt).all() and start[-1] == lens.size == lay["offs"].size
    # shapes: 0, 1, 2, 3 and long (4) in both full rounds; the two empty messages
    shape = np.where(cnt > 3, 4, cnt)
    assert ((cnt <= 3) | ((cnt >= 17) & (cnt <= 40))).all()
    for rnd in (0, 1):
        assert set(shape[rnd * per:(rnd + 1) * per].tolist()) == {0, 1, 2, 3, 4}, rnd
    assert cnt[per] == 0 and cnt[nmsg - 1] == 0
    longs = np.flatnonzero(cnt >= 17)
    assert (longs % LONG_EVERY == 0).all() and longs.size >= nmsg // LONG_EVERY - 2
    assert cnt.max() > 32  # at 4 lanes nine store events of a lane in one message: its two held stores wrap
    # another shape for every place in the next round
    assert (shape[:per] != shape[per:2 * per]).all()
    tail = shape[2 * per:]
    assert ((tail != shape[:tail.size]) | (tail != shape[per:per + tail.size])).all()
    # every length in both full rounds
    for rnd in (0, 1):
        seen = lens[start[rnd * per]:start[(rnd + 1) * per]]
        assert set(seen.tolist()) == set(table), rnd
    # the fold-basis cache inside a message: built, hit, rebuilt, rebuilt again -- in every round it can be
    for rnd in (0, 1):
        k = longs[(longs >= rnd * per) & (longs < (rnd + 1) * per)]
        assert k.size and all(_has_rebuild_pattern(lens[start[m]:start[m + 1]]) for m in k), rnd
    # ... and across the messages of a lane group: the previous one is m - per
    m = np.arange(per, nmsg)
    m = m[(cnt[m] > 0) & (cnt[m - per] > 0)]
    same = lens[start[m]] == lens[start[m - per + 1] - 1]
    carried = m % 3 == 0
    assert same[carried].all() and carried.sum() > 16
    assert (~same).sum() > 16
    # both already in round two (round three has 64 / g + 1 messages)
    assert same[m < 2 * per].any() and (~same[m < 2 * per]).any()
    # sources inside the pool, the batch within the budget
    assert (lay["offs"] >= 0).all() and (lay["offs"] + lens <= POOL).all()
    assert int(lens.sum()) <= BUDGET


@pytest.mark.parametrize("g", GS)
def test_device_memory_of_a_256_cu_device(g):
    for rows in (2, 4):
        for k in (1, 2):
            nbytes, count = full_row_shape(256, g, rows, k)
            assert nbytes % (2 * 16 * g * rows) == 0 and nbytes // (16 * g * rows) == 2 * k
            assert nbytes * count + 64 <= BUDGET, (g, rows, k)
    base, stride, nbytes, count = generic64_shape(256, g)
    assert base % 16 and nbytes % 16 and stride >= nbytes
    assert base + (count - 1) * stride + nbytes + 64 <= BUDGET
    for r in (2, 4):  # descriptors, starts, seeds and both outputs of the largest message batch
        lay = fused_msgs(256, g, r)
        assert POOL + 16 * lay["lens"].size + 8 * lay["start"].size + 12 * lay["cnt"].size + 4 * lay["lens"].size <= BUDGET


def test_largest_and_smallest_full_row_cases():
    assert full_row_shape(256, 64, 4, 2) == (16384, 8194)
    assert full_row_shape(256, 4, 2, 1) == (256, 131089)


@pytest.mark.parametrize("cus", CUS)
def test_full_row_auto_case(cus):
    nbytes, stride, count = full_row_auto_shape(cus)
    # what launch_batch(const Batch64Args&) asks for 8 lanes, 4 rows and the full-row kernel
    assert nbytes == AUTO_NBYTES == 8192 and nbytes % (2 * 16 * 8 * 4) == 0
    assert stride % 16 == 0 and 0 < stride
    assert count == units(cus, 8, False)
    if cus == 256:
        assert (count - 1) * stride + nbytes + 64 <= BUDGET

"""Several rounds of the persistent loop of the CRC-only batch kernels: the
CRC-64 full-row kernel (all 20 builds and the automatic 8 KiB one), the
CRC-32C plain batch at every lane-group size and rows per step (the iovec,
strided and two-kernel message forms), the fused message forms at every
lane-group size, and the CRC-64 generic batch.

A wavefront takes unit wv, then wv + waves of the grid, and so on. The plain
CRC-32C launcher honours set_batch_grid(1): a pass is the 16 wavefronts of one
workgroup. The CRC-64 plain batch and the fused message form do not: their
grid is one workgroup per CU, so their rounds are produced by count,
16 * CUs wavefronts per pass. units() gives every build three rounds: two full
passes, then two wavefronts, the last with one active lane group.

Every CRC is bit-exact against the pinned oracle (tests/_oracle.py) over the
HOST copy of the data, one C call per launch. Outputs are pre-filled with -1
and one element longer than the batch; the tail element must stay untouched.
The case generators are plain numpy code (no device) and are checked on their
own in tests/test_batch_rounds_cases.py."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen

pytestmark = pytest.mark.gpu

POOL = 4 << 20
GS = [4, 8, 16, 32, 64]
K_WAVES = 16  # wavefronts of a workgroup (kWaves)
BUDGET = 160 << 20  # bytes of the largest device allocation of a case
SEED64 = 0xFEDCBA9876543210
SEED32 = 0x9E3779B9


# ------------------------------------------------------------ host-side cases

def pass_waves(cus, capped):
    """Wavefronts of one pass of the grid: one workgroup under set_batch_grid(1), else one per CU."""
    return K_WAVES if capped else K_WAVES * cus


def units(cus, g, capped):
    """Units (buffers, segments or messages) that give the grid three rounds:
    two full passes, then two wavefronts, the last with one active group."""
    gpw = 64 // g
    return 2 * pass_waves(cus, capped) * gpw + gpw + 1


def shape_index(count, per, k):
    """The shape of unit i: (i + i // per) % k, so the cycle moves on by one per
    round and a wavefront position meets other work in each round."""
    i = np.arange(count, dtype=np.int64)
    return (i + i // per) % k


def default_rows(g):
    return 2 if g == 16 else 4


def full_row_shape(cus, g, rows, k):
    """CRC-64 full-row kernel: (nbytes, count) of k step pairs per buffer."""
    return 2 * 16 * g * rows * k, units(cus, g, False)


AUTO_NBYTES, AUTO_STRIDE = 8192, 2048


def full_row_auto_shape(cus):
    """The automatic build for 8 KiB buffers (8 lanes, 4 rows, prefetch):
    (nbytes, stride, count). 65,545 buffers of 8 KiB laid end to end would be
    537 MB; shorter buffers would take another build. The buffers overlap
    instead: a 16-byte-aligned stride of 2 KiB, every buffer another window."""
    return AUTO_NBYTES, AUTO_STRIDE, units(cus, 8, False)


def batch_lens(g, u):
    """Length classes of the plain batch: empty, tiny, under and at one block row,
    and bodies of U-row steps with and without lead rows, partial rows and tails."""
    return [0, 1, 63, 64, 16 * g - 1, 16 * g * u + 17, 16 * g * (2 * u + 1) + 5, 16 * g * (3 * u + 2)]


def _pool_offsets(count):
    """Alignments 0, 5 and 15 mod 16, moving on every eight units: a block of eight
    holds every length class once, so each class meets all three."""
    i = np.arange(count, dtype=np.int64)
    return 4096 * (i % 61) + 16 * (i % 5) + np.asarray([0, 5, 15], np.int64)[i // 8 % 3]


def iov_cases(cus, g, u):
    """Plain batch, iovec form, capped grid: (pool offsets, lengths, class of every buffer)."""
    count, per = units(cus, g, True), pass_waves(cus, True) * (64 // g)
    cls = shape_index(count, per, 8)
    return _pool_offsets(count), np.asarray(batch_lens(g, u), np.int64)[cls], cls


def strided_cases(cus, g, u):
    """Plain batch, strided form, capped grid: (base, stride, nbytes, count, seeded).
    A 16-byte-aligned base and stride without seeds is the shift_init path; base + 5
    with an odd stride and per-buffer seeds the seeded one."""
    count = units(cus, g, True)
    out = []
    for nbytes in (64, 2 * 16 * g * u, 3 * 16 * g * u + 48, 5000):
        out.append((0, (nbytes + 15) // 16 * 16 + 16, nbytes, count, False))
        out.append((5, nbytes + 3, nbytes, count, True))
    return out


def two_kernel_msgs(cus, g):
    """Two-kernel message form under the cap: units(cus, g, True) segments with
    the plain batch's length cycle, over messages of 0 to 5 segments."""
    offs, lens, cls = iov_cases(cus, g, default_rows(g))
    nseg = lens.size
    start, m = [0], 0
    while start[-1] < nseg:
        start.append(min(nseg, start[-1] + m % 6))
        m += 1
    start.append(nseg)  # an empty message at the end
    return {"offs": offs, "lens": lens, "cls": cls, "start": np.asarray(start, np.uint64)}


LONG_EVERY = 50  # every 50th message is a long one
SHORT_COUNTS = [0, 1, 2, 3]


def msg_lens(g, r):
    """Segment lengths of the fused message forms (r rows per step)."""
    return [0, 1, 15, 16, 16 * g - 1, 16 * g, 16 * g * r + 17, 2 * 16 * g * r]


def fused_msgs(cus, g, r):
    """Fused message forms, uncapped: three rounds of messages.
    * 0 to 3 segments by the shape cycle; every 50th message 17 to 40 segments,
      so a lane's held segment-CRC stores wrap several times; the first message
      of round two and the last of the batch are empty.
    * Lengths drawn from msg_lens. Segments 1..4 of a long message are
      a, a, b, a: the fold basis is built, hit, rebuilt, and rebuilt again.
    * In rounds two and three every third message of a lane group that follows
      a non-empty one (message m - per) opens with the length that one closed
      with; the others open with a drawn length."""
    rs = np.random.RandomState(0xB7C0 + 131 * g + r)
    nmsg, per = units(cus, g, False), pass_waves(cus, False) * (64 // g)
    m = np.arange(nmsg, dtype=np.int64)
    cnt = np.asarray(SHORT_COUNTS, np.int64)[shape_index(nmsg, per, len(SHORT_COUNTS))]
    long_ = m % LONG_EVERY == 0
    cnt[long_] = rs.randint(17, 41, int(long_.sum()))
    cnt[per] = 0
    cnt[nmsg - 1] = 0
    long_ &= cnt > 0
    start = np.zeros(nmsg + 1, np.int64)
    np.cumsum(cnt, out=start[1:])
    nseg = int(start[-1])
    table = np.asarray(msg_lens(g, r), np.int64)
    li = rs.randint(0, table.size, nseg)
    s = start[:-1][long_]
    a = rs.randint(0, table.size, s.size)
    b = (a + 1 + rs.randint(0, table.size - 1, s.size)) % table.size
    li[s + 1], li[s + 2], li[s + 3], li[s + 4] = a, a, b, a
    lens = table[li]
    first, last = start[:-1], start[1:] - 1
    for rnd in (1, 2):  # in round order: a carried length may be carried on
        k = m[rnd * per:(rnd + 1) * per]
        k = k[(k % 3 == 0) & (cnt[k] > 0) & (cnt[k - per] > 0)]
        lens[first[k]] = lens[last[k - per]]
    offs = rs.randint(0, POOL - int(table.max()), nseg).astype(np.int64)
    return {"cnt": cnt, "start": start.astype(np.uint64), "lens": lens, "offs": offs, "per": per}


def generic64_shape(cus, g):
    """CRC-64 generic batch: (base, stride, nbytes, count), nothing aligned."""
    nbytes = 16 * g * 2 + 5
    return 5, nbytes + 3, nbytes, units(cus, g, False)


# ------------------------------------------------------------------- fixtures

@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def dev_pool(dev):
    torch, cus = dev
    host = datagen.stream_bytes(0xB7C1, POOL)
    d = torch.from_numpy(host.copy()).cuda()
    assert d.data_ptr() % 16 == 0
    return torch, cus, host, d


@pytest.fixture(autouse=True)
def _reset():
    yield
    ck.set_lanes_per_buffer(0)
    ck.set_generic_rows(-1)
    ck.set_msg_mode(0)
    ck.set_msg_rows(2)
    ck.set_full_rows64(3, 2)
    ck.set_batch_grid(0)


def _i64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def _i32(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).cuda()


def _out(torch, n, dtype):
    return torch.full((n + 1,), -1, dtype=dtype, device="cuda")


def _check(out, ref, per, what, unit="buffer"):
    """out: n + 1 words pre-filled with -1; ref: the n expected ones."""
    got = out.cpu().numpy().view(ref.dtype)
    n = ref.size
    bad = np.flatnonzero(got[:n] != ref)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {unit} {i} (round {i // per}, place {i % per} of {per}) is {int(got[i]):#x}, "
                             f"want {int(ref[i]):#x}; {bad.size} of {n} differ")
    assert int(got[n]) == int(np.iinfo(ref.dtype).max), f"{what}: the word behind the last {unit} was written"


def _iov(base, offs, lens):
    iov = np.zeros((len(lens), 2), np.uint64)
    iov[:, 0] = np.uint64(base) + np.asarray(offs, np.uint64)
    iov[:, 1] = np.asarray(lens, np.uint64)
    return iov


def _buffer_crcs(oracle, host, offs, lens, seeds, seed0):
    """CRC of host[o:o+n] per buffer, seeded per buffer or with seed0 (one C call)."""
    return oracle.msg_chain(_iov(host.ctypes.data, offs, lens), np.arange(len(lens) + 1, dtype=np.uint64),
                            seeds=seeds, seed0=seed0)


def _seeds32(n, salt):
    s = np.random.RandomState(salt).randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s[::4] = 0
    return s


# ------------------------------------------- 1: CRC-64 full-row kernel, rounds

def _run_full64(torch, oracle, nbytes, stride, count, per, fill, what):
    size = (count - 1) * stride + nbytes
    assert size + 64 <= BUDGET, (size, what)
    d = torch.empty(size + 64, dtype=torch.uint8, device="cuda")
    assert d.data_ptr() % 16 == 0
    # one stream over the whole span: overlapping buffers are windows of it
    ck.fill_splitmix(d, size, size, 1, fill)
    host = d.cpu().numpy()
    for seed in (0, SEED64):
        out = _out(torch, count, torch.int64)
        ck.batch64_strided(d, stride, nbytes, count, out, seed=seed)
        torch.cuda.synchronize()
        _check(out, oracle.crc64ecma_strided(host, stride, nbytes, count, seed), per,
               f"{what}, {count} x {nbytes} B every {stride}, seed {seed:#x}")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("rows", [2, 4])
@pytest.mark.parametrize("g", GS)
def test_full_row_rounds(dev, oracle, g, rows, mode):
    """crc64_full_kernel<G, U, XB> past `if (!more) break`: the next round's
    pointer, the reload of a[] behind the store (mode 1) or the select between
    the buffer's third step and the next buffer (mode 2), and the groups past
    the end of the batch in round three. One step pair per buffer (the select
    goes straight to the next buffer) and two (the loop runs once)."""
    torch, cus = dev
    ck.set_full_rows64(mode, rows)
    ck.set_lanes_per_buffer(g)
    for k in (1, 2):
        nbytes, count = full_row_shape(cus, g, rows, k)
        _run_full64(torch, oracle, nbytes, nbytes, count, pass_waves(cus, False) * (64 // g),
                    0x6B00 + 64 * g + 8 * rows + k, f"lanes {g}, rows {rows}, mode {mode}")


def test_full_row_rounds_auto(dev, oracle):
    """The build the automatic mode takes for 8 KiB buffers (8 lanes, 4 rows,
    prefetch), eight steps per buffer; overlapping buffers (full_row_auto_shape)."""
    torch, cus = dev
    assert ck.lanes_for(AUTO_NBYTES) == 8
    nbytes, stride, count = full_row_auto_shape(cus)
    _run_full64(torch, oracle, nbytes, stride, count, pass_waves(cus, False) * 8, 0x6B0A, "automatic")


# --------------------------------- 2: CRC-32C plain batch, one workgroup, rounds

@pytest.mark.parametrize("seeding", ["seeds", "seed0", "none"])
@pytest.mark.parametrize("u", [2, 4, 8])
@pytest.mark.parametrize("g", GS)
def test_plain_iov_rounds(dev_pool, oracle, g, u, seeding):
    """crc32c_batch_kernel<G, U, 0, false> over three rounds on one workgroup:
    at 32 and 64 lanes with 2 or 4 rows the overlap loop, whose first buffer is
    loaded across the table barrier and every later one in the `!first` branch."""
    torch, cus, host, d = dev_pool
    offs, lens, _ = iov_cases(cus, g, u)
    count = lens.size
    seeds = _seeds32(count, 0x5EED + g + u) if seeding == "seeds" else None
    seed0 = SEED32 if seeding == "seed0" else 0
    ck.set_lanes_per_buffer(g)
    ck.set_generic_rows(u)
    ck.set_batch_grid(1)
    out = _out(torch, count, torch.int32)
    ck.batch_iov(_i64(torch, _iov(d.data_ptr(), offs, lens)), count, out, seed=seed0,
                 seeds=None if seeds is None else _i32(torch, seeds))
    torch.cuda.synchronize()
    _check(out, _buffer_crcs(oracle, host, offs, lens, seeds, seed0), K_WAVES * (64 // g),
           f"lanes {g}, rows {u}, {seeding}")


@pytest.mark.parametrize("u", [2, 4, 8])
@pytest.mark.parametrize("g", GS)
def test_plain_strided_rounds(dev_pool, oracle, g, u):
    torch, cus, host, d = dev_pool
    ck.set_lanes_per_buffer(g)
    ck.set_generic_rows(u)
    ck.set_batch_grid(1)
    for base, stride, nbytes, count, seeded in strided_cases(cus, g, u):
        assert base + (count - 1) * stride + nbytes <= POOL
        seeds = _seeds32(count, 0x57 + nbytes) if seeded else None
        out = _out(torch, count, torch.int32)
        ck.batch_strided(d.data_ptr() + base, stride, nbytes, count, out, seed=SEED32,
                         seeds=None if seeds is None else _i32(torch, seeds))
        torch.cuda.synchronize()
        ref = _buffer_crcs(oracle, host, base + stride * np.arange(count, dtype=np.int64),
                           np.full(count, nbytes, np.int64), seeds, SEED32)
        _check(out, ref, K_WAVES * (64 // g),
               f"lanes {g}, rows {u}, {count} x {nbytes} B every {stride} from {base}, seeds {seeded}")


@pytest.mark.parametrize("g", GS)
def test_two_kernel_message_rounds(dev_pool, oracle, g):
    """set_msg_mode(2): the segments go through the plain batch's launcher, under
    the cap three rounds of them, and a second kernel folds them per message."""
    torch, cus, host, d = dev_pool
    lay = two_kernel_msgs(cus, g)
    nseg, nmsg = lay["lens"].size, lay["start"].size - 1
    seeds = _seeds32(nmsg, 0x2C + g)
    ck.set_msg_mode(2)
    ck.set_lanes_per_buffer(g)
    ck.set_batch_grid(1)
    out, seg = _out(torch, nmsg, torch.int32), _out(torch, nseg, torch.int32)
    ck.batch_msg_n(_i64(torch, _iov(d.data_ptr(), lay["offs"], lay["lens"])), _i64(torch, lay["start"]), nmsg, nseg,
                   seg, out, seeds=_i32(torch, seeds))
    torch.cuda.synchronize()
    host_iov = _iov(host.ctypes.data, lay["offs"], lay["lens"])
    _check(seg, oracle.crc32c_iov(host_iov), K_WAVES * (64 // g), f"lanes {g}", "segment")
    _check(out, oracle.msg_chain(host_iov, lay["start"], seeds=seeds), nmsg, f"lanes {g}", "message")


# ------------------------------------------ 3: fused message forms, by count

@pytest.fixture(scope="module")
def fused_cases(dev_pool, oracle):
    """Layout, seeds and expected CRCs per (lanes, rows): made once, shared by
    the runs with and without segment CRCs, and left unchanged."""
    torch, cus, host, d = dev_pool
    made = {}

    def get(g, r):
        if (g, r) not in made:
            lay = fused_msgs(cus, g, r)
            seeds = _seeds32(lay["cnt"].size, 0xF5 + g + r)
            host_iov = _iov(host.ctypes.data, lay["offs"], lay["lens"])
            made[g, r] = (lay, seeds, oracle.msg_chain(host_iov, lay["start"], seeds=seeds),
                          oracle.crc32c_iov(host_iov))
        return made[g, r]
    return get


@pytest.mark.parametrize("with_seg", [False, True])
@pytest.mark.parametrize("r", [2, 4])
@pytest.mark.parametrize("g", GS)
def test_fused_message_rounds(dev_pool, fused_cases, g, r, with_seg):
    """crc32c_batch_kernel<G, U, 1> (chained through the seed) and <G, U, 2>
    (segment CRCs held back two per lane, folded with the cached basis) over
    three rounds of the full grid."""
    torch, cus, host, d = dev_pool
    lay, seeds, ref_out, ref_seg = fused_cases(g, r)
    nmsg, nseg = lay["cnt"].size, lay["lens"].size
    ck.set_msg_mode(1)
    ck.set_msg_rows(r)
    ck.set_lanes_per_buffer(g)
    out = _out(torch, nmsg, torch.int32)
    seg = _out(torch, nseg, torch.int32) if with_seg else None
    ck.batch_msg_n(_i64(torch, _iov(d.data_ptr(), lay["offs"], lay["lens"])), _i64(torch, lay["start"]), nmsg, nseg,
                   seg, out, seeds=_i32(torch, seeds))
    torch.cuda.synchronize()
    what = f"lanes {g}, rows {r}, segment CRCs {with_seg}"
    _check(out, ref_out, lay["per"], what, "message")
    if with_seg:
        _check(seg, ref_seg, nseg, what, "segment")


# ------------------------------------------ 4: CRC-64 generic batch, by count

@pytest.mark.parametrize("g", GS)
def test_generic64_rounds(dev, oracle, g):
    torch, cus = dev
    base, stride, nbytes, count = generic64_shape(cus, g)
    size = base + (count - 1) * stride + nbytes
    d = torch.empty(size + 64, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(d, size, size, 1, 0x6C00 + g)
    host = d.cpu().numpy()
    ck.set_full_rows64(0, 2)
    ck.set_lanes_per_buffer(g)
    out = _out(torch, count, torch.int64)
    ck.batch64_strided(d.data_ptr() + base, stride, nbytes, count, out, seed=SEED64)
    torch.cuda.synchronize()
    _check(out, oracle.crc64ecma_strided(host[base:], stride, nbytes, count, SEED64),
           pass_waves(cus, False) * (64 // g), f"lanes {g}, {count} x {nbytes} B every {stride}")

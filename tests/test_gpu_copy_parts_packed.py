"""Copy + CRC of mixed-size parts with the piece tasks packed on the device
(photon_crc32c_copy_parts_packed_n / photon_crc64ecma_copy_parts_packed_n and
the CRC-only photon_crc32c_batch_parts_packed_n /
photon_crc64ecma_batch_parts_packed_n), by the method of
tests/test_gpu_copy_parts.py, whose batch builder is used as it is: every CRC
bit-exact against the pinned oracle over the HOST copy of the sources, every
destination arena pre-filled with 0xA5 with at least 64 guard bytes on each
side and compared WHOLE, the sources compared afterwards, and the workspace,
d_out and d_report pre-filled with garbage. The piece is 4 KiB unless a test
says otherwise. The report is compared with {overflow, T, sum n_i, C} worked
out on the host from the definition of the cut; tests/test_copy_parts_packed_abi.py
checks the plan itself without a GPU."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from tests.test_copy_parts_abi import LENGTHS, OFFSETS, SEED32, SEED64
from tests.test_copy_parts_packed_abi import SHAPES
from tests.test_gpu_copy_crc import CANARY, GUARD
from tests.test_gpu_copy_crc64 import _first_diff
from tests.test_gpu_copy_parts import FORM_IDS, FORMS, GARBAGE, MIB, MIXED, Parts, _seeds, env, want_crc  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = (1 << 64) - 1
REPORT_GARBAGE = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(autouse=True)
def small_pieces():
    ck.set_parts_piece(4096)
    yield
    ck.set_parts_piece(0)
    ck.set_lanes_per_buffer(0)
    ck.set_batch_grid(0)


def pieces_of(addr, n, piece):
    """parts_count from its definition: the body behind the head to the first 4 KiB boundary, in pieces."""
    if n == 0:
        return 0
    body = n - min((-addr) % 4096, n)
    return -(-body // piece) if body else 1


class Packed(Parts):
    """tests/test_gpu_copy_parts.py's batch, run through the packed calls."""

    def total(self, cap=ALL):
        return sum(min(n, cap) for n in self.lens)

    def want_report(self, cap, max_total, piece=4096):
        t = sum(pieces_of(p, min(n, cap), piece) for p, n in zip(self.src_ptr, self.lens))
        c = max_total // piece + self.n
        return [1 if t > c else 0, t, self.total(cap), c]

    def buffers(self, crc64, max_total):
        torch = self.torch
        out = torch.full((self.n,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
        report = torch.full((4,), REPORT_GARBAGE, dtype=torch.int64, device="cuda")
        work = torch.full((max(ck.parts_packed_work_bytes(self.n, max_total, crc64), 8),), GARBAGE,
                          dtype=torch.uint8, device="cuda")
        return out, report, work

    def run_packed(self, crc64, copy, cap, max_total, seed=0, seeds=None, stream=None, bufs=None):
        torch = self.torch
        out, report, work = bufs if bufs is not None else self.buffers(crc64, max_total)
        d_seeds = None
        if seeds is not None:
            d_seeds = torch.from_numpy(np.array(seeds, np.uint64 if crc64 else np.uint32)
                                       .view(np.int64 if crc64 else np.int32)).cuda()
        self.keep = (work, d_seeds)
        wb = ck.parts_packed_work_bytes(self.n, max_total, crc64)
        if copy:
            (ck.copy_parts64_packed_device if crc64 else ck.copy_parts_packed_device)(
                self.iov, self.dst, self.n, cap, max_total, out, report, work, wb, seed=seed, seeds=d_seeds,
                stream=stream)
        else:
            (ck.batch_parts64_packed_device if crc64 else ck.batch_parts_packed_device)(
                self.iov, self.n, cap, max_total, out, report, work, wb, seed=seed, seeds=d_seeds, stream=stream)
        return out, report

    def check_report(self, report, cap, max_total, piece=4096, what=""):
        got = [int(x) for x in report.cpu().numpy().view(np.uint64)]
        assert got == self.want_report(cap, max_total, piece), f"{what}: report {got}"
        return got


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_lengths_and_offsets(env, want_crc, crc64, copy):
    torch, payload = env
    for layout in (0, 9, "packed") if copy else (0,):
        for seeds in (None, _seeds(len(SHAPES), crc64)):
            what = f"layout {layout} seeds {seeds is not None}"
            b = Packed(torch, payload, SHAPES, layout)
            total = b.total()
            out, report = b.run_packed(crc64, copy, ALL, total, seed=0, seeds=seeds)
            torch.cuda.synchronize()
            got = b.check_report(report, ALL, total, what=what)
            assert got[0] == 0 and got[1] <= got[3]
            b.check(want_crc, out, crc64, copy, ALL, 0, seeds, what)
            old = b.run(crc64, copy, max(LENGTHS), seed=0, seeds=seeds)  # the call of §4.9 on the same inputs
            torch.cuda.synchronize()
            assert torch.equal(out, old), what


def mixed_shapes():
    rng = np.random.default_rng(0x4D12)
    pick = [0, 0, 1, 17, 100, 4095, 4096, 4097, 8193, 12289, 20487, 70001]
    shapes = [(int(rng.choice(pick)), int(rng.choice(OFFSETS))) for _ in range(298)]
    shapes += [(MIB + 13, 5), (MIB + 13, 0)]
    rng.shuffle(shapes)
    shapes = [(int(n), int(off)) for n, off in shapes]
    assert sum(1 for n, _ in shapes if n == 0) >= 10 and {1, 17, 4095, 70001} <= {n for n, _ in shapes}
    return shapes


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_mixed_sizes(env, want_crc, crc64, copy):
    """About 300 parts from 0 bytes to 1 MiB + 13 under max_part_bytes = ~0: the calls of §4.9 cannot take
    this (their workspace follows the cap), the packed workspace follows the bytes."""
    torch, payload = env
    shapes = mixed_shapes()
    old = ck.parts_work_bytes(len(shapes), ALL, crc64)
    assert old == ALL or old > torch.cuda.get_device_properties(0).total_memory
    seeds = _seeds(len(shapes), crc64)
    b = Packed(torch, payload, shapes, "packed")
    total = b.total()
    assert ck.parts_packed_work_bytes(b.n, total, crc64) < MIB
    out, report = b.run_packed(crc64, copy, ALL, total, seeds=seeds)
    torch.cuda.synchronize()
    b.check_report(report, ALL, total, what="mixed sizes")
    b.check(want_crc, out, crc64, copy, ALL, 0, seeds, "mixed sizes")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_cap(env, want_crc, crc64, copy):
    torch, payload = env
    shapes = [(n, off) for n in LENGTHS for off in (0, 1, 4081)]
    seed = SEED64 if crc64 else SEED32
    # inside a piece of the 12,289-byte parts; on a piece boundary of the parts at offset 0 (8192) and at
    # offset 1 (head 4095 + 4096); 0. The bytes past n_i stay 0xA5: the arena is compared whole.
    for cap in (10000, 8192, 8191, 0):
        for layout in (0, "packed") if copy else (0,):
            what = f"cap {cap} layout {layout}"
            b = Packed(torch, payload, shapes, layout)
            total = b.total(cap)
            out, report = b.run_packed(crc64, copy, cap, total, seed=seed)
            torch.cuda.synchronize()
            assert b.check_report(report, cap, total, what=what)[0] == 0
            b.check(want_crc, out, crc64, copy, cap, seed, None, what)


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_overflow_writes_nothing(env, want_crc, crc64, copy):
    """max_total_bytes below what the parts hold: the report says so and nothing else is written. Every
    source and destination is sized for the real lengths, so no access leaves the arenas whatever is run."""
    torch, payload = env
    b = Packed(torch, payload, SHAPES, "packed")
    total = b.total()
    seeds = _seeds(b.n, crc64)
    for short in (total // 2, total - 4096 * (b.n + 1)):
        bufs = b.buffers(crc64, total)  # the workspace of the sufficient total: more than the short call needs
        out, report = b.run_packed(crc64, copy, ALL, short, seeds=seeds, bufs=bufs)
        torch.cuda.synchronize()
        got = b.check_report(report, ALL, short, what=f"total {short}")
        assert got[0] == 1 and got[1] > got[3]
        assert bool((out == -1).all()), "d_out was written"
        assert bool((b.arena == CANARY).all()), "a destination byte was written"
        assert np.array_equal(b.src.cpu().numpy(), b.src_image)
        # the same buffers with a sufficient total
        bufs[1].fill_(REPORT_GARBAGE)
        bufs[2].fill_(GARBAGE)
        out, report = b.run_packed(crc64, copy, ALL, total, seeds=seeds, bufs=bufs)
        torch.cuda.synchronize()
        assert b.check_report(report, ALL, total)[0] == 0
        b.check(want_crc, out, crc64, copy, ALL, 0, seeds, f"after the overflow at {short}")
        b.arena.fill_(CANARY)


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_task_rounds(env, want_crc, crc64, copy):
    torch, payload = env
    shapes = mixed_shapes()
    seeds = _seeds(len(shapes), crc64)
    ck.set_batch_grid(1)  # one workgroup: 1,332 tasks in dozens of rounds of its 16 wavefronts
    b = Packed(torch, payload, shapes, "packed")
    total = b.total()
    out, report = b.run_packed(crc64, copy, ALL, total + 12345, seeds=seeds)
    torch.cuda.synchronize()
    assert b.check_report(report, ALL, total + 12345)[1] == 1332
    b.check(want_crc, out, crc64, copy, ALL, 0, seeds, "the mixed parts on one workgroup")
    ck.set_batch_grid(0)
    for count in (1, 2, 3, 17):
        b = Packed(torch, payload, shapes[40:40 + count], 0)
        out, report = b.run_packed(crc64, copy, ALL, b.total(), seed=7)
        torch.cuda.synchronize()
        b.check_report(report, ALL, b.total(), what=f"{count} parts")
        b.check(want_crc, out, crc64, copy, ALL, 7, None, f"{count} parts")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_lane_groups(env, want_crc, crc64, copy):
    torch, payload = env
    seeds = _seeds(len(MIXED), crc64)
    for piece, groups in ((4096, (4, 8, 16, 32, 64)), (65536, (32, 64))):
        ck.set_parts_piece(piece)
        for g in groups:
            ck.set_lanes_per_buffer(g)
            for layout in (0, 9) if copy else (0,):
                what = f"piece {piece} lanes {g} layout {layout}"
                b = Packed(torch, payload, MIXED, layout)
                out, report = b.run_packed(crc64, copy, ALL, b.total(), seeds=seeds)
                torch.cuda.synchronize()
                b.check_report(report, ALL, b.total(), piece, what)
                b.check(want_crc, out, crc64, copy, ALL, 0, seeds, what)


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_default_plan(env, crc64, copy):
    """Automatic piece; 24 parts of 3 MiB + odd lengths mixed with 24 parts of under 8 KiB, from buf+1,
    against extend_device per part and a comparison of the landed bytes on the device."""
    torch, _ = env
    ck.set_parts_piece(0)
    lens = []
    for k in range(24):
        lens += [3 * MIB + (2 * k + 1) * 37, 1 + (k * 337) % 8191]
    slot = 3 * MIB + 8192
    src = torch.empty(24 * slot + 24 * 8192 + 4096, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0x9A29)
    s0 = (-src.data_ptr()) % 4096 + 1
    src_at, pos = [], s0
    for n in lens:
        src_at.append(pos)
        pos += slot if n > MIB else 8192
    assert src_at[-1] + lens[-1] <= src.numel()
    arena = torch.full((GUARD + sum(lens) + GUARD + 16,), CANARY, dtype=torch.uint8, device="cuda")
    at = GUARD + (src.data_ptr() + s0 - (arena.data_ptr() + GUARD)) % 16  # part 0 co-aligned, the rest as they fall
    dst_at = [at + sum(lens[:k]) for k in range(48)]
    iov = np.array([[src.data_ptr() + a, n] for a, n in zip(src_at, lens)], np.uint64)
    d_iov = torch.from_numpy(iov.view(np.int64)).cuda()
    d_dst = torch.from_numpy(np.array([arena.data_ptr() + a for a in dst_at], np.uint64).view(np.int64)).cuda()
    dt = torch.int64 if crc64 else torch.int32
    out = torch.full((48,), -1, dtype=dt, device="cuda")
    ref = torch.full((48,), -1, dtype=dt, device="cuda")
    report = torch.full((4,), REPORT_GARBAGE, dtype=torch.int64, device="cuda")
    total = sum(lens)
    wb = ck.parts_packed_work_bytes(48, total, crc64)
    work = torch.full((wb,), GARBAGE, dtype=torch.uint8, device="cuda")
    seed = SEED64 if crc64 else SEED32
    if copy:
        (ck.copy_parts64_packed_device if crc64 else ck.copy_parts_packed_device)(
            d_iov, d_dst, 48, ALL, total, out, report, work, seed=seed)
    else:
        (ck.batch_parts64_packed_device if crc64 else ck.batch_parts_packed_device)(
            d_iov, 48, ALL, total, out, report, work, seed=seed)
    for k in range(48):
        p = src.data_ptr() + src_at[k]
        if crc64:
            ck.extend64_device(p, lens[k], ref[k:], seed=seed)
        else:
            ck.extend_device(p, lens[k], seed, ref[k:])
    torch.cuda.synchronize()
    assert torch.equal(out, ref), (out, ref)
    assert int(out[0]) != -1
    t = sum(pieces_of(src.data_ptr() + a, n, 32768) for a, n in zip(src_at, lens))
    assert [int(x) for x in report.cpu().numpy().view(np.uint64)] == [0, t, total, total // 32768 + 48]
    if copy:
        for k in range(48):
            assert torch.equal(arena[dst_at[k]:dst_at[k] + lens[k]], src[src_at[k]:src_at[k] + lens[k]]), k
        end = dst_at[-1] + lens[-1]
        assert bool((arena[:at] == CANARY).all()) and bool((arena[end:] == CANARY).all())
    else:
        assert bool((arena == CANARY).all())


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_then_fold_parts(env, oracle, want_crc, crc64, copy):
    """The call, then fold_parts_n on the same stream with no synchronisation between them: the object's
    CRC over the assembled bytes."""
    torch, payload = env
    shapes = [(70001, 1), (12289, 0), (0, 5), (20487, 4095), (4097, 2048), (65, 1)]
    b = Packed(torch, payload, shapes, "packed")
    st = torch.cuda.Stream()
    lens = torch.from_numpy(np.array(b.lens, np.uint64).view(np.int64)).cuda()
    obj = torch.full((1,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
    seed = SEED64 if crc64 else SEED32
    torch.cuda.synchronize()
    out, report = b.run_packed(crc64, copy, ALL, b.total(), seed=0, stream=st)
    (ck.fold_parts64_device if crc64 else ck.fold_parts_device)(out, lens, None, 1, b.n, obj, seed=seed, stream=st)
    torch.cuda.synchronize()
    b.check_report(report, ALL, b.total())
    b.check(want_crc, out, crc64, copy, ALL, 0, None, "parts before the fold")
    whole = np.concatenate([payload[s:s + n] for s, n in zip(b.starts, b.lens)])
    want = oracle.crc64ecma(whole, seed) if crc64 else oracle.crc32c(whole, seed)
    got = int(obj.cpu().numpy().view(np.uint64 if crc64 else np.uint32)[0])
    assert got == want, f"{got:#x} != {want:#x}"
    if copy:  # the object lies assembled in the arena
        a = b.arena.cpu().numpy()
        assert np.array_equal(a[b.dst_at[0]:b.dst_at[0] + whole.size], whole)


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_pinned_host_source(env, want_crc, crc64, copy):
    # the kernel reads pinned host memory in place
    torch, payload = env
    shapes = [(70001, 1), (20487, 0), (0, 0), (4097, 4095), (63, 5)]
    seeds = _seeds(len(shapes), crc64)
    for layout in (0, 9) if copy else (0,):
        b = Packed(torch, payload, shapes, layout, pinned=True)
        out, report = b.run_packed(crc64, copy, ALL, b.total(), seeds=seeds)
        torch.cuda.synchronize()
        b.check_report(report, ALL, b.total())
        b.check(want_crc, out, crc64, copy, ALL, 0, seeds, f"pinned sources, layout {layout}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_streams(env, want_crc, crc64, copy):
    # four streams at once, each with its own parts, outputs, report and workspace; three calls each
    torch, payload = env
    jobs = []
    for k in range(4):
        shapes = [(n + k, off) for n, off in MIXED[k:k + 8]]
        b = Packed(torch, payload, shapes, (0, 9, "packed", 0)[k])
        cap = (ALL, 10000, 300000, 8192)[k]
        total = b.total(cap) + (0, 1, 4096, 100000)[k]
        jobs.append((b, cap, total, b.buffers(crc64, total), torch.cuda.Stream()))
    torch.cuda.synchronize()
    for rep in range(3):
        for k, (b, cap, total, bufs, st) in enumerate(jobs):
            b.run_packed(crc64, copy, cap, total, seed=100 + k, stream=st, bufs=bufs)
    torch.cuda.synchronize()
    for k, (b, cap, total, bufs, st) in enumerate(jobs):
        b.check_report(bufs[1], cap, total, what=f"stream {k}")
        b.check(want_crc, bufs[0], crc64, copy, cap, 100 + k, None, f"stream {k}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_graph_capture_lengths_change(env, want_crc, crc64, copy):
    """One call captured and replayed; then the DEVICE descriptors are rewritten so that T and every part
    boundary differ, the workspace is re-garbled, and the same graph is replayed: the plan is rebuilt by the
    captured launches, nothing of it lives on the host."""
    torch, payload = env
    first = Packed(torch, payload, [(70001, 1), (12289, 0), (0, 5), (20487, 4095), (200001, 5)], 0)
    second = Packed(torch, payload, [(5, 4095), (150000, 2048), (8193, 0), (0, 0), (64, 1)], 9)
    assert first.want_report(ALL, 0)[1] != second.want_report(ALL, 0)[1]
    max_total = max(first.total(), second.total())
    seed = SEED64 if crc64 else SEED32
    bufs = first.buffers(crc64, max_total)
    first.run_packed(crc64, copy, ALL, max_total, seed=seed, bufs=bufs)  # first-call set-up outside the capture
    torch.cuda.synchronize()
    first.arena.fill_(CANARY)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        first.run_packed(crc64, copy, ALL, max_total, seed=seed, bufs=bufs, stream=torch.cuda.current_stream())
    for rep, b in enumerate((first, second)):
        # the captured launches read first.iov / first.dst: the descriptors of this replay go there
        first.iov.copy_(b.iov)
        first.dst.copy_(b.dst)
        bufs[0].fill_(-1)
        bufs[1].fill_(REPORT_GARBAGE)
        bufs[2].fill_(GARBAGE + 1 + rep)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        b.check_report(bufs[1], ALL, max_total, what=f"replay {rep}")
        b.check(want_crc, bufs[0], crc64, copy, ALL, seed, None, f"replay {rep}")
    _first_diff(first.arena.cpu().numpy(), _landed(first, copy), "the first batch's arena after both replays")


def _landed(b, copy):
    want = np.full(b.arena.numel(), CANARY, np.uint8)
    if copy:
        for k, n in enumerate(b.lens):
            want[b.dst_at[k]:b.dst_at[k] + n] = b.payload[b.starts[k]:b.starts[k] + n]
    return want

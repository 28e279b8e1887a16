"""Copy + CRC of many large parts in one launch, each cut over the chip
(photon_crc32c_copy_parts_n / photon_crc64ecma_copy_parts_n and the CRC-only
photon_crc32c_batch_parts_n / photon_crc64ecma_batch_parts_n, DESIGN.md
§4.9), by the method of tests/test_gpu_copy_crc.py: every CRC bit-exact
against the pinned oracle over the HOST copy of the sources, every
destination arena pre-filled with 0xA5 with at least 64 guard bytes on each
side and compared WHOLE, the sources compared afterwards, and the workspace
pre-filled with garbage. The piece is 4 KiB unless a test says otherwise, so
that parts of a few KiB have several pieces: the lengths and source offsets
are those of tests/test_copy_parts_abi.py, which checks the cut itself
without a GPU. A source "at offset off" starts off bytes after a 4 KiB
boundary, which is what the cut is anchored at."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_copy_parts_abi import LENGTHS, OFFSETS, SEED32, SEED64
from tests.test_gpu_copy_crc import CANARY, GUARD
from tests.test_gpu_copy_crc64 import _first_diff

pytestmark = pytest.mark.gpu

MIB = 1 << 20
FORMS = [(False, True), (True, True), (False, False), (True, False)]  # (crc64, copy)
FORM_IDS = ["crc32c-copy", "crc64-copy", "crc32c-only", "crc64-only"]
POOL = 4 * MIB
GARBAGE = 0x5A


@pytest.fixture(scope="module")
def env():
    """torch and one host payload; part k's bytes are a slice of it."""
    import torch
    assert torch.cuda.is_available()
    return torch, datagen.stream_bytes(0x9A27, POOL)


@pytest.fixture(scope="module")
def want_crc(oracle, env):
    """The oracle's CRC of payload[start:start + n] from a seed, computed once per key."""
    payload = env[1]
    made = {}

    def get(start, n, seed, crc64):
        k = (start, n, seed, crc64)
        if k not in made:
            data = payload[start:start + n]
            made[k] = oracle.crc64ecma(data, seed) if crc64 else oracle.crc32c(data, seed)
        return made[k]
    return get


@pytest.fixture(autouse=True)
def small_pieces():
    ck.set_parts_piece(4096)
    yield
    ck.set_parts_piece(0)
    ck.set_lanes_per_buffer(0)
    ck.set_batch_grid(0)


class Parts:
    """A batch of parts on the device: sources (each in its own 4 KiB-aligned slot, at its offset),
    descriptors, and for the copying forms an arena of 0xA5 with the destinations in it."""

    def __init__(self, torch, payload, shapes, layout=0, pinned=False):
        # shapes: [(length, source offset from a 4 KiB boundary)]; layout: 0 / 9 = every destination at that
        # (dst - src) % 16, "packed" = back to back from an odd address
        self.torch, self.payload, self.shapes, self.n = torch, payload, shapes, len(shapes)
        self.lens = [n for n, _ in shapes]
        self.starts, self.src_at = [], []
        pos = 0
        rng = np.random.default_rng(len(shapes) * 7919 + sum(self.lens))
        for n, off in shapes:
            self.starts.append(int(rng.integers(0, POOL - n + 1)))
            self.src_at.append(pos + off)
            pos += (off + n + 4095) // 4096 * 4096 + 4096
        size = max(pos, 4096)
        kw = dict(pin_memory=True) if pinned else dict(device="cuda")
        self.src = torch.empty(size + 4096, dtype=torch.uint8, **kw)
        self.shift = (-self.src.data_ptr()) % 4096
        self.src_image = np.full(self.src.numel(), 0x11, np.uint8)
        for k, (n, off) in enumerate(shapes):
            a = self.shift + self.src_at[k]
            self.src_image[a:a + n] = payload[self.starts[k]:self.starts[k] + n]
        self.src.copy_(torch.from_numpy(self.src_image))
        base = self.src.data_ptr() + self.shift
        self.src_ptr = [base + a for a in self.src_at]
        for k, (n, off) in enumerate(shapes):
            assert self.src_ptr[k] % 4096 == off % 4096
        iov = np.array([[p, n] for p, n in zip(self.src_ptr, self.lens)], np.uint64).reshape(-1, 2)
        self.iov = torch.from_numpy(iov.view(np.int64)).cuda()
        # destinations
        self.arena = torch.empty(GUARD + sum(self.lens) + 32 * (self.n + 1) + GUARD, dtype=torch.uint8,
                                 device="cuda")
        self.arena.fill_(CANARY)
        self.dst_at = []
        at = GUARD + (1 - (self.arena.data_ptr() + GUARD)) % 2  # odd address
        for k, n in enumerate(self.lens):
            if layout != "packed":
                at += (self.src_ptr[k] + layout - (self.arena.data_ptr() + at)) % 16
                assert (self.arena.data_ptr() + at - self.src_ptr[k]) % 16 == layout
            self.dst_at.append(at)
            at += n
        assert at + GUARD <= self.arena.numel()
        if layout == "packed":
            assert (self.arena.data_ptr() + self.dst_at[0]) % 2 == 1
        dst = np.array([self.arena.data_ptr() + a for a in self.dst_at], np.uint64)
        self.dst = torch.from_numpy(dst.view(np.int64)).cuda()

    def run(self, crc64, copy, cap, seed=0, seeds=None, stream=None, out=None, work=None):
        torch = self.torch
        if out is None:
            out = torch.full((self.n,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
        if work is None:
            work = torch.full((max(ck.parts_work_bytes(self.n, cap, crc64), 8),), GARBAGE, dtype=torch.uint8,
                              device="cuda")
        d_seeds = None
        if seeds is not None:
            d_seeds = torch.from_numpy(np.array(seeds, np.uint64 if crc64 else np.uint32)
                                       .view(np.int64 if crc64 else np.int32)).cuda()
        self.keep = (work, d_seeds)
        wb = ck.parts_work_bytes(self.n, cap, crc64)
        if copy:
            (ck.copy_parts64_device if crc64 else ck.copy_parts_device)(
                self.iov, self.dst, self.n, cap, out, work, wb, seed=seed, seeds=d_seeds, stream=stream)
        else:
            (ck.batch_parts64_device if crc64 else ck.batch_parts_device)(
                self.iov, self.n, cap, out, work, wb, seed=seed, seeds=d_seeds, stream=stream)
        return out

    def check(self, want_crc, out, crc64, copy, cap, seed=0, seeds=None, what=""):
        got = out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
        for k, n in enumerate(self.lens):
            s = seeds[k] if seeds is not None else seed
            ref = want_crc(self.starts[k], min(n, cap), s, crc64)
            assert int(got[k]) == ref, f"{what}: part {k} {self.shapes[k]} cap {cap}: {int(got[k]):#x}, want {ref:#x}"
        want = np.full(self.arena.numel(), CANARY, np.uint8)
        if copy:
            for k, n in enumerate(self.lens):
                m = min(n, cap)
                want[self.dst_at[k]:self.dst_at[k] + m] = self.payload[self.starts[k]:self.starts[k] + m]
        _first_diff(self.arena.cpu().numpy(), want, what)
        assert np.array_equal(self.src.cpu().numpy(), self.src_image), f"{what}: the sources changed"


def _seeds(n, crc64):
    base = SEED64 if crc64 else SEED32
    mask = (1 << 64) - 1 if crc64 else (1 << 32) - 1
    return [(base * (2 * k + 1) + k) & mask or 1 for k in range(n)]


GRID_SHAPES = [(n, off) for n in LENGTHS for off in OFFSETS]


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_lengths_and_offsets(env, want_crc, crc64, copy):
    torch, payload = env
    cap = max(LENGTHS)
    for layout in (0, 9, "packed") if copy else (0,):
        for seeds in (None, _seeds(len(GRID_SHAPES), crc64)):
            b = Parts(torch, payload, GRID_SHAPES, layout)
            out = b.run(crc64, copy, cap, seed=0, seeds=seeds)
            torch.cuda.synchronize()
            b.check(want_crc, out, crc64, copy, cap, 0, seeds, f"layout {layout} seeds {seeds is not None}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_cap(env, want_crc, crc64, copy):
    torch, payload = env
    shapes = [(n, off) for n in LENGTHS for off in (0, 1, 4081)]
    seed = SEED64 if crc64 else SEED32
    # above every length (trailing empty tasks); inside a piece of the 12,289-byte parts; on a piece boundary
    # of the parts at offset 0 (8192) and at offset 1 (head 4095 + 4096); 0
    for cap in (MIB, 10000, 8192, 8191, 0):
        for layout in (0, "packed") if copy else (0,):
            b = Parts(torch, payload, shapes, layout)
            out = b.run(crc64, copy, cap, seed=seed)
            torch.cuda.synchronize()
            b.check(want_crc, out, crc64, copy, cap, seed, None, f"cap {cap} layout {layout}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_task_rounds(env, want_crc, crc64, copy):
    torch, payload = env
    rng = np.random.default_rng(300)
    pick = [0, 0, 1, 100, 4096, 5000, 8193, 12289, 20487, 40000]
    shapes = [(int(rng.choice(pick)), int(rng.choice(OFFSETS))) for _ in range(300)]
    assert sum(1 for n, _ in shapes if n == 0) >= 10
    cap = 40000
    seeds = _seeds(300, crc64)
    ck.set_batch_grid(1)  # one workgroup: 3,000 tasks in dozens of rounds of its 16 wavefronts
    b = Parts(torch, payload, shapes, "packed")
    out = b.run(crc64, copy, cap, seeds=seeds)
    torch.cuda.synchronize()
    b.check(want_crc, out, crc64, copy, cap, 0, seeds, "300 parts on one workgroup")
    ck.set_batch_grid(0)
    for count in (1, 2, 3, 17):
        b = Parts(torch, payload, shapes[40:40 + count], 0)
        out = b.run(crc64, copy, cap, seed=7)
        torch.cuda.synchronize()
        b.check(want_crc, out, crc64, copy, cap, 7, None, f"{count} parts")


MIXED = [(70001, 1), (0, 0), (20487, 4095), (64, 5), (12289, 0), (63, 2048), (8193, 4081), (200001, 5), (4096, 0),
         (1, 4095), (65, 1), (300000, 0)]


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_lane_groups(env, want_crc, crc64, copy):
    torch, payload = env
    seeds = _seeds(len(MIXED), crc64)
    for piece, groups in ((4096, (4, 8, 16, 32, 64)), (65536, (32, 64))):
        ck.set_parts_piece(piece)
        for g in groups:
            ck.set_lanes_per_buffer(g)
            for layout in (0, 9) if copy else (0,):
                b = Parts(torch, payload, MIXED, layout)
                out = b.run(crc64, copy, 300000, seeds=seeds)
                torch.cuda.synchronize()
                b.check(want_crc, out, crc64, copy, 300000, 0, seeds, f"piece {piece} lanes {g} layout {layout}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_default_plan(env, crc64, copy):
    """Automatic piece; 24 parts of 3 MiB + odd lengths from buf+1 (about 72 MiB), against
    copy_extend_device / extend_device per part and a comparison of the landed bytes on the device."""
    torch, _ = env
    ck.set_parts_piece(0)
    lens = [3 * MIB + (2 * k + 1) * 37 for k in range(24)]
    slot = 3 * MIB + 8192
    src = torch.empty(24 * slot + 4096, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0x9A28)
    s0 = (-src.data_ptr()) % 4096 + 1
    arena = torch.full((GUARD + sum(lens) + GUARD + 16,), CANARY, dtype=torch.uint8, device="cuda")
    at = GUARD + (src.data_ptr() + s0 - (arena.data_ptr() + GUARD)) % 16  # part 0 co-aligned, the rest as they fall
    src_at = [s0 + k * slot for k in range(24)]
    dst_at = [at + sum(lens[:k]) for k in range(24)]
    iov = np.array([[src.data_ptr() + a, n] for a, n in zip(src_at, lens)], np.uint64)
    d_iov = torch.from_numpy(iov.view(np.int64)).cuda()
    d_dst = torch.from_numpy(np.array([arena.data_ptr() + a for a in dst_at], np.uint64).view(np.int64)).cuda()
    dt = torch.int64 if crc64 else torch.int32
    out = torch.full((24,), -1, dtype=dt, device="cuda")
    ref = torch.full((24,), -1, dtype=dt, device="cuda")
    cap = max(lens)
    wb = ck.parts_work_bytes(24, cap, crc64)
    assert wb == 24 * 97 * (8 if crc64 else 4)  # 32 KiB pieces
    work = torch.full((wb,), GARBAGE, dtype=torch.uint8, device="cuda")
    seed = SEED64 if crc64 else SEED32
    if copy:
        (ck.copy_parts64_device if crc64 else ck.copy_parts_device)(d_iov, d_dst, 24, cap, out, work, seed=seed)
        scratch = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    else:
        (ck.batch_parts64_device if crc64 else ck.batch_parts_device)(d_iov, 24, cap, out, work, seed=seed)
    for k in range(24):
        p = src.data_ptr() + src_at[k]
        if copy and crc64:
            ck.copy_extend64_device(p, scratch, lens[k], ref[k:], seed=seed)
        elif copy:
            ck.copy_extend_device(p, scratch, lens[k], seed, ref[k:])
        elif crc64:
            ck.extend64_device(p, lens[k], ref[k:], seed=seed)
        else:
            ck.extend_device(p, lens[k], seed, ref[k:])
    torch.cuda.synchronize()
    assert torch.equal(out, ref), (out, ref)
    assert int(out[0]) != -1
    if copy:
        for k in range(24):
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
    b = Parts(torch, payload, shapes, "packed")
    cap = 70001
    st = torch.cuda.Stream()
    lens = torch.from_numpy(np.array(b.lens, np.uint64).view(np.int64)).cuda()
    obj = torch.full((1,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
    seed = SEED64 if crc64 else SEED32
    torch.cuda.synchronize()
    out = b.run(crc64, copy, cap, seed=0, stream=st)
    (ck.fold_parts64_device if crc64 else ck.fold_parts_device)(out, lens, None, 1, b.n, obj, seed=seed, stream=st)
    torch.cuda.synchronize()
    b.check(want_crc, out, crc64, copy, cap, 0, None, "parts before the fold")
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
        b = Parts(torch, payload, shapes, layout, pinned=True)
        out = b.run(crc64, copy, 70001, seeds=seeds)
        torch.cuda.synchronize()
        b.check(want_crc, out, crc64, copy, 70001, 0, seeds, f"pinned sources, layout {layout}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_streams(env, want_crc, crc64, copy):
    # four streams at once, each with its own parts, outputs and workspace
    torch, payload = env
    jobs = []
    for k in range(4):
        shapes = [(n + k, off) for n, off in MIXED[k:k + 8]]
        b = Parts(torch, payload, shapes, (0, 9, "packed", 0)[k])
        cap = (300000, 10000, 300000, 8192)[k]
        out = torch.full((b.n,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
        work = torch.full((ck.parts_work_bytes(b.n, cap, crc64),), GARBAGE, dtype=torch.uint8, device="cuda")
        jobs.append((b, cap, out, work, torch.cuda.Stream()))
    torch.cuda.synchronize()
    for rep in range(3):
        for k, (b, cap, out, work, st) in enumerate(jobs):
            b.run(crc64, copy, cap, seed=100 + k, stream=st, out=out, work=work)
    torch.cuda.synchronize()
    for k, (b, cap, out, work, st) in enumerate(jobs):
        b.check(want_crc, out, crc64, copy, cap, 100 + k, None, f"stream {k}")


@pytest.mark.parametrize("crc64,copy", FORMS, ids=FORM_IDS)
def test_graph_capture(env, oracle, crc64, copy):
    # one call captured; both replays run over refilled sources, with the workspace re-garbled
    torch, payload = env
    shapes = [(70001, 1), (12289, 0), (0, 5), (20487, 4095), (200001, 5)]
    b = Parts(torch, payload, shapes, 0)
    cap = 100000
    seed = SEED64 if crc64 else SEED32
    out = torch.full((b.n,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
    work = torch.full((ck.parts_work_bytes(b.n, cap, crc64),), GARBAGE, dtype=torch.uint8, device="cuda")
    b.run(crc64, copy, cap, seed=seed, out=out, work=work)  # first-call set-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        b.run(crc64, copy, cap, seed=seed, out=out, work=work, stream=torch.cuda.current_stream())
    crc = oracle.crc64ecma if crc64 else oracle.crc32c
    for rep in range(2):
        ck.fill_splitmix(b.src, b.src.numel(), b.src.numel(), 1, 0x9A30 + rep)
        b.arena.fill_(CANARY)
        out.fill_(-1)
        work.fill_(GARBAGE + rep)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        host = b.src.cpu().numpy()
        got = out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
        want = np.full(b.arena.numel(), CANARY, np.uint8)
        for k, n in enumerate(b.lens):
            m = min(n, cap)
            data = host[b.shift + b.src_at[k]:b.shift + b.src_at[k] + m]
            assert int(got[k]) == crc(data, seed), (rep, k)
            if copy:
                want[b.dst_at[k]:b.dst_at[k] + m] = data
        _first_diff(b.arena.cpu().numpy(), want, f"replay {rep}")

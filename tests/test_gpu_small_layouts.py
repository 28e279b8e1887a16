"""The end-anchored one-buffer layouts (crc32c_kernels.h "one small buffer":
crc32c_small_kernel<V, R> / crc64_small_kernel<V, R>, small and mid) at every
edge of their geometry, by the method of tests/test_gpu_copy_long.py: every
CRC bit-exact against the pinned oracle over the HOST copy of the bytes.

The shapes are those of tests/test_small_layout_cases.py, which asserts
(without a GPU, through photon_crc_test_small_plan) that each reaches the
state it is there for: wave and workgroup edges of a partial grid, full rows,
a first row of one block, every row count of both layouts, the hand-overs
small -> mid -> long, and for buffers of up to 40 bytes at every start every
tail factor and every way head, seed and tail masks share blocks.

Two paths, both CRC widths, three seeds:
  A  photon_crc32c_extend_device / photon_crc64ecma_extend_device: the calls
     of a test queued on ONE stream (its launches of different grid sizes
     share the stream's reduce state) to distinct elements of one output
     tensor pre-filled with -1, one synchronise, a guard element behind;
  B  the routed crc32c_extend / crc64ecma_extend with the resident service
     off: tagged per-workgroup slots XORed by the host (small), the tagged
     reduce (mid). No call may be served by the service or recomputed on the
     host: either would hide a wrong kernel.
One host payload; a case's data is its first n bytes, on the device once per
start offset, so the oracle hashes the payload once per (width, seed)."""
import numpy as np
import pytest

from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests import test_small_layout_cases as cases

pytestmark = pytest.mark.gpu

CRCS = cases.CRCS
IDS = cases.IDS
SEEDS = {False: (0, 0xFFFFFFFF, 0x9E3779B1), True: (0, 0xFFFFFFFFFFFFFFFF, 0xFEDCBA9876543210)}
SLACK = 64
POOL = cases.MAX_N + SLACK
TINY_MAX = max(n for _, n in cases.TINY)
KINDS = ["small-1wg", "small-multi", "mid-partial", "mid-full"]
DEFAULT_IDLE_US, DEFAULT_LIFE_US = 200, 2000  # the library's defaults (tuning.h)


def _place(torch, host, s0):
    """host on the device, s0 bytes after a 16-byte boundary: (tensor, address of its first byte)."""
    t = torch.zeros(16 + host.size, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[s0:s0 + host.size] = torch.from_numpy(host)
    return t, t.data_ptr() + s0


@pytest.fixture(scope="module")
def pool():
    """The payload, its device copies by start offset (each with SLACK bytes behind the longest
    case) and the tiny matrix's copies, one stream for every queued call."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    payload = datagen.stream_bytes(0x51A7, POOL)
    starts = sorted({s0 for s0, _ in cases.VARIANTS} | {s0 for s0, _ in cases.HANDOVERS})
    big = {s0: _place(torch, payload, s0) for s0 in starts}
    tiny = {s0: _place(torch, payload[:TINY_MAX + SLACK], s0) for s0 in range(16)}
    torch.cuda.synchronize()
    return torch, payload, big, tiny, torch.cuda.Stream()


@pytest.fixture(scope="module")
def want(pool, oracle):
    """want(crc64, seed)[n] = the oracle's CRC of the payload's first n bytes from seed, for every
    n of the tables: built once per (width, seed) over the sorted lengths, each extending the one
    before over the bytes added."""
    payload = pool[1]
    ns = sorted({cases.case_n(*c) for cs in cases.CASES.values() for c in cs} | {n for _, n in cases.HANDOVERS} |
                {n for _, n in cases.TINY} | {16 * (cases.SMALL_BLOCKS + 1)})
    made = {}

    def get(crc64, seed):
        if (crc64, seed) not in made:
            crc = oracle.crc64ecma if crc64 else oracle.crc32c
            tab, acc, at = {}, seed, 0
            for n in ns:
                acc = crc(payload[at:n], acc)
                tab[n], at = acc, n
            made[(crc64, seed)] = tab
        return made[(crc64, seed)]
    return get


@pytest.fixture(autouse=True)
def _defaults():
    """Every test leaves the library at its defaults."""
    yield
    ck.set_small_service(0)
    ck.set_small_service(DEFAULT_IDLE_US)
    ck.set_small_service_life(DEFAULT_LIFE_US)
    ck.set_service_doorbell(True)
    ck.set_device_dispatch(False)
    ck.set_mid_kernel(True)


@pytest.fixture
def routed(_defaults):
    """Routed calls on the launch path: dispatch on, the service off; none served, none recomputed."""
    fb0 = ck.dispatch_fallbacks()
    ck.set_device_dispatch(True)
    ck.set_small_service(0)
    served0 = ck.small_service_stats()[0]
    yield
    assert ck.small_service_stats()[0] == served0, "a call was served by the resident service"
    assert ck.dispatch_fallbacks() == fb0, "a routed call failed on the device and was recomputed on the host"


def _table_calls(big, cls, crc64):
    """(label, address, n) of a class's cases; each real pointer reaches the case's state."""
    calls = []
    for nb, s0, k in cases.CASES[cls]:
        n = cases.case_n(nb, s0, k)
        addr = big[s0][1]
        p = cases.plan_at(addr, n, crc64)
        assert (p["layout"], p["nb"], p["s0"], p["k"]) == (cases.LAYOUT[cls], nb, s0, k), (cls, nb, s0, k, p)
        calls.append((cls, addr, n))
    return calls


def _tiny_calls(tiny, crc64, min_n=0):
    calls = []
    for s0, n in cases.TINY:
        if n >= min_n:
            assert cases.plan_at(tiny[s0][1], n, crc64)["s0"] == s0
            calls.append(("tiny", tiny[s0][1], n))
    return calls


def _alternate(calls, crc64):
    """The calls reordered so that the four launch shapes take turns."""
    by = {k: [] for k in KINDS}
    for c in calls:
        by[cases.kind(cases.plan_at(c[1], c[2], crc64))].append(c)
    out = []
    while any(by.values()):
        out += [by[k].pop(0) for k in KINDS if by[k]]
    return out


def _with_seeds(calls, crc64):
    return [c + (s,) for s in SEEDS[crc64] for c in calls]


def _run_extend(pool, crc64, calls):
    """Path A: every call queued on the one stream, one synchronise; the values in call order."""
    torch, st = pool[0], pool[4]
    out = torch.full((len(calls) + 1,), -1, dtype=torch.int64 if crc64 else torch.int32, device="cuda")
    size = out.element_size()
    torch.cuda.synchronize()
    for i, (_, addr, n, seed) in enumerate(calls):
        if crc64:
            ck.extend64_device(addr, n, out.data_ptr() + i * size, seed=seed, stream=st)
        else:
            ck.extend_device(addr, n, seed, out.data_ptr() + i * size, stream=st)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint64 if crc64 else np.uint32)
    assert int(got[-1]) == (1 << (8 * size)) - 1, "the element behind the last result was written"
    return [int(x) for x in got[:-1]]


def _run_routed(crc64, calls):
    """Path B: one synchronous routed call each."""
    call = ck.crc64ecma_extend_at if crc64 else ck.crc32c_extend_at
    return [call(addr, n, seed) for _, addr, n, seed in calls]


def _check(path, crc64, calls, got, want):
    """Every value against the oracle; a failure names its class and its state by the hook."""
    bad = []
    for (label, addr, n, seed), g in zip(calls, got):
        w = want(crc64, seed)[n]
        if g != w:
            p = cases.plan_at(addr, n, crc64)
            bad.append(f"{label}: (nb, s0, k, rows, Z, grid) = ({p['nb']}, {p['s0']}, {p['k']}, {p['rows']}, "
                       f"{p['Z']}, {p['grid']}), layout {p['layout']}, n {n}, seed {seed:#x}: {g:#x}, want {w:#x}")
    print(f"path {path} {IDS[crc64]}: {len(calls)} calls, {len(bad)} wrong")
    assert not bad, f"path {path} {IDS[crc64]}: {len(bad)} of {len(calls)} wrong:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
@pytest.mark.parametrize("cls", cases.CLASSES)
def test_extend_device_table(pool, want, cls, crc64):
    calls = _with_seeds(_alternate(_table_calls(pool[2], cls, crc64), crc64), crc64)
    _check("A", crc64, calls, _run_extend(pool, crc64, calls), want)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
@pytest.mark.parametrize("cls", cases.CLASSES)
def test_routed_table(pool, want, routed, cls, crc64):
    calls = _with_seeds(_alternate(_table_calls(pool[2], cls, crc64), crc64), crc64)
    _check("B", crc64, calls, _run_routed(crc64, calls), want)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_extend_device_tiny(pool, want, crc64):
    calls = _with_seeds(_tiny_calls(pool[3], crc64), crc64)
    _check("A", crc64, calls, _run_extend(pool, crc64, calls), want)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_routed_tiny(pool, want, routed, crc64):
    calls = _with_seeds(_tiny_calls(pool[3], crc64, min_n=1), crc64)  # no bytes: the host returns the seed
    _check("B", crc64, calls, _run_routed(crc64, calls), want)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_alternating_launch_shapes(pool, want, crc64):
    """Every class on one stream, one-workgroup small, multi-workgroup small, partial mid and full
    mid launches taking turns (a direct store, then reduces of 2..512 workgroup values over the
    stream's one reduce state), the seeds taking turns too."""
    table = [c for cls in cases.CLASSES for c in _table_calls(pool[2], cls, crc64)]
    order = _alternate(table + _tiny_calls(pool[3], crc64)[::7], crc64)
    assert [cases.kind(cases.plan_at(a, n, crc64)) for _, a, n in order[:4]] == KINDS
    calls = [c + (SEEDS[crc64][i % 3],) for i, c in enumerate(order)]
    _check("A", crc64, calls, _run_extend(pool, crc64, calls), want)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
@pytest.mark.parametrize("mid", [True, False], ids=["mid-on", "mid-off"])
def test_handovers(pool, want, mid, crc64):
    """The last span of each layout and the first of the next, and the smallest mid span, on
    whichever kernel the mid switch gives them (tests/test_small_layout_cases.py owns which)."""
    big = pool[2]
    spans = cases.HANDOVERS + [(0, 16 * (cases.SMALL_BLOCKS + 1))]
    ck.set_mid_kernel(mid)
    got_layouts = [cases.plan_at(big[s0][1], n, crc64)["layout"] for s0, n in cases.HANDOVERS]
    assert got_layouts == cases.HANDOVER_LAYOUTS[mid]
    calls = _with_seeds([(f"handover {'mid-on' if mid else 'mid-off'}", big[s0][1], n) for s0, n in spans], crc64)
    _check("A", crc64, calls, _run_extend(pool, crc64, calls), want)

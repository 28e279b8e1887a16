"""The case table of tests/test_gpu_small_layouts.py and, without a GPU, the
proof that each case reaches the state of the end-anchored one-buffer layout
(crc32c_kernels.h "one small buffer": crc32c_small_kernel<V, R>,
crc64_small_kernel<V, R>) it is there for, asked of the library through
photon_crc_test_small_plan -- the launch paths' own small_args / mid_args.

The layout: nb = ceil((s0 + max(n, seed bytes)) / 16) blocks walked by V
virtual lanes anchored at the END of the buffer, rows = ceil(nb / V), Z = rows
V - nb leading zero blocks; for nb <= V only the last ceil(nb / 256)
workgroups are launched (wg0 = the first one's place in the full layout);
head / seed and tail masks in blocks 0, 1, nb - 2, nb - 1; a tail factor
x^(-8k) picked by k = 16 nb - (s0 + n). Every constant (V, workgroups, block
limits, rows, seed bytes) is read from the hook, none is written down here.

A table case is (nb, s0, k) with n = 16 nb - s0 - k. CPU only."""
import os

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

BASE = 1 << 32  # a 16-byte aligned address; the hook never dereferences it
CRCS = [False, True]
IDS = ["crc32c", "crc64"]
VARIANTS = ((0, 0), (1, 15), (15, 1), (9, 7))  # (s0, k)
MIN_N = 8  # shorter buffers belong to the tiny matrix


def plan_at(addr, n, crc64):
    """The hook's plan for n bytes at addr, with Z (the leading zero blocks) added."""
    p = ck.small_plan(addr, n, crc64)
    v = (p["small_v"], p["mid_v"], 0)[p["layout"]]
    p["Z"] = p["rows"] * v - p["nb"]
    return p


def plan(s0, n, crc64):
    """plan_at for a buffer that starts s0 bytes after a 16-byte boundary."""
    return plan_at(BASE + s0, n, crc64)


_K = plan(0, MIN_N, False)
V1, WG1, V2, WG2 = _K["small_v"], _K["small_wg"], _K["mid_v"], _K["mid_wg"]
SMALL_BLOCKS, MID_BLOCKS = _K["small_blocks"], _K["mid_blocks"]
SMALL_ROWS, MID_ROWS = _K["small_rows"], _K["mid_rows"]
SMALL, MID, LONG = 0, 1, 2

CLASSES = ["small-1row", "small-2rows", "mid-1row", "mid-rows2-8"]
LAYOUT = {"small-1row": SMALL, "small-2rows": SMALL, "mid-1row": MID, "mid-rows2-8": MID}
NB = {
    # a wave edge; grid 1 -> 2 (the result leaves directly / through the reduce); the reference's
    # 128 KiB at buf+0 / +1; a full row
    "small-1row": [5, 63, 64, 65, 255, 256, 257, 513, 8191, 8192, 8193, V1 - 1, V1],
    # a first row of one block; wave and workgroup edges in the first row; the maximum
    "small-2rows": [V1 + 1, V1 + 63, V1 + 64, V1 + 65, V1 + 256, V1 + 257, 12672, SMALL_BLOCKS - 1, SMALL_BLOCKS],
    # the smallest; one block in the first launched workgroup; over half the grid; a full row
    "mid-1row": [SMALL_BLOCKS + 1, SMALL_BLOCKS + 1 + 255, 25600, 25601, 66000, V2 - 1, V2],
    # row boundaries from both sides, every row count (6 V2 - 1 is the one six-row case), the maximum
    "mid-rows2-8": [V2 + 1, V2 + 64, V2 + 65, 2 * V2 - 257, 2 * V2 - 1, 2 * V2, 2 * V2 + 1, 3 * V2 + 1, 4 * V2,
                    5 * V2 - 63, 6 * V2 - 1, 6 * V2 + 256, 7 * V2 + 1, MID_ROWS * V2 - 1, MID_ROWS * V2],
}


def case_n(nb, s0, k):
    return 16 * nb - s0 - k


CASES = {c: [(nb, s0, k) for nb in NB[c] for s0, k in VARIANTS if case_n(nb, s0, k) >= MIN_N] for c in CLASSES}

# (s0, n): the last span of the small layout and the first of the mid one, the last of the mid
# layout and the first of the long kernel; the layouts with the mid kernel on / off
HANDOVERS = [(0, 16 * SMALL_BLOCKS), (1, 16 * SMALL_BLOCKS), (0, 16 * MID_BLOCKS), (1, 16 * MID_BLOCKS)]
HANDOVER_LAYOUTS = {True: [SMALL, MID, MID, LONG], False: [SMALL, LONG, LONG, LONG]}

# every start in a block x every length up to 2.5 blocks: (s0, n)
TINY = [(s0, n) for s0 in range(16) for n in range(41)]

MAX_N = max([case_n(*c) for cs in CASES.values() for c in cs] + [n for _, n in HANDOVERS])


def kind(p):
    """The four launch shapes one stream alternates between (tests/test_gpu_small_layouts.py)."""
    if p["layout"] == SMALL:
        return "small-1wg" if p["grid"] == 1 else "small-multi"
    return "mid-partial" if p["grid"] < p["mid_wg"] else "mid-full"


def _ceil(a, b):
    return -(-a // b)


def test_hook_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert "photon_crc_test_small_plan" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    header = open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", "tuning.h")).read()
    assert "int photon_crc_test_small_plan(" in header
    L = _native.lib()
    import ctypes
    out = (ctypes.c_uint64 * len(ck.SMALL_PLAN_FIELDS))()
    assert L.photon_crc_test_small_plan(BASE, 100, 0, None, 64) == -22
    assert L.photon_crc_test_small_plan(BASE, 100, 0, out, len(out) - 1) == -22
    assert L.photon_crc_test_small_plan(BASE, 100, 1, out, len(out)) == len(out)
    assert L.photon_crc_test_small_plan(0, 0, 0, out, len(out)) == len(out)  # a null buffer of no bytes


def test_constants_are_consistent():
    from tests.test_gpu_service import SVC_MAX_BLOCKS
    a, b = plan(0, MIN_N, False), plan(0, MIN_N, True)
    consts = ck.SMALL_PLAN_FIELDS[9:18]
    assert [a[f] for f in consts] == [b[f] for f in consts]  # one geometry for both widths
    assert (a["seed_bytes"], b["seed_bytes"]) == (4, 8)      # sizeof the CRC
    assert V1 == 256 * WG1 and V2 == 256 * WG2
    assert MID_BLOCKS == MID_ROWS * V2 and (SMALL_ROWS - 1) * V1 < SMALL_BLOCKS <= SMALL_ROWS * V1
    assert SMALL_BLOCKS < V2  # the smallest mid span is a partial grid
    assert a["svc_max_blocks"] == SVC_MAX_BLOCKS
    # the sizes the hand-overs and the reference's perf shape are quoted at
    assert 16 * SMALL_BLOCKS == 256 << 10 and 16 * MID_BLOCKS == 16 << 20
    assert plan(1, 128 << 10, False)["nb"] == 8193 <= V1  # 128 KiB at buf+1: one row


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
@pytest.mark.parametrize("cls", CLASSES)
def test_cases_reach_their_state(cls, crc64):
    v, wg = (V1, WG1) if LAYOUT[cls] == SMALL else (V2, WG2)
    assert len({nb for nb, _, _ in CASES[cls]}) == len(NB[cls])  # no nb lost all its variants
    for nb, s0, k in CASES[cls]:
        n = case_n(nb, s0, k)
        p = plan(s0, n, crc64)
        rows = _ceil(nb, v)
        want = dict(layout=LAYOUT[cls], nb=nb, s0=s0, k=k, eoff=s0 + n, rows=rows, Z=rows * v - nb,
                    grid=wg if nb > v else _ceil(nb, 256), fits_service=int(nb <= p["svc_max_blocks"]))
        want["wg0"] = wg - want["grid"]
        assert {f: p[f] for f in want} == want, (cls, nb, s0, k, p)
        assert (rows == 1) == cls.endswith("1row"), (cls, nb)


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_named_states(crc64):
    """The states the table is there for, by name."""
    def at(nb, s0=0, k=0):
        return plan(s0, case_n(nb, s0, k), crc64)
    # small, one row: the result leaves directly (one workgroup) or through the reduce
    assert [at(nb)["grid"] for nb in (255, 256, 257)] == [1, 1, 2]
    assert at(V1)["Z"] == 0 and at(V1)["grid"] == WG1 and at(V1 - 1)["grid"] == WG1 and at(V1 - 1)["wg0"] == 0
    assert (at(8192)["nb"], plan(1, 128 << 10, crc64)["nb"]) == (8192, 8193)
    # small, two rows: a first row of one block; the maximum leaves zero blocks, never a full first row
    assert at(V1 + 1)["Z"] == V1 - 1
    zs = [at(nb)["Z"] for nb in NB["small-2rows"]]
    assert min(zs) == at(SMALL_BLOCKS)["Z"] == SMALL_ROWS * V1 - SMALL_BLOCKS > 0
    assert at(SMALL_BLOCKS - 1)["Z"] == at(SMALL_BLOCKS)["Z"] + 1
    assert {at(nb)["rows"] for nb in NB["small-2rows"]} == {SMALL_ROWS} == {2}
    # mid, one row: partial grids from the smallest to over half the layout, a full row
    assert at(SMALL_BLOCKS + 1)["grid"] == _ceil(SMALL_BLOCKS + 1, 256) == 65
    assert [at(nb)["grid"] for nb in (25600, 25601)] == [100, 101]
    assert at(66000)["grid"] == 258 > WG2 // 2
    assert (at(V2)["grid"], at(V2)["Z"], at(V2 - 1)["grid"], at(V2 - 1)["Z"]) == (WG2, 0, WG2, 1)
    # mid, rows 2..8: every row count, row boundaries from both sides, the 16 MiB maximum
    assert at(V2 + 1)["Z"] == V2 - 1 and at(V2 + 1)["grid"] == WG2
    assert {at(nb)["rows"] for nb in NB["mid-rows2-8"]} == set(range(2, MID_ROWS + 1))
    assert [at(nb)["Z"] for nb in (2 * V2 - 1, 2 * V2, 2 * V2 + 1)] == [1, 0, V2 - 1]
    assert at(MID_BLOCKS)["Z"] == 0 and at(MID_BLOCKS)["rows"] == MID_ROWS and at(MID_BLOCKS - 1)["Z"] == 1


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_handovers(crc64):
    try:
        for mid in (True, False):
            ck.set_mid_kernel(mid)
            got = [plan(s0, n, crc64)["layout"] for s0, n in HANDOVERS]
            assert got == HANDOVER_LAYOUTS[mid], (mid, got)
            # the smallest mid span: the long kernel's with the switch off; the largest small one stays
            assert plan(0, 16 * (SMALL_BLOCKS + 1), crc64)["layout"] == (MID if mid else LONG)
            assert plan(0, 16 * SMALL_BLOCKS, crc64)["layout"] == SMALL
            p = plan(1, 16 * MID_BLOCKS, crc64)
            assert [p[f] for f in ("nb", "rows", "grid", "wg0", "fits_service")] == [0, 0, 0, 0, 0]
    finally:
        ck.set_mid_kernel(True)
    assert plan(0, 16 * MID_BLOCKS, crc64)["nb"] == MID_BLOCKS and plan(1, 16 * SMALL_BLOCKS, crc64)["Z"] == V2 - \
        SMALL_BLOCKS - 1


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_tiny_matrix_reaches_every_edge(crc64):
    ps = {(s0, n): plan(s0, n, crc64) for s0, n in TINY}
    seed_bytes = plan(0, 0, crc64)["seed_bytes"]
    for (s0, n), p in ps.items():
        nb = _ceil(s0 + max(n, seed_bytes), 16)
        want = dict(layout=SMALL, nb=nb, s0=s0, eoff=s0 + n, k=16 * nb - s0 - n, rows=1, grid=1, wg0=WG1 - 1)
        assert {f: p[f] for f in want} == want, (s0, n, p)
    assert {p["nb"] for p in ps.values()} == {1, 2, 3, 4}
    # exactly the tail factors the geometry can ask for (a wider sweep finds no other), all inside
    # the kernels' table of 32
    sweep = {plan(s0, n, crc64)["k"] for s0 in range(16) for n in range(64)}
    ks = {p["k"] for p in ps.values()}
    assert ks == sweep == set(range(max(sweep) + 1)) and 16 <= max(sweep) < 32
    assert max(sweep) == 15 + seed_bytes  # the seed alone, one byte into a second block
    # a seed that starts in block 0 and ends in block 1; a tail whose zero bytes start in block nb - 2
    assert any(s0 < 16 < s0 + seed_bytes for s0, _ in ps)
    assert any(p["k"] > 16 and p["nb"] >= 2 for p in ps.values())
    # head and tail masks in ONE block, and in the two blocks of a two-block grid
    assert any(p["nb"] == 1 and p["s0"] and p["k"] for p in ps.values())
    assert any(p["nb"] == 2 and p["s0"] and p["k"] for p in ps.values())
    # n below the seed's bytes, at every start
    assert {s0 for (s0, n) in ps if n < seed_bytes} == set(range(16))


@pytest.mark.parametrize("crc64", CRCS, ids=IDS)
def test_every_row_count_and_launch_shape(crc64):
    ps = [plan(s0, case_n(nb, s0, k), crc64) for c in CLASSES for nb, s0, k in CASES[c]]
    ps += [plan(s0, n, crc64) for s0, n in TINY]
    assert {p["rows"] for p in ps if p["layout"] == SMALL} == set(range(1, SMALL_ROWS + 1))
    assert {p["rows"] for p in ps if p["layout"] == MID} == set(range(1, MID_ROWS + 1))
    assert {kind(p) for p in ps} == {"small-1wg", "small-multi", "mid-partial", "mid-full"}
    assert MAX_N == 16 * MID_BLOCKS

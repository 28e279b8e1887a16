"""Copy + CRC of mixed-size parts with the piece tasks packed on the device
(photon_crc32c_copy_parts_packed_n, photon_crc64ecma_copy_parts_packed_n,
photon_crc32c_batch_parts_packed_n, photon_crc64ecma_batch_parts_packed_n,
photon_crc_parts_packed_work_bytes) without a GPU: exported,
declared, argument checks, a loud failure where there is no device, the
workspace size against the formula the header states, and the plan itself --
asked of the library through photon_crc_test_parts_packed_plan, which replays
the steps the plan kernels run (photonlibos_amd/csrc/parts_packed_plan.h) --
against photon_crc_test_parts_plan's cut of every part and against the oracle.
The parts are tests/test_copy_parts_abi.py's 17 lengths x 6 source offsets as
ONE batch of 102. CPU only."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen
from tests.test_copy_parts_abi import LENGTHS, OFFSETS, PIECES, SEED32, SEED64, parts_plan

COPY_NAMES = ["photon_crc32c_copy_parts_packed_n", "photon_crc64ecma_copy_parts_packed_n"]
BATCH_NAMES = ["photon_crc32c_batch_parts_packed_n", "photon_crc64ecma_batch_parts_packed_n"]
ARGC = {**{n: 12 for n in COPY_NAMES}, **{n: 11 for n in BATCH_NAMES}, "photon_crc_parts_packed_work_bytes": 3}
WRAPPERS = ["copy_parts_packed_device", "copy_parts64_packed_device", "batch_parts_packed_device",
            "batch_parts64_packed_device", "parts_packed_work_bytes"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
ALL = (1 << 64) - 1
CAPS = [ALL, 10000, 8192, 8191, 0]

# shared with tests/test_gpu_copy_parts_packed.py: the 102 parts, in file order
SHAPES = [(n, off) for n in LENGTHS for off in OFFSETS]


@pytest.fixture()
def piece_setting():
    yield ck.set_parts_piece
    ck.set_parts_piece(0)


def _header(name):
    return open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", name)).read()


def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    header = _header("crc32c_gpu.h")
    assert len(ARGC) == 5
    for n, argc in ARGC.items():
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == argc, n  # prototype set by _native._declare
        assert f" {n}(" in header, n
    n = "photon_crc_test_parts_packed_plan"
    assert n in exported and f"int {n}(" in _header("tuning.h")
    assert len(getattr(L, n).argtypes) == 10


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


S, D, O, R, W = 0x10000, 0x20000, 0x30000, 0x50000, 0x40000  # never dereferenced: the checks come first
BIG = 1 << 40


def _raw(name, src, dst, nparts, max_bytes, max_total, out, report, work, work_bytes):
    f = getattr(_native.lib(), name)
    if name in COPY_NAMES:
        return f(src, dst, nparts, max_bytes, max_total, 7, None, out, report, work, work_bytes, None)
    return f(src, nparts, max_bytes, max_total, 7, None, out, report, work, work_bytes, None)


def _text():
    return _native.lib().photon_crc_last_error().decode()


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_null_arguments_are_einval(name):
    rows = [(None, D, O, R, W), (S, D, None, R, W), (S, D, O, None, W), (S, D, O, R, None)]
    if name in COPY_NAMES:
        rows.append((S, None, O, R, W))
    for src, dst, out, report, work in rows:
        assert _raw(name, src, dst, 3, ALL, 100, out, report, work, BIG) == -22, (src, dst, out, report, work)
        assert "null" in _text(), (src, dst, out, report, work)


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_short_workspace_is_einval(name, piece_setting):
    crc64 = "crc64" in name
    for piece in (0, 4096):
        piece_setting(piece)
        need = ck.parts_packed_work_bytes(3, 100000, crc64)
        assert need > 0
        for have in (0, need - 1):
            assert _raw(name, S, D, 3, ALL, 100000, O, R, W, have) == -22
            assert str(have) in _text() and str(need) in _text(), _text()


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_limits_are_einval(name, piece_setting):
    piece_setting(4096)
    # C = total / piece + nparts above 2^40
    total = 4096 << 40
    assert _raw(name, S, D, 1, ALL, total, O, R, W, 1 << 62) == -22
    assert "slots" in _text() and str((1 << 40) + 1) in _text() and str(1 << 40) in _text(), _text()
    assert _raw(name, S, D, 2, ALL, total - 4096, O, R, W, 1 << 62) == -22
    assert ck.parts_packed_work_bytes(1, total) == ALL
    assert ck.parts_packed_work_bytes(1, total - 4096) != ALL  # C == 2^40 is taken
    # nparts above 2^31
    n = (1 << 31) + 1
    assert _raw(name, S, D, n, ALL, 0, O, R, W, 1 << 62) == -22
    assert "parts" in _text() and str(n) in _text() and str(1 << 31) in _text(), _text()
    assert ck.parts_packed_work_bytes(n, 0) == ALL
    assert ck.parts_packed_work_bytes(1 << 31, 0) != ALL


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_no_parts_returns_zero(name):
    assert _raw(name, None, None, 0, 100, 100, None, None, None, 0) == 0
    assert _raw(name, S, D, 0, 0, 0, O, R, W, 0) == 0


def test_wrappers_raise():
    c, c64, b, b64 = (ck.copy_parts_packed_device, ck.copy_parts64_packed_device, ck.batch_parts_packed_device,
                      ck.batch_parts64_packed_device)
    for call, word in ((lambda: c(None, D, 2, ALL, 100, O, R, W, BIG), "null"),
                       (lambda: c(S, None, 2, ALL, 100, O, R, W, BIG), "null"),
                       (lambda: c64(S, D, 2, ALL, 100, None, R, W, BIG, seed=5), "null"),
                       (lambda: c64(S, D, 2, ALL, 100, O, None, W, BIG), "null"),
                       (lambda: c(S, D, 2, ALL, 100, O, R, None, BIG), "null"),
                       (lambda: b(None, 2, ALL, 100, O, R, W, BIG), "null"),
                       (lambda: b64(S, 2, ALL, 100, O, R, None, BIG), "null"),
                       (lambda: b(S, 2, ALL, 100, None, R, W, BIG), "null"),
                       (lambda: c(S, D, 2, ALL, 100, O, R, W, 7), "7"),
                       (lambda: c64(S, D, 2, ALL, 100, O, R, W, 15), "15"),
                       (lambda: b(S, 2, ALL, 100, O, R, W, 0), "workspace"),
                       (lambda: b64(S, 2, ALL, 100, O, R, W, 8), "workspace"),
                       (lambda: b(S, (1 << 31) + 1, ALL, 100, O, R, W, 1 << 62), "parts"),
                       (lambda: c64(S, D, 2, ALL, ALL, O, R, W, 1 << 62), "slots")):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code == -22 and word in str(e.value)


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for call in (lambda: ck.copy_parts_packed_device(S, D, 2, ALL, 100, O, R, W, BIG),
                 lambda: ck.copy_parts64_packed_device(S, D, 2, ALL, 100, O, R, W, BIG, seed=1),
                 lambda: ck.batch_parts_packed_device(S, 2, 100, 100, O, R, W, BIG),
                 lambda: ck.batch_parts64_packed_device(S, 2, 0, 0, O, R, W, BIG)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code < 0 and e.value.code != -22


def _header_formula():
    """The workspace formula as the header states it, made callable: (nparts, C, w) -> bytes."""
    header = _header("crc32c_gpu.h")
    assert "C = floor(max_total_bytes / piece) + nparts" in header
    m = re.search(r"photon_crc_parts_packed_work_bytes\(nparts, max_total_bytes, crc64\)\s*\*\s*=([^\n]*)\n", header)
    assert m, "the header does not state the formula"
    text = m.group(1).strip()
    assert text == "8 (nparts + 1) + 16 ceil(nparts / 1024) + 8 ceil(C w / 8) + 8 ceil(C / 2)"
    code = re.sub(r"(\d+) (?=[(c])", r"\1 * ", text).replace("C w", "C * w")
    return lambda nparts, c, w: int(eval(code, {"ceil": math.ceil, "nparts": Fraction(nparts), "C": Fraction(c),
                                                "w": w}))


def test_work_bytes_is_the_formula_in_the_header(piece_setting):
    formula = _header_formula()
    assert formula(3, 5, 4) == 8 * 4 + 16 + 8 * 3 + 8 * 3
    for piece in (0, 4096, 65536):
        piece_setting(piece)
        eff = piece or 32768
        for nparts in (1, 2, 3, 102, 1024, 1025, 5000, 1 << 20):
            for total in (0, 1, eff - 1, eff, eff + 1, 10 * eff + 7, 1 << 30, (1 << 36) + 12345):
                c = total // eff + nparts
                for crc64 in (False, True):
                    got = ck.parts_packed_work_bytes(nparts, total, crc64)
                    assert got == formula(nparts, c, 8 if crc64 else 4), (piece, nparts, total, crc64)
                    assert got % 8 == 0
    assert ck.parts_packed_work_bytes(0, 1 << 20) == 0


def packed_plan(addrs, lens, cap, total, piece):
    """(first[0..nparts], report[0..3], [(part, offset, length) per task]) of one call, replayed on the CPU."""
    n = len(addrs)
    a = (ctypes.c_uint64 * n)(*addrs)
    ln = (ctypes.c_uint64 * n)(*lens)
    first = (ctypes.c_uint64 * (n + 1))()
    report = (ctypes.c_uint64 * 4)()
    task_cap = sum(min(x, cap) for x in lens) // piece + n
    tasks = (ctypes.c_uint64 * (3 * max(task_cap, 1)))()
    rc = _native.lib().photon_crc_test_parts_packed_plan(a, ln, n, cap, total, piece, first, report, tasks, task_cap)
    assert rc == 0, _text()
    ntasks = 0 if report[0] else int(report[1])
    return ([int(x) for x in first], [int(x) for x in report],
            [(int(tasks[3 * t]), int(tasks[3 * t + 1]), int(tasks[3 * t + 2])) for t in range(ntasks)])


def _orders():
    base = list(SHAPES)
    empties = [(0, 1), (0, 0), (0, 4095)]
    return {"file order": base, "reversed": base[::-1],
            "empties at the front, in the middle and at the end":
                empties + base[:50] + empties + empties + base[50:] + empties}


@pytest.fixture(scope="module")
def payload():
    return datagen.stream_bytes(0x9A27, 4096 + max(LENGTHS))


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("order", list(_orders()))
def test_plan(oracle, payload, order, piece):
    shapes = _orders()[order]
    n = len(shapes)
    addrs = [(1 << 32) + (k << 20) + off for k, (_, off) in enumerate(shapes)]
    lens = [ln for ln, _ in shapes]
    for cap in CAPS:
        what = (order, piece, cap)
        capped = [min(x, cap) for x in lens]
        total = sum(capped)
        # every part's cut by the hook of the calls of §4.9 (the same n_i under a cap the old plan takes)
        cuts = [parts_plan(a, ln, min(cap, max(LENGTHS)), piece)[1] for a, ln in zip(addrs, lens)]
        want_first = [0]
        for c in cuts:
            want_first.append(want_first[-1] + len(c))
        T = want_first[-1]
        for max_total in (total, total + 1, total + 12345, 1 << 40):
            first, report, tasks = packed_plan(addrs, lens, cap, max_total, piece)
            C = max_total // piece + n
            assert T <= C, what  # the bound the header derives
            assert report == [0, T, total, C], (what, max_total)
            assert first == want_first, (what, max_total)
            assert len(tasks) == T
            for i, c in enumerate(cuts):  # tasks first[i] .. first[i+1] are part i's pieces, in order
                assert tasks[first[i]:first[i + 1]] == [(i, o, ln) for o, ln in c], (what, i)
        if T > n:  # a total that leaves one slot too few: the flag, and no task
            for max_total in (0, piece * (T - n - 1), piece * (T - n) - 1):
                first, report, tasks = packed_plan(addrs, lens, cap, max_total, piece)
                assert report == [1, T, total, max_total // piece + n] and T > report[3], (what, max_total)
                assert first == want_first and tasks == [], (what, max_total)
            first, report, tasks = packed_plan(addrs, lens, cap, piece * (T - n), piece)  # C == T
            assert report == [0, T, total, T] and len(tasks) == T, what
        else:
            assert packed_plan(addrs, lens, cap, 0, piece)[1] == [0, T, total, n], what
        if order != "file order":
            continue
        # the oracle's piece CRCs, folded by the host combine in task order, give the oracle's CRC of each part
        first, report, tasks = packed_plan(addrs, lens, cap, total, piece)
        for i, (ln, off) in enumerate(shapes):
            data = payload[off:off + capped[i]]
            for seed32, seed64 in ((0, 0), (SEED32, SEED64)):
                a32, a64 = seed32, seed64
                for part, o, m in tasks[first[i]:first[i + 1]]:
                    assert part == i
                    a32 = ck.crc32c_combine(a32, oracle.crc32c(data[o:o + m], 0), m)
                    a64 = ck.crc64ecma_combine(a64, oracle.crc64ecma(data[o:o + m], 0), m)
                assert a32 == oracle.crc32c(data, seed32), (what, i)
                assert a64 == oracle.crc64ecma(data, seed64), (what, i)


def test_plan_over_several_tiles():
    # 2,500 parts: three plan tiles of 1,024, the last one short
    rng = np.random.default_rng(2500)
    lens = [int(x) for x in rng.choice([0, 0, 1, 100, 4096, 5000, 8193, 12289, 70001], 2500)]
    offs = [int(x) for x in rng.choice(OFFSETS, 2500)]
    addrs = [(1 << 32) + (k << 20) + off for k, off in enumerate(offs)]
    cuts = [parts_plan(a, ln, max(LENGTHS), 4096)[1] for a, ln in zip(addrs, lens)]
    first, report, tasks = packed_plan(addrs, lens, ALL, sum(lens), 4096)
    assert first == [sum(len(c) for c in cuts[:i]) for i in range(2501)]
    assert report == [0, first[-1], sum(lens), sum(lens) // 4096 + 2500]
    assert tasks == [(i, o, ln) for i, c in enumerate(cuts) for o, ln in c]


def test_plan_rejects_bad_arguments():
    L = _native.lib()
    a = (ctypes.c_uint64 * 2)(1 << 32, 1 << 33)
    ln = (ctypes.c_uint64 * 2)(70001, 5)
    first, report, tasks = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 4)(), (ctypes.c_uint64 * 300)()
    f = L.photon_crc_test_parts_packed_plan
    assert f(a, ln, 2, ALL, 1 << 20, 1000, first, report, tasks, 100) == -22  # piece
    assert f(a, ln, 2, ALL, 1 << 20, 4096, first, report, tasks, 5) == -22    # 19 tasks do not fit
    assert f(None, ln, 2, ALL, 1 << 20, 4096, first, report, tasks, 100) == -22
    assert f(a, ln, 0, ALL, 1 << 20, 4096, first, report, tasks, 100) == -22
    assert f(a, ln, 2, ALL, 1 << 20, 4096, first, report, tasks, 100) == 0
    assert list(first) == [0, 18, 19] and list(report) == [0, 19, 70006, 258]

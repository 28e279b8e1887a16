"""Copy + CRC of many large parts in one launch, each cut over the chip
(photon_crc32c_copy_parts_n, photon_crc64ecma_copy_parts_n,
photon_crc32c_batch_parts_n, photon_crc64ecma_batch_parts_n,
photon_crc_parts_work_bytes) without a GPU: exported,
declared, argument checks, a loud failure where there is no device, the
workspace size, and the cut itself -- asked of the library through
photon_crc_test_parts_plan, which runs the derivation the piece kernels run
(photonlibos_amd/csrc/parts_plan.h) -- checked for tiling, alignment, the
slot bound, and against the oracle: the pieces' CRCs from seed 0 folded with
the host combine give the CRC of the capped part. CPU only."""
import ctypes
import os

import numpy as np
import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck
from photonlibos_amd import datagen

COPY_NAMES = ["photon_crc32c_copy_parts_n", "photon_crc64ecma_copy_parts_n"]
BATCH_NAMES = ["photon_crc32c_batch_parts_n", "photon_crc64ecma_batch_parts_n"]
ARGC = {**{n: 10 for n in COPY_NAMES}, **{n: 9 for n in BATCH_NAMES}, "photon_crc_parts_work_bytes": 3}
WRAPPERS = ["copy_parts_device", "copy_parts64_device", "batch_parts_device", "batch_parts64_device",
            "parts_work_bytes", "set_parts_piece"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))

# shared with tests/test_gpu_copy_parts.py
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 20487, 70001]
OFFSETS = [0, 1, 5, 2048, 4081, 4095]  # of the source from a 4 KiB boundary
PIECES = [4096, 65536]
SEED32, SEED64 = 0x9E3779B1, 0xFEDCBA9876543210


@pytest.fixture()
def piece_setting():
    yield ck.set_parts_piece
    ck.set_parts_piece(0)


def parts_plan(addr, length, max_part_bytes, piece):
    """(P, [(offset, length), ...]) of one part, as the piece kernels cut it."""
    out = (ctypes.c_uint64 * 4096)()
    k = _native.lib().photon_crc_test_parts_plan(addr, length, max_part_bytes, piece, out, len(out))
    assert k >= 2, _native.lib().photon_crc_last_error()
    assert k == 2 + 2 * int(out[1])
    return int(out[0]), [(int(out[2 + 2 * j]), int(out[3 + 2 * j])) for j in range(int(out[1]))]


def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    header = open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", "crc32c_gpu.h")).read()
    assert len(ARGC) == 5
    for n, argc in ARGC.items():
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == argc, n  # prototype set by _native._declare
        assert f" {n}(" in header, n
    tuning = open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", "tuning.h")).read()
    for n in ("photon_crc_set_parts_piece", "photon_crc_test_parts_plan"):
        assert n in exported and f"int {n}(" in tuning, n


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


S, D, O, W = 0x10000, 0x20000, 0x30000, 0x40000  # never dereferenced: the checks come first
BIG = 1 << 30


def _raw(name, src, dst, nparts, max_bytes, out, work, work_bytes):
    f = getattr(_native.lib(), name)
    if name in COPY_NAMES:
        return f(src, dst, nparts, max_bytes, 7, None, out, work, work_bytes, None)
    return f(src, nparts, max_bytes, 7, None, out, work, work_bytes, None)


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_null_arguments_are_einval(name):
    L = _native.lib()
    rows = [(None, D, O, W), (S, D, None, W), (S, D, O, None)]
    if name in COPY_NAMES:
        rows.append((S, None, O, W))
    for src, dst, out, work in rows:
        assert _raw(name, src, dst, 3, 100, out, work, BIG) == -22, (src, dst, out, work)
        assert b"null" in L.photon_crc_last_error(), (src, dst, out, work)


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_short_workspace_is_einval(name, piece_setting):
    L = _native.lib()
    crc64 = "crc64" in name
    for piece in (0, 4096):
        piece_setting(piece)
        need = ck.parts_work_bytes(3, 100000, crc64)
        assert need > 0
        for have in (0, need - 1):
            assert _raw(name, S, D, 3, 100000, O, W, have) == -22
            text = L.photon_crc_last_error().decode()
            assert str(have) in text and str(need) in text, text


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_too_many_tasks_is_einval(name):
    assert _raw(name, S, D, 1 << 39, 1 << 30, O, W, 1 << 62) == -22
    assert b"tasks" in _native.lib().photon_crc_last_error()


@pytest.mark.parametrize("name", COPY_NAMES + BATCH_NAMES)
def test_no_parts_returns_zero(name):
    assert _raw(name, None, None, 0, 100, None, None, 0) == 0
    assert _raw(name, S, D, 0, 0, O, W, 0) == 0


def test_wrappers_raise():
    for call, word in ((lambda: ck.copy_parts_device(None, D, 2, 100, O, W, BIG), "null"),
                       (lambda: ck.copy_parts_device(S, None, 2, 100, O, W, BIG), "null"),
                       (lambda: ck.copy_parts64_device(S, D, 2, 100, None, W, BIG, seed=5), "null"),
                       (lambda: ck.copy_parts64_device(S, D, 2, 100, O, None, BIG), "null"),
                       (lambda: ck.batch_parts_device(None, 2, 100, O, W, BIG), "null"),
                       (lambda: ck.batch_parts64_device(S, 2, 100, O, None, BIG), "null"),
                       (lambda: ck.copy_parts_device(S, D, 2, 100, O, W, 7), "7"),
                       (lambda: ck.copy_parts64_device(S, D, 2, 100, O, W, 15), "15"),
                       (lambda: ck.batch_parts_device(S, 2, 100, O, W, 0), "workspace"),
                       (lambda: ck.batch_parts64_device(S, 2, 100, O, W, 8), "workspace")):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code == -22 and word in str(e.value)
    with pytest.raises(ck.CrcError):
        ck.set_parts_piece(4097)
    with pytest.raises(ck.CrcError):
        ck.set_parts_piece(2048)


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for call in (lambda: ck.copy_parts_device(S, D, 2, 100, O, W, BIG),
                 lambda: ck.copy_parts64_device(S, D, 2, 100, O, W, BIG, seed=1),
                 lambda: ck.batch_parts_device(S, 2, 100, O, W, BIG),
                 lambda: ck.batch_parts64_device(S, 2, 0, O, W, BIG)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code < 0 and e.value.code != -22


def test_work_bytes(piece_setting):
    for piece in (0, 4096, 65536, 128 << 10):
        piece_setting(piece)
        for max_bytes in (0, 1, 4096, 4097, 10000, 65536, 65537, 3 << 20, (16 << 20) + 5):
            p, _ = parts_plan(1 << 32, 0, max_bytes, 0)  # piece 0: the current setting
            eff = piece or 32768
            assert p == max(1, -(-max_bytes // eff)), (piece, max_bytes, p)
            for nparts in (1, 3, 1024):
                assert ck.parts_work_bytes(nparts, max_bytes) == nparts * p * 4
                assert ck.parts_work_bytes(nparts, max_bytes, True) == nparts * p * 8
    assert ck.parts_work_bytes(0, 1 << 20) == 0


@pytest.fixture(scope="module")
def payload():
    return datagen.stream_bytes(0x9A27, 4096 + max(LENGTHS))


def _caps(length, off, piece):
    head = (-off) % 4096
    # above the length, below it, on a piece boundary (the head's end and the first piece's end), 0
    return sorted({length + 1000, length // 2, head + piece, head + 2 * piece, head, 0})


@pytest.mark.parametrize("piece", PIECES)
@pytest.mark.parametrize("off", OFFSETS)
def test_cut(oracle, payload, off, piece):
    addr = (1 << 32) + off
    for length in LENGTHS:
        for cap in _caps(length, off, piece):
            what = (length, off, piece, cap)
            n = min(length, cap)
            p, pieces = parts_plan(addr, length, cap, piece)
            assert p == max(1, -(-cap // piece)), what
            assert len(pieces) <= p, what
            assert len(pieces) == 0 if n == 0 else len(pieces) >= 1, what
            pos = 0
            for j, (o, ln) in enumerate(pieces):  # the pieces tile [0, n) in order
                assert o == pos and ln > 0, what
                if j:
                    assert (addr + o) % 4096 == 0, what
                    assert ln == piece or j == len(pieces) - 1, what  # every middle piece is full
                pos += ln
            assert pos == n, what
            if len(pieces) > 1:
                assert pieces[0][1] == (-off) % 4096 + piece and pieces[-1][1] <= piece, what
            data = payload[off:off + n]
            for seed32, seed64 in ((0, 0), (SEED32, SEED64)):
                a32, a64 = seed32, seed64
                for o, ln in pieces:
                    a32 = ck.crc32c_combine(a32, oracle.crc32c(data[o:o + ln], 0), ln)
                    a64 = ck.crc64ecma_combine(a64, oracle.crc64ecma(data[o:o + ln], 0), ln)
                assert a32 == oracle.crc32c(data, seed32), what
                assert a64 == oracle.crc64ecma(data, seed64), what


def test_cut_rejects_bad_piece():
    out = (ctypes.c_uint64 * 16)()
    L = _native.lib()
    assert L.photon_crc_test_parts_plan(1 << 32, 100, 100, 1000, out, 16) == -22
    assert L.photon_crc_test_parts_plan(1 << 32, 70001, 70001, 4096, out, 16) == -22  # 18 pieces do not fit
    assert L.photon_crc_test_parts_plan(1 << 32, 100, 100, 4096, None, 16) == -22

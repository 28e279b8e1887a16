"""Copy + CRC of one long buffer over the whole device
(photon_crc32c_copy_extend_device, photon_crc64ecma_copy_extend_device)
without a GPU: exported, declared, argument checks, a loud failure where
there is no device, and the plan conditions of tests/test_gpu_copy_long.py --
that each of its shapes reaches the state of the cut it is there for (the
head slot alone, a merged head, empty leading slots, a tiny last chunk,
several rounds, every workgroup factor), asked of the library through
photon_crc_test_long_plan. CPU only."""
import ctypes
import os

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = ["photon_crc32c_copy_extend_device", "photon_crc64ecma_copy_extend_device"]
WRAPPERS = ["copy_extend_device", "copy_extend64_device"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
MIB = 1 << 20

# (source offset from a 4 KiB boundary, nbytes, forced lanes, forced rounds, expected plan); 0 = automatic.
# The same for both CRCs. head / chunk / T / L / R / grid / S / D as photon_crc_test_long_plan names them.
PLAN_SHAPES = [
    (5, 63, 0, 0, dict(head=63, T=0)),                                    # the head slot alone
    (0, 4096, 0, 0, dict(T=1, D=15)),                                     # 15 empty leading slots
    (5, 65539, 0, 0, dict(head=4091, chunk=4096, T=16, L=8, D=0)),        # tiny last chunk, merged head
    (0, MIB, 64, 2, dict(chunk=8192, T=128, R=2, grid=4, D=0)),
    (1, MIB, 64, 2, dict(head=4095, L=4097, D=0)),
    (0, 1000013, 64, 2, dict(T=123, L=589, D=5)),
    (4095, 1000013, 32, 2, dict(head=1, L=588, grid=2, S=64, D=5)),
    (0, 3 * MIB + 5, 64, 3, dict(T=385, L=5, R=3, grid=9, D=47)),
    (9, 3 * MIB + 5, 32, 3, dict(head=4087, T=384, L=4110, grid=4, D=0)),
    (0, 36 * MIB, 0, 0, dict(chunk=9216, T=4096, grid=256, D=0)),         # every workgroup factor
    (1, 36 * MIB - 100000, 0, 0, dict(T=4085, L=6497, grid=256, D=11)),
]


def long_plan(addr, n, lanes, rounds, crc64, cus=256):
    out = (ctypes.c_uint64 * 512)()
    k = _native.lib().photon_crc_test_long_plan(addr, n, cus, lanes, rounds, int(crc64), out, len(out))
    assert k >= 9, _native.lib().photon_crc_last_error()
    return dict(zip(("head", "chunk", "T", "L", "R", "grid", "S", "D", "lanes"), (int(x) for x in out[:9])))


def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    header = open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", "crc32c_gpu.h")).read()
    for n in NAMES:
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == 6, n  # prototype set by _native._declare
        assert f"int {n}(" in header, n


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


S, D, O = 0x10000, 0x20000, 0x30000  # never dereferenced: the checks come first


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_einval(name):
    L = _native.lib()
    f = getattr(L, name)
    for src, dst, n, out in ((S, D, 100, None),     # d_out
                             (S, D, 0, None),       # d_out, also for an empty buffer
                             (None, None, 0, None),
                             (None, D, 100, O),     # src with nbytes > 0
                             (S, None, 100, O),     # d_dst with nbytes > 0
                             (None, None, 1, O)):
        assert f(src, dst, n, 7, out, None) == -22, (src, dst, n, out)
        assert b"null" in L.photon_crc_last_error(), (src, dst, n, out)


def test_wrappers_raise():
    for call in (lambda: ck.copy_extend_device(S, D, 100, 0, None),
                 lambda: ck.copy_extend_device(None, D, 100, 0, O),
                 lambda: ck.copy_extend_device(S, None, 100, 0, O),
                 lambda: ck.copy_extend64_device(S, D, 100, None),
                 lambda: ck.copy_extend64_device(None, D, 100, O, seed=5),
                 lambda: ck.copy_extend64_device(S, None, 100, O)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code == -22 and "null" in str(e.value)


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for call in (lambda: ck.copy_extend_device(S, D, 100, 1, O),
                 lambda: ck.copy_extend_device(None, None, 0, 1, O),
                 lambda: ck.copy_extend64_device(S, D, 1 << 30, O, seed=1),
                 lambda: ck.copy_extend64_device(None, None, 0, O)):
        with pytest.raises(ck.CrcError) as e:
            call()
        assert e.value.code < 0


@pytest.mark.parametrize("crc64", [False, True])
@pytest.mark.parametrize("row", range(len(PLAN_SHAPES)))
def test_plan_conditions(row, crc64):
    off, n, lanes, rounds, want = PLAN_SHAPES[row]
    p = long_plan((1 << 32) + off, n, lanes, rounds, crc64)
    got = {k: p[k] for k in want}
    assert got == want, (PLAN_SHAPES[row], p)
    if lanes:
        assert p["lanes"] == lanes and p["R"] == rounds
    # what the kernels rely on: T chunks in R S slots, D empty ones in front
    assert p["D"] == p["R"] * p["S"] - p["T"] and p["S"] == p["grid"] * 16 * (64 // p["lanes"])
    assert p["head"] + (p["T"] - 1) * p["chunk"] + p["L"] == n if p["T"] else p["head"] == n

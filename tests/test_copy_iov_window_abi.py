"""The ranged read from checksummed blocks
(photon_crc32c_copy_msg_iov_window_n, photon_crc64ecma_copy_msg_iov_window_n,
photon_crc_window_work_bytes) without a GPU: exported, declared, the workspace
size, argument checks, and a loud failure where there is no device. CPU only."""
import os

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = ["photon_crc32c_copy_msg_iov_window_n", "photon_crc64ecma_copy_msg_iov_window_n"]
WRAPPERS = ["copy_msg_iov_window_n", "copy_msg64_iov_window_n"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))


def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    for n in NAMES:
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == 16, n  # prototype set by _native._declare
    assert "photon_crc_window_work_bytes" in exported
    assert len(L.photon_crc_window_work_bytes.argtypes) == 1
    header = open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", "crc32c_gpu.h")).read()
    for n in NAMES:
        assert f"int {n}(" in header, n
    assert "uint64_t photon_crc_window_work_bytes(uint64_t nmsg);" in header


def test_wrappers_in_all():
    for n in WRAPPERS + ["window_work_bytes"]:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


def test_work_bytes():
    for nmsg in (0, 1, 2, 63, 64, 65, 1000, 1 << 16, (1 << 40) + 7):
        assert ck.window_work_bytes(nmsg) == 16 * nmsg
        assert _native.lib().photon_crc_window_work_bytes(nmsg) == 16 * nmsg


@pytest.mark.parametrize("name", NAMES)
def test_zero_messages_return_0(name):
    f = getattr(_native.lib(), name)
    assert f(None, None, 0, None, None, 0, 0, None, None, 0, None, None, None, None, None, None) == 0
    # before any check
    assert f(None, None, 5, None, None, 7, 0, None, None, 0, None, None, None, None, None, None) == 0


# never dereferenced: the checks come first
S, SS, D, DS, GS, O, W = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x68000


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_einval(name):
    L = _native.lib()
    f = getattr(L, name)

    def call(s, ss, nsrc, d, ds, ndst, gs, o, w):
        return f(s, ss, nsrc, d, ds, ndst, 2, None, None, 0, None, gs, o, None, w, None)

    cases = ((S, None, 3, D, DS, 3, GS, O, W),      # d_src_start
             (S, SS, 3, D, None, 3, GS, O, W),      # d_dst_start
             (S, SS, 3, D, DS, 3, GS, None, W),     # d_out
             (S, SS, 3, D, DS, 3, None, O, W),      # d_src_seg_out
             (S, SS, 3, D, DS, 3, GS, O, None),     # d_work
             (None, SS, 3, D, DS, 3, GS, O, W),     # d_src with nsrc > 0
             (S, SS, 3, None, DS, 3, GS, O, W))     # d_dst with ndst > 0
    assert len(cases) == 7
    for args in cases:
        assert call(*args) == -22, args
        assert b"null" in L.photon_crc_last_error(), args


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_wrapper_raises(wrapper):
    with pytest.raises(ck.CrcError) as e:  # null d_src_seg_out
        getattr(ck, wrapper)(S, SS, 1, D, DS, 1, 1, None, O, W)
    assert e.value.code == -22 and "null" in str(e.value)
    with pytest.raises(ck.CrcError) as e:  # null d_work
        getattr(ck, wrapper)(S, SS, 1, D, DS, 1, 1, GS, O, None)
    assert e.value.code == -22 and "null" in str(e.value)


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_calls_fail_loudly_without_gpu(wrapper):
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    with pytest.raises(ck.CrcError) as e:
        getattr(ck, wrapper)(S, SS, 1, D, DS, 1, 1, GS, O, W, skip=0x6C000, size=0x70000, seeds=0x80000,
                             copied=0x90000)
    assert e.value.code < 0
    # null descriptor arrays are fine when there are no segments: still no device
    with pytest.raises(ck.CrcError) as e:
        getattr(ck, wrapper)(None, SS, 0, None, DS, 0, 1, GS, O, W)
    assert e.value.code < 0

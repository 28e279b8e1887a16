"""Copy + CRC between iovectors (photon_crc32c_copy_msg_iov_n,
photon_crc64ecma_copy_msg_iov_n) without a GPU: exported, declared, argument
checks, and a loud failure where there is no device. CPU only."""
import os

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = ["photon_crc32c_copy_msg_iov_n", "photon_crc64ecma_copy_msg_iov_n"]
WRAPPERS = ["copy_msg_iov_n", "copy_msg64_iov_n"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))


def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    for n in NAMES:
        assert n in exported, n
        assert len(getattr(L, n).argtypes) == 13, n  # prototype set by _native._declare
    header = open(os.path.join(os.path.dirname(_native._HERE), "include", "photon_crc", "crc32c_gpu.h")).read()
    for n in NAMES:
        assert f"int {n}(" in header, n


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


@pytest.mark.parametrize("name", NAMES)
def test_zero_messages_return_0(name):
    f = getattr(_native.lib(), name)
    assert f(None, None, 0, None, None, 0, 0, None, 0, None, None, None, None) == 0
    assert f(None, None, 5, None, None, 7, 0, None, 0, None, None, None, None) == 0


@pytest.mark.parametrize("name", NAMES)
def test_null_arguments_are_einval(name):
    L = _native.lib()
    f = getattr(L, name)
    S, SS, D, DS, O = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # never dereferenced: the checks come first

    def call(s, ss, nsrc, d, ds, ndst, o):
        return f(s, ss, nsrc, d, ds, ndst, 2, None, 0, None, o, None, None)

    for args in ((S, None, 3, D, DS, 3, O),      # d_src_start
                 (S, SS, 3, D, None, 3, O),      # d_dst_start
                 (S, SS, 3, D, DS, 3, None),     # d_out
                 (None, SS, 3, D, DS, 3, O),     # d_src with nsrc > 0
                 (S, SS, 3, None, DS, 3, O)):    # d_dst with ndst > 0
        assert call(*args) == -22, args
        assert b"null" in L.photon_crc_last_error(), args


@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_wrapper_raises(wrapper):
    with pytest.raises(ck.CrcError) as e:
        getattr(ck, wrapper)(0x10000, None, 1, 0x30000, 0x40000, 1, 1, 0x50000)
    assert e.value.code == -22


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
@pytest.mark.parametrize("wrapper", WRAPPERS)
def test_calls_fail_loudly_without_gpu(wrapper):
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    with pytest.raises(ck.CrcError) as e:
        getattr(ck, wrapper)(0x10000, 0x20000, 1, 0x30000, 0x40000, 1, 1, 0x50000, size=0x60000, seeds=0x70000,
                             copied=0x80000)
    assert e.value.code < 0
    # null descriptor arrays are fine when there are no segments: still no device
    with pytest.raises(ck.CrcError) as e:
        getattr(ck, wrapper)(None, 0x20000, 0, None, 0x40000, 0, 1, 0x50000)
    assert e.value.code < 0

"""Copy + CRC-64/ECMA entry points without a GPU: exported, declared, argument
checks, and a loud failure where there is no device. CPU only."""
import os

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = ["photon_crc64ecma_copy_batch_strided", "photon_crc64ecma_copy_batch_iov", "photon_crc64ecma_gather_msg_n"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))


def test_symbols_exported_and_declared():
    import subprocess
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    for n in NAMES:
        assert n in exported, n
        assert getattr(L, n).argtypes, n  # prototype set by _native._declare


def test_wrappers_in_all():
    for n in ("copy_batch64_strided", "copy_batch64_iov", "gather64_msg_n"):
        assert n in ck.__all__ and callable(getattr(ck, n)), n


def test_zero_counts_return_0():
    L = _native.lib()
    assert L.photon_crc64ecma_copy_batch_strided(None, 0, None, 0, 4096, 0, 0, None, None, None) == 0
    assert L.photon_crc64ecma_copy_batch_iov(None, None, 0, 0, None, None, None) == 0
    assert L.photon_crc64ecma_gather_msg_n(None, None, 0, 0, None, 0, None, None, None, None) == 0


def test_null_arguments_are_einval():
    L = _native.lib()
    S, D, O, I, M = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000  # never dereferenced: the checks come first
    strided = lambda s, d, o: L.photon_crc64ecma_copy_batch_strided(s, 4096, d, 4096, 4096, 2, 0, None, o, None)
    for s in (None, S):
        for d in (None, D):
            for o in (None, O):
                if s and d and o:
                    continue
                assert strided(s, d, o) == -22, (s, d, o)
                assert b"null" in L.photon_crc_last_error()
    iov = lambda i, d, o: L.photon_crc64ecma_copy_batch_iov(i, d, 2, 0, None, o, None)
    for i in (None, I):
        for d in (None, D):
            for o in (None, O):
                if i and d and o:
                    continue
                assert iov(i, d, o) == -22, (i, d, o)
                assert b"null" in L.photon_crc_last_error()
    gather = lambda i, m, d, o, seg: L.photon_crc64ecma_gather_msg_n(i, m, 2, 3, d, 0, None, seg, o, None)
    for i in (None, I):
        for m in (None, M):
            for d in (None, D):
                for o in (None, O):
                    if i and m and d and o:
                        continue
                    for seg in (None, O + 0x100):  # optional: decides nothing
                        assert gather(i, m, d, o, seg) == -22, (i, m, d, o, seg)
                        assert b"null" in L.photon_crc_last_error()
    with pytest.raises(ck.CrcError) as e:
        ck.copy_batch64_strided(None, 4096, None, 4096, 4096, 4, None)
    assert e.value.code == -22
    with pytest.raises(ck.CrcError) as e:
        ck.copy_batch64_iov(None, None, 4, None)
    assert e.value.code == -22
    with pytest.raises(ck.CrcError) as e:
        ck.gather64_msg_n(None, None, 4, 4, None, None, None)
    assert e.value.code == -22


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    with pytest.raises(ck.CrcError) as e:
        ck.copy_batch64_strided(0x10000, 4096, 0x20000, 4096, 4096, 1, 0x30000)
    assert e.value.code < 0
    with pytest.raises(ck.CrcError) as e:
        ck.copy_batch64_iov(0x40000, 0x20000, 1, 0x30000)
    assert e.value.code < 0
    with pytest.raises(ck.CrcError) as e:
        ck.gather64_msg_n(0x40000, 0x50000, 1, 1, 0x20000, None, 0x30000)
    assert e.value.code < 0
    with pytest.raises(ck.CrcError) as e:
        ck.gather64_msg_n(0x40000, 0x50000, 1, 1, 0x20000, 0x60000, 0x30000)
    assert e.value.code < 0

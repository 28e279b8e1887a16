"""Overwrite + CRC delta and patch entry points without a GPU: exported,
declared, argument checks, and a loud failure where there is no device.
CPU only."""
import os
import subprocess

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = ["photon_crc32c_overwrite_batch_strided", "photon_crc32c_overwrite_batch_iov",
         "photon_crc64ecma_overwrite_batch_strided", "photon_crc64ecma_overwrite_batch_iov",
         "photon_crc32c_patch_n", "photon_crc64ecma_patch_n"]
WRAPPERS = ["overwrite_batch_strided", "overwrite_batch_iov", "overwrite_batch64_strided", "overwrite_batch64_iov",
            "patch_device", "patch64_device"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
WIDTHS = ["crc32c", "crc64ecma"]


def test_symbols_exported_and_declared():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    for n in NAMES + ["photon_crc_test_patch"]:
        assert n in exported, n
        assert getattr(L, n).argtypes, n  # prototype set by _native._declare


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


@pytest.mark.parametrize("w", WIDTHS)
def test_zero_counts_return_0(w):
    L = _native.lib()
    assert getattr(L, f"photon_{w}_overwrite_batch_strided")(None, 0, None, 0, 4096, 0, None, None) == 0
    assert getattr(L, f"photon_{w}_overwrite_batch_iov")(None, None, 0, None, None) == 0
    assert getattr(L, f"photon_{w}_patch_n")(None, None, 0, None, 0, None, None, None) == 0
    assert getattr(L, f"photon_{w}_patch_n")(None, None, 5, None, 0, None, None, None) == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_null_arguments_are_einval(w):
    L = _native.lib()
    S, D, O, I, T, G, C = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000  # never dereferenced

    def einval(rc):
        assert rc == -22
        assert b"null" in L.photon_crc_last_error()

    strided = lambda s, d, o: getattr(L, f"photon_{w}_overwrite_batch_strided")(s, 4096, d, 4096, 4096, 2, o, None)
    einval(strided(None, D, O))
    einval(strided(S, None, O))
    einval(strided(S, D, None))
    iov = lambda i, d, o: getattr(L, f"photon_{w}_overwrite_batch_iov")(i, d, 2, o, None)
    einval(iov(None, D, O))
    einval(iov(I, None, O))
    einval(iov(I, D, None))
    patch = getattr(L, f"photon_{w}_patch_n")
    einval(patch(None, T, 3, G, 2, C, C, None))  # null deltas, nwrites > 0
    einval(patch(O, None, 3, G, 2, C, C, None))  # null tails
    einval(patch(O, T, 3, G, 2, None, C, None))  # null input words
    einval(patch(O, T, 3, G, 2, C, None, None))  # null output words
    einval(patch(O, T, 3, None, 2, C, C, None))  # null tgt_start with ntgt != nwrites
    for fn in (ck.overwrite_batch_strided, ck.overwrite_batch64_strided):
        with pytest.raises(ck.CrcError) as e:
            fn(None, 4096, None, 4096, 4096, 4, None)
        assert e.value.code == -22


def test_replay_argument_checks():
    L = _native.lib()
    assert L.photon_crc_test_patch(0, None, None, 0, None, 0, None, None, 64) == 0
    assert L.photon_crc_test_patch(0, None, None, 0, None, 1, None, None, 64) == -22
    assert L.photon_crc_test_patch(1, 0x1000, 0x1000, 2, None, 3, 0x1000, 0x1000, 64) == -22
    assert L.photon_crc_test_patch(1, 0x1000, 0x1000, 2, None, 2, 0x1000, 0x1000, 0) == -22


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for strided, iov, patch in ((ck.overwrite_batch_strided, ck.overwrite_batch_iov, ck.patch_device),
                                (ck.overwrite_batch64_strided, ck.overwrite_batch64_iov, ck.patch64_device)):
        with pytest.raises(ck.CrcError) as e:
            strided(0x10000, 4096, 0x20000, 4096, 4096, 1, 0x30000)
        assert e.value.code < 0
        with pytest.raises(ck.CrcError) as e:
            iov(0x40000, 0x20000, 1, 0x30000)
        assert e.value.code < 0
        with pytest.raises(ck.CrcError) as e:
            patch(0x30000, 0x50000, 1, None, 1, 0x70000, 0x70000)
        assert e.value.code < 0

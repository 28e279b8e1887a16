"""Stripe parity + CRC and the expected-word entry points without a GPU:
exported, declared, argument checks, and a loud failure where there is no
device. CPU only."""
import ctypes
import os
import subprocess

import pytest

from photonlibos_amd import _native
from photonlibos_amd import checksum as ck

NAMES = ["photon_crc32c_xor_batch_strided", "photon_crc32c_xor_batch_ptr",
         "photon_crc64ecma_xor_batch_strided", "photon_crc64ecma_xor_batch_ptr",
         "photon_crc32c_xor_expect_n", "photon_crc64ecma_xor_expect_n"]
WRAPPERS = ["xor_batch_strided", "xor_batch_ptr", "xor_batch64_strided", "xor_batch64_ptr",
            "xor_expect_device", "xor_expect64_device"]
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))
WIDTHS = ["crc32c", "crc64ecma"]
S, D, O, P, V, C, G, N, W = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000


def test_symbols_exported_and_declared():
    out = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    L = _native.lib()
    for n in NAMES + ["photon_crc_test_xor_expect", "photon_crc_xor_geometry"]:
        assert n in exported, n
        assert getattr(L, n).argtypes, n  # prototype set by _native._declare


def test_wrappers_in_all():
    for n in WRAPPERS:
        assert n in ck.__all__ and callable(getattr(ck, n)), n


def test_geometry_query():
    L = _native.lib()
    f, u, u64, m = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert L.photon_crc_xor_geometry(ctypes.addressof(f), ctypes.addressof(u), ctypes.addressof(u64),
                                     ctypes.addressof(m)) == 0
    assert 1 <= f.value <= 8 and u.value in (1, 2, 4) and u64.value in (1, 2, 4) and m.value == 64
    assert L.photon_crc_xor_geometry(None, None, None, None) == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_zero_counts_return_0(w):
    L = _native.lib()
    # count == 0 comes first: nothing else is looked at, k outside 1..64 included
    assert getattr(L, f"photon_{w}_xor_batch_strided")(None, 0, 0, 4, None, 0, 4096, 0, 0, None, None, None) == 0
    assert getattr(L, f"photon_{w}_xor_batch_strided")(None, 0, 0, 0, None, 0, 4096, 0, 0, None, None, None) == 0
    assert getattr(L, f"photon_{w}_xor_batch_ptr")(None, 4, None, 0, 0, None, None, None) == 0
    assert getattr(L, f"photon_{w}_xor_batch_ptr")(None, 65, None, 0, 0, None, None, None) == 0
    assert getattr(L, f"photon_{w}_xor_expect_n")(None, 0, None, 4, None, 4096, 0, 0, None, None) == 0
    assert getattr(L, f"photon_{w}_xor_expect_n")(None, 7, None, 0, None, 4096, 0, 0, None, None) == 0


@pytest.mark.parametrize("w", WIDTHS)
def test_null_arguments_are_einval(w):
    L = _native.lib()  # the addresses are never dereferenced

    def einval(rc):
        assert rc == -22
        assert b"null" in L.photon_crc_last_error()

    strided = lambda s, d, o: getattr(L, f"photon_{w}_xor_batch_strided")(s, 16384, 4096, 4, d, 4096, 4096, 2, 0,
                                                                          None, o, None)
    einval(strided(None, D, O))
    einval(strided(S, None, O))
    einval(strided(S, D, None))
    ptr = lambda p, v, o: getattr(L, f"photon_{w}_xor_batch_ptr")(p, 4, v, 2, 0, None, o, None)
    einval(ptr(None, V, O))
    einval(ptr(P, None, O))
    einval(ptr(P, V, None))
    expect = getattr(L, f"photon_{w}_xor_expect_n")
    einval(expect(None, 8, None, 4, None, 4096, 2, 0, W, None))  # null words, ncrc > 0
    einval(expect(C, 8, None, 4, None, 4096, 2, 0, None, None))  # null output
    einval(expect(C, 8, G, 4, N, 0, 2, 0, None, None))
    for fn in (ck.xor_batch_strided, ck.xor_batch64_strided):
        with pytest.raises(ck.CrcError) as e:
            fn(None, 16384, 4096, 4, None, 4096, 4096, 4, None)
        assert e.value.code == -22
    for fn in (ck.xor_batch_ptr, ck.xor_batch64_ptr):
        with pytest.raises(ck.CrcError) as e:
            fn(None, 4, None, 4, None)
        assert e.value.code == -22


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("k", [0, 65, 1 << 31])
def test_source_count_outside_1_to_64_is_einval(w, k):
    L = _native.lib()
    assert getattr(L, f"photon_{w}_xor_batch_strided")(S, 16384, 4096, k, D, 4096, 4096, 2, 0, None, O, None) == -22
    assert b"1 to 64" in L.photon_crc_last_error()
    assert getattr(L, f"photon_{w}_xor_batch_ptr")(P, k, V, 2, 0, None, O, None) == -22
    assert b"1 to 64" in L.photon_crc_last_error()
    # the uniform-k form of the expected word takes the same range; with groups k is not looked at
    assert getattr(L, f"photon_{w}_xor_expect_n")(C, 8, None, k, None, 4096, 2, 0, W, None) == -22


def test_replay_argument_checks():
    L = _native.lib()
    assert L.photon_crc_test_xor_expect(0, None, 0, None, 4, None, 0, 0, 0, None) == 0      # count == 0
    assert L.photon_crc_test_xor_expect(1, None, 0, None, 4, None, 0, 1, 0, None) == -22    # null output
    assert b"null" in L.photon_crc_last_error()
    assert L.photon_crc_test_xor_expect(0, None, 3, None, 4, None, 0, 1, 0, W) == -22       # null words, ncrc > 0
    assert L.photon_crc_test_xor_expect(1, C, 3, None, 0, None, 0, 1, 0, W) == -22          # uniform k = 0
    assert L.photon_crc_test_xor_expect(1, C, 3, None, 65, None, 0, 1, 0, W) == -22
    # no words at all is an ordinary call: every group is empty
    want = (ctypes.c_uint32 * 2)(1, 1)
    assert L.photon_crc_test_xor_expect(0, None, 0, None, 4, None, 0, 2, 0, ctypes.addressof(want)) == 0
    assert list(want) == [0, 0]  # CRC-32C of no bytes from seed 0


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_calls_fail_loudly_without_gpu():
    # valid-looking arguments: no device, so a negative code and no compute (no CPU fallback)
    for strided, ptr, expect in ((ck.xor_batch_strided, ck.xor_batch_ptr, ck.xor_expect_device),
                                 (ck.xor_batch64_strided, ck.xor_batch64_ptr, ck.xor_expect64_device)):
        with pytest.raises(ck.CrcError) as e:
            strided(S, 16384, 4096, 4, D, 4096, 4096, 1, O)
        assert e.value.code < 0
        with pytest.raises(ck.CrcError) as e:
            ptr(P, 4, V, 1, O)
        assert e.value.code < 0
        with pytest.raises(ck.CrcError) as e:
            expect(C, 4, None, 4, None, 4096, 1, W)
        assert e.value.code < 0

"""tests/cpp/xor_expect_replay.cpp: the expected parity CRC from stored block
CRCs (photonlibos_amd/csrc/xor_expect.h) stand-alone on the host under
-fsanitize=address,undefined, over the fuzz of tests/test_xor_expect_abi.py
with the oracle's words (grouped and uniform k) and its large lengths. Every
array is heap memory of exactly its size, so an access outside an array shows.
Host code only: nothing is loaded into Python under a sanitizer. CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_xor_expect_abi import fuzz_cases, large_length_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words_of(crcs, start, k, lens, nbytes, seed, want):
    """One case of the file: crcs / seed / want are {c64: ...}."""
    count, ncrc = len(want[False]), len(crcs[False])
    arrays = [[count, ncrc, int(start is not None), k, int(lens is not None), nbytes, seed[False], seed[True]],
              crcs[False], crcs[True]]
    if start is not None:
        arrays.append(start)
    if lens is not None:
        arrays.append(lens)
    arrays += [want[False], want[True]]
    return np.concatenate([np.asarray(a, np.uint64) for a in arrays])


def all_cases(oracle):
    out = []
    for c in fuzz_cases(oracle):
        out.append(words_of(c.crcs, c.start, 0, c.lens, 0, c.seed, c.want))
        if c.k:
            out.append(words_of(c.crcs, None, c.k, c.lens, 0, c.seed, c.want))
    big = {c64: large_length_case(c64) for c64 in (False, True)}
    assert np.array_equal(big[False][1], big[True][1]) and np.array_equal(big[False][2], big[True][2])
    pick = lambda i: {c64: big[c64][i] for c64 in (False, True)}
    out.append(words_of(pick(0), big[False][1], 0, big[False][2], 0, pick(3), pick(4)))
    return out


def test_xor_expect_replay_under_asan(oracle, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    cases = all_cases(oracle)
    words = np.concatenate([np.array([len(cases)], np.uint64)] + cases)
    path = str(tmp_path / "cases.bin")
    words.astype("<u8").tofile(path)
    exe = str(tmp_path / "xor_expect_replay")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "photonlibos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "xor_expect_replay.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases" in r.stdout and " 0 mismatches" in r.stdout

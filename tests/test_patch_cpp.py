"""tests/cpp/patch_replay.cpp: the patch of stored CRCs
(photonlibos_amd/csrc/patch_crc.h) stand-alone on the host under
-fsanitize=address,undefined, over the fuzz of tests/test_patch_abi.py with
the oracle's words (per block, per object and one write per word) and its
large tails. Every array is heap memory of exactly its size, so an access
outside an array shows. Host code only: nothing is loaded into Python under a
sanitizer. CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_patch_abi import fuzz_cases, large_tail_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words_of(delta, tail, start, crc_in, want):
    """One case of the file: delta / crc_in / want are {c64: array}."""
    nwrites, ntgt = len(tail), len(want[False])
    arrays = [[nwrites, ntgt, int(start is not None)], delta[False], delta[True], tail]
    if start is not None:
        arrays.append(start)
    arrays += [crc_in[False], crc_in[True], want[False], want[True]]
    return np.concatenate([np.asarray(a, np.uint64) for a in arrays])


def all_cases(oracle):
    out = []
    for c in fuzz_cases(oracle):
        out.append(words_of(c.delta, c.block_tail, c.block_start, c.block_old, c.block_new))
        out.append(words_of(c.delta, c.object_tail, [0, len(c.pieces)], c.object_old, c.object_new))
        if c.pieces:
            idx = [k for k, _, _ in c.pieces]
            words = {c64: c.block_old[c64][idx] for c64 in (False, True)}
            out.append(words_of(c.delta, c.block_tail, None, words, c.alone))
    big = {c64: large_tail_case(c64) for c64 in (False, True)}
    assert np.array_equal(big[False][1], big[True][1]) and np.array_equal(big[False][2], big[True][2])
    pick = lambda k: {c64: big[c64][k] for c64 in (False, True)}
    out.append(words_of(pick(0), big[False][1], big[False][2], pick(3), pick(4)))
    return out


def test_patch_replay_under_asan(oracle, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    cases = all_cases(oracle)
    words = np.concatenate([np.array([len(cases)], np.uint64)] + cases)
    path = str(tmp_path / "cases.bin")
    words.astype("<u8").tofile(path)
    exe = str(tmp_path / "patch_replay")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "photonlibos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "patch_replay.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases" in r.stdout and " 0 mismatches" in r.stdout

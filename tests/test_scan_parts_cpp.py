"""tests/cpp/scan_parts_replay.cpp: the scan's three steps
(photonlibos_amd/csrc/scan_parts.h) stand-alone on the host under
-fsanitize=address,undefined, over the boundary fuzz of
tests/test_scan_parts_abi.py with the oracle's running words. Every array is
heap memory of exactly its size and the workspace is never cleared, so an
access outside an array or a workspace word read before it was written shows.
Host code only: nothing is loaded into Python under a sanitizer. CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_fold_parts_abi import SEEDS
from tests.test_scan_parts_abi import fuzz_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_words(i, case):
    per_object = i % 2
    seed = {c64: SEEDS[c64][(i // 2) % 2] for c64 in (False, True)}
    want = [case.want[c64] if per_object else case.want0[c64, seed[c64]] for c64 in (False, True)]
    arrays = [[case.nobj, case.nparts, per_object, seed[False], seed[True]], case.start, case.len, case.crc[False],
              case.crc[True], case.seeds[False], case.seeds[True], want[0], want[1], case.end]
    return np.concatenate([np.asarray(a, np.uint64) for a in arrays])


def test_scan_replay_under_asan(oracle, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    cases = fuzz_cases(oracle)
    words = np.concatenate([np.array([len(cases)], np.uint64)] + [case_words(i, c) for i, c in enumerate(cases)])
    path = str(tmp_path / "cases.bin")
    words.astype("<u8").tofile(path)
    exe = str(tmp_path / "scan_parts_replay")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "photonlibos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "scan_parts_replay.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(cases)} cases" in r.stdout and " 0 mismatches" in r.stdout

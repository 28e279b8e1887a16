"""tests/cpp/parts_packed_search.cpp: the task-to-part search and the plan
replay of the packed parts calls (photonlibos_amd/csrc/parts_packed_plan.h,
DESIGN.md §4.12) stand-alone on the host under -fsanitize=address,undefined:
first[] arrays with runs of zero-count parts, a single part, counts of 1 only
and one count of 2^33, and the four plan steps over mixed parts on heap arrays
of exactly their size with a workspace that is never cleared. Host code only:
nothing is loaded into Python under a sanitizer. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_search_and_replay_under_asan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "parts_packed_search")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "photonlibos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "parts_packed_search.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout and not r.stdout.startswith("0 tasks")

"""tests/cpp/iov_walk_replay.cpp: the two-cursor walk of copy + CRC between
iovectors (photonlibos_amd/csrc/iov_walk.h, photon_crc*_copy_msg_iov_n and its
_seg, _seg2 and _window forms) stand-alone on the host, once plain and once
under -fsanitize=address,undefined. The program makes its own cases and checks
them against a direct model of its own (see its head comment); this side builds
it, runs it, and knows how many cases there have to be. Host code only: nothing
is loaded into Python under a sanitizer. CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photonlibos_amd", "csrc")

# The program's cases: every pair of sides out of all tuples of 0 to 3 lengths
# from 5 values and all tuples of 4 lengths from 3 values, each with 6 caps.
SIDES = sum(5 ** count for count in range(4)) + 3 ** 4
CASES = SIDES * SIDES * 6

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "sanitized"])
def test_iov_walk_replay(flags, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "iov_walk_replay")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", *flags, "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "iov_walk_replay.cpp"), os.path.join(CSRC, "crc32c_cpu.cpp"),
                    os.path.join(CSRC, "crc64_cpu.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"iov_walk_replay: {CASES} cases, 0 mismatches"

"""tests/cpp/window_finish_replay.cpp: the finish of the windowed copy + CRC
(photonlibos_amd/csrc/window_finish.h, photon_crc*_copy_msg_iov_window_n)
stand-alone on the host, once as it is and once under
-fsanitize=address,undefined. The program makes its own cases, models the walk
with the CPU CRC engines (crc32c_cpu.cpp, crc64_cpu.cpp, linked in) and
compares window_replay_msg's per-segment CRCs, window CRC and k with what
those engines compute directly. Host code only: nothing is loaded into Python
under a sanitizer. CPU only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photonlibos_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "window_finish_replay.cpp"), os.path.join(CSRC, "crc32c_cpu.cpp"),
           os.path.join(CSRC, "crc64_cpu.cpp")]
# cases(): 8 source layouts x (10 + its segment count) skips x 11 sizes x 6 destination layouts, then 5 x 3 x 6
NCASES = sum((10 + nseg) * 11 * 6 for nseg in (3, 4, 4, 4, 6, 1, 0, 2)) + 5 * 3 * 6
RUNS = 3 * 3 * 2  # step widths x call modes x CRCs


def _build_and_run(tmp_path, name, flags):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    subprocess.run([gxx, "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"window_finish_replay: (\d+) cases, (\d+) runs, (\d+) mismatches", r.stdout)
    assert m, r.stdout + r.stderr
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (NCASES, RUNS, 0), r.stdout + r.stderr


def test_window_replay(tmp_path):
    _build_and_run(tmp_path, "window_finish_replay", ["-O2"])


def test_window_replay_under_asan(tmp_path):
    _build_and_run(tmp_path, "window_finish_replay_san",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])

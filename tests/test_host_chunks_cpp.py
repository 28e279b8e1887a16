"""tests/cpp/host_chunks_replay.cpp: the host-side chunking of the host-memory
pipeline and of photon_crc32c_file_strided (photonlibos_amd/csrc/host_chunks.h)
stand-alone on the host: once as it is, once under
-fsanitize=address,undefined and once under -fsanitize=thread. The program
sweeps the staging plan, the file chunk geometry and the piece cut of the
parallel read, and runs the two-buffer reader / consumer loop on real temporary
files (end of file at every edge, slow consumer, slow reader, failing consumer,
read errors, two pipelines at once) with the CPU CRC engine (crc32c_cpu.cpp,
linked in) as the consumer, every record against a plain read of the file.
Host code only: nothing is loaded into Python under a sanitizer. CPU only."""
import os
import platform
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "photonlibos_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "host_chunks_replay.cpp"), os.path.join(CSRC, "crc32c_cpu.cpp")]
# check_stage_plans(): 19 sizes x 6 spans x (6 multiples x 3 - 1) counts
PLANS = 19 * 6 * 17
# check_file_geometry(): 3 chunk spans x 5 offsets x 7 strides x 4 sizes x 12 counts, less the empty counts
# (1 * per - 1 == 0 where a chunk holds one record: 4 of the 7 strides of every span, and stride 4096 at span 4096)
GEOMS = 3 * 5 * 7 * 4 * 12 - (3 * 4 + 1) * 5 * 4
# check_piece_cuts(): (every 4 KiB multiple up to 2 MiB + 4 large spans) x 4 tails
CUTS = (512 + 4) * 4
# check_file_reads(): 2 chunk spans x 2 shapes x cases x 3 paces, + 1 O_DIRECT: 5 cases each, the rounded tail for
# the ragged shape, the earlier piece for the parallel cut
READS = ((5 + 5 + 1) + (5 + 1 + 5 + 1 + 1)) * 3 + 1
# check_pipelines(): 5 chunk counts x 2 tails x 2 shapes x 3 paces, 3 x 3 failing consumers, 3 read errors, 3 x 2 at once
PIPES = 5 * 2 * 2 * 3 + 3 * 3 + 3 + 3 * 2
TSAN_NO_START = "ThreadSanitizer: unexpected memory mapping"


def _build_and_run(tmp_path, name, flags):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    subprocess.run([gxx, "-std=c++17", *flags, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *SOURCES,
                    "-lpthread", "-o", exe], check=True, timeout=600)
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and TSAN_NO_START in r.stderr:
        # ThreadSanitizer's runtime ended before main: with many bits of address-space randomisation the kernel
        # can place the program outside the ranges the runtime knows. Run it again with randomisation off.
        setarch = shutil.which("setarch")
        if setarch:
            r = subprocess.run([setarch, platform.machine(), "-R", exe, str(tmp_path)], capture_output=True,
                               text=True, timeout=600)
        if r.returncode != 0 and (TSAN_NO_START in r.stderr or "setarch:" in r.stderr) and not r.stdout:
            pytest.skip("ThreadSanitizer's runtime cannot start here: " + r.stderr.strip()[:200])
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"host_chunks_replay: (\d+) stage plans, (\d+) file geometries, (\d+) piece cuts, (\d+) file reads, "
                  r"(\d+) pipelines, o_direct (ok|refused), (\d+) mismatches", r.stdout)
    assert m, r.stdout + r.stderr
    got = tuple(int(m.group(k)) for k in (1, 2, 3, 4, 5, 7))
    assert got == (PLANS, GEOMS, CUTS, READS, PIPES, 0), r.stdout + r.stderr


def test_host_chunks_replay(tmp_path):
    _build_and_run(tmp_path, "host_chunks_replay", ["-O2"])


def test_host_chunks_replay_under_asan(tmp_path):
    _build_and_run(tmp_path, "host_chunks_replay_asan",
                   ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_host_chunks_replay_under_tsan(tmp_path):
    _build_and_run(tmp_path, "host_chunks_replay_tsan", ["-O1", "-g", "-fsanitize=thread"])


def test_knob_ranges():
    """photon_crc_set_host_stage_bytes / photon_crc_set_file_chunk_bytes (tuning.h): declared in the header, the
    valid values taken, every other value -EINVAL with a message, 0 restores the default."""
    from photonlibos_amd import checksum as ck
    header = open(os.path.join(ROOT, "include", "photon_crc", "tuning.h")).read()
    assert "int photon_crc_set_host_stage_bytes(uint64_t bytes);" in header
    assert "int photon_crc_set_file_chunk_bytes(uint64_t bytes);" in header
    try:
        for ok in (0, 64 << 10, (64 << 10) + 256, 1 << 20, 256 << 20):
            ck.set_host_stage_bytes(ok)
        for bad in (1, 256, (64 << 10) - 256, (64 << 10) + 1, (1 << 20) + 255, (256 << 20) + 256, 1 << 63):
            with pytest.raises(ck.CrcError) as e:
                ck.set_host_stage_bytes(bad)
            assert e.value.code == -22 and "host stage bytes" in str(e.value), bad
        for ok in (0, 4096, 64 << 10, 256 << 10, 64 << 20):
            ck.set_file_chunk_bytes(ok)
        for bad in (1, 4095, 4097, 2048, (64 << 20) + 4096, 1 << 63):
            with pytest.raises(ck.CrcError) as e:
                ck.set_file_chunk_bytes(bad)
            assert e.value.code == -22 and "file chunk bytes" in str(e.value), bad
    finally:
        ck.set_host_stage_bytes(0)
        ck.set_file_chunk_bytes(0)

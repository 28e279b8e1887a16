"""tests/cpp/seg_unscan_replay.cpp: the un-scan of the two-sided copy + CRC
(photonlibos_amd/csrc/seg_unscan.h, photon_crc*_copy_msg_iov_seg2_n)
stand-alone on the host under -fsanitize=address,undefined. This side makes
the inputs: messages as lists of segment lengths, a host model of the walk
that says which entries receive a running value (`stored_entries`, written
here from the walk's definition; the pieces themselves are `_walk`'s of
tests/test_gpu_copy_iov_seg.py), the oracle's running values in those entries
and a canary in every other one, and the oracle's per-segment CRCs over the
landed bytes as the expected result. Every array in the program is heap memory
of exactly its size. Host code only: nothing is loaded into Python under a
sanitizer. CPU only."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from photonlibos_amd import datagen
from tests.test_gpu_copy_iov_seg import _walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNLIMITED = (1 << 64) - 1
CANARY = {False: 0xA5A5A5A5, True: 0xA5A5A5A5A5A5A5A5}
STEP_COUNTS = (0, 1, 2, 63, 64, 65, 129)  # the un-scan step's width and its neighbours


def stored_entries(src_lens, dst_lens, size):
    """Where the walk stores its running value: ([(entry, stream position)] for
    the source side, the same for the destination side), in the order of the
    stores. A side's entry is stored when its cursor leaves the segment (its
    last byte consumed and the cap not yet reached) and, after the walk, for
    the segment the cursor still stands in. Position = the bytes copied when
    the store happens."""
    s_st, d_st = [], []
    si = di = so = do = pos = 0
    left = UNLIMITED if size is None else size
    while left and si < len(src_lens) and di < len(dst_lens):
        n = min(left, src_lens[si] - so, dst_lens[di] - do)
        left, so, do, pos = left - n, so + n, do + n, pos + n
        if not left:
            break
        if so == src_lens[si]:
            s_st.append((si, pos))
            si, so = si + 1, 0
        if do == dst_lens[di]:
            d_st.append((di, pos))
            di, do = di + 1, 0
    if si < len(src_lens):
        s_st.append((si, pos))
    if di < len(dst_lens):
        d_st.append((di, pos))
    return s_st, d_st


def landed_bytes(src_lens, dst_lens, size):
    """Per side, the bytes of every segment that land (from `_walk`'s pieces
    over a stream laid out from position 0 on both sides)."""
    def at(lens):
        out, p = [], 0
        for n in lens:
            out.append((p, n))
            p += n
        return out
    ls, ld = [0] * len(src_lens), [0] * len(dst_lens)
    for _, _, n, si, di in _walk(at(src_lens), at(dst_lens), size):
        ls[si] += n
        ld[di] += n
    return ls, ld


def test_models():
    # no GPU, no compiler: the two models on cases worked out by hand
    assert stored_entries([10], [4, 6], None) == ([(0, 10)], [(0, 4), (1, 10)])
    assert stored_entries([4, 6], [4, 6, 5], None) == ([(0, 4), (1, 10)], [(0, 4), (1, 10), (2, 10)])
    assert stored_entries([4, 6], [10], 4) == ([(0, 4)], [(0, 4)])          # the cap on a source boundary
    assert stored_entries([0, 0, 5], [5], None) == ([(0, 0), (1, 0), (2, 5)], [(0, 5)])
    assert stored_entries([5], [], None) == ([(0, 0)], []) and stored_entries([5, 5], [9], 0) == ([(0, 0)], [(0, 0)])
    assert landed_bytes([4, 6, 3], [7], None) == ([4, 3, 0], [7])
    assert landed_bytes([10], [4, 6, 9], 7) == ([7], [4, 3, 0])


def message_cases():
    """[(source lengths, destination lengths, cap or None)]."""
    rnd = random.Random(0x5E62)
    cases = []
    edges = tuple(range(0, 201, 20))
    cases += [([a, 200 - a], [b, 200 - b], None) for a in edges for b in edges]   # boundary order
    assert len(cases) == 121
    # caps: inside a segment, on a source boundary (100, 300), on a destination boundary (150, 400), beyond
    for size in (0, 1, 99, 100, 101, 120, 150, 151, 299, 300, 400, 599, 600, 601, 800, 10 ** 6, UNLIMITED):
        cases.append(([100, 200, 300], [150, 250, 400], size))
    for size in (99, 100, 101, 299, 300, 301):                                    # on a boundary of both sides
        cases.append(([100, 200, 50], [100, 200, 50], size))
    # a shorter source, a shorter destination, empty sides, size 0
    cases += [([300, 500, 77, 9], [100, 250, 450], None), ([300, 500, 77], [700], None), ([50, 30, 9], [50, 30], None),
              ([100, 64], [50, 1000, 30, 40], None), ([97], [30, 30, 30, 30, 30], None), ([50, 30], [50, 30, 9], None),
              ([], [100], None), ([100], [], None), ([], [], None), ([], [], 0), ([5, 6], [7, 8], 0)]
    # zero-length runs: at the start, in the middle, coinciding on both sides, trailing, everywhere, alone
    a, b = 50, 70
    cases += [([0, 0, 0, a, b], [a + b], None), ([a, b], [0, 0, a + b], None),
              ([a, b, 0, 0], [a, b], None), ([a, b], [a, b, 0, 0, 0], None),
              ([a, 0, 0, b], [a + b], None), ([a, b], [a - 7, 0, 0, 0, b + 7], None),
              ([a, 0, 0, b], [a, 0, 0, 0, b], None), ([0, a, 0, b, 0], [0, a, 0, b, 0], None),
              ([0, 0], [10], None), ([a], [0, 0, 0], None), ([a, 0, 0, b], [a, 0, 0, 0, b], a),
              ([a, b, 0, 0, 9], [a, b, 0, 4], None)]
    # the step's width and its neighbours, the two sides' counts different, with and without a cap
    for i, ns in enumerate(STEP_COUNTS):
        for nd in (STEP_COUNTS[(i + 3) % 7], STEP_COUNTS[(i + 5) % 7], ns):
            sl = [rnd.choice((0, 1, 2, 3, 5, 8)) for _ in range(ns)]
            dl = [rnd.choice((0, 1, 2, 3, 5, 8)) for _ in range(nd)]
            total = min(sum(sl), sum(dl))
            cases.append((sl, dl, None))
            cases.append((sl, dl, rnd.randrange(0, total + 2)))
            cases.append(([4] * ns, [4] * nd, None))   # every boundary of the shorter side coincides
    # fuzz
    for _ in range(150):
        sl = [rnd.choice((0, 0, 1, 7, 16, 33, 100, 257)) for _ in range(rnd.randrange(0, 9))]
        dl = [rnd.choice((0, 0, 1, 7, 16, 33, 100, 257)) for _ in range(rnd.randrange(0, 9))]
        total = min(sum(sl), sum(dl))
        r = rnd.random()
        cases.append((sl, dl, None if r < 0.4 else rnd.randrange(0, total + 2) if r < 0.8 else total + 1000))
    assert len(cases) == 121 + 17 + 6 + 11 + 12 + 63 + 150
    return cases


def call_words(oracle, cases, seed0, seeds, rnd):
    """One call of the program's input: every case a message. seed0: (CRC-32C,
    CRC-64) seeds for all, or seeds: per message (c32, c64)."""
    crcs = {False: oracle.crc32c, True: oracle.crc64ecma}
    src_start, dst_start, src_len, dst_len, size = [0], [0], [], [], []
    run = {(side, w): [] for side in "sd" for w in (False, True)}
    want = {(side, w): [] for side in "sd" for w in (False, True)}
    for m, (sl, dl, cap) in enumerate(cases):
        k = min(sum(sl), sum(dl), UNLIMITED if cap is None else cap)
        data = datagen.stream_bytes(rnd.getrandbits(32), max(k, 1))[:k].tobytes()
        s_st, d_st = stored_entries(sl, dl, cap)
        assert all(pos <= k for _, pos in s_st + d_st)
        ls, ld = landed_bytes(sl, dl, cap)
        assert sum(ls) == sum(ld) == k
        for w in (False, True):
            seed = (seeds[m] if seeds else seed0)[w]
            for side, lens, st, landed in (("s", sl, s_st, ls), ("d", dl, d_st, ld)):
                r = [CANARY[w]] * len(lens)
                for j, pos in st:
                    r[j] = crcs[w](data[:pos], seed)
                run[side, w] += r
                p = 0
                for n in landed:
                    want[side, w].append(crcs[w](data[p:p + n], 0))
                    p += n
        src_len += sl
        dst_len += dl
        src_start.append(len(src_len))
        dst_start.append(len(dst_len))
        size.append(UNLIMITED if cap is None else cap)
    nmsg = len(cases)
    head = [nmsg, len(src_len), len(dst_len), 1, 1 if seeds else 0] + list(seed0 or (0, 0))
    arrays = [head, src_start, dst_start, src_len, dst_len, size,
              [s[0] for s in seeds] if seeds else [0] * nmsg, [s[1] for s in seeds] if seeds else [0] * nmsg,
              run["s", False], run["s", True], run["d", False], run["d", True],
              want["s", False], want["s", True], want["d", False], want["d", True]]
    return np.concatenate([np.asarray(a, np.uint64) for a in arrays])


def test_unscan_replay_under_asan(oracle, tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    rnd = random.Random(0x5EED2)
    cases = message_cases()
    per_msg = [(0, 0) if m % 3 == 0 else (rnd.getrandbits(32), rnd.getrandbits(64)) for m in range(len(cases))]
    calls = [call_words(oracle, cases, (0, 0), None, rnd),
             call_words(oracle, cases, (0xFEEDC0DE, 0xFEEDC0DE5EED0001), None, rnd),
             call_words(oracle, cases, None, per_msg, rnd)]
    # no size array: the uncapped cases alone
    uncapped = call_words(oracle, [c for c in cases if c[2] is None], (0x12345678, 0x123456789ABCDEF0), None, rnd)
    uncapped[3] = 0
    calls.append(uncapped)
    ncases = 3 * len(cases) + sum(1 for c in cases if c[2] is None)
    words = np.concatenate([np.array([len(calls)], np.uint64)] + calls)
    path = str(tmp_path / "cases.bin")
    words.astype("<u8").tofile(path)
    exe = str(tmp_path / "seg_unscan_replay")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "photonlibos_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "seg_unscan_replay.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{ncases} cases" in r.stdout and " 0 mismatches" in r.stdout

#!/usr/bin/env python3
"""A/B of the ranged read from checksummed blocks by the
method of §4.3: one process, device to device, window source and destination
co-aligned, 5 alternations of 20 timed launches after 5 warm-ups per arm, HIP
events on the launch stream, the same lane-group size for every arm.

Arms:
  a  the unfused pair on one stream, both existing calls: batch_iov over the
     blocks (the CRCs to verify), then copy_msg_iov_n over window descriptors
     offset on the host beforehand (the bytes and the window's CRC). The window
     is read twice.
  b  the fused call, copy_msg_iov_window_n: every block read once.

Shapes:
  P  pages: 64 Ki messages, one 64 KiB block each, a 4 KiB window at a random
     4 KiB multiple.
  R  ranges: 4 Ki messages, 17 blocks of 64 KiB each, a 1 MiB window that
     starts at a random 4 KiB multiple strictly inside block 0 (and so ends
     inside block 16). Per message the pair moves 3.0625 MiB, the fused call
     2.0625 MiB.

Before anything is timed the fused call's results are compared with the host
oracle on --check sampled messages (block CRCs, window CRC, copied) and the
landed bytes of every message with the source; the pair's results are compared
with the fused call's.

Writes one JSON line per shape and CRC; --out appends them to a file
(profiles/window_crc_ab.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from photonlibos_amd import checksum as ck  # noqa: E402
from tests import _oracle as oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="P,R")
ap.add_argument("--crc", default="crc32c,crc64")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--check", type=int, default=64, help="messages whose results are compared with the host oracle")
ap.add_argument("--scale", type=int, default=1, help="divide the message counts by this (smoke runs)")
ap.add_argument("--lanes", type=int, default=0, help="lanes per buffer for every arm (0: the library's for a block)")
ap.add_argument("--out")
args = ap.parse_args()

BLOCK, PAGE = 65536, 4096
# name: (messages, blocks per message, window bytes)
SHAPES = {"P": (1 << 16, 1, PAGE), "R": (1 << 12, 17, 1 << 20)}
SEED = 0xDEADBEEF
st = torch.cuda.Stream()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def bench(shape, c64):
    nmsg, nblk, win = SHAPES[shape]
    nmsg //= args.scale
    dt = torch.int64 if c64 else torch.int32
    npdt = np.uint64 if c64 else np.uint32
    crc = oracle.crc64ecma if c64 else oracle.crc32c
    batch_iov = ck.batch64_iov if c64 else ck.batch_iov
    copy_msg = ck.copy_msg64_iov_n if c64 else ck.copy_msg_iov_n
    window = ck.copy_msg64_iov_window_n if c64 else ck.copy_msg_iov_window_n
    lanes = args.lanes or ck.lanes_for(BLOCK)
    ck.set_lanes_per_buffer(lanes)

    span = nblk * BLOCK  # a message's blocks lie back to back
    src = torch.empty(span * nmsg, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, BLOCK, BLOCK, nblk * nmsg, 0x5EED0001)
    dst = torch.zeros(win * nmsg, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(7)
    if shape == "P":
        skip = rng.integers(0, BLOCK // PAGE, nmsg).astype(np.uint64) * PAGE
    else:
        skip = rng.integers(1, BLOCK // PAGE, nmsg).astype(np.uint64) * PAGE  # strictly inside block 0
    assert np.all(skip + win <= span) and np.all(skip % 16 == 0)
    sbase, dbase = src.data_ptr(), dst.data_ptr()
    assert sbase % 16 == 0 and dbase % 16 == 0

    m = np.arange(nmsg, dtype=np.uint64)
    blk = np.arange(nblk * nmsg, dtype=np.uint64)
    blocks = dev(np.stack([sbase + blk * BLOCK, np.full_like(blk, BLOCK)], 1))
    blk_start = dev(np.arange(nmsg + 1, dtype=np.uint64) * nblk)
    dsts = dev(np.stack([dbase + m * win, np.full_like(m, win)], 1))
    dst_start = dev(np.arange(nmsg + 1, dtype=np.uint64))
    d_skip = dev(skip)
    d_size = dev(np.full(nmsg, win, np.uint64))
    # the pair's window descriptors: the blocks' ranges cut to the window, on the host
    if shape == "P":
        wsrc = dev(np.stack([sbase + m * span + skip, np.full_like(m, win)], 1))
        wsrc_start, nwsrc = dst_start, nmsg
    else:
        rows = np.empty((nmsg, nblk, 2), np.uint64)
        rows[:, :, 0] = (sbase + blk * BLOCK).reshape(nmsg, nblk)
        rows[:, :, 1] = BLOCK
        rows[:, 0, 0] += skip
        rows[:, 0, 1] -= skip
        rows[:, nblk - 1, 1] = skip
        assert np.all(rows[:, :, 1].sum(1) == win)
        wsrc, wsrc_start, nwsrc = dev(rows.reshape(-1, 2)), blk_start, nblk * nmsg

    seg = torch.zeros(nblk * nmsg, dtype=dt, device="cuda")
    out = torch.zeros(nmsg, dtype=dt, device="cuda")
    copied = torch.zeros(nmsg, dtype=torch.int64, device="cuda")
    seg2 = torch.zeros(nblk * nmsg, dtype=dt, device="cuda")
    out2 = torch.zeros(nmsg, dtype=dt, device="cuda")
    work = torch.empty(ck.window_work_bytes(nmsg), dtype=torch.uint8, device="cuda")

    def pair():
        batch_iov(blocks, nblk * nmsg, seg2, stream=st)
        copy_msg(wsrc, wsrc_start, nwsrc, dsts, dst_start, nmsg, nmsg, out2, seed=SEED, stream=st)

    def fused():
        window(blocks, blk_start, nblk * nmsg, dsts, dst_start, nmsg, nmsg, seg, out, work, skip=d_skip, size=d_size,
               seed=SEED, copied=copied, stream=st)

    arms = {"a_pair": pair, "b_fused": fused}

    # correctness before anything is timed
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        fused()
    torch.cuda.synchronize()
    sample = np.unique(np.concatenate([np.arange(min(nmsg, 4)), np.arange(max(nmsg - 4, 0), nmsg),
                                       rng.integers(0, nmsg, args.check)]))
    g_seg = seg.cpu().numpy().view(npdt).reshape(nmsg, nblk)
    g_out = out.cpu().numpy().view(npdt)
    assert np.all(copied.cpu().numpy() == win), f"{shape}: copied"
    for k in sample:
        k = int(k)
        host = src[k * span:(k + 1) * span].cpu().numpy()
        for b in range(nblk):
            assert int(g_seg[k, b]) == crc(host[b * BLOCK:(b + 1) * BLOCK].tobytes(), 0), (shape, "block crc", k, b)
        a = int(skip[k])
        assert int(g_out[k]) == crc(host[a:a + win].tobytes(), SEED), (shape, "window crc", k)
    if shape == "P":
        page = torch.from_numpy((skip // PAGE).astype(np.int64)).cuda()
        landed = src.view(nmsg, BLOCK // PAGE, PAGE)[torch.arange(nmsg, device="cuda"), page]
        assert torch.equal(dst.view(nmsg, PAGE), landed), f"{shape}: landed bytes differ from the source"
    else:
        for k in range(nmsg):
            a = int(skip[k])
            assert torch.equal(dst[k * win:(k + 1) * win], src[k * span + a:k * span + a + win]), (shape, "landed", k)
    dst.zero_()
    with torch.cuda.stream(st):
        pair()
    torch.cuda.synchronize()
    assert torch.equal(seg2, seg) and torch.equal(out2, out), f"{shape}: the pair and the fused call disagree"

    means = {k: [] for k in arms}
    times = {k: [] for k in arms}
    for r in range(args.rounds):
        for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            fn = arms[name]
            for _ in range(args.warmup):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record(st)
            for k in range(args.reps):
                fn()
                ev[k + 1].record(st)
            torch.cuda.synchronize()
            t = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.reps)]
            times[name] += t
            means[name].append(float(np.mean(t)))
    res = {"bench": "window_crc", "shape": shape, "crc": "crc64ecma" if c64 else "crc32c", "nmsg": nmsg,
           "blocks_per_msg": nblk, "block": BLOCK, "window": win, "lanes": lanes, "rounds": args.rounds,
           "reps": args.reps, "warmup": args.warmup, "messages_checked": int(sample.size),
           "MiB_per_msg": {"a_pair": (nblk * BLOCK + 2 * win) / 2.0**20, "b_fused": (nblk * BLOCK + win) / 2.0**20}}
    for name in arms:
        ms = np.asarray(times[name])
        moved = res["MiB_per_msg"][name] * nmsg / 1024.0
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "moved_GiBps_mean": round(moved / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(x, 5) for x in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    res["ratio_b_over_a"] = round(res["b_fused"]["ms_mean"] / res["a_pair"]["ms_mean"], 4)
    res["b_faster_than_a"] = bool(res["b_fused"]["ms_mean"] < res["a_pair"]["ms_mean"])
    # the bound of shape P: not slower than the pair by more than the pair's own spread
    res["b_slower_than_a_beyond_a_spread"] = bool(res["b_fused"]["ms_mean"] - res["a_pair"]["ms_mean"]
                                                  > res["a_pair"]["spread_ms"])
    ck.set_lanes_per_buffer(0)
    return res


for shape in args.shapes.split(","):
    for name in args.crc.split(","):
        line = json.dumps(bench(shape, name.startswith("crc64")))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        torch.cuda.empty_cache()

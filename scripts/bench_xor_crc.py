#!/usr/bin/env python3
"""A/B of the stripe parity + CRC call by the method of §4.3
/ §4.14: one process, one device, device to device, sources and parity
co-aligned, 5 alternations of 20 timed launches after 5 warm-ups per arm, HIP
events on the launch stream, the same lanes in every arm, random non-zero data.

Arms:
  a  what a caller does without the call: a chain of k-1
     torch.bitwise_xor(..., out=) launches into the parity, then batch_strided
     over the parity (3(k-1) + 1 block-sized transfers per stripe).
  b  the fused call, xor_batch_strided (k + 1 transfers per stripe).
  c  for scale only: the read-only stream kernel over the same source bytes.

Shapes: k+1 stripes of 4 KiB and of 64 KiB blocks for k = 4 and 8, about 4 GiB
of sources each, and the in-place small write P ^= D_old ^ D_new (k = 3, the
parity its own first source) on 4 KiB pages. Before anything is timed, the
parities and CRCs of --check sampled stripes are compared with the host oracle
over host copies of their blocks.

Writes one JSON line per shape and CRC; --out appends them to a file
(profiles/xor_crc_ab.jsonl)."""
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
ap.add_argument("--shapes", default="4+1x4k,8+1x4k,4+1x64k,8+1x64k,small4k")
ap.add_argument("--crc", default="crc32c,crc64")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--check", type=int, default=512, help="stripes compared with the host oracle")
ap.add_argument("--scale", type=int, default=1, help="divide the counts by this (smoke runs)")
ap.add_argument("--lanes", type=int, default=0, help="lanes per buffer for every arm (0: the library's for the size)")
ap.add_argument("--out")
args = ap.parse_args()

GIB4 = 1 << 32
# name: (k, block bytes, stripes, in place)
SHAPES = {"4+1x4k": (4, 4096, GIB4 // (4 * 4096), False), "8+1x4k": (8, 4096, GIB4 // (8 * 4096), False),
          "4+1x64k": (4, 65536, GIB4 // (4 * 65536), False), "8+1x64k": (8, 65536, GIB4 // (8 * 65536), False),
          "small4k": (3, 4096, 1 << 18, True)}
SEED = 0xDEADBEEF
st = torch.cuda.Stream()


def bench(shape, c64):
    k, bs, count, in_place = SHAPES[shape]
    count //= args.scale
    dt = torch.int64 if c64 else torch.int32
    npdt = np.uint64 if c64 else np.uint32
    crc = oracle.crc64ecma if c64 else oracle.crc32c
    batch_strided = ck.batch64_strided if c64 else ck.batch_strided
    xor_strided = ck.xor_batch64_strided if c64 else ck.xor_batch_strided
    xor_ptr = ck.xor_batch64_ptr if c64 else ck.xor_batch_ptr
    lanes = args.lanes or ck.lanes_for(bs)
    ck.set_lanes_per_buffer(lanes)

    nsrc = k - 1 if in_place else k            # blocks per stripe that are not the parity
    src = torch.empty(count * nsrc * bs, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, bs, bs, count * nsrc, 0x5EED0001)
    parity = torch.empty(count * bs, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(parity, bs, bs, count, 0x0A7170001)
    out = torch.zeros(count, dtype=dt, device="cuda")
    sink = torch.zeros(1 << 22, dtype=torch.int32, device="cuda")
    w = src.view(torch.int64).view(count, nsrc, bs // 8)     # the caller's view for the XOR chain
    pw = parity.view(torch.int64).view(count, bs // 8)
    if in_place:  # the _ptr form: source 0 is the parity itself
        at = torch.arange(count, dtype=torch.int64, device="cuda")
        ptrs = torch.stack([parity.data_ptr() + at * bs] + [src.data_ptr() + (at * nsrc + i) * bs for i in range(nsrc)],
                           dim=1).contiguous()
        iov = torch.stack([parity.data_ptr() + at * bs, torch.full_like(at, bs)], dim=1).contiguous()

    def chain():
        with torch.cuda.stream(st):
            if in_place:
                for i in range(nsrc):
                    torch.bitwise_xor(pw, w[:, i], out=pw)
            else:
                torch.bitwise_xor(w[:, 0], w[:, 1], out=pw) if k > 1 else pw.copy_(w[:, 0])
                for i in range(2, k):
                    torch.bitwise_xor(pw, w[:, i], out=pw)
        batch_strided(parity, bs, bs, count, out, seed=SEED, stream=st)

    def fused():
        if in_place:
            xor_ptr(ptrs, k, iov, count, out, seed=SEED, stream=st)
        else:
            xor_strided(src, k * bs, bs, k, parity, bs, bs, count, out, seed=SEED, stream=st)

    def stream_read():
        ck.read_stream(src.data_ptr(), src.numel(), sink, sink.numel(), stream=st)

    arms = {"a_chain": chain, "b_fused": fused, "c_read": stream_read}

    # correctness before anything is timed: sampled stripes against the host oracle
    torch.cuda.synchronize()
    sample = np.unique(np.concatenate([np.arange(min(count, 32)), np.arange(max(count - 32, 0), count),
                                       np.random.default_rng(1).integers(0, count, args.check)]))
    idx = torch.from_numpy(sample).cuda()
    blocks = src.view(count, nsrc, bs)[idx].cpu().numpy()
    want_p = np.bitwise_xor.reduce(blocks, axis=1)
    if in_place:
        want_p ^= parity.view(count, bs)[idx].cpu().numpy()
    assert all(b.any() for b in want_p), "a zero parity block in the sample"
    fused()
    torch.cuda.synchronize()
    got_p = parity.view(count, bs)[idx].cpu().numpy()
    assert np.array_equal(got_p, want_p), f"{shape}: sampled parities differ from the host's XOR"
    got = out.cpu().numpy().view(npdt)[sample]
    want = np.array([crc(p, SEED) for p in want_p], npdt)
    assert np.array_equal(got, want), f"{shape}: {np.count_nonzero(got != want)} of {sample.size} sampled CRCs differ"
    if not in_place:  # and arm (a) lands the same words
        out.zero_()
        chain()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(npdt)[sample], want), f"{shape}: arm (a) differs"

    means = {name: [] for name in arms}
    times = {name: [] for name in arms}
    for r in range(args.rounds):
        for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            fn = arms[name]
            for _ in range(args.warmup):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record(st)
            for i in range(args.reps):
                fn()
                ev[i + 1].record(st)
            torch.cuda.synchronize()
            t = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.reps)]
            times[name] += t
            means[name].append(float(np.mean(t)))
    block_bytes = bs * count
    moved = {"a_chain": (3 * (k - 1) + 1) * block_bytes, "b_fused": (k + 1) * block_bytes, "c_read": nsrc * block_bytes}
    res = {"bench": "xor_crc", "shape": shape, "crc": "crc64ecma" if c64 else "crc32c", "k": k, "nbytes": bs,
           "count": count, "in_place": in_place, "lanes": lanes, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup, "stripes_checked": int(sample.size)}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "bytes_moved": moved[name], "TBps_mean": round(moved[name] / (ms.mean() * 1e-3) / 1e12, 3),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    a, b = res["a_chain"], res["b_fused"]
    res["ratio_b_over_a"] = round(b["ms_mean"] / a["ms_mean"], 4)
    spread = max(a["spread_ms"], b["spread_ms"])
    res["b_faster_than_a_beyond_spread"] = bool(a["ms_mean"] - b["ms_mean"] > spread)
    res["b_slower_than_a_beyond_spread"] = bool(b["ms_mean"] - a["ms_mean"] > spread)
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

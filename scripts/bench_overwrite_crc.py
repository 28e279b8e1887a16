#!/usr/bin/env python3
"""A/B of the overwrite + CRC delta call by the method of
§4.3: one process, device to device, source and destination co-aligned, 5
alternations of 20 timed launches after 5 warm-ups per arm, HIP events on the
launch stream.

Arms:
  a  the unfused pair on one stream: batch_iov over the old destination
     ranges, then copy_batch_iov. The XOR kernel a caller would still need for
     the deltas is left out, in (a)'s favour.
  b  the fused call, overwrite_batch_iov.
  c  (partial blocks only) what a caller without deltas does: copy_batch_iov
     of the pages, then batch_strided over the whole blocks.

Shapes: 1 Mi x 4 KiB, 64 Ki x 64 KiB, and 64 Ki pages of 4 KiB each into its
own 64 KiB block. Every launch writes bytes that differ from the ones in place
(two source sets taken in turn), so the CRC bodies never run on a zero XOR.
The lane-group size is the library's choice for the write size, set for every
arm alike. Before anything is timed, the deltas of --check sampled writes are
compared with the host oracle over host copies of their old and new bytes, and
the landed bytes of every write with the source.

Writes one JSON line per shape and CRC; --out appends them to a file
(profiles/overwrite_crc_ab.jsonl)."""
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
ap.add_argument("--shapes", default="4k,64k,partial")
ap.add_argument("--crc", default="crc32c,crc64")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--check", type=int, default=2048, help="writes whose deltas are compared with the host oracle")
ap.add_argument("--scale", type=int, default=1, help="divide the counts by this (smoke runs)")
ap.add_argument("--lanes", type=int, default=0, help="lanes per buffer for every arm (0: the library's for the size)")
ap.add_argument("--out")
args = ap.parse_args()

# name: (write bytes, writes, destination stride)
SHAPES = {"4k": (4096, 1 << 20, 4096), "64k": (65536, 1 << 16, 65536), "partial": (4096, 1 << 16, 65536)}
st = torch.cuda.Stream()


def iov_of(t, stride, nbytes, count):
    ptr = t.data_ptr() + torch.arange(count, dtype=torch.int64, device="cuda") * stride
    return torch.stack([ptr, torch.full_like(ptr, nbytes)], dim=1).contiguous(), ptr.contiguous()


def bench(shape, c64):
    nbytes, count, dstride = SHAPES[shape]
    count //= args.scale
    dt = torch.int64 if c64 else torch.int32
    npdt = np.uint64 if c64 else np.uint32
    crc = oracle.crc64ecma if c64 else oracle.crc32c
    batch_iov = ck.batch64_iov if c64 else ck.batch_iov
    copy_iov = ck.copy_batch64_iov if c64 else ck.copy_batch_iov
    overwrite_iov = ck.overwrite_batch64_iov if c64 else ck.overwrite_batch_iov
    batch_strided = ck.batch64_strided if c64 else ck.batch_strided
    lanes = args.lanes or ck.lanes_for(nbytes)
    ck.set_lanes_per_buffer(lanes)

    srcs = [torch.empty(nbytes * count, dtype=torch.uint8, device="cuda") for _ in range(2)]
    for k, s in enumerate(srcs):
        ck.fill_splitmix(s, nbytes, nbytes, count, 0x5EED0001 + (k << 32))
    dst = torch.empty(dstride * count, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(dst, dstride, dstride, count, 0x01D0001)
    src_iov = [iov_of(s, nbytes, nbytes, count)[0] for s in srcs]
    dst_iov, dst_ptr = iov_of(dst, dstride, nbytes, count)
    out = torch.zeros(count, dtype=dt, device="cuda")
    out2 = torch.zeros(count, dtype=dt, device="cuda")
    turn = [0]

    def pair():
        batch_iov(dst_iov, count, out2, stream=st)
        copy_iov(src_iov[turn[0]], dst_ptr, count, out, stream=st)
        turn[0] ^= 1

    def fused():
        overwrite_iov(src_iov[turn[0]], dst_ptr, count, out, stream=st)
        turn[0] ^= 1

    def reread():
        copy_iov(src_iov[turn[0]], dst_ptr, count, out, stream=st)
        batch_strided(dst, dstride, dstride, count, out2, stream=st)
        turn[0] ^= 1

    arms = {"a_pair": pair, "b_fused": fused}
    if shape == "partial":
        arms["c_reread"] = reread

    # correctness before anything is timed: deltas against the host oracle on a sample, landed bytes everywhere
    torch.cuda.synchronize()
    sample = np.unique(np.concatenate([np.arange(min(count, 64)), np.arange(max(count - 64, 0), count),
                                       np.random.default_rng(1).integers(0, count, args.check)]))
    view = lambda t, stride: t.view(count, stride)[:, :nbytes]
    old = view(dst, dstride)[torch.from_numpy(sample).cuda()].cpu().numpy()
    new = view(srcs[0], nbytes)[torch.from_numpy(sample).cuda()].cpu().numpy()
    image = dst.clone()
    with torch.cuda.stream(st):
        fused()
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(npdt)[sample]
    want = np.array([crc(o, 0xDEADBEEF) ^ crc(n, 0xDEADBEEF) for o, n in zip(old, new)], npdt)
    assert np.array_equal(got, want), f"{shape}: {np.count_nonzero(got != want)} of {sample.size} sampled deltas differ"
    assert torch.equal(view(dst, dstride), view(srcs[0], nbytes)), f"{shape}: landed bytes differ from the source"
    if dstride != nbytes:  # and nothing outside the pages
        assert torch.equal(dst.view(count, dstride)[:, nbytes:], image.view(count, dstride)[:, nbytes:])
    del image

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
    gib = nbytes * count / 2.0**30
    res = {"bench": "overwrite_crc", "shape": shape, "crc": "crc64ecma" if c64 else "crc32c", "nbytes": nbytes,
           "count": count, "dst_stride": dstride, "lanes": lanes, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup, "deltas_checked": int(sample.size)}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "payload_GiBps_mean": round(gib / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    for other in [k for k in arms if k != "b_fused"]:
        res[f"ratio_b_over_{other[0]}"] = round(res["b_fused"]["ms_mean"] / res[other]["ms_mean"], 4)
        spread = max(res["b_fused"]["spread_ms"], res[other]["spread_ms"])
        res[f"b_faster_than_{other[0]}_beyond_spread"] = bool(res[other]["ms_mean"] - res["b_fused"]["ms_mean"] > spread)
        res[f"b_slower_than_{other[0]}_beyond_spread"] = bool(res["b_fused"]["ms_mean"] - res[other]["ms_mean"] > spread)
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

#!/usr/bin/env python3
"""A/B of copy + CRC-32C in ONE process, device to device, co-aligned:
  (a) the unfused pair on one stream: photon_crc_memcpy_async, then
      photon_crc32c_batch_strided over the copy -- what a caller did before
      the fused call existed (3 bytes moved per payload byte);
  (b) photon_crc32c_copy_batch_strided (2 bytes moved per payload byte;
      floor for (b)/(a) ~ 0.67).
The arms alternate (--rounds alternations of --reps timed launches each after
--warmup launches), every launch timed with HIP events on the launch stream.
Both arms' CRCs and destination bytes must agree before a number is printed.
One JSON line per shape: each arm's mean / median time and GiB/s of payload,
the ratio (b)/(a), and the spread between the alternations of each arm;
"faster" is true only when (a) - (b) exceeds the larger of the two spreads.

  --pmc-run SHAPE : only a few launches of (b) on SHAPE, for counters-only runs
                    `rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR/fetch -o p -- python ...`
                    and the same with WRITE_SIZE into DIR/write (one counter
                    per run: the profiler refuses both in one pass)
  --pmc-summary DIR : read those runs' counter CSVs: bytes fetched and written
                    per launch over the payload (FETCH_SIZE counts half the
                    bytes of wide reads on gfx950, see summarize_profile.py;
                    both scalings are printed)
  --crc64 : the same A/B, runs and summary for CRC-64/ECMA
                    (photon_crc64ecma_batch_strided after the copy against
                    photon_crc64ecma_copy_batch_strided); adds "margin_over_spread"
                    = ((a) - (b)) / the larger spread and "faster_3x" (margin > 3)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

SHAPES = {"c2": (65536, 65536), "c3": (4096, 1 << 20)}

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="c2,c3")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", help="also write the JSON lines to this file")
ap.add_argument("--pmc-run")
ap.add_argument("--pmc-summary")
ap.add_argument("--crc64", action="store_true")
args = ap.parse_args()


def pmc_summary(d):
    per = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if ("crc64_batch_kernel" if args.crc64 else "crc32c_batch_kernel") in r["Kernel_Name"]:
                    per.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    nbytes, count = SHAPES["c2"]
    payload = nbytes * count
    res = {"shape": "c2", "payload_bytes": payload, "launches": {k: len(v) for k, v in per.items()}}
    for name in ("FETCH_SIZE", "WRITE_SIZE"):
        if name in per:
            kib = statistics.mean(per[name])
            res[name + "_KiB_avg"] = kib
            res[name + "_x1024_over_payload"] = round(kib * 1024 / payload, 5)
            res[name + "_x2048_over_payload"] = round(kib * 2048 / payload, 5)
    return res


if args.pmc_summary:
    line = json.dumps(pmc_summary(args.pmc_summary))
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from photonlibos_amd import checksum as ck  # noqa: E402
from photonlibos_amd._native import lib  # noqa: E402

st = torch.cuda.current_stream()


def arm_pair(src, dst, nbytes, count, out):
    ck._check(lib().photon_crc_memcpy_async(dst.data_ptr(), src.data_ptr(), nbytes * count, st.cuda_stream))
    (ck.batch64_strided if args.crc64 else ck.batch_strided)(dst, nbytes, nbytes, count, out, stream=st)


def arm_fused(src, dst, nbytes, count, out):
    (ck.copy_batch64_strided if args.crc64 else ck.copy_batch_strided)(src, nbytes, dst, nbytes, nbytes, count, out,
                                                                       stream=st)


def bench(shape):
    nbytes, count = SHAPES[shape]
    src = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(nbytes * count, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, nbytes, nbytes, count, 0x5EED0001)
    out = torch.zeros(count, dtype=torch.int64 if args.crc64 else torch.int32, device="cuda")
    if args.pmc_run:
        for _ in range(3):
            arm_fused(src, dst, nbytes, count, out)
        torch.cuda.synchronize()
        return None
    arms = {"pair": arm_pair, "fused": arm_fused}
    crcs = {}
    for name, fn in arms.items():  # same CRCs, same bytes landed, before anything is timed
        dst.zero_()
        out.zero_()
        fn(src, dst, nbytes, count, out)
        torch.cuda.synchronize()
        assert torch.equal(src, dst), f"{name}: destination differs from the source"
        crcs[name] = out.cpu().numpy().copy()
    assert np.array_equal(crcs["pair"], crcs["fused"]), "the arms' CRCs differ"
    means = {k: [] for k in arms}
    times = {k: [] for k in arms}
    for r in range(args.rounds):
        for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            fn = arms[name]
            for _ in range(args.warmup):
                fn(src, dst, nbytes, count, out)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record(st)
            for k in range(args.reps):
                fn(src, dst, nbytes, count, out)
                ev[k + 1].record(st)
            torch.cuda.synchronize()
            t = [ev[k].elapsed_time(ev[k + 1]) for k in range(args.reps)]
            times[name] += t
            means[name].append(float(np.mean(t)))
    gib = nbytes * count / 2.0**30
    res = {"shape": shape, "nbytes": nbytes, "count": count, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "payload_GiBps_mean": round(gib / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    res["ratio_fused_over_pair"] = round(res["fused"]["ms_mean"] / res["pair"]["ms_mean"], 4)
    res["faster"] = bool(res["pair"]["ms_mean"] - res["fused"]["ms_mean"] >
                         max(res["pair"]["spread_ms"], res["fused"]["spread_ms"]))
    if args.crc64:
        res["crc"] = "crc64ecma"
        spread = max(res["pair"]["spread_ms"], res["fused"]["spread_ms"])
        res["margin_over_spread"] = round((res["pair"]["ms_mean"] - res["fused"]["ms_mean"]) / max(spread, 1e-9), 2)
        res["faster_3x"] = bool(res["margin_over_spread"] > 3)
    return res


lines = []
for shape in ([args.pmc_run] if args.pmc_run else args.shapes.split(",")):
    r = bench(shape)
    if r is not None:
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
if args.out and lines:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

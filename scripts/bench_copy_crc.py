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
  --iov : copy + CRC between iovectors (photon_crc32c_copy_msg_iov_n; with
                    --crc64 photon_crc64ecma_copy_msg_iov_n), the same method, three
                    arms over 8,192 messages of 8 co-aligned 8 KiB source segments:
                    "gather" = photon_crc32c_gather_msg_n into one 64 KiB run per
                    message; "iov" = the new call into ONE 64 KiB destination
                    segment per message (the same loads and stores); "reseg" = the
                    new call into 16 destination segments of 4 KiB per message
                    (no equal-work baseline). "within" is true when |iov - gather|
                    is at most the larger of 3 % of gather and three times the
                    spread between gather's alternations. --out appends here, so
                    the CRC-32C and the CRC-64 run share one file.
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
ap.add_argument("--iov", action="store_true")
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


def bench_iov():
    nmsg, nseg_m, seg, blk = 8192, 8, 8192, 4096
    nseg, msg = nmsg * nseg_m, nseg_m * seg
    nblk = nmsg * msg // blk
    total = nmsg * msg
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, seg, seg, nseg, 0x5EED0101)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    # segment s of the stream of messages sits in source slot (4099 s) mod nseg: a scatter-gather list
    slot = (np.arange(nseg, dtype=np.uint64) * np.uint64(4099)) % np.uint64(nseg)
    siov = np.empty((nseg, 2), np.uint64)
    siov[:, 0] = np.uint64(src.data_ptr()) + slot * np.uint64(seg)
    siov[:, 1] = seg
    # "iov": one destination segment per message; "reseg": block q of the stream in slot (8191 q) mod nblk
    d1 = np.empty((nmsg, 2), np.uint64)
    d1[:, 0] = np.uint64(dst.data_ptr()) + np.arange(nmsg, dtype=np.uint64) * np.uint64(msg)
    d1[:, 1] = msg
    bslot = (np.arange(nblk, dtype=np.uint64) * np.uint64(8191)) % np.uint64(nblk)
    d16 = np.empty((nblk, 2), np.uint64)
    d16[:, 0] = np.uint64(dst.data_ptr()) + bslot * np.uint64(blk)
    d16[:, 1] = blk
    d_siov, d_sstart = i64(siov), i64(np.arange(nmsg + 1, dtype=np.uint64) * np.uint64(nseg_m))
    d_d1, d_d1start = i64(d1), i64(np.arange(nmsg + 1, dtype=np.uint64))
    d_d16, d_d16start = i64(d16), i64(np.arange(nmsg + 1, dtype=np.uint64) * np.uint64(msg // blk))
    d_ptrs = i64(d1[:, 0])
    out = torch.zeros(nmsg, dtype=torch.int64 if args.crc64 else torch.int32, device="cuda")
    gather = ck.gather64_msg_n if args.crc64 else ck.gather_msg_n
    copy_iov = ck.copy_msg64_iov_n if args.crc64 else ck.copy_msg_iov_n
    arms = {
        "gather": lambda: gather(d_siov, d_sstart, nmsg, nseg, d_ptrs, None, out, stream=st),
        "iov": lambda: copy_iov(d_siov, d_sstart, nseg, d_d1, d_d1start, nmsg, nmsg, out, stream=st),
        "reseg": lambda: copy_iov(d_siov, d_sstart, nseg, d_d16, d_d16start, nblk, nmsg, out, stream=st),
    }
    stream_bytes = src.view(nseg, seg)[torch.from_numpy(slot.astype(np.int64)).cuda()].reshape(-1)
    crcs = {}
    for name, fn in arms.items():  # same CRCs, the right bytes landed, before anything is timed
        dst.zero_()
        out.zero_()
        fn()
        torch.cuda.synchronize()
        landed = dst if name != "reseg" else dst.view(nblk, blk)[torch.from_numpy(bslot.astype(np.int64)).cuda()].reshape(-1)
        assert torch.equal(landed, stream_bytes), f"{name}: destination differs from the source stream"
        crcs[name] = out.cpu().numpy().copy()
    assert np.array_equal(crcs["gather"], crcs["iov"]) and np.array_equal(crcs["gather"], crcs["reseg"]), \
        "the arms' CRCs differ"
    del stream_bytes
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
    gib = total / 2.0**30
    res = {"shape": "iov", "crc": "crc64ecma" if args.crc64 else "crc32c", "nmsg": nmsg, "src_segments": nseg_m,
           "src_segment_bytes": seg, "reseg_block_bytes": blk, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "payload_GiBps_mean": round(gib / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    a, b = res["gather"]["ms_mean"], res["iov"]["ms_mean"]
    res["ratio_iov_over_gather"] = round(b / a, 4)
    res["ratio_reseg_over_gather"] = round(res["reseg"]["ms_mean"] / a, 4)
    res["allowed_ms"] = round(max(0.03 * a, 3 * res["gather"]["spread_ms"]), 5)
    res["within"] = bool(abs(b - a) <= res["allowed_ms"])
    return res


if args.iov:
    line = json.dumps(bench_iov())
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    sys.exit(0)

lines = []
for shape in ([args.pmc_run] if args.pmc_run else args.shapes.split(",")):
    r = bench(shape)
    if r is not None:
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
if args.out and lines:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")

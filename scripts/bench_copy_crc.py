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
  --iov-seg : per-segment CRCs from the copy between iovectors
                    (photon_crc32c_copy_msg_iov_seg_n; with --crc64 the CRC-64 call), the
                    same method over the "reseg" shape of --iov: 8,192 messages of 8
                    co-aligned 8 KiB source segments in permuted slots into 16 blocks
                    of 4 KiB in permuted slots. "plain" = copy_msg_iov_n alone (no
                    segment CRCs: the floor); "pair" = what a caller did before:
                    copy_msg_iov_n, then batch_iov over the 131,072 destination blocks
                    on the same stream (3 bytes moved per payload byte); "seg_dst" =
                    the new call, a CRC per destination block (2 bytes per payload
                    byte; floor for seg_dst/pair ~ 0.67); "plain_mirror" / "seg_src" =
                    the mirrored shape (16 blocks of 4 KiB into 8 segments of 8 KiB)
                    through copy_msg_iov_n and through the new call with a CRC per
                    source block. "faster_3x" is true when pair - seg_dst exceeds three
                    times the spread between pair's alternations. --out appends.
  --iov-seg2 : the segment CRCs of BOTH sides from the copy between iovectors
                    (photon_crc32c_copy_msg_iov_seg2_n; with --crc64 the CRC-64 call), the same
                    method over the shape of --iov-seg (8 x 8 KiB source segments into 16 x 4 KiB
                    blocks per message). "plain" = copy_msg_iov_n alone (the floor); "seg_dst" =
                    the one-side call, a CRC per destination block; "today" = what a caller did
                    before: the one-side call, then batch_iov over the 65,536 source segments on
                    the same stream (3 bytes moved per payload byte); "seg2" = the new call (2
                    bytes per payload byte). Every arm's message CRCs, both sides' segment CRCs and
                    the landed bytes are compared before anything is timed. "faster_3x" is true
                    when today - seg2 exceeds three times the spread between today's alternations.
                    --out appends.
  --long : copy + CRC of ONE long buffer over the whole device
                    (photon_crc32c_copy_extend_device; with --crc64 the CRC-64 call), the
                    same method, one JSON line per size (--sizes, MiB), source at buf+1,
                    destination at dbuf+1 (the reference's perf shape, co-aligned) and one
                    last row not co-aligned (destination at dbuf+10, no claim): "pair" =
                    photon_crc_memcpy_async, then extend_device over the copy (3 bytes
                    moved per payload byte); "fused" = the new call (2 bytes per payload
                    byte; floor for fused/pair ~ 0.67); "pieces" = copy_batch_strided over
                    64 KiB pieces of the same bytes, then combine_series_device (CRC-64:
                    combine_series64_device), both timed. "faster_3x" is true when pair - fused
                    exceeds three times the spread between pair's alternations; "within" is
                    true when |fused - pieces| is at most the larger of 3 % of pieces and
                    three times the spread of pieces. --out appends.
  --fold : part CRCs folded into object CRCs (photon_crc32c_fold_parts_n and
                    photon_crc64ecma_fold_parts_n, both in one run), the same alternations,
                    one JSON line per CRC and shape (1 object x 16 parts, 1 x 10,000, 4,096 x
                    16; parts of 1 to 16 MiB, the last of each object short): "host" = the
                    route before the call existed, natively (photon_crc_util_fold_on_host:
                    photon_crc_stream_sync, the part CRCs copied to the host, a loop of the
                    host crc32c_combine / crc64ecma_combine), wall clock in us from the call
                    to the value in hand; "device" = the new call, wall clock from the launch
                    to the stream sync that returns d_out (pinned host memory);
                    "device_kernel" = the launch alone by HIP events. The arms' values and
                    the CPU replay of the kernel are compared before anything is timed.
                    "faster_3x" is true when host - device exceeds three times the spread
                    between host's alternations. --out appends.
  --verify : stored CRCs checked on the device (photon_crc32c_verify_n and
                    photon_crc64ecma_verify_n, both in one run), the same alternations, one JSON
                    line per CRC and row (65,536 and 1,048,576 entries with 0 and 3 bad ones,
                    bad_cap 64, and 1,048,576 with 1 % bad, bad_cap = the count; dense expected
                    words): "host" = the route before the calls existed, natively
                    (photon_crc_util_verify_on_host: photon_crc_stream_sync, the CRC words copied
                    to pinned host memory, a compare loop against a host array), wall clock in us
                    from the call to the verdict in hand; "device" = the new call with report and
                    list in pinned host memory, wall clock from the launch to the stream sync;
                    "device_kernels" = its three launches alone by HIP events. Both arms' reports
                    and lists are compared with the expected ones before anything is timed.
                    "faster_3x" is true when host - device exceeds three times the spread between
                    host's alternations. --tiles 1024,4096,... measures those tiles in place of the
                    default (photon_crc_set_verify_tile); with the default alone, two more lines
                    give the C2 batch alone against the batch followed by verify_n, by events.
                    --out appends.
  --scan : running CRCs of objects over their parts (photon_crc32c_scan_parts_n and
                    photon_crc64ecma_scan_parts_n, both in one run), the same alternations, one JSON
                    line per CRC and shape (1 object x 16 parts, 1 x 10,000, 1 x 1,048,576, 4,096 x
                    16; parts of 1 to 16 MiB, the 1 Mi shape uniform 4 KiB): "host" = the route
                    before the calls existed, natively (photon_crc_util_scan_on_host:
                    photon_crc_stream_sync, the part CRCs copied to pinned host memory, a serial
                    chain of the host crc32c_combine / crc64ecma_combine, the running words copied
                    back), wall clock in us; "device" = the new call, wall clock from the launch to
                    the stream sync; "device_kernel" = its launches alone by HIP events; for one
                    object "fold" / "fold_kernel" = fold_parts_n over the same pairs (the last value
                    only). The arms' values, the fold's and the positions are compared before
                    anything is timed. At 100,000 parts and more the host and fold arms run a tenth
                    of --reps ("slow_arm_reps"). --tiles 256,1024,... measures those tiles
                    (photon_crc_set_scan_tile); --scan-shapes 1x16,... picks shapes. --out appends.
  --parts : copy + CRC of many large parts in one launch
                    (photon_crc32c_copy_parts_n; with --crc64 the CRC-64 call), the same method,
                    device to device, the parts back to back from buf+1 to dbuf+1 (co-aligned):
                    1,024 x 4 MiB, 256 x 16 MiB, 64 x 64 MiB, 512 parts of seeded lengths of 1 to
                    16 MiB, and 256 x 16 MiB to dbuf+10 (not co-aligned, no claim). "loop" = one
                    copy_extend_device call per part on one stream (the route documented before);
                    "parts" = the new call; "batch_iov" = copy_batch_iov over the same parts;
                    "hand_built" (uniform shapes) = copy_batch_strided over 64 KiB pieces of the same
                    bytes, then combine_series_device per part; "fold_only" = the new call's second
                    launch alone (photon_crc_util_parts_fold); "parts_cap_1GiB" (ragged shape) = the
                    new call with max_part_bytes = 1 GiB, whose difference to "parts" is the time of
                    the empty tasks. Then "parts" at 32, 64 and 128 KiB pieces on the first two
                    shapes, and the CRC-only calls (loop of extend_device, batch_parts, batch_iov; no
                    claim). "faster_3x_than_X" is true when X - parts exceeds three times the spread
                    between X's alternations; "not_slower_than_hand_built" when parts - hand_built is
                    at most the larger of 3 % of hand_built and three times its spread. --shapes
                    picks shapes by name; --out appends.
  --parts-packed : copy + CRC of mixed-size parts with the piece tasks packed on the
                    device (photon_crc32c_copy_parts_packed_n and the CRC-64 call, both in one run),
                    the same method and layout: 512 parts of seeded lengths of 1 to 16 MiB, 1,024 x
                    4 MiB, 256 x 16 MiB, and 2,048 parts of seeded log-uniform lengths from 4 KiB to
                    32 MiB. "packed" = the new call with max_part_bytes = ~0 and max_total_bytes =
                    the exact sum; "parts" = copy_parts_n with the cap at the longest part;
                    "parts_cap_1GiB" (ragged shape) = copy_parts_n under a 1 GiB cap; "batch_iov"
                    (mixed shape) = copy_batch_iov; "plan_only" = the new call's four plan launches
                    alone (photon_crc_util_parts_packed_plan). "faster_3x_than_parts_cap_1GiB" is true
                    when parts_cap_1GiB - packed exceeds three times the spread between
                    parts_cap_1GiB's alternations; "not_slower_than_parts" (uniform shapes) when
                    packed - parts is at most the larger of 3 % of parts and three times its spread.
                    --shapes picks shapes by name; --out appends.
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
ap.add_argument("--iov-seg", action="store_true")
ap.add_argument("--iov-seg2", action="store_true")
ap.add_argument("--long", action="store_true")
ap.add_argument("--sizes", default="64,256,1024", help="--long: payload sizes in MiB")
ap.add_argument("--fold", action="store_true")
ap.add_argument("--parts", action="store_true")
ap.add_argument("--parts-packed", action="store_true")
ap.add_argument("--verify", action="store_true")
ap.add_argument("--tiles", default="0", help="--verify, --scan: tiles in entries to measure, 0 = the default")
ap.add_argument("--scan", action="store_true")
ap.add_argument("--scan-shapes", help="--scan: objects x parts per object, e.g. 1x16,4096x16 (default: all four)")
ap.add_argument("--tree", default="working tree", help="--fold: a label of the tree measured, written to each line")
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


def bench_iov_seg():
    nmsg, big, small = 8192, 8192, 4096
    nbig_m, nsmall_m = 8, 16
    msg = nbig_m * big
    nbig, nsmall, total = nmsg * nbig_m, nmsg * nsmall_m, nmsg * msg
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, big, big, nbig, 0x5EED0101)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    # segment s of the stream of messages sits in 8 KiB slot (4099 s) mod nbig, block q in 4 KiB slot (8191 q) mod nsmall
    slot = (np.arange(nbig, dtype=np.uint64) * np.uint64(4099)) % np.uint64(nbig)
    bslot = (np.arange(nsmall, dtype=np.uint64) * np.uint64(8191)) % np.uint64(nsmall)

    def iov(buf, slots, n):
        a = np.empty((slots.size, 2), np.uint64)
        a[:, 0] = np.uint64(buf.data_ptr()) + slots * np.uint64(n)
        a[:, 1] = n
        return i64(a)
    big_start = i64(np.arange(nmsg + 1, dtype=np.uint64) * np.uint64(nbig_m))
    small_start = i64(np.arange(nmsg + 1, dtype=np.uint64) * np.uint64(nsmall_m))
    s_big, d_small = iov(src, slot, big), iov(dst, bslot, small)      # scatter into blocks
    s_small, d_big = iov(src, bslot, small), iov(dst, slot, big)      # mirrored: blocks into segments
    dt = torch.int64 if args.crc64 else torch.int32
    out = torch.zeros(nmsg, dtype=dt, device="cuda")
    seg = torch.zeros(nsmall, dtype=dt, device="cuda")
    copy_iov = ck.copy_msg64_iov_n if args.crc64 else ck.copy_msg_iov_n
    copy_seg = ck.copy_msg64_iov_seg_n if args.crc64 else ck.copy_msg_iov_seg_n
    batch_iov = ck.batch64_iov if args.crc64 else ck.batch_iov

    def pair():
        copy_iov(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, out, stream=st)
        batch_iov(d_small, nsmall, seg, stream=st)
    arms = {
        "plain": lambda: copy_iov(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, out, stream=st),
        "pair": pair,
        "seg_dst": lambda: copy_seg(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, ck.SEG_OF_DST, seg,
                                    out, stream=st),
        "plain_mirror": lambda: copy_iov(s_small, small_start, nsmall, d_big, big_start, nbig, nmsg, out, stream=st),
        "seg_src": lambda: copy_seg(s_small, small_start, nsmall, d_big, big_start, nbig, nmsg, ck.SEG_OF_SRC, seg,
                                    out, stream=st),
    }
    idx = lambda a: torch.from_numpy(a.astype(np.int64)).cuda()
    stream_a = src.view(nbig, big)[idx(slot)].reshape(-1)
    stream_m = src.view(nsmall, small)[idx(bslot)].reshape(-1)
    # the CRC of every 4 KiB source block of the mirrored shape, by the batch kernel
    src_blocks = torch.zeros(nsmall, dtype=dt, device="cuda")
    batch_iov(s_small, nsmall, src_blocks, stream=st)
    crcs, segs = {}, {}
    for name, fn in arms.items():  # same CRCs, the right bytes landed, before anything is timed
        dst.zero_()
        out.fill_(-1)
        seg.fill_(-1)
        fn()
        torch.cuda.synchronize()
        if name in ("plain", "pair", "seg_dst"):
            landed, want = dst.view(nsmall, small)[idx(bslot)].reshape(-1), stream_a
        else:
            landed, want = dst.view(nbig, big)[idx(slot)].reshape(-1), stream_m
        assert torch.equal(landed, want), f"{name}: destination differs from the source stream"
        crcs[name] = out.cpu().numpy().copy()
        segs[name] = seg.cpu().numpy().copy()
    assert np.array_equal(crcs["plain"], crcs["pair"]) and np.array_equal(crcs["plain"], crcs["seg_dst"]), \
        "the arms' message CRCs differ"
    assert np.array_equal(segs["pair"], segs["seg_dst"]), "the block CRCs of pair and seg_dst differ"
    assert np.array_equal(crcs["plain_mirror"], crcs["seg_src"]), "the mirrored arms' message CRCs differ"
    assert np.array_equal(segs["seg_src"], src_blocks.cpu().numpy()), "seg_src differs from batch_iov over the source blocks"
    del stream_a, stream_m
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
    res = {"shape": "iov_seg", "crc": "crc64ecma" if args.crc64 else "crc32c", "nmsg": nmsg, "segments": nbig_m,
           "segment_bytes": big, "blocks": nsmall_m, "block_bytes": small, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "payload_GiBps_mean": round(gib / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    a, p, b = res["plain"]["ms_mean"], res["pair"]["ms_mean"], res["seg_dst"]["ms_mean"]
    res["ratio_seg_dst_over_pair"] = round(b / p, 4)
    res["ratio_seg_dst_over_plain"] = round(b / a, 4)
    res["ratio_seg_src_over_plain"] = round(res["seg_src"]["ms_mean"] / a, 4)
    res["ratio_seg_src_over_plain_mirror"] = round(res["seg_src"]["ms_mean"] / res["plain_mirror"]["ms_mean"], 4)
    res["margin_over_pair_spread"] = round((p - b) / max(res["pair"]["spread_ms"], 1e-9), 2)
    res["faster_3x"] = bool(p - b > 3 * res["pair"]["spread_ms"])
    return res


def bench_iov_seg2():
    nmsg, big, small = 8192, 8192, 4096
    nbig_m, nsmall_m = 8, 16
    msg = nbig_m * big
    nbig, nsmall, total = nmsg * nbig_m, nmsg * nsmall_m, nmsg * msg
    src = torch.empty(total, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(total, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(src, big, big, nbig, 0x5EED0101)
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    # the shape of --iov-seg: segment s in 8 KiB slot (4099 s) mod nbig, block q in 4 KiB slot (8191 q) mod nsmall
    slot = (np.arange(nbig, dtype=np.uint64) * np.uint64(4099)) % np.uint64(nbig)
    bslot = (np.arange(nsmall, dtype=np.uint64) * np.uint64(8191)) % np.uint64(nsmall)

    def iov(buf, slots, n):
        a = np.empty((slots.size, 2), np.uint64)
        a[:, 0] = np.uint64(buf.data_ptr()) + slots * np.uint64(n)
        a[:, 1] = n
        return i64(a)
    big_start = i64(np.arange(nmsg + 1, dtype=np.uint64) * np.uint64(nbig_m))
    small_start = i64(np.arange(nmsg + 1, dtype=np.uint64) * np.uint64(nsmall_m))
    s_big, d_small = iov(src, slot, big), iov(dst, bslot, small)
    dt = torch.int64 if args.crc64 else torch.int32
    out = torch.zeros(nmsg, dtype=dt, device="cuda")
    sseg = torch.zeros(nbig, dtype=dt, device="cuda")
    dseg = torch.zeros(nsmall, dtype=dt, device="cuda")
    copy_iov = ck.copy_msg64_iov_n if args.crc64 else ck.copy_msg_iov_n
    copy_seg = ck.copy_msg64_iov_seg_n if args.crc64 else ck.copy_msg_iov_seg_n
    copy_seg2 = ck.copy_msg64_iov_seg2_n if args.crc64 else ck.copy_msg_iov_seg2_n
    batch_iov = ck.batch64_iov if args.crc64 else ck.batch_iov

    def today():
        copy_seg(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, ck.SEG_OF_DST, dseg, out, stream=st)
        batch_iov(s_big, nbig, sseg, stream=st)
    arms = {
        "plain": lambda: copy_iov(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, out, stream=st),
        "seg_dst": lambda: copy_seg(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, ck.SEG_OF_DST, dseg,
                                    out, stream=st),
        "today": today,
        "seg2": lambda: copy_seg2(s_big, big_start, nbig, d_small, small_start, nsmall, nmsg, sseg, dseg, out,
                                  stream=st),
    }
    idx = lambda a: torch.from_numpy(a.astype(np.int64)).cuda()
    stream_a = src.view(nbig, big)[idx(slot)].reshape(-1)
    crcs, ssegs, dsegs = {}, {}, {}
    for name, fn in arms.items():  # same CRCs, the right bytes landed, before anything is timed
        dst.zero_()
        out.fill_(-1)
        sseg.fill_(-1)
        dseg.fill_(-1)
        fn()
        torch.cuda.synchronize()
        landed = dst.view(nsmall, small)[idx(bslot)].reshape(-1)
        assert torch.equal(landed, stream_a), f"{name}: destination differs from the source stream"
        crcs[name] = out.cpu().numpy().copy()
        ssegs[name] = sseg.cpu().numpy().copy()
        dsegs[name] = dseg.cpu().numpy().copy()
    assert all(np.array_equal(crcs["plain"], crcs[k]) for k in arms), "the arms' message CRCs differ"
    assert np.array_equal(dsegs["seg_dst"], dsegs["seg2"]) and np.array_equal(dsegs["today"], dsegs["seg2"]), \
        "the destination block CRCs of seg2 differ from the one-side call's"
    assert np.array_equal(ssegs["today"], ssegs["seg2"]), "the source segment CRCs of seg2 differ from batch_iov's"
    del stream_a
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
    res = {"shape": "iov_seg2", "crc": "crc64ecma" if args.crc64 else "crc32c", "nmsg": nmsg, "segments": nbig_m,
           "segment_bytes": big, "blocks": nsmall_m, "block_bytes": small, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "payload_GiBps_mean": round(gib / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    a, b, p, b2 = (res[k]["ms_mean"] for k in ("plain", "seg_dst", "today", "seg2"))
    res["ratio_seg2_over_today"] = round(b2 / p, 4)
    res["ratio_seg2_over_plain"] = round(b2 / a, 4)
    res["ratio_seg2_over_seg_dst"] = round(b2 / b, 4)
    res["margin_over_today_spread"] = round((p - b2) / max(res["today"]["spread_ms"], 1e-9), 2)
    res["faster_3x"] = bool(p - b2 > 3 * res["today"]["spread_ms"])
    return res


def bench_long(mib, delta):
    n, piece = mib << 20, 65536
    count = n // piece
    assert count * piece == n
    src = torch.empty(n + 4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n + 4096, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 4096 == 0 and dst.data_ptr() % 4096 == 0
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0x5EED0201)
    sp, dp = src.data_ptr() + 1, dst.data_ptr() + 1 + delta
    dt = torch.int64 if args.crc64 else torch.int32
    out = torch.zeros(1, dtype=dt, device="cuda")
    parts = torch.zeros(count, dtype=dt, device="cuda")

    def pair():
        ck._check(lib().photon_crc_memcpy_async(dp, sp, n, st.cuda_stream))
        if args.crc64:
            ck.extend64_device(dp, n, out, stream=st)
        else:
            ck.extend_device(dp, n, 0, out, stream=st)

    def fused():
        if args.crc64:
            ck.copy_extend64_device(sp, dp, n, out, stream=st)
        else:
            ck.copy_extend_device(sp, dp, n, 0, out, stream=st)

    def pieces():
        if args.crc64:
            ck.copy_batch64_strided(sp, piece, dp, piece, piece, count, parts, stream=st)
            ck.combine_series64_device(parts, piece, count, out, stream=st)
        else:
            ck.copy_batch_strided(sp, piece, dp, piece, piece, count, parts, stream=st)
            ck.combine_series_device(parts, piece, count, out, stream=st)
    arms = {"pair": pair, "fused": fused, "pieces": pieces}
    crcs = {}
    for name, fn in arms.items():  # same CRC, same bytes landed, before anything is timed
        dst.zero_()
        out.fill_(-1)
        fn()
        torch.cuda.synchronize()
        assert torch.equal(dst[1 + delta:1 + delta + n], src[1:1 + n]), f"{name}: destination differs from the source"
        assert not bool(dst[:1 + delta].any()) and not bool(dst[1 + delta + n:].any()), f"{name}: wrote outside"
        crcs[name] = int(out.cpu().numpy().view(np.uint64 if args.crc64 else np.uint32)[0])
    assert crcs["pair"] == crcs["fused"] == crcs["pieces"], f"the arms' CRCs differ: {crcs}"
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
    gib = n / 2.0**30
    res = {"shape": "long", "crc": "crc64ecma" if args.crc64 else "crc32c", "MiB": mib, "src": "buf+1",
           "dst": f"dbuf+{1 + delta}", "co_aligned": delta % 16 == 0, "piece_bytes": piece,
           "pieces_fold": "combine_series64_device" if args.crc64 else "combine_series_device", "rounds": args.rounds,
           "reps": args.reps, "warmup": args.warmup}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "payload_GiBps_mean": round(gib / (ms.mean() * 1e-3), 1),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    a, b, c = res["pair"]["ms_mean"], res["fused"]["ms_mean"], res["pieces"]["ms_mean"]
    res["ratio_fused_over_pair"] = round(b / a, 4)
    res["margin_over_pair_spread"] = round((a - b) / max(res["pair"]["spread_ms"], 1e-9), 2)
    res["faster_3x"] = bool(a - b > 3 * res["pair"]["spread_ms"])
    res["ratio_fused_over_pieces"] = round(b / c, 4)
    res["allowed_ms"] = round(max(0.03 * c, 3 * res["pieces"]["spread_ms"]), 5)
    res["within"] = bool(abs(b - c) <= res["allowed_ms"])
    res["fused_slower_than_pieces"] = bool(b - c > res["allowed_ms"])
    return res


FOLD_SHAPES = [(1, 16), (1, 10000), (4096, 16)]  # objects x parts per object


def bench_fold(crc64, nobj, per):
    import time
    rng = np.random.default_rng(0xF01D + nobj + per)
    nparts = nobj * per
    wdt = np.uint64 if crc64 else np.uint32
    lens = rng.integers(1 << 20, 1 << 24, nparts).astype(np.uint64)  # unequal parts of 1 to 16 MiB ...
    lens[per - 1::per] = rng.integers(1, 1 << 20, nobj)              # ... and a short last part
    crcs = rng.integers(0, 1 << 63, nparts, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    crcs = crcs if crc64 else (crcs >> np.uint64(32)).astype(np.uint32)
    start = np.arange(nobj + 1, dtype=np.uint64) * np.uint64(per)
    seed = 0xFEDCBA9876543210 if crc64 else 0x9E3779B1
    d_crc = torch.from_numpy(crcs.view(np.int64 if crc64 else np.int32)).cuda()
    d_len = torch.from_numpy(lens.view(np.int64)).cuda()
    d_start = torch.from_numpy(start.view(np.int64)).cuda()
    out_b = torch.zeros(nobj, dtype=torch.int64 if crc64 else torch.int32).pin_memory()  # in hand after the sync
    out_a = np.zeros(nobj, wdt)
    fold = ck.fold_parts64_device if crc64 else ck.fold_parts_device
    sh = st.cuda_stream

    def host():    # (a): sync, part CRCs to the host, a loop of the library's host combine
        ck._check(lib().photon_crc_util_fold_on_host(int(crc64), d_crc.data_ptr(), lens.ctypes.data,
                                                     start.ctypes.data, nobj, nparts, seed, out_a.ctypes.data, sh))

    def launch():
        fold(d_crc, d_len, d_start, nobj, nparts, out_b, seed=seed, stream=st)

    def device():  # (b): the launch, then the stream sync that returns d_out
        launch()
        ck._check(lib().photon_crc_stream_sync(sh))

    torch.cuda.synchronize()
    host()
    device()
    got = out_b.numpy().view(wdt)
    assert np.array_equal(out_a, got), f"the arms' values differ: {out_a[:4]} {got[:4]}"
    import ctypes
    res0, nt = ctypes.c_uint64(0), 64 if per <= 64 else 256 if per <= 1024 else 1024
    ck._check(lib().photon_crc_test_fold_parts(int(crc64), crcs.ctypes.data, lens.ctypes.data, per, seed, nt,
                                               ctypes.addressof(res0), None))
    assert res0.value == int(got[0]), "the device fold differs from its CPU replay"
    arms = {"host": host, "device": device}
    times = {"host": [], "device": [], "device_kernel": []}
    means = {k: [] for k in times}
    for r in range(args.rounds):
        for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            fn = arms[name]
            for _ in range(args.warmup):
                fn()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            times[name] += t
            means[name].append(float(np.mean(t)))
            if name == "device":  # the kernel alone, by events on the launch stream
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
                ev[0].record(st)
                for k in range(args.reps):
                    launch()
                    ev[k + 1].record(st)
                torch.cuda.synchronize()
                t = [ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(args.reps)]
                times["device_kernel"] += t
                means["device_kernel"].append(float(np.mean(t)))
    res = {"shape": "fold", "crc": "crc64ecma" if crc64 else "crc32c", "objects": nobj, "parts_per_object": per,
           "workgroup_threads": nt, "tree": args.tree, "rounds": args.rounds, "reps": args.reps,
           "warmup": args.warmup}
    for name in times:
        us = np.asarray(times[name])
        res[name] = {"us_mean": round(float(us.mean()), 3), "us_median": round(float(np.median(us)), 3),
                     "round_means_us": [round(m, 3) for m in means[name]],
                     "spread_us": round(max(means[name]) - min(means[name]), 3)}
    a, b = res["host"]["us_mean"], res["device"]["us_mean"]
    res["ratio_device_over_host"] = round(b / a, 4)
    res["margin_over_host_spread"] = round((a - b) / max(res["host"]["spread_us"], 1e-9), 2)
    res["faster_3x"] = bool(a - b > 3 * res["host"]["spread_us"])
    return res


SCAN_SHAPES = [(1, 16), (1, 10000), (1, 1 << 20), (4096, 16)]  # objects x parts per object


def bench_scan(crc64, nobj, per, tile):
    """Running CRCs on the device (scan_parts*_device) against the route before the call existed
    (photon_crc_util_scan_on_host) and, for one object, against fold_parts*_device of the same pairs, which
    yields the last value only. Wall time per call with its stream sync, and kernel time by events."""
    import time
    rng = np.random.default_rng(0x5CA9 + nobj + per)
    nparts = nobj * per
    wdt = np.uint64 if crc64 else np.uint32
    if per >= 1 << 20:
        lens = np.full(nparts, 4096, np.uint64)  # a 4 GiB object in 4 KiB blocks
    else:
        lens = rng.integers(1 << 20, 1 << 24, nparts).astype(np.uint64)  # unequal parts of 1 to 16 MiB ...
        lens[per - 1::per] = rng.integers(1, 1 << 20, nobj)              # ... and a short last part
    crcs = rng.integers(0, 1 << 63, nparts, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    crcs = crcs if crc64 else (crcs >> np.uint64(32)).astype(np.uint32)
    start = np.arange(nobj + 1, dtype=np.uint64) * np.uint64(per)
    seed = 0xFEDCBA9876543210 if crc64 else 0x9E3779B1
    tdt = torch.int64 if crc64 else torch.int32
    d_crc = torch.from_numpy(crcs.view(np.int64 if crc64 else np.int32)).cuda()
    d_len = torch.from_numpy(lens.view(np.int64)).cuda()
    d_start = torch.from_numpy(start.view(np.int64)).cuda()
    h_crc, h_run = torch.zeros(nparts, dtype=tdt).pin_memory(), torch.zeros(nparts, dtype=tdt).pin_memory()
    run_a, run_b = torch.zeros(nparts, dtype=tdt, device="cuda"), torch.zeros(nparts, dtype=tdt, device="cuda")
    end_b = torch.zeros(nparts, dtype=torch.int64, device="cuda")
    out_f = torch.zeros(nobj, dtype=tdt).pin_memory()
    ck.set_scan_tile(tile)
    work = torch.empty(ck.scan_work_bytes(nparts), dtype=torch.uint8, device="cuda")
    scan = ck.scan_parts64_device if crc64 else ck.scan_parts_device
    fold = ck.fold_parts64_device if crc64 else ck.fold_parts_device
    sh = st.cuda_stream

    def host():    # (a): sync, part CRCs to the host, a serial chain of the library's host combine, words back
        ck._check(lib().photon_crc_util_scan_on_host(int(crc64), d_crc.data_ptr(), h_crc.data_ptr(), lens.ctypes.data,
                                                     start.ctypes.data, nobj, nparts, seed, h_run.data_ptr(),
                                                     run_a.data_ptr(), sh))

    def launch():
        scan(d_crc, d_len, d_start, nobj, nparts, run_b, work, seed=seed, end=end_b, stream=st)

    def device():  # (b): the launches, then the stream sync
        launch()
        ck._check(lib().photon_crc_stream_sync(sh))

    def fold_launch():
        fold(d_crc, d_len, d_start, nobj, nparts, out_f, seed=seed, stream=st)

    def fold_device():  # the parent's call on the same pairs: the last value only
        fold_launch()
        ck._check(lib().photon_crc_stream_sync(sh))

    torch.cuda.synchronize()
    host()
    device()
    fold_device()
    got = run_b.cpu().numpy().view(wdt)
    assert np.array_equal(run_a.cpu().numpy().view(wdt), got), "the arms' values differ"
    assert np.array_equal(got[per - 1::per], out_f.numpy().view(wdt)), "the scan's last entries differ from the fold"
    assert np.array_equal(end_b.cpu().numpy().view(np.uint64).reshape(nobj, per),
                          np.cumsum(lens.reshape(nobj, per), axis=1))
    arms = {"host": host, "device": device}
    kernels = {"device": ("device_kernel", launch)}
    if nobj == 1:
        arms["fold"] = fold_device
        kernels["fold"] = ("fold_kernel", fold_launch)
    slow = nparts >= 100000  # the host chain and the one-workgroup fold take long here: fewer calls of them
    times = {k: [] for k in list(arms) + [v[0] for v in kernels.values()]}
    means = {k: [] for k in times}
    for r in range(args.rounds):
        for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            fn = arms[name]
            few = slow and name != "device"
            reps, warmup = (max(2, args.reps // 10), 1) if few else (args.reps, args.warmup)
            for _ in range(warmup):
                fn()
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            times[name] += t
            means[name].append(float(np.mean(t)))
            if name in kernels:  # the kernels alone, by events on the launch stream
                kname, kfn = kernels[name]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
                ev[0].record(st)
                for k in range(reps):
                    kfn()
                    ev[k + 1].record(st)
                torch.cuda.synchronize()
                t = [ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(reps)]
                times[kname] += t
                means[kname].append(float(np.mean(t)))
    ck.set_scan_tile(0)
    res = {"shape": "scan", "crc": "crc64ecma" if crc64 else "crc32c", "objects": nobj, "parts_per_object": per,
           "tile": tile or "default", "tiles": (nparts + (tile or 1024) - 1) // (tile or 1024),
           "part_bytes": "4096" if per >= 1 << 20 else "1-16 MiB", "tree": args.tree, "rounds": args.rounds,
           "reps": args.reps, "warmup": args.warmup,
           "slow_arm_reps": max(2, args.reps // 10) if slow else args.reps}
    for name in times:
        us = np.asarray(times[name])
        res[name] = {"us_mean": round(float(us.mean()), 3), "us_median": round(float(np.median(us)), 3),
                     "round_means_us": [round(m, 3) for m in means[name]],
                     "spread_us": round(max(means[name]) - min(means[name]), 3)}
    a, b = res["host"]["us_mean"], res["device"]["us_mean"]
    res["ratio_device_over_host"] = round(b / a, 4)
    res["margin_over_host_spread"] = round((a - b) / max(res["host"]["spread_us"], 1e-9), 2)
    res["faster_3x"] = bool(a - b > 3 * res["host"]["spread_us"])
    if nobj == 1:
        res["ratio_scan_kernel_over_fold_kernel"] = round(res["device_kernel"]["us_mean"] /
                                                          res["fold_kernel"]["us_mean"], 4)
    return res


VERIFY_ROWS = [(65536, "0"), (65536, "3"), (1 << 20, "0"), (1 << 20, "3"), (1 << 20, "1%")]  # entries, bad ones


def bench_verify(crc64, count, bad, tile):
    """(a) photon_crc_util_verify_on_host against (b) verify_n with report and list in pinned memory."""
    import time
    rng = np.random.default_rng(0x7E21F + count)
    wdt = np.uint64 if crc64 else np.uint32
    crcs = rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    crcs = crcs if crc64 else (crcs >> np.uint64(32)).astype(np.uint32)
    if bad == "1%":
        hit = np.nonzero(rng.random(count) < 0.01)[0]
    else:
        hit = np.array([17, count // 2 + 1, count - 1][:int(bad)], np.int64)
    cap = count if bad == "1%" else 64
    exp = crcs.copy()
    exp[hit] ^= wdt(0x80000001)
    sdt = torch.int64 if crc64 else torch.int32
    d_crc = torch.from_numpy(crcs.view(np.int64 if crc64 else np.int32)).cuda()
    d_exp = torch.from_numpy(exp.view(np.int64 if crc64 else np.int32)).cuda()
    h_crc = torch.zeros(count, dtype=sdt).pin_memory()  # (a)'s landing buffer for the CRC words
    rep_b = torch.zeros(4, dtype=torch.int64).pin_memory()  # in hand after the sync
    lst_b = torch.zeros(cap, dtype=torch.int64).pin_memory()
    rep_a, lst_a = np.zeros(4, np.uint64), np.zeros(cap, np.uint64)
    ck.set_verify_tile(tile)
    work = torch.empty(ck.verify_work_bytes(count), dtype=torch.uint8, device="cuda")
    verify = ck.verify64_device if crc64 else ck.verify_device
    sh = st.cuda_stream

    def host():    # (a): sync, CRC words to the host, a compare loop on the host
        ck._check(lib().photon_crc_util_verify_on_host(int(crc64), d_crc.data_ptr(), h_crc.data_ptr(),
                                                       exp.ctypes.data, count, rep_a.ctypes.data, lst_a.ctypes.data,
                                                       cap, sh))

    def launch():
        verify(d_crc, d_exp, 8 if crc64 else 4, count, rep_b, lst_b, cap, work, stream=st)

    def device():  # (b): the launches, then the stream sync that returns report and list
        launch()
        ck._check(lib().photon_crc_stream_sync(sh))

    torch.cuda.synchronize()
    host()
    device()
    want = [hit.size, int(hit[0]) if hit.size else (1 << 64) - 1, min(hit.size, cap), count]
    got = rep_b.numpy().view(np.uint64)
    assert list(rep_a) == want and list(got) == want, f"the reports differ: {rep_a} {got} {want}"
    assert np.array_equal(lst_a[:hit.size], hit) and np.array_equal(lst_b.numpy()[:hit.size], hit), "the lists differ"
    arms = {"host": host, "device": device}
    times = {"host": [], "device": [], "device_kernels": []}
    means = {k: [] for k in times}
    for r in range(args.rounds):
        for name in (list(arms) if r % 2 == 0 else list(arms)[::-1]):
            fn = arms[name]
            for _ in range(args.warmup):
                fn()
            t = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fn()
                t.append((time.perf_counter() - t0) * 1e6)
            times[name] += t
            means[name].append(float(np.mean(t)))
            if name == "device":  # the three kernels alone, by events on the launch stream
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
                ev[0].record(st)
                for k in range(args.reps):
                    launch()
                    ev[k + 1].record(st)
                torch.cuda.synchronize()
                t = [ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(args.reps)]
                times["device_kernels"] += t
                means["device_kernels"].append(float(np.mean(t)))
    ck.set_verify_tile(0)
    res = {"shape": "verify", "crc": "crc64ecma" if crc64 else "crc32c", "entries": count, "bad": int(hit.size),
           "bad_cap": cap, "tile": tile or "default", "tiles": -(-count // (tile or 1024)), "tree": args.tree,
           "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}
    for name in times:
        us = np.asarray(times[name])
        res[name] = {"us_mean": round(float(us.mean()), 3), "us_median": round(float(np.median(us)), 3),
                     "round_means_us": [round(m, 3) for m in means[name]],
                     "spread_us": round(max(means[name]) - min(means[name]), 3)}
    a, b = res["host"]["us_mean"], res["device"]["us_mean"]
    res["ratio_device_over_host"] = round(b / a, 4)
    res["margin_over_host_spread"] = round((a - b) / max(res["host"]["spread_us"], 1e-9), 2)
    res["faster_3x"] = bool(a - b > 3 * res["host"]["spread_us"])
    return res


def bench_verify_after_batch(crc64):
    """The C2 batch alone against the batch followed by verify_n on the same stream, by events."""
    nbytes, count = SHAPES["c2"]
    buf = torch.empty(nbytes * count, dtype=torch.uint8, device="cuda")
    ck.fill_splitmix(buf, nbytes, nbytes, count, 0x5EED0001)
    sdt = torch.int64 if crc64 else torch.int32
    out, stored = torch.zeros(count, dtype=sdt, device="cuda"), torch.zeros(count, dtype=sdt, device="cuda")
    rep = torch.zeros(4, dtype=torch.int64).pin_memory()
    lst = torch.zeros(64, dtype=torch.int64).pin_memory()
    work = torch.empty(ck.verify_work_bytes(count), dtype=torch.uint8, device="cuda")
    batch = ck.batch64_strided if crc64 else ck.batch_strided
    verify = ck.verify64_device if crc64 else ck.verify_device
    batch(buf, nbytes, nbytes, count, stored, stream=st)  # the stored words: none is bad

    def alone():
        batch(buf, nbytes, nbytes, count, out, stream=st)

    def with_verify():
        batch(buf, nbytes, nbytes, count, out, stream=st)
        verify(out, stored, 8 if crc64 else 4, count, rep, lst, 64, work, stream=st)

    with_verify()
    torch.cuda.synchronize()
    assert list(rep.numpy().view(np.uint64)) == [0, (1 << 64) - 1, 0, count], rep
    res = {"shape": "verify_after_c2_batch", "crc": "crc64ecma" if crc64 else "crc32c", "nbytes": nbytes,
           "count": count, "tree": args.tree, "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}
    res.update(alternate({"batch": alone, "batch_verify": with_verify}))
    res["added_us"] = round((res["batch_verify"]["ms_mean"] - res["batch"]["ms_mean"]) * 1e3, 3)
    return res


def alternate(arms):
    """The §4.3 protocol over callables: --rounds alternations of --reps timed calls after --warmup each."""
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
    res = {}
    for name in arms:
        ms = np.asarray(times[name])
        res[name] = {"ms_mean": round(float(ms.mean()), 5), "ms_median": round(float(np.median(ms)), 5),
                     "round_means_ms": [round(m, 5) for m in means[name]],
                     "spread_ms": round(max(means[name]) - min(means[name]), 5)}
    return res


PARTS_SHAPES = {  # name: (parts, part MiB or None = seeded lengths of 1 to 16 MiB, destination delta)
    "1024x4MiB": (1024, 4, 0), "256x16MiB": (256, 16, 0), "64x64MiB": (64, 64, 0), "512xragged": (512, None, 0),
    "256x16MiB+9": (256, 16, 9),
}


def bench_parts(shape, what):
    """what: "copy" = arms (a) loop of copy_extend_device, (b) copy_parts, (c) copy_batch_iov, (d) copy_batch_strided
    over 64 KiB pieces + combine_series_device per part (uniform shapes), plus the part fold alone and, on the
    ragged shape, (b) with max_part_bytes = 1 GiB (the empty tasks); "pieces" = (b) at 32, 64 and 128 KiB pieces;
    "crc" = the CRC-only calls: loop of extend_device, batch_parts, batch_iov."""
    nparts, mib, delta = PARTS_SHAPES[shape]
    c64 = args.crc64
    if mib is None:
        lens = np.random.default_rng(0x9A27).integers(1 << 20, (16 << 20) + 1, nparts).astype(np.uint64)
    else:
        lens = np.full(nparts, mib << 20, np.uint64)
    total, cap = int(lens.sum()), int(lens.max())
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    src = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(total + 4096, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 4096 == 0 and dst.data_ptr() % 4096 == 0
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0x5EED0301)
    s0, d0 = 1, 1 + delta
    sp, dp = src.data_ptr() + s0, dst.data_ptr() + d0
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    iov = np.empty((nparts, 2), np.uint64)
    iov[:, 0] = np.uint64(sp) + offs
    iov[:, 1] = lens
    d_iov, d_dst = i64(iov), i64(np.uint64(dp) + offs)
    dt, wdt = (torch.int64, np.uint64) if c64 else (torch.int32, np.uint32)
    out = torch.zeros(nparts, dtype=dt, device="cuda")
    pieces_k = (32, 64, 128)
    ck.set_parts_piece(32 << 10)
    work = torch.empty(max(ck.parts_work_bytes(nparts, 1 << 30 if mib is None else cap, c64), 8), dtype=torch.uint8,
                       device="cuda")
    ck.set_parts_piece(0)
    wb = work.numel()
    copy_parts = ck.copy_parts64_device if c64 else ck.copy_parts_device
    batch_parts = ck.batch_parts64_device if c64 else ck.batch_parts_device
    hl, ho = [int(x) for x in lens], [int(x) for x in offs]
    op = [out.data_ptr() + k * out.element_size() for k in range(nparts)]

    def loop():
        for k in range(nparts):
            if c64:
                ck.copy_extend64_device(sp + ho[k], dp + ho[k], hl[k], op[k], stream=st)
            else:
                ck.copy_extend_device(sp + ho[k], dp + ho[k], hl[k], 0, op[k], stream=st)

    def crc_loop():
        for k in range(nparts):
            if c64:
                ck.extend64_device(sp + ho[k], hl[k], op[k], stream=st)
            else:
                ck.extend_device(sp + ho[k], hl[k], 0, op[k], stream=st)

    def parts(max_bytes=cap):
        copy_parts(d_iov, d_dst, nparts, max_bytes, out, work, wb, stream=st)

    def sized(kib):
        def f():
            ck.set_parts_piece(kib << 10)
            parts()
        return f

    def fold_only():
        ck._check(lib().photon_crc_util_parts_fold(int(c64), d_iov.data_ptr(), nparts, cap, 0, None, out.data_ptr(),
                                                   work.data_ptr(), st.cuda_stream))
    piece = 65536
    npiece = total // piece
    pcrc = torch.zeros(max(npiece, 1), dtype=dt, device="cuda")
    per = (mib << 20) // piece if mib else 0
    pp = pcrc.data_ptr()

    def hand_built():
        if c64:
            ck.copy_batch64_strided(sp, piece, dp, piece, piece, npiece, pcrc, stream=st)
            for k in range(nparts):
                ck.combine_series64_device(pp + k * per * out.element_size(), piece, per, op[k], stream=st)
        else:
            ck.copy_batch_strided(sp, piece, dp, piece, piece, npiece, pcrc, stream=st)
            for k in range(nparts):
                ck.combine_series_device(pp + k * per * out.element_size(), piece, per, op[k], stream=st)
    if what == "copy":
        arms = {"loop": loop, "parts": parts,
                "batch_iov": lambda: (ck.copy_batch64_iov if c64 else ck.copy_batch_iov)(d_iov, d_dst, nparts, out,
                                                                                         stream=st)}
        if mib is not None and delta % 16 == 0:
            arms["hand_built"] = hand_built
        if mib is None:
            arms["parts_cap_1GiB"] = lambda: parts(1 << 30)
    elif what == "pieces":
        arms = {f"parts_{k}KiB": sized(k) for k in pieces_k}
    else:
        arms = {"loop": crc_loop, "parts": lambda: batch_parts(d_iov, nparts, cap, out, work, wb, stream=st),
                "batch_iov": lambda: (ck.batch64_iov if c64 else ck.batch_iov)(d_iov, nparts, out, stream=st)}
    crcs = {}
    for name, fn in arms.items():  # same CRCs, the right bytes landed, before anything is timed
        dst.zero_()
        out.fill_(-1)
        work.fill_(0x5A)
        fn()
        torch.cuda.synchronize()
        if what != "crc":
            assert torch.equal(dst[d0:d0 + total], src[s0:s0 + total]), f"{name}: destination differs from the source"
            assert not bool(dst[:d0].any()) and not bool(dst[d0 + total:].any()), f"{name}: wrote outside"
        crcs[name] = out.cpu().numpy().view(wdt).copy()
    first = next(iter(crcs))
    for name in crcs:
        assert np.array_equal(crcs[first], crcs[name]), f"the CRCs of {first} and {name} differ"
    if what == "copy":
        arms["fold_only"] = fold_only  # the second launch of "parts" alone, over the workspace it left
        parts()
        fold_only()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy().view(wdt), crcs[first]), "fold_only differs"
    res = {"shape": "parts", "what": what, "crc": "crc64ecma" if c64 else "crc32c", "layout": shape, "nparts": nparts,
           "bytes": total, "src": "buf+1", "dst": f"dbuf+{d0}", "co_aligned": delta % 16 == 0,
           "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}
    res.update(alternate(arms))
    ck.set_parts_piece(0)
    gib = total / 2.0**30
    for name in arms:
        if name != "fold_only":
            res[name]["payload_GiBps_mean"] = round(gib / (res[name]["ms_mean"] * 1e-3), 1)
    if what != "pieces":
        b = res["parts"]["ms_mean"]
        for other in ("loop", "batch_iov"):
            o = res[other]
            res[f"margin_over_{other}_spread"] = round((o["ms_mean"] - b) / max(o["spread_ms"], 1e-9), 2)
            res[f"faster_3x_than_{other}"] = bool(o["ms_mean"] - b > 3 * o["spread_ms"])
        if "hand_built" in res:
            d = res["hand_built"]
            res["allowed_over_hand_built_ms"] = round(max(0.03 * d["ms_mean"], 3 * d["spread_ms"]), 5)
            res["not_slower_than_hand_built"] = bool(b - d["ms_mean"] <= res["allowed_over_hand_built_ms"])
        if "parts_cap_1GiB" in res:
            res["empty_tasks_ms"] = round(res["parts_cap_1GiB"]["ms_mean"] - b, 5)
    return res


PACKED_SHAPES = ["512xragged", "1024x4MiB", "256x16MiB", "2048xmixed"]


def bench_parts_packed(shape, c64):
    """copy_parts*_packed_device ("packed": max_part_bytes = ~0, max_total_bytes = the exact sum) against the
    calls that were here before it, in one process: "parts" = copy_parts*_device with the cap at the longest
    part, "parts_cap_1GiB" (ragged) = the same under a 1 GiB cap, "batch_iov" (mixed) = copy_batch*_iov;
    "plan_only" = the packed call's four plan launches alone (photon_crc_util_parts_packed_plan)."""
    if shape == "2048xmixed":  # log-uniform from 4 KiB to 32 MiB
        nparts = 2048
        u = np.random.default_rng(0x9A31).uniform(np.log(4096.0), np.log(float(32 << 20)), nparts)
        lens = np.minimum(np.exp(u).astype(np.uint64), np.uint64(32 << 20))
    else:
        nparts, mib, _ = PARTS_SHAPES[shape]
        if mib is None:
            lens = np.random.default_rng(0x9A27).integers(1 << 20, (16 << 20) + 1, nparts).astype(np.uint64)
        else:
            lens = np.full(nparts, mib << 20, np.uint64)
    total, cap = int(lens.sum()), int(lens.max())
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    src = torch.empty(total + 4096, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(total + 4096, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 4096 == 0 and dst.data_ptr() % 4096 == 0
    ck.fill_splitmix(src, src.numel(), src.numel(), 1, 0x5EED0301)
    s0 = d0 = 1
    sp, dp = src.data_ptr() + s0, dst.data_ptr() + d0
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    iov = np.empty((nparts, 2), np.uint64)
    iov[:, 0] = np.uint64(sp) + offs
    iov[:, 1] = lens
    d_iov, d_dst = i64(iov), i64(np.uint64(dp) + offs)
    dt, wdt = (torch.int64, np.uint64) if c64 else (torch.int32, np.uint32)
    out = torch.zeros(nparts, dtype=dt, device="cuda")
    report = torch.zeros(4, dtype=torch.int64, device="cuda")
    everything = (1 << 64) - 1
    ck.set_parts_piece(0)
    big = shape == "512xragged"
    work = torch.empty(max(ck.parts_work_bytes(nparts, 1 << 30 if big else cap, c64), 8), dtype=torch.uint8,
                       device="cuda")
    pwork = torch.empty(ck.parts_packed_work_bytes(nparts, total, c64), dtype=torch.uint8, device="cuda")
    copy_parts = ck.copy_parts64_device if c64 else ck.copy_parts_device
    copy_packed = ck.copy_parts64_packed_device if c64 else ck.copy_parts_packed_device

    def parts(max_bytes=cap):
        copy_parts(d_iov, d_dst, nparts, max_bytes, out, work, work.numel(), stream=st)

    def packed():
        copy_packed(d_iov, d_dst, nparts, everything, total, out, report, pwork, pwork.numel(), stream=st)

    def plan_only():
        ck._check(lib().photon_crc_util_parts_packed_plan(int(c64), d_iov.data_ptr(), nparts, everything, total,
                                                          report.data_ptr(), pwork.data_ptr(), st.cuda_stream))
    arms = {"parts": parts, "packed": packed}
    if big:
        arms["parts_cap_1GiB"] = lambda: parts(1 << 30)
    if shape == "2048xmixed":
        arms["batch_iov"] = lambda: (ck.copy_batch64_iov if c64 else ck.copy_batch_iov)(d_iov, d_dst, nparts, out,
                                                                                        stream=st)
    crcs = {}
    for name, fn in arms.items():  # same CRCs, the right bytes landed, before anything is timed
        dst.zero_()
        out.fill_(-1)
        work.fill_(0x5A)
        pwork.fill_(0x5A)
        fn()
        torch.cuda.synchronize()
        assert torch.equal(dst[d0:d0 + total], src[s0:s0 + total]), f"{name}: destination differs from the source"
        assert not bool(dst[:d0].any()) and not bool(dst[d0 + total:].any()), f"{name}: wrote outside"
        crcs[name] = out.cpu().numpy().view(wdt).copy()
    for name in crcs:
        assert np.array_equal(crcs["parts"], crcs[name]), f"the CRCs of parts and {name} differ"
    rep = [int(x) for x in report.cpu().numpy().view(np.uint64)]
    assert rep[0] == 0 and rep[2] == total and rep[1] <= rep[3], rep
    arms["plan_only"] = plan_only
    res = {"shape": "parts_packed", "crc": "crc64ecma" if c64 else "crc32c", "layout": shape, "nparts": nparts,
           "bytes": total, "longest": cap, "tasks": rep[1], "slots": rep[3], "packed_work_bytes": pwork.numel(),
           "parts_work_bytes": ck.parts_work_bytes(nparts, cap, c64), "src": "buf+1", "dst": "dbuf+1",
           "rounds": args.rounds, "reps": args.reps, "warmup": args.warmup}
    res.update(alternate(arms))
    gib = total / 2.0**30
    for name in arms:
        if name != "plan_only":
            res[name]["payload_GiBps_mean"] = round(gib / (res[name]["ms_mean"] * 1e-3), 1)
    e = res["packed"]["ms_mean"]
    if big:
        o = res["parts_cap_1GiB"]
        res["margin_over_parts_cap_1GiB_spread"] = round((o["ms_mean"] - e) / max(o["spread_ms"], 1e-9), 2)
        res["faster_3x_than_parts_cap_1GiB"] = bool(o["ms_mean"] - e > 3 * o["spread_ms"])
    b = res["parts"]
    res["packed_minus_parts_ms"] = round(e - b["ms_mean"], 5)
    if shape in ("1024x4MiB", "256x16MiB"):
        res["allowed_over_parts_ms"] = round(max(0.03 * b["ms_mean"], 3 * b["spread_ms"]), 5)
        res["not_slower_than_parts"] = bool(e - b["ms_mean"] <= res["allowed_over_parts_ms"])
    return res


if args.parts_packed:
    for shape in PACKED_SHAPES:
        if args.shapes != "c2,c3" and shape not in args.shapes.split(","):
            continue
        for c64 in (False, True):
            line = json.dumps(bench_parts_packed(shape, c64))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    sys.exit(0)

if args.parts:
    plan = [(s, "copy") for s in PARTS_SHAPES] + [("1024x4MiB", "pieces"), ("256x16MiB", "pieces"),
                                                  ("256x16MiB", "crc")]
    for shape, what in plan:
        if args.shapes != "c2,c3" and shape not in args.shapes.split(","):
            continue
        line = json.dumps(bench_parts(shape, what))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    sys.exit(0)

if args.verify:
    plan = [(bench_verify, (c64, count, bad, int(tile))) for tile in args.tiles.split(",") for c64 in (False, True)
            for count, bad in VERIFY_ROWS]
    if args.tiles == "0":
        plan += [(bench_verify_after_batch, (c64,)) for c64 in (False, True)]
    for fn, a in plan:
        line = json.dumps(fn(*a))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    sys.exit(0)

if args.scan:
    shapes = [tuple(int(x) for x in sh.split("x")) for sh in args.scan_shapes.split(",")] if args.scan_shapes \
        else SCAN_SHAPES
    for tile in args.tiles.split(","):
        for c64 in (False, True):
            for nobj, per in shapes:
                line = json.dumps(bench_scan(c64, nobj, per, int(tile)))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")
    sys.exit(0)

if args.fold:
    for c64 in (False, True):
        for nobj, per in FOLD_SHAPES:
            line = json.dumps(bench_fold(c64, nobj, per))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
    sys.exit(0)

if args.long:
    sizes = [int(x) for x in args.sizes.split(",")]
    for mib, delta in [(m, 0) for m in sizes] + [(max(sizes), 9)]:
        line = json.dumps(bench_long(mib, delta))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    sys.exit(0)

if args.iov or args.iov_seg or args.iov_seg2:
    line = json.dumps(bench_iov_seg2() if args.iov_seg2 else bench_iov_seg() if args.iov_seg else bench_iov())
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

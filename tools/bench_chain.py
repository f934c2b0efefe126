"""Throughput of the trajectory step (vslam_chain_dev) on the lists of the 256-frame workload: tools/bench_pose.py's chain
(detect -> describe -> match -> epipolar -> pose on 256 synthetic 1080p frames) leaves 255 poses, inlier lists, point rows and
front bits on the device, and the trajectory step runs on them as they are.  Those lists hold a few records of a capacity of
65536 each, so that case times an almost empty grid; a second case runs the same call with every list full: planted
two-camera lists (tools/bench_epipolar.py's data) of 255 x 65536 records, 16.7 M in all, every record with the indices i, i, so
that every record in front is linked; a third times the sequential walk at the largest pair count, 65535 pairs of 64 records
built directly as buffers.  HIP events around each call, 2 warm-up calls, the median of --runs calls; every kernel alone
through the library's timing hook.  The rate is match records per second: the records considered, sum over pairs of min(count,
capacity), over the kernel's time.  A first measurement, not a pass criterion.

  python tools/bench_chain.py [--runs 10] [--frames 256] [--out profiles/chain_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_epipolar import timed
from tools.bench_pose import K, hooked, planted_lists, workload_lists
from visualslam_amd import capi

DEV = "cuda:0"
KERNELS = ("k_chain_link", "k_chain_ratio", "k_chain_median", "k_chain_walk", "k_chain_map")


def pose_outputs(ctx, models, lists, counts, qpts, tpts):
    n, cap = lists.shape[0], lists.shape[1]
    poses = torch.zeros((n, 28), dtype=torch.int32, device=DEV)
    points = torch.zeros((n, cap, 3), dtype=torch.float64, device=DEV)
    bits = torch.zeros((n, (cap + 63) // 64), dtype=torch.int64, device=DEV)
    ctx.pose(models, lists, counts, qpts, tpts, K, n_pairs=n, poses=poses, points=points, front_bits=bits)
    torch.cuda.synchronize()
    return poses, lists, counts, points, bits


def measure(ctx, label, poses, lists, counts, points, bits, point_cap, runs, min_links=16):
    n, cap = lists.shape[0], lists.shape[1]
    chain = torch.zeros((n, 44), dtype=torch.int32, device=DEV)
    world = torch.zeros((n, cap, 3), dtype=torch.float64, device=DEV)
    call = lambda: ctx.chain(poses, lists, counts, points, bits, point_cap, min_links, n_pairs=n, chain=chain, map=world)
    med, lo, hi = timed(call, runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    rate = lambda ms: round(records / (ms * 1e-3), 1) if ms > 0 and records else None
    out = dict(case=label, pairs=n, capacity=cap, point_cap=point_cap, records=records, runs=runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4),
               call_ms_max=round(hi, 4), records_per_s_call=rate(med))
    for k in KERNELS:
        ms = hooked(ctx, call, k, runs)
        out[k + "_ms"] = round(ms, 4)
        out["records_per_s_" + k[2:]] = rate(ms)
    hc = chain.cpu().numpy().view(capi.CHAIN_DTYPE).reshape(-1)
    out.update(valid_pairs=int(hc["valid"].sum()), linked_pairs=int(hc["linked"].sum()), usable_links=int(hc["n_links"].sum()),
               segments=int(len(np.unique(hc["segment"]))))
    return out


def walk_lists(pairs, m):
    """`pairs` pairs of m records built directly as buffers: random rotations, unit translations, points in front, indices i, i."""
    rng = np.random.default_rng(pairs)
    axis = rng.normal(size=(pairs, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(-0.1, 0.1, pairs)
    A = np.zeros((pairs, 3, 3))
    A[:, 0, 1], A[:, 0, 2], A[:, 1, 0], A[:, 1, 2], A[:, 2, 0], A[:, 2, 1] = -axis[:, 2], axis[:, 1], axis[:, 2], -axis[:, 0], -axis[:, 1], axis[:, 0]
    R = np.eye(3) + np.sin(ang)[:, None, None] * A + (1 - np.cos(ang))[:, None, None] * (A @ A)
    t = rng.normal(size=(pairs, 3))
    poses = np.zeros(pairs, capi.POSE_DTYPE)
    poses["R"], poses["t"], poses["valid"], poses["n_matches"] = R.reshape(pairs, 9), t / np.linalg.norm(t, axis=1, keepdims=True), 1, m
    mt = np.zeros((pairs, m), capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(m)
    pts = rng.uniform(-5, 5, (pairs, m, 3)) + np.array([0, 0, 9.0])
    bits = np.full((pairs, (m + 63) // 64), -1, np.int64)
    dev = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape)).to(DEV)
    return (dev(poses, (pairs, 28), np.int32), dev(mt, (pairs, m, 3), np.int32), torch.full((pairs,), m, dtype=torch.int32, device=DEV),
            dev(pts, (pairs, m, 3), np.float64), dev(bits, bits.shape, np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "intrinsics": K, "min_links": 16, "cases": []}

    def add(case):
        res["cases"].append(case)
        print(json.dumps(case), flush=True)

    args, info = workload_lists(ctx, a.frames, a.rows, a.cols, a.octaves)
    res["workload"] = info
    print(json.dumps(info), flush=True)
    add(measure(ctx, "workload inlier lists", *pose_outputs(ctx, *args), info["oriented_cap"], a.runs))
    del args
    add(measure(ctx, "planted lists, every list full", *pose_outputs(ctx, *planted_lists(ctx, 255, 65536)), 65536, a.runs))
    add(measure(ctx, "65535 pairs of 64 records", *walk_lists(65535, 64), 64, a.runs))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

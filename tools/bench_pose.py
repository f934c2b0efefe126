"""Throughput of the relative-pose step (vslam_pose_dev) on the match lists of the 256-frame workload: bench.py's 256
synthetic 1080p frames (every second one the noise frame, which populates the orientation stage) go through detect -> describe
-> match (255 consecutive pairs) -> epipolar (512 hypotheses) on the device, and the pose step runs on the inlier lists that
leaves behind.  Those lists hold a few records of a capacity of 65536 each, so that case times an almost empty grid; a second
case runs the same call with every list full: planted two-camera lists (tools/bench_epipolar.py's data) of 65536 records per
pair, 16.7 M records in all, the model of each pair found from its first 2048.  HIP events around each call, 2 warm-up
calls, the median of --runs calls; k_pose_vote and k_pose_points alone through the library's timing hook.  The rate is match
records per second: the records considered, sum over pairs of min(count, capacity), over the kernel's time.  A first
measurement, not a pass criterion.

  python tools/bench_pose.py [--runs 10] [--frames 256] [--out profiles/pose_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_epipolar import planted, timed
from visualslam_amd import capi, synth

DEV = "cuda:0"
K = (800.0, 800.0, 960.0, 540.0)


def hooked(ctx, call, name, runs):
    ctx.kernel_timing_enable(name)
    for _ in range(runs):
        call()
    launches, ms = ctx.kernel_timing_read()
    ctx.kernel_timing_enable(None)
    return ms / max(launches, 1)


def measure(ctx, label, models, lists, counts, qpts, tpts, runs):
    n, cap = lists.shape[0], lists.shape[1]
    poses = torch.zeros((n, 28), dtype=torch.int32, device=DEV)
    points = torch.zeros((n, cap, 3), dtype=torch.float64, device=DEV)
    bits = torch.zeros((n, (cap + 63) // 64), dtype=torch.int64, device=DEV)
    call = lambda: ctx.pose(models, lists, counts, qpts, tpts, K, n_pairs=n, poses=poses, points=points, front_bits=bits)
    med, lo, hi = timed(call, runs)
    vote_ms, points_ms = hooked(ctx, call, "k_pose_vote", runs), hooked(ctx, call, "k_pose_points", runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    hp = poses.cpu().numpy().view(capi.POSE_DTYPE).reshape(-1)
    rate = lambda ms: round(records / (ms * 1e-3), 1) if ms > 0 and records else None
    return dict(case=label, pairs=n, capacity=cap, records=records, runs=runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4),
                call_ms_max=round(hi, 4), k_pose_vote_ms=round(vote_ms, 4), k_pose_points_ms=round(points_ms, 4),
                records_per_s_vote=rate(vote_ms), records_per_s_points=rate(points_ms), records_per_s_call=rate(med),
                pairs_with_a_pose=int((hp["best"] >= 0).sum()), records_in_front=int(hp["n_front"].sum()))


def workload_lists(ctx, frames_n, rows, cols, octaves, full_lists=False):
    """detect -> describe -> match -> epipolar on the synthetic frames -> (models, inliers, inlier counts, points of the pairs);
    full_lists: the match lists epipolar read in place of its inlier lists (tools/bench_refit.py)."""
    frames = synth.frames_torch(frames_n, rows, cols, stream_id=0, device=DEV, noise_every=2)
    p = capi.default_params(rows, cols, n_octaves=octaves, localize=1, orient=1)
    L = capi.batch_layout(p)
    n, cap = frames_n, p.oriented_cap
    o = dict(pyramid=torch.empty((n, L.pyramid_frame_bytes), dtype=torch.uint8, device=DEV),
             dog_points=torch.zeros((n, p.dog_cap, 6), dtype=torch.int32, device=DEV), dog_counts=torch.zeros(n, dtype=torch.int32, device=DEV),
             oriented_points=torch.zeros((n, cap, 6), dtype=torch.int32, device=DEV), oriented_counts=torch.zeros(n, dtype=torch.int32, device=DEV),
             descriptors=torch.zeros((n, cap, 128), dtype=torch.float32, device=DEV),
             descriptor_defined=torch.zeros((n, cap), dtype=torch.uint8, device=DEV))
    p.do_harris = 0
    ctx.detect_batch(p, frames, **o)
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    pairs = n - 1
    matches = torch.zeros((pairs, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    ctx.match(capi.desc_sets(d[:-1], c[:-1], df[:-1]), capi.desc_sets(d[1:], c[1:], df[1:]), pairs, 0.64, False, matches=matches, match_counts=counts)
    models = torch.zeros((pairs, 22), dtype=torch.int32, device=DEV)
    inliers = torch.zeros((pairs, cap, 3), dtype=torch.int32, device=DEV)
    icounts = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:-1], pts[1:], pairs, 512, 1, 4.0, models=models, inliers=inliers, inlier_counts=icounts)
    torch.cuda.synchronize()
    info = dict(frames=n, rows=rows, cols=cols, octaves=octaves, oriented_cap=int(cap), oriented_points=int(c.sum()), accepted_matches=int(counts.sum()),
                inlier_matches=int(icounts.sum()))
    return ((models, matches, counts, pts[:-1], pts[1:]) if full_lists else (models, inliers, icounts, pts[:-1], pts[1:])), info


def planted_lists(ctx, pairs, m, model_from=2048):
    mt, qp, tp = planted(np.random.default_rng(pairs + m), pairs, m)
    dev = lambda a, k: torch.from_numpy(a.view(np.int32).reshape(pairs, m, k)).to(DEV)
    lists, counts, qpts, tpts = dev(mt, 3), torch.full((pairs,), m, dtype=torch.int32, device=DEV), dev(qp, 6), dev(tp, 6)
    models = torch.zeros((pairs, 22), dtype=torch.int32, device=DEV)
    first = torch.full((pairs,), min(m, model_from), dtype=torch.int32, device=DEV)  # (every record of a pair has the same geometry)
    ctx.epipolar(lists, first, qpts, tpts, pairs, 512, 1, 4.0, models=models)
    torch.cuda.synchronize()
    return models, lists, counts, qpts, tpts


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
    res = {"device": torch.cuda.get_device_name(0), "intrinsics": K, "cases": []}
    args, info = workload_lists(ctx, a.frames, a.rows, a.cols, a.octaves)
    res["workload"] = info
    print(json.dumps(info), flush=True)
    res["cases"].append(measure(ctx, "workload inlier lists", *args, a.runs))
    print(json.dumps(res["cases"][-1]), flush=True)
    del args
    res["cases"].append(measure(ctx, "planted lists, every list full", *planted_lists(ctx, 255, 65536), a.runs))
    print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

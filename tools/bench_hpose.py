"""Throughput of pose from homography (vslam_hpose_dev) on two sets of lists: the inlier lists of the 256-frame workload
(tools/bench_pose.py's: detect -> describe -> match -> epipolar on the device; a few records of a capacity of 65536 each, so an
almost empty grid), and planted lists with every list full: 255 pairs of 65536 records on the plane Z = 8 + 0.3 X - 0.2 Y seen by
the planted cameras (tools/bench_epipolar.py's, 30 % of the train points noise), 16.7 M records in all, the homography and the
fundamental matrix of each pair found from its first 2048.  Every pair with an H is selected (only_degenerate = 0).  HIP events
around each call, 2 warm-up calls, the median of --runs calls; k_hpose_vote and k_hpose_points alone through the library's
timing hook, and in the same run on the same lists k_pose_vote (vslam_pose_dev) and k_hom_score at ONE hypothesis
(vslam_homography_dev) and at 512: per record the vote is one transfer test plus two cheirality evaluations, so the expectation
to confirm or refute is k_pose_vote's time plus a 1/512 share of k_hom_score's at 512 hypotheses (k_hom_score gives a lane to a
hypothesis, so at one hypothesis it runs one lane in 256 and its time says nothing about a transfer test's cost; it is reported
all the same).  A first measurement, not a pass criterion.

  python tools/bench_hpose.py [--runs 10] [--frames 256] [--out profiles/hpose_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_epipolar import timed
from tools.bench_pose import hooked, workload_lists
from visualslam_amd import capi

DEV = "cuda:0"
K = (800.0, 800.0, 960.0, 540.0)


def planted_plane(rng, pairs, m, width=1920, height=1080):
    """tools/bench_epipolar.py's planted lists with every point on the plane Z = 8 + 0.3 X - 0.2 Y."""
    X = np.stack([rng.uniform(-6, 6, (pairs, m)), rng.uniform(-3.5, 3.5, (pairs, m)), np.zeros((pairs, m))], axis=-1)
    X[..., 2] = 8 + 0.3 * X[..., 0] - 0.2 * X[..., 1]
    c, s = np.cos(0.05), np.sin(0.05)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    Y = X @ R.T + np.array([-0.5, 0, 0])
    proj = lambda P: np.stack([800 * P[..., 0] / P[..., 2] + width / 2, 800 * P[..., 1] / P[..., 2] + height / 2], axis=-1)
    q, t = proj(X), proj(Y)
    noise = np.stack([rng.uniform(0, width, (pairs, m)), rng.uniform(0, height, (pairs, m))], axis=-1)
    t = np.where(rng.random((pairs, m, 1)) < 0.3, noise, t)
    pts = []
    for xy in (q, t):
        p = np.zeros((pairs, m), capi.POINT_DTYPE)
        p["col"], p["row"], p["octave"] = np.rint(xy[..., 0]), np.rint(xy[..., 1]), 1
        pts.append(p)
    mt = np.zeros((pairs, m), capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(m)
    return mt, pts[0], pts[1]


def planted_lists(ctx, pairs, m, model_from=2048):
    mt, qp, tp = planted_plane(np.random.default_rng(pairs + m), pairs, m)
    dev = lambda a, k: torch.from_numpy(a.view(np.int32).reshape(pairs, m, k)).to(DEV)
    lists, counts, qpts, tpts = dev(mt, 3), torch.full((pairs,), m, dtype=torch.int32, device=DEV), dev(qp, 6), dev(tp, 6)
    first = torch.full((pairs,), min(m, model_from), dtype=torch.int32, device=DEV)  # (every record of a pair has the same geometry)
    return models_of(ctx, lists, first, qpts, tpts) + (lists, counts, qpts, tpts)


def models_of(ctx, lists, counts, qpts, tpts):
    n = lists.shape[0]
    emodels = torch.zeros((n, 22), dtype=torch.int32, device=DEV)
    hmodels = torch.zeros((n, 42), dtype=torch.int32, device=DEV)
    ctx.epipolar(lists, counts, qpts, tpts, n, 512, 1, 4.0, models=emodels)
    ctx.homography(lists, counts, qpts, tpts, n, 512, 1, 4.0, epipolar_models=emodels, models=hmodels)
    torch.cuda.synchronize()
    return emodels, hmodels


def measure(ctx, label, emodels, hmodels, lists, counts, qpts, tpts, runs):
    n, cap = lists.shape[0], lists.shape[1]
    poses = torch.zeros((n, 28), dtype=torch.int32, device=DEV)
    info = torch.zeros((n, 36), dtype=torch.int32, device=DEV)
    points = torch.zeros((n, cap, 3), dtype=torch.float64, device=DEV)
    bits = torch.zeros((n, (cap + 63) // 64), dtype=torch.int64, device=DEV)
    call = lambda: ctx.hpose(hmodels, lists, counts, qpts, tpts, K, only_degenerate=False, n_pairs=n, poses=poses, info=info, points=points, front_bits=bits)
    med, lo, hi = timed(call, runs)
    own = {k: hooked(ctx, call, k, runs) for k in ("k_hpose_candidates", "k_hpose_vote", "k_hpose_select", "k_hpose_points", "k_epi_coords")}
    hi_ = info.cpu().numpy().view(capi.HPOSE_DTYPE).reshape(-1)
    hp = poses.cpu().numpy().view(capi.POSE_DTYPE).reshape(-1)
    # the two kernels the vote is made of, on the same lists in the same run
    pose_call = lambda: ctx.pose(emodels, lists, counts, qpts, tpts, K, n_pairs=n, poses=poses, points=points, front_bits=bits)
    pose_vote = hooked(ctx, pose_call, "k_pose_vote", runs)
    scratch = torch.zeros((n, 42), dtype=torch.int32, device=DEV)
    hom_call = lambda: ctx.homography(lists, counts, qpts, tpts, n, 1, 1, 4.0, models=scratch)
    hom_score = hooked(ctx, hom_call, "k_hom_score", runs)
    hom_call512 = lambda: ctx.homography(lists, counts, qpts, tpts, n, 512, 1, 4.0, models=scratch)
    hom_score512 = hooked(ctx, hom_call512, "k_hom_score", max(runs // 3, 1))   # (one lane per hypothesis: one hypothesis leaves 255 of 256 lanes idle)
    share = hom_score512 / 512
    posed = (hp["best"] >= 0) & (hi_["kind"] == capi.HPOSE_PLANE)                 # (a pair that is not selected keeps the caller's pose record)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    rate = lambda ms: round(records / (ms * 1e-3), 1) if ms > 0 and records else None
    vote = own["k_hpose_vote"]
    return dict(case=label, pairs=n, capacity=cap, records=records, runs=runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4),
                call_ms_max=round(hi, 4), **{k + "_ms": round(v, 4) for k, v in own.items()}, k_pose_vote_ms=round(pose_vote, 4),
                k_hom_score_1_hypothesis_ms=round(hom_score, 4), k_hom_score_512_hypotheses_ms=round(hom_score512, 4),
                k_hom_score_512th_share_ms=round(share, 5), vote_over_k_pose_vote=round(vote / pose_vote, 3) if pose_vote > 0 else None,
                vote_over_expectation=round(vote / (pose_vote + share), 3) if pose_vote + share > 0 else None,
                records_per_s_vote=rate(vote), records_per_s_call=rate(med),
                # the vote reads one 32-byte coordinate record per match record: its share of the HBM peak of 8 TB/s
                vote_read_fraction_of_hbm_peak=round(records * 32 / (vote * 1e-3) / 8e12, 3) if vote > 0 else None,
                kinds=[int((hi_["kind"] == k).sum()) for k in (0, 1, 2)], ambiguous=int(hi_["ambiguous"].sum()),
                pairs_with_a_pose=int(posed.sum()), records_supported=int(hi_["n_support"].sum()), records_in_front=int(hp["n_front"][posed].sum()))


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
    res = {"device": torch.cuda.get_device_name(0), "boxes": 1, "intrinsics": K, "cases": []}
    (emodels, inliers, icounts, qpts, tpts), info = workload_lists(ctx, a.frames, a.rows, a.cols, a.octaves)
    res["workload"] = info
    print(json.dumps(info), flush=True)
    hmodels = models_of(ctx, inliers, icounts, qpts, tpts)[1]
    res["cases"].append(measure(ctx, "workload inlier lists", emodels, hmodels, inliers, icounts, qpts, tpts, a.runs))
    print(json.dumps(res["cases"][-1]), flush=True)
    del emodels, hmodels, inliers, icounts, qpts, tpts
    res["cases"].append(measure(ctx, "planted plane lists, every list full", *planted_lists(ctx, 255, 65536), a.runs))
    print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

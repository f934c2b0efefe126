"""Throughput of the two-view geometry step (vslam_epipolar_dev): 255 pairs x 2 k matches x 512 hypotheses (a batch of
consecutive frames) and one pair x 16 k matches x 2048 hypotheses, on planted two-camera data with 30 % wrong matches.  HIP
events around each call, 2 warm-up calls, the median of --runs calls; the hot kernel alone through the library's timing hook.
The rate is Sampson tests per second, pairs x hypotheses x matches / time.  One test is 33 f64 operations, none of them fused
(17 multiplications, 16 additions; include/vslam.h), so the f64 vector peak of 78.6 TF - which counts a fused multiply-add as
two - allows 39.3e12 / 33 = 1.19e12 tests per second.  A record, not a pass criterion.

  python tools/bench_epipolar.py [--runs 10] [--out profiles/epipolar_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from visualslam_amd import capi

F64_PEAK_TF = 78.6
OPS_PER_TEST = 33
PEAK_TESTS = F64_PEAK_TF / 2 * 1e12 / OPS_PER_TEST
DEV = "cuda:0"


def timed(fn, runs):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def planted(rng, pairs, m, width=1920, height=1080):
    """Matches of `pairs` two-camera scenes (f = 800, 0.05 rad yaw, baseline 0.5), octave 1 lattice, 30 % of the train points noise."""
    X = np.stack([rng.uniform(-6, 6, (pairs, m)), rng.uniform(-3.5, 3.5, (pairs, m)), rng.uniform(4, 12, (pairs, m))], axis=-1)
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


def case(ctx, pairs, m, H, runs):
    mt, qp, tp = planted(np.random.default_rng(pairs + m), pairs, m)
    dev = lambda a, k: torch.from_numpy(a.view(np.int32).reshape(pairs, m, k)).to(DEV)
    d_in = (dev(mt, 3), torch.full((pairs,), m, dtype=torch.int32, device=DEV), dev(qp, 6), dev(tp, 6))
    models = torch.zeros((pairs, 22), dtype=torch.int32, device=DEV)
    inliers = torch.zeros((pairs, m, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    call = lambda: ctx.epipolar(*d_in, n_pairs=pairs, n_hypotheses=H, seed=1, max_dist2=4.0, models=models, inliers=inliers, inlier_counts=counts)
    med, lo, hi = timed(call, runs)
    ctx.kernel_timing_enable("k_epi_score")
    for _ in range(runs):
        call()
    launches, score_ms = ctx.kernel_timing_read()
    ctx.kernel_timing_enable(None)
    score_ms /= max(launches, 1)
    tests = float(pairs) * H * m
    mod = models.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1)
    return dict(pairs=pairs, matches=m, hypotheses=H, runs=runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4), call_ms_max=round(hi, 4),
                k_epi_score_ms=round(score_ms, 4), sampson_tests=tests, tests_per_s_call=round(tests / (med * 1e-3), 1),
                tests_per_s_kernel=round(tests / (score_ms * 1e-3), 1) if score_ms > 0 else None,
                kernel_of_f64_vector_peak=round(tests / (score_ms * 1e-3) / PEAK_TESTS, 3) if score_ms > 0 else None,
                mean_inlier_fraction=round(float(mod["n_inliers"].mean()) / m, 3), mean_valid_fraction=round(float(mod["n_valid"].mean()) / H, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "f64_vector_peak_tflops": F64_PEAK_TF, "f64_ops_per_test": OPS_PER_TEST,
           "peak_tests_per_s": PEAK_TESTS, "bound": "compute (f64 VALU): the records of a pair are read once per 256 hypotheses, from LDS", "cases": []}
    for pairs, m, H in ((255, 2048, 512), (1, 16384, 2048)):
        res["cases"].append(case(ctx, pairs, m, H, a.runs))
        print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

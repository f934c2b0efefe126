"""Guided matching (vslam_match_guided_dev) against the matcher (vslam_match_dev) on the same sets in the same run: per launch,
k_match_guided against k_match_nn2 through the library's kernel timing hook (HIP events around the launch), and the whole call of
each with HIP events around it.  One-pair calls at 1 k / 4 k / 16 k / 64 k rows and 255 pairs at 2 k rows; the points are a
planted two-camera scene (tests/epiref.py's cameras) and F the exact fundamental matrix of those cameras, so the band holds
under 1 % of the (query, train) pairs, as it does on matched frames.  2 warm-up calls, the median of --runs calls.

  python tools/bench_guided.py [--runs 10] [--out profiles/guided_bench.json]
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

DEV = "cuda:0"


def planted_points(rng, n, width=1920, height=1080, f=800.0, yaw=0.05, baseline=0.5):
    """n scene points seen by two cameras -> (query points, train points) int32 [n, 6] at octaves 0 .. 2, and the exact F of the pair."""
    K = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1.0]])
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.array([-baseline, 0, 0])
    X = np.stack([rng.uniform(-4, 4, n), rng.uniform(-2.5, 2.5, n), rng.uniform(6, 12, n)], axis=1)
    a, b = X @ K.T, (X @ R.T + t) @ K.T
    a, b = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    F /= np.linalg.norm(F)
    octave = rng.integers(0, 3, n)
    pts = []
    for xy in (a, b):
        p = np.zeros((n, 6), np.int32)
        pitch = 2.0 ** (octave - 1)
        p[:, 0], p[:, 1], p[:, 4], p[:, 5] = np.rint(xy[:, 1] / pitch), np.rint(xy[:, 0] / pitch), octave, 1
        pts.append(p)
    return pts[0], pts[1][rng.permutation(n)], F


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
    return statistics.median(ms)


def kernel_ms(ctx, name, fn, runs, launches=1):
    """Median time of the launches of kernel `name` over `runs` calls of fn (`launches` per call, summed)."""
    for _ in range(2):
        fn()
    ms = []
    ctx.kernel_timing_enable(name)
    for _ in range(runs):
        fn()
        n, total = ctx.kernel_timing_read()
        assert n == launches, (name, n)
        ms.append(total)
    ctx.kernel_timing_enable(None)
    return statistics.median(ms)


def case(ctx, pairs, rows, runs):
    rng = np.random.default_rng(rows + pairs)
    g = torch.Generator(device=DEV).manual_seed(rows + pairs)
    d = torch.rand((pairs + 1, rows, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((pairs + 1,), rows, dtype=torch.int32, device=DEV)
    qp, tp, F = planted_points(rng, rows)
    qpts = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(qp, (pairs, rows, 6)))).to(DEV)
    tpts = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(tp, (pairs, rows, 6)))).to(DEV)
    model = np.zeros(pairs, capi.EPIPOLAR_DTYPE)
    model["F"] = F.reshape(9)
    models = torch.from_numpy(model.view(np.int32).reshape(pairs, 22)).to(DEV)
    nn = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    matches = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    mc = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:pairs], counts, None, qpts), capi.desc_sets(d[1:], counts[1:], None, tpts)
    plain = lambda: ctx.match(Q, T, pairs, 0.64, False, nn=nn, matches=matches, match_counts=mc)
    guided = lambda: ctx.match_guided(Q, T, models, pairs, 0.64, float("inf"), 4.0, False, nn=nn, matches=matches, match_counts=mc)
    out = dict(pairs=pairs, rows=rows, runs=runs)
    out["k_match_nn2_ms"] = round(kernel_ms(ctx, "k_match_nn2", plain, runs), 4)
    out["k_match_guided_ms"] = round(kernel_ms(ctx, "k_match_guided", guided, runs), 4)
    out["kernel_ratio"] = round(out["k_match_guided_ms"] / out["k_match_nn2_ms"], 3)
    out["match_call_ms"] = round(timed(plain, runs), 4)
    plain_accepted = int(mc.sum())
    out["guided_call_ms"] = round(timed(guided, runs), 4)
    out["call_ratio"] = round(out["guided_call_ms"] / out["match_call_ms"], 3)
    found = (nn.view(pairs * rows, 3)[:, 0] >= 0).sum()
    out.update(accepted_unguided=plain_accepted, accepted_guided=int(mc.sum()), queries_with_a_candidate=int(found))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "max_dist2": 4.0, "cases": []}
    for pairs, rows in ((1, 1024), (1, 4096), (1, 16384), (1, 65536), (255, 2048)):
        res["cases"].append(case(ctx, pairs, rows, a.runs))
        print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

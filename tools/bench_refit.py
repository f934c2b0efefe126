"""Throughput of the least-squares refit (vslam_refit_dev) on the match lists of the 256-frame workload and on full planted
lists: the two cases of tools/bench_pose.py, with the FULL match lists (the refit computes membership itself) and the models
vslam_epipolar_dev found.  HIP events around each call, 2 warm-up calls, the median of --runs calls; every kernel of the stage
alone through the library's timing hook: one call per reading, the time per launch, the median of --runs readings.  The
kernel readings come from calls with rounds = 1: there no pair has stopped before a launch (a stopped pair's workgroups leave
at once, so the later launches of a longer call read fewer records), and each launch of the three streaming kernels reads
every considered record once, 32 bytes: their time is set against that floor at the 8 TB/s peak of the device.  No target is
set - there is no earlier refit to compare with.

  python tools/bench_refit.py [--runs 10] [--rounds 4] [--frames 256] [--out profiles/refit_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_epipolar import timed
from tools.bench_pose import planted_lists, workload_lists
from visualslam_amd import capi

DEV = "cuda:0"
PEAK_BYTES_PER_S = 8.0e12
STREAMING = ("k_refit_count", "k_refit_dist", "k_refit_moments")
PER_PAIR = ("k_refit_init", "k_refit_begin", "k_refit_scale", "k_refit_solve")


def per_launch(ctx, call, name, runs):
    """Median over `runs` calls of the hook's time per launch of kernel `name`, ms."""
    ctx.kernel_timing_enable(name)
    vals = []
    for _ in range(runs):
        call()
        launches, ms = ctx.kernel_timing_read()
        vals.append(ms / max(launches, 1))
    ctx.kernel_timing_enable(None)
    return statistics.median(vals)


def measure(ctx, label, models, lists, counts, qpts, tpts, runs, rounds):
    n, cap = lists.shape[0], lists.shape[1]
    out = torch.zeros((n, 22), dtype=torch.int32, device=DEV)
    info = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
    call = lambda: ctx.refit(models, lists, counts, qpts, tpts, n_pairs=n, rounds=rounds, max_dist2=4.0, models=out, info=info)
    med, lo, hi = timed(call, runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    hi_ = info.cpu().numpy().view(capi.REFIT_DTYPE).reshape(-1)
    floor_ms = records * 32 / PEAK_BYTES_PER_S * 1e3
    res = dict(case=label, pairs=n, capacity=cap, records=records, rounds=rounds, runs=runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4),
               call_ms_max=round(hi, 4), floor_ms_per_pass_at_8TBps=round(floor_ms, 5), stops={str(s): int((hi_["stop"] == s).sum()) for s in range(6)},
               inliers_before=int(hi_["n_before"].sum()), inliers_after=int(hi_["n_after"].sum()), rounds_accepted=int(hi_["accepted"].sum()), kernels_note="calls with rounds = 1", kernels={})
    one_round = lambda: ctx.refit(models, lists, counts, qpts, tpts, n_pairs=n, rounds=1, max_dist2=4.0, models=out, info=info)
    for name in STREAMING + PER_PAIR:
        ms = per_launch(ctx, one_round, name, runs)
        k = dict(ms_per_launch=round(ms, 5))
        if name in STREAMING and ms > 0:
            k["fraction_of_peak"] = round(floor_ms / ms, 4)
        res["kernels"][name] = k
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--rows", type=int, default=1080)
    ap.add_argument("--cols", type=int, default=1920)
    ap.add_argument("--octaves", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box", "cases": []}
    args, info = workload_lists(ctx, a.frames, a.rows, a.cols, a.octaves, full_lists=True)
    res["workload"] = info
    print(json.dumps(info), flush=True)
    res["cases"].append(measure(ctx, "workload match lists", *args, a.runs, a.rounds))
    print(json.dumps(res["cases"][-1]), flush=True)
    del args
    res["cases"].append(measure(ctx, "planted lists, every list full", *planted_lists(ctx, 255, 65536), a.runs, a.rounds))
    print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

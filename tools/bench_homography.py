"""Throughput of the homography stage (vslam_homography_dev) on the match lists of the 256-frame workload and on full planted
lists: the two cases of tools/bench_refit.py, 512 hypotheses, with the models vslam_epipolar_dev finds over the same lists as
the verdict's input and the gate written.  HIP events around each call, 2 warm-up calls, the median of --runs calls; every kernel of the stage
alone through the library's timing hook: one call per reading, the time per launch, the median of --runs readings.  In the
same run, on the same lists, k_epi_score is timed the same way: both kernels walk pairs x hypotheses x records with the model
in registers and the records in LDS.  One symmetric-transfer test is 42 f64 operations, none of them fused (24 multiplications,
18 additions, and 4 comparisons beside them; include/vslam.h) against the Sampson test's 33; the ratio of the two kernels' time
per test is reported beside that.  No target is set - there is no earlier homography stage to compare with.

  python tools/bench_homography.py [--runs 10] [--frames 256] [--out profiles/homography_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_epipolar import F64_PEAK_TF, timed
from tools.bench_pose import planted_lists, workload_lists
from tools.bench_refit import per_launch
from visualslam_amd import capi

DEV = "cuda:0"
HYPOTHESES = 512
OPS_HOM, OPS_EPI = 42, 33
KERNELS = ("k_hom_models", "k_hom_score", "k_hom_select", "k_hom_verdict", "k_hom_flags")


def measure(ctx, label, _models, lists, counts, qpts, tpts, runs):
    n, cap = lists.shape[0], lists.shape[1]
    z = lambda shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    hm, gated, icounts, em = z((n, 42)), z((n, 22)), z((n,)), z((n, 22))
    call = lambda: ctx.homography(lists, counts, qpts, tpts, n_pairs=n, n_hypotheses=HYPOTHESES, seed=1, max_dist2=4.0, epipolar_models=em, models=hm,
                                  inlier_counts=icounts, gated_models=gated)
    epi = lambda: ctx.epipolar(lists, counts, qpts, tpts, n_pairs=n, n_hypotheses=HYPOTHESES, seed=1, max_dist2=4.0, models=em)
    emed, elo, ehi = timed(epi, runs)  # (first: `em` is the verdict's input below)
    med, lo, hi = timed(call, runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    tests = float(records) * HYPOTHESES
    h = hm.cpu().numpy().view(capi.HOMOGRAPHY_DTYPE).reshape(-1)
    res = dict(case=label, pairs=n, capacity=cap, records=records, hypotheses=HYPOTHESES, runs=runs, tests=tests, call_ms_median=round(med, 4),
               call_ms_min=round(lo, 4), call_ms_max=round(hi, 4), epipolar_call_ms_median=round(emed, 4), epipolar_call_ms_min=round(elo, 4),
               epipolar_call_ms_max=round(ehi, 4), pairs_with_a_homography=int((h["best"] >= 0).sum()), pairs_degenerate=int(h["degenerate"].sum()),
               homography_inliers=int(h["n_inliers"].sum()), epipolar_inliers=int(h["n_epipolar"].sum()), kernels={})
    for name in KERNELS:
        res["kernels"][name] = dict(ms_per_launch=round(per_launch(ctx, call, name, runs), 5))
    res["kernels"]["k_epi_score"] = dict(ms_per_launch=round(per_launch(ctx, epi, "k_epi_score", runs), 5))
    hs, es = res["kernels"]["k_hom_score"]["ms_per_launch"], res["kernels"]["k_epi_score"]["ms_per_launch"]
    if hs > 0 and es > 0 and tests > 0:
        peak_ops = F64_PEAK_TF / 2 * 1e12  # unfused operations per second
        res["score"] = dict(k_hom_score_ps_per_test=round(hs * 1e9 / tests, 4), k_epi_score_ps_per_test=round(es * 1e9 / tests, 4), ratio=round(hs / es, 3),
                            ratio_of_f64_operations=round(OPS_HOM / OPS_EPI, 3), k_hom_score_of_f64_vector_peak=round(tests * OPS_HOM / (hs * 1e-3) / peak_ops, 3),
                            k_epi_score_of_f64_vector_peak=round(tests * OPS_EPI / (es * 1e-3) / peak_ops, 3))
    return res


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
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box", "f64_vector_peak_tflops": F64_PEAK_TF, "f64_ops_per_transfer_test": OPS_HOM,
           "f64_ops_per_sampson_test": OPS_EPI, "cases": []}
    args, info = workload_lists(ctx, a.frames, a.rows, a.cols, a.octaves, full_lists=True)
    res["workload"] = info
    print(json.dumps(info), flush=True)
    res["cases"].append(measure(ctx, "workload match lists", *args, a.runs))
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

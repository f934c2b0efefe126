"""Throughput of the resection stage (vslam_resect_dev) on the lists of the 256-frame workload and on full planted lists: the
two cases of tools/bench_chain.py - the poses, inlier lists, point rows and front bits vslam_pose_dev leaves for 255 pairs - as
the structure side, the same lists as the observation side, 512 hypotheses.  The planted pairs are independent two-camera
scenes whose records carry the indices i, i: every record in front is linked and usable, so the score kernel walks full lists
(its time does not depend on how many tests pass).  HIP events around each call, 2 warm-up calls, the median of --runs calls;
every kernel of the stage alone through the library's timing hook: the time per launch.  In the same run, on the same lists,
k_epi_score is timed the same way: both kernels walk pairs x hypotheses x records with the model in registers and the records
in LDS.  One reprojection test is 29 f64 operations, none of them fused (17 multiplications, 12 additions, and 2 comparisons
beside them; include/vslam.h) against the Sampson test's 33.  No target is set - there is no earlier resection stage to compare
with.

  python tools/bench_resect.py [--runs 10] [--frames 256] [--out profiles/resect_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_chain import pose_outputs
from tools.bench_epipolar import F64_PEAK_TF, timed
from tools.bench_pose import K, hooked, planted_lists, workload_lists
from visualslam_amd import capi

DEV = "cuda:0"
HYPOTHESES = 512
OPS_RES, OPS_EPI = 29, 33
KERNELS = ("k_chain_link", "k_res_corr", "k_flag_count", "k_chunk_scan", "k_flag_scatter", "k_res_gather", "k_res_models", "k_res_score", "k_res_select",
           "k_res_flags")


def measure(ctx, label, args, point_cap, runs):
    models, lists, counts, qpts, tpts = args
    poses, lists, counts, points, bits = pose_outputs(ctx, *args)
    n, cap = lists.shape[0], lists.shape[1]
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=DEV)
    rm, ib, em = z((n, 30)), z((n, (cap + 63) // 64), torch.int64), z((n, 22))
    call = lambda: ctx.resect(poses, lists, counts, points, bits, point_cap, lists, counts, tpts, K, HYPOTHESES, 1, 4.0, n_pairs=n, models=rm, inlier_bits=ib)
    epi = lambda: ctx.epipolar(lists, counts, qpts, tpts, n_pairs=n, n_hypotheses=HYPOTHESES, seed=1, max_dist2=4.0, models=em)
    med, lo, hi = timed(call, runs)
    emed, elo, ehi = timed(epi, runs)
    r = rm.cpu().numpy().view(capi.RESECT_DTYPE).reshape(-1)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    corr = int(r["n_corr"].astype("int64").sum())
    res = dict(case=label, pairs=n, capacity=cap, point_cap=point_cap, records=records, correspondences=corr, hypotheses=HYPOTHESES, runs=runs,
               resect_tests=float(corr) * HYPOTHESES, epipolar_tests=float(records) * HYPOTHESES, call_ms_median=round(med, 4), call_ms_min=round(lo, 4),
               call_ms_max=round(hi, 4), epipolar_call_ms_median=round(emed, 4), epipolar_call_ms_min=round(elo, 4), epipolar_call_ms_max=round(ehi, 4),
               pairs_with_a_model=int((r["best"] >= 0).sum()), inliers=int(r["n_inliers"].astype("int64").sum()), kernels={})
    for name in KERNELS:
        res["kernels"][name] = dict(ms_per_launch=round(hooked(ctx, call, name, runs), 5))
    res["kernels"]["k_epi_score"] = dict(ms_per_launch=round(hooked(ctx, epi, "k_epi_score", runs), 5))
    rs, es = res["kernels"]["k_res_score"]["ms_per_launch"], res["kernels"]["k_epi_score"]["ms_per_launch"]
    if rs > 0 and es > 0 and corr > 0 and records > 0:
        peak_ops = F64_PEAK_TF / 2 * 1e12  # unfused operations per second
        rt, et = res["resect_tests"], res["epipolar_tests"]
        res["score"] = dict(k_res_score_ps_per_test=round(rs * 1e9 / rt, 4), k_epi_score_ps_per_test=round(es * 1e9 / et, 4),
                            ratio_of_time_per_test=round((rs / rt) / (es / et), 3), ratio_of_f64_operations=round(OPS_RES / OPS_EPI, 3),
                            k_res_score_of_f64_vector_peak=round(rt * OPS_RES / (rs * 1e-3) / peak_ops, 3),
                            k_epi_score_of_f64_vector_peak=round(et * OPS_EPI / (es * 1e-3) / peak_ops, 3))
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
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box", "intrinsics": K, "f64_vector_peak_tflops": F64_PEAK_TF,
           "f64_ops_per_reprojection_test": OPS_RES, "f64_ops_per_sampson_test": OPS_EPI, "cases": []}
    args, info = workload_lists(ctx, a.frames, a.rows, a.cols, a.octaves)
    res["workload"] = info
    print(json.dumps(info), flush=True)
    res["cases"].append(measure(ctx, "workload inlier lists", args, info["oriented_cap"], a.runs))
    print(json.dumps(res["cases"][-1]), flush=True)
    del args
    res["cases"].append(measure(ctx, "planted lists, every list full", planted_lists(ctx, 255, 65536), 65536, a.runs))
    print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

"""Throughput of the refinement of the resected pose (vslam_resect_refine_dev) on full planted lists: the planted case of
tools/bench_resect.py - 255 pairs x 65536 records, every record in front linked and usable - resected with 512 hypotheses, then
refined over the dense correspondence lists that call wrote.  The planted pairs are independent two-camera scenes, so no pose
explains a pair's rows as the resection leaves them (its winners have a handful of inliers and every pair would stop at once):
the observations u, v of every row are therefore replaced, on the device, by the projection of its Y under one fixed pose plus
half a pixel of noise, and the input pose is that pose off by 0.03 degrees and 2 mm - every list stays full, nearly every row
is a member, and every pair runs its rounds.  HIP events around each 4-round call, 2 warm-up calls, the median
of --runs calls; every kernel of the stage alone through the library's timing hook: one call per reading, the time per launch,
the median of --runs readings.  The kernel readings come from calls with rounds = 1: there no pair has stopped before a launch
(a stopped pair's workgroups leave at once, so the later passes of a longer call read fewer rows), and each launch of the
streaming pass reads every row of the dense lists once, 48 bytes: its time is set against that floor at the 8 TB/s peak of the
device.  In the same run k_refit_moments - the widest pass of the fundamental matrix's refit, 45 sums over 32-byte records - is
timed the same way on the same planted lists, against its own floor.  No target is set - there is no earlier refinement to
compare with.

  python tools/bench_resect_refine.py [--runs 10] [--rounds 4] [--out profiles/resect_refine_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_chain import pose_outputs
from tools.bench_epipolar import timed
from tools.bench_pose import K, planted_lists
from tools.bench_refit import PEAK_BYTES_PER_S, per_launch
from visualslam_amd import capi

DEV = "cuda:0"
HYPOTHESES = 512
KERNELS = ("k_rr_init", "k_rr_pass", "k_rr_step", "k_rr_flags_zero", "k_rr_flags")


def measure(ctx, label, args, point_cap, runs, rounds):
    models, lists, counts, qpts, tpts = args
    poses, lists, counts, points, bits = pose_outputs(ctx, *args)
    n, cap = lists.shape[0], lists.shape[1]
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=DEV)
    rm, corr = z((n, 30)), z((n, cap, 6), torch.int64)
    ctx.resect(poses, lists, counts, points, bits, point_cap, lists, counts, tpts, K, HYPOTHESES, 1, 4.0, n_pairs=n, models=rm, correspondences=corr)
    torch.cuda.synchronize()
    # a pose that explains the rows: u, v = the projection of Y under (R0, t0) plus noise; the input pose is a little off it
    def rot(w):
        A = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        th = np.linalg.norm(w)
        return np.eye(3) + np.sin(th) / th * A + (1 - np.cos(th)) / th ** 2 * A @ A

    R0, t0 = rot(np.array([0.01, -0.02, 0.005])), np.array([0.2, -0.1, 0.05])
    c = corr.view(torch.float64)
    Z = c[..., :3] @ torch.from_numpy(R0.T.copy()).to(DEV) + torch.from_numpy(t0).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    c[..., 3] = Z[..., 0] / Z[..., 2] + torch.randn(Z.shape[:2], generator=gen, device=DEV, dtype=torch.float64) * (0.5 / K[0])
    c[..., 4] = Z[..., 1] / Z[..., 2] + torch.randn(Z.shape[:2], generator=gen, device=DEV, dtype=torch.float64) * (0.5 / K[1])
    del Z
    r = rm.cpu().numpy().view(capi.RESECT_DTYPE).reshape(-1).copy()
    r["R"], r["t"], r["best"] = (rot(np.array([0.0003, 0.0002, -0.0004])) @ R0).reshape(9), t0 + [0.002, -0.001, 0.001], np.where(r["n_corr"] >= 6, 0, -1)
    rm = torch.from_numpy(r.view(np.int32).reshape(n, 30)).to(DEV)
    out, info, ib = z((n, 30)), z((n, 8)), z((n, (cap + 63) // 64), torch.int64)
    call = lambda r=rounds: ctx.resect_refine(rm, corr, cap, K, r, 4.0, n_pairs=n, models=out, info=info, inlier_bits=ib)
    med, lo, hi = timed(call, runs)
    inf = info.cpu().numpy().view(capi.RESECT_REFINE_DTYPE).reshape(-1)
    rows = int(r["n_corr"].astype("int64").sum())
    floor_ms = rows * 48 / PEAK_BYTES_PER_S * 1e3
    res = dict(case=label, pairs=n, capacity=cap, rows=rows, rounds=rounds, runs=runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4),
               call_ms_max=round(hi, 4), floor_ms_per_pass_at_8TBps=round(floor_ms, 5), stops={str(s): int((inf["stop"] == s).sum()) for s in range(6)},
               inliers_before=int(inf["n_before"].astype("int64").sum()), inliers_after=int(inf["n_after"].astype("int64").sum()),
               rounds_accepted=int(inf["accepted"].sum()), kernels_note="calls with rounds = 1", kernels={})
    for name in KERNELS:
        ms = per_launch(ctx, lambda: call(1), name, runs)
        k = dict(ms_per_launch=round(ms, 5))
        if name == "k_rr_pass" and ms > 0:
            k["fraction_of_peak"] = round(floor_ms / ms, 4)
        res["kernels"][name] = k
    # the refit's widest pass on the same planted lists, in the same run
    em, einfo = z((n, 22)), z((n, 4))
    refit = lambda: ctx.refit(models, lists, counts, qpts, tpts, n_pairs=n, rounds=1, max_dist2=4.0, models=em, info=einfo)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    ms = per_launch(ctx, refit, "k_refit_moments", runs)
    res["kernels"]["k_refit_moments"] = dict(ms_per_launch=round(ms, 5), records=records, floor_ms_at_8TBps=round(records * 32 / PEAK_BYTES_PER_S * 1e3, 5),
                                             fraction_of_peak=round(records * 32 / PEAK_BYTES_PER_S * 1e3 / ms, 4) if ms > 0 else None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=255)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box", "intrinsics": K, "bytes_per_row": 48, "sums_per_pass": 29, "cases": []}
    res["cases"].append(measure(ctx, "planted lists, every list full", planted_lists(ctx, a.pairs, a.records), a.records, a.runs, a.rounds))
    print(json.dumps(res["cases"][-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

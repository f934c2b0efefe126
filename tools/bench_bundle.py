"""Throughput of the bundle adjustment (vslam_bundle_dev) on the full planted lists of tools/bench_tracks.py: 255 pairs x 65536
records after vslam_pose_dev, vslam_chain_dev and vslam_tracks_dev on the same lists, 4 sweeps.  (The planted pairs are
independent two-camera scenes, so the views of a long track do not meet in one point: the walks, the gathers and the arithmetic
are the full ones, the adjusted points are not meaningful; max_dist2 is wide so that views are members and steps are taken.)
HIP events around each call, 2 warm-up calls, the median of --runs calls; every kernel per launch through the library's timing
hook; and, in the same run on the same lists, k_trk_walk of vslam_tracks_dev (against k_ba_points) and k_rr_pass of
vslam_resect_refine_dev over the resection's dense rows (against k_ba_cam_pass: the same 29 sums per row, streamed instead of
gathered).  A first measurement, not a pass criterion.

  python tools/bench_bundle.py [--runs 10] [--sweeps 4] [--pairs 255] [--records 65536] [--out profiles/bundle_bench.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_chain import pose_outputs
from tools.bench_epipolar import timed
from tools.bench_pose import K, hooked, planted_lists
from visualslam_amd import capi

DEV = "cuda:0"
KERNELS = ("k_chain_link", "k_trk_next", "k_ba_init", "k_ba_points", "k_ba_cam_pass", "k_ba_cam_step", "k_ba_member_bits", "k_ba_points_final")
WIDE = 1e7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--pairs", type=int, default=255)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    n, cap = a.pairs, a.records
    models, lists, counts, qpts, tpts = planted_lists(ctx, n, cap)
    poses, lists, counts, points, bits = pose_outputs(ctx, models, lists, counts, qpts, tpts)
    frames = torch.cat([qpts, tpts[-1:]]).contiguous()
    del models
    z = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=DEV)
    chain = z((n, 44))
    ctx.chain(poses, lists, counts, points, bits, cap, 16, n_pairs=n, chain=chain)
    tracks_in, refs = z((n, cap, 6), torch.int64), z((n, cap, 2))
    tracks_call = lambda: ctx.tracks(poses, lists, counts, bits, cap, chain, frames, K, WIDE, 2, n_pairs=n, tracks=tracks_in, refs=refs)
    tracks_call()
    tracks, cams = z((n, cap, 6), torch.int64), z((n, 20), torch.int64)
    info, mbits = z((n, cap, 5), torch.int64), z((n, 2, (cap + 63) // 64), torch.int64)
    call = lambda: ctx.bundle(poses, lists, counts, bits, cap, chain, frames, tracks_in, refs, K, WIDE, 2, a.sweeps, n_pairs=n, tracks=tracks, cams=cams,
                              point_info=info, member_bits=mbits)
    med, lo, hi = timed(call, a.runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    out = dict(device=torch.cuda.get_device_name(0), intrinsics=K, max_dist2=WIDE, min_views=2, sweeps=a.sweeps, case="planted lists, every list full", pairs=n,
               capacity=cap, point_cap=cap, records=records, runs=a.runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4), call_ms_max=round(hi, 4),
               note="one run on one box", kernels={})
    for k in KERNELS:
        out["kernels"][k] = dict(ms_per_launch=round(hooked(ctx, call, k, a.runs), 5))
    hc = cams.cpu().numpy().view(capi.BUNDLE_CAM_DTYPE).reshape(-1)
    ht = tracks_in.cpu().numpy().view(capi.TRACK_DTYPE).reshape(-1)
    hr = refs.cpu().numpy().view(capi.TRACK_REF_DTYPE).reshape(n, cap)
    hl = chain.cpu().numpy().view(capi.CHAIN_DTYPE).reshape(-1)["linked"]
    m = np.minimum(counts[:n].cpu().numpy().astype(np.int64), cap)
    active = (ht["status"] & 1).astype(bool) & (ht["n_views"] >= 2)
    views = int(ht["n_views"][active].astype(np.int64).sum())
    rows = int(m.sum() + sum(int(m[j + 1]) for j in range(n - 1) if hl[j + 1]))
    out.update(active_tracks=int(active.sum()), views_of_active_tracks=views, camera_rows=rows,
               member_rows_before=int(hc["n_before"].astype(np.int64).sum()), member_rows_after=int(hc["n_after"].astype(np.int64).sum()),
               camera_sweeps=dict(accepted=int(hc["accepted"].sum()), rejected=int(hc["rejected"].sum()), invalid=int(hc["invalid"].sum()), skipped=int(hc["skipped"].sum())))
    del hr
    p = out["kernels"]
    p["k_ba_points"]["views_per_s"] = round(3 * views / (p["k_ba_points"]["ms_per_launch"] * 1e-3), 1)      # at most three walks per launch: the sums, the candidate (and none when skipped)
    p["k_ba_cam_pass"]["rows_per_s"] = round(rows / (p["k_ba_cam_pass"]["ms_per_launch"] * 1e-3), 1)
    # k_trk_walk on the same lists, in the same run: two walks of every track
    ms = hooked(ctx, tracks_call, "k_trk_walk", a.runs)
    all_views = int(ht["n_views"].astype(np.int64).sum())
    p["k_trk_walk"] = dict(ms_per_launch=round(ms, 5), views_per_s=round(2 * all_views / (ms * 1e-3), 1))
    # k_rr_pass over the resection's dense rows of the same lists, in the same run: 48-byte rows streamed, the same 29 sums
    rm, corr = z((n, 30)), z((n, cap, 6), torch.int64)
    ctx.resect(poses, lists, counts, points, bits, cap, lists, counts, tpts, K, 64, 1, WIDE, n_pairs=n, models=rm, correspondences=corr)
    rr_out = z((n, 30))
    rr_call = lambda: ctx.resect_refine(rm, corr, cap, K, 1, WIDE, n_pairs=n, models=rr_out)
    ms = hooked(ctx, rr_call, "k_rr_pass", a.runs)
    r = rm.cpu().numpy().view(capi.RESECT_DTYPE).reshape(-1)
    rr_rows = int(r["n_corr"][r["best"] >= 0].astype(np.int64).sum())
    p["k_rr_pass"] = dict(ms_per_launch=round(ms, 5), rows=rr_rows, rows_per_s=round(rr_rows / (ms * 1e-3), 1) if ms > 0 else None)
    if ms > 0 and rr_rows:
        out["cam_pass_row_cost_over_rr_pass"] = round((p["k_ba_cam_pass"]["ms_per_launch"] / rows) / (ms / rr_rows), 3)
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

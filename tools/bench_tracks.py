"""Throughput of the tracks step (vslam_tracks_dev) on the full planted lists of tools/bench_chain.py: 255 pairs x 65536 records,
16.7 M in all, every record with the indices i, i, so that every record in front under its pair's pose continues the record
of the same index in the pair before - paths up to 255 records long.  vslam_pose_dev and vslam_chain_dev run first and leave
their outputs on the device; the frames' point lists are the pairs' query lists with the last pair's train list behind them
(the planted pairs are independent two-camera scenes, so the views of a long track do not meet in one point: the walk, its
gathers and its arithmetic are the full ones, the points are not meaningful).  HIP events around each call, 2 warm-up calls,
the median of --runs calls; every kernel alone through the library's timing hook, and k_chain_ratio and k_chain_map of
vslam_chain_dev on the same lists in the same run, for comparison.  The rate is match records per second: the records
considered, sum over pairs of min(count, capacity), over the kernel's time.  A first measurement, not a pass criterion.

  python tools/bench_tracks.py [--runs 10] [--pairs 255] [--records 65536] [--out profiles/tracks_bench.json]
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
KERNELS = ("k_chain_link", "k_trk_next", "k_trk_walk", "k_trk_rows")
CHAIN_KERNELS = ("k_chain_ratio", "k_chain_map")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=255)
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    n, cap = a.pairs, a.records
    models, lists, counts, qpts, tpts = planted_lists(ctx, n, cap)
    poses, lists, counts, points, bits = pose_outputs(ctx, models, lists, counts, qpts, tpts)
    frames = torch.cat([qpts, tpts[-1:]]).contiguous()
    del models, tpts
    chain = torch.zeros((n, 44), dtype=torch.int32, device=DEV)
    world = torch.zeros((n, cap, 3), dtype=torch.float64, device=DEV)
    chain_call = lambda: ctx.chain(poses, lists, counts, points, bits, cap, 16, n_pairs=n, chain=chain, map=world)
    chain_call()
    tracks = torch.zeros((n, cap, 6), dtype=torch.int64, device=DEV)
    refs = torch.zeros((n, cap, 2), dtype=torch.int32, device=DEV)
    good = torch.zeros((n, (cap + 63) // 64), dtype=torch.int64, device=DEV)
    summary = torch.zeros((n, 4), dtype=torch.int32, device=DEV)
    call = lambda: ctx.tracks(poses, lists, counts, bits, cap, chain, frames, K, 4.0, 2, n_pairs=n, tracks=tracks, refs=refs, good_bits=good, summary=summary)
    med, lo, hi = timed(call, a.runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    rate = lambda ms: round(records / (ms * 1e-3), 1) if ms > 0 and records else None
    out = dict(device=torch.cuda.get_device_name(0), intrinsics=K, max_dist2=4.0, min_views=2, case="planted lists, every list full", pairs=n, capacity=cap,
               point_cap=cap, records=records, runs=a.runs, call_ms_median=round(med, 4), call_ms_min=round(lo, 4), call_ms_max=round(hi, 4),
               records_per_s_call=rate(med))
    for k in KERNELS:
        ms = hooked(ctx, call, k, a.runs)
        out[k + "_ms"] = round(ms, 4)
        out["records_per_s_" + k[2:]] = rate(ms)
    for k in CHAIN_KERNELS:
        ms = hooked(ctx, chain_call, k, a.runs)
        out[k + "_ms"] = round(ms, 4)
        out["records_per_s_" + k[2:]] = rate(ms)
    hs = summary.cpu().numpy().view(capi.TRACK_SUMMARY_DTYPE).reshape(-1)
    hc = chain.cpu().numpy().view(capi.CHAIN_DTYPE).reshape(-1)
    ht = tracks.cpu().numpy().view(capi.TRACK_DTYPE).reshape(-1)
    views = ht["n_views"][ht["n_views"] > 0]
    out.update(linked_pairs=int(hc["linked"].sum()), heads=int(hs["n_heads"].sum()), good_tracks=int(hs["n_good"].sum()), max_views=int(hs["max_views"].max()),
               mean_views=round(float(views.mean()), 3) if len(views) else None, records_on_tracks=int((views - 1).sum()),
               solved_tracks=int((ht["status"] & 1).sum()))
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

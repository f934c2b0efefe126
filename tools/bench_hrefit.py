"""Cost and effect of the least-squares refit of the homography (vslam_hrefit_dev), one run on one box.

Timing, on planted plane lists with every list full (tools/bench_hpose.py's: the plane Z = 8 + 0.3 X - 0.2 Y, 30 % of the train
points noise, H and F of each pair found from its first 2048 records): one pair of 1 k, 4 k, 16 k and 64 k records, and 255 pairs of
2 k.  HIP events around each call, 2 warm-up calls, the median of --runs calls at --rounds rounds; every streaming kernel alone
through the library's timing hook from calls with rounds = 1 (there no pair has stopped before a launch, so each launch reads every
record once, 32 bytes).  The yardstick is the refit of F (vslam_refit_dev) on the same lists in the same run: the ratio of the two
calls, of the two moment passes, and k_hrefit_moments against the floor of its 32-byte records at the 8 TB/s peak of the device.  No
ratio is fixed in advance: this file is where the values live.

Accuracy, on the device: the 16 planted plane scenes of tests/homref.py (seeds 0 .. 15, 300 records) through homography -> hpose
with and without the refit between, rotation and translation-direction errors against the planted motion; and the five-frame plane
chain of tests/hposeref.py (seeds 1 .. 8, 300 records) through pose -> hpose -> chain the same way, the scale and centre errors of
DESIGN 5.24 before and after.

  python tools/bench_hrefit.py [--runs 10] [--rounds 4] [--out profiles/hrefit_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tests import homref, hposeref
from tools.bench_epipolar import timed
from tools.bench_hpose import planted_lists
from tools.bench_refit import per_launch
from visualslam_amd import capi

DEV = "cuda:0"
PEAK_BYTES_PER_S = 8.0e12
K = hposeref.K_PLANTED
H_STREAMING = ("k_hrefit_count", "k_hrefit_dist", "k_hrefit_moments")
F_STREAMING = ("k_refit_count", "k_refit_dist", "k_refit_moments")


def z(*shape, dt=torch.int32):
    return torch.zeros(shape, dtype=dt, device=DEV)


def measure(ctx, label, emodels, hmodels, lists, counts, qpts, tpts, runs, rounds):
    n, cap = lists.shape[0], lists.shape[1]
    hout, eout, hinfo, einfo = z(n, 42), z(n, 22), z(n, 4), z(n, 4)
    hcall = lambda r=rounds: ctx.hrefit(hmodels, lists, counts, qpts, tpts, n_pairs=n, rounds=r, max_dist2=4.0, models=hout, info=hinfo)
    fcall = lambda r=rounds: ctx.refit(emodels, lists, counts, qpts, tpts, n_pairs=n, rounds=r, max_dist2=4.0, models=eout, info=einfo)
    h_ms, f_ms = timed(hcall, runs), timed(fcall, runs)
    records = int(torch.clamp(counts[:n].to(torch.int64), max=cap).sum())
    floor_ms = records * 32 / PEAK_BYTES_PER_S * 1e3
    hi, fi = (t.cpu().numpy().view(capi.REFIT_DTYPE).reshape(-1) for t in (hinfo, einfo))
    res = dict(case=label, pairs=n, capacity=cap, records=records, rounds=rounds, runs=runs, floor_ms_per_pass_at_8TBps=round(floor_ms, 6),
               hrefit_call_ms=[round(v, 4) for v in h_ms], refit_call_ms=[round(v, 4) for v in f_ms], call_ms_note="median, min, max",
               call_ratio_hrefit_over_refit=round(h_ms[0] / f_ms[0], 4),
               hrefit=dict(stops={str(s): int((hi["stop"] == s).sum()) for s in range(6)}, inliers_before=int(hi["n_before"].sum()),
                           inliers_after=int(hi["n_after"].sum()), rounds_accepted=int(hi["accepted"].sum())),
               refit=dict(stops={str(s): int((fi["stop"] == s).sum()) for s in range(6)}, inliers_before=int(fi["n_before"].sum()),
                          inliers_after=int(fi["n_after"].sum()), rounds_accepted=int(fi["accepted"].sum())),
               kernels_note="ms per launch, calls with rounds = 1", kernels={})
    for names, call in ((H_STREAMING + ("k_hrefit_solve",), lambda: hcall(1)), (F_STREAMING + ("k_refit_solve",), lambda: fcall(1))):
        for name in names:
            res["kernels"][name] = round(per_launch(ctx, call, name, runs), 6)
    k = res["kernels"]
    res["moments_ratio_hrefit_over_refit"] = round(k["k_hrefit_moments"] / k["k_refit_moments"], 4)
    res["hrefit_moments_fraction_of_hbm_floor"] = round(floor_ms / k["k_hrefit_moments"], 4)
    res["refit_moments_fraction_of_hbm_floor"] = round(floor_ms / k["k_refit_moments"], 4)
    return res


def angle(c):
    return float(np.degrees(np.arccos(np.clip(c, -1, 1))))


def plane_scenes(ctx, rounds, seeds=range(16), n=300):
    """homography -> [hrefit] -> hpose on the device over the planted plane scenes, one call of len(seeds) pairs."""
    scenes = [homref.planted_scene(seed, n, "plane") for seed in seeds]
    p = len(scenes)
    dev = lambda a, k: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(p, n, k)).to(DEV)
    mt, qp, tp = (dev(np.stack([s[i] for s in scenes]), k) for i, k in ((0, 3), (1, 6), (2, 6)))
    cnt = torch.full((p,), n, dtype=torch.int32, device=DEV)
    hmod, inl, icnt = z(p, 42), z(p, n, 3), z(p)
    ctx.homography(mt, cnt, qp, tp, p, 512, 1, 4.0, models=hmod, inliers=inl, inlier_counts=icnt)
    yaw = 0.05
    Rt = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    out = {}
    for label in ("ransac", "refit"):
        if label == "refit":
            rinfo = z(p, 4)
            ctx.hrefit(hmod, mt, cnt, qp, tp, p, rounds, 4.0, models=hmod, info=rinfo, inliers=inl, inlier_counts=icnt)
        poses, info = z(p, 28), z(p, 36)
        pn = np.zeros(p, capi.POSE_DTYPE)  # "no pose" records: hpose writes the pairs it selects
        pn["best"] = -1
        poses.copy_(torch.from_numpy(pn.view(np.int32).reshape(p, 28)))
        ctx.hpose(hmod, inl, icnt, qp, tp, K, only_degenerate=False, n_pairs=p, poses=poses, info=info)
        torch.cuda.synchronize()
        ps = poses.cpu().numpy().view(capi.POSE_DTYPE).reshape(-1)
        hm = hmod.cpu().numpy().view(capi.HOMOGRAPHY_DTYPE).reshape(-1)
        rows = []
        for j, seed in enumerate(seeds):
            row = dict(seed=int(seed), n_inliers=int(hm["n_inliers"][j]), best=int(ps["best"][j]))
            if row["best"] >= 0:
                R, t = ps["R"][j].reshape(3, 3), ps["t"][j]
                row["rotation_deg"] = round(angle((np.trace(R @ Rt.T) - 1) / 2), 4)
                row["direction_deg"] = round(angle(t @ np.array([-1.0, 0, 0]) / max(np.linalg.norm(t), 1e-300)), 4)
            rows.append(row)
        posed = [r for r in rows if r["best"] >= 0]
        out[label] = dict(scenes=rows, posed=len(posed), worst_rotation_deg=max(r["rotation_deg"] for r in posed), worst_direction_deg=max(r["direction_deg"] for r in posed),
                          median_rotation_deg=round(statistics.median(r["rotation_deg"] for r in posed), 4),
                          median_direction_deg=round(statistics.median(r["direction_deg"] for r in posed), 4))
        if label == "refit":
            ri = rinfo.cpu().numpy().view(capi.HREFIT_DTYPE).reshape(-1)
            out[label]["stops"] = {str(s): int((ri["stop"] == s).sum()) for s in range(6)}
    return out


def plane_chain(ctx, rounds, seeds=range(1, 9), n=300):
    """The five-frame plane chain: pose over the gated models, hpose over the RANSAC or the refitted H, chain; DESIGN 5.24's errors."""
    rows = []
    for seed in seeds:
        d = hposeref.plane_chain_inputs(seed, n)
        full = np.stack(hposeref.five_plane_frames(seed, n)[0])
        dev = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(shape)).to(DEV)
        lists = (dev(d["matches"], (4, n, 3)), torch.from_numpy(d["counts"].astype(np.int32)).to(DEV), dev(d["query"], (4, n, 6)), dev(d["train"], (4, n, 6)))
        hmod = dev(d["models"], (4, 42))
        row = dict(seed=int(seed))
        for label in ("ransac", "refit"):
            if label == "refit":
                ctx.hrefit(hmod, dev(full, (4, n, 3)), torch.full((4,), n, dtype=torch.int32, device=DEV), lists[2], lists[3], 4, rounds, 4.0, models=hmod)
            poses, X, fb, chain = z(4, 28), z(4, n, 3, dt=torch.float64), z(4, (n + 63) // 64, dt=torch.int64), z(4, 44)
            ctx.pose(dev(d["gated"], (4, 22)), *lists, K, poses=poses, points=X, front_bits=fb)
            ctx.hpose(hmod, *lists, K, poses=poses, info=z(4, 36), points=X, front_bits=fb)
            ctx.chain(poses, lists[0], lists[1], X, fb, n, 16, chain=chain)
            torch.cuda.synchronize()
            ch = chain.cpu().numpy().view(capi.CHAIN_DTYPE).reshape(-1)
            B, scale_err, centre_err = hposeref.BASELINES, 0.0, 0.0
            for j in range(4):
                scale_err = max(scale_err, abs(ch["scale"][j] - B[j] / B[0]) / (B[j] / B[0]))
                for (R, t), C_ in ((d["cams"][j], ch["C"][j]), (d["cams"][j + 1], ch["Ct"][j])):
                    centre_err = max(centre_err, float(np.abs(C_ - (-R.T @ t) / B[0]).max()))
            row[label] = dict(one_segment=bool(ch["valid"].all() and (ch["segment"] == 0).all()), worst_relative_scale_error=round(float(scale_err), 4),
                              worst_centre_error=round(centre_err, 4))
        rows.append(row)
    worst = lambda label, key: max(r[label][key] for r in rows)
    return dict(seeds=rows, worst={label: dict(scale=worst(label, "worst_relative_scale_error"), centre=worst(label, "worst_centre_error")) for label in ("ransac", "refit")})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box; timing and accuracy both from this GPU run", "timing": []}
    for pairs, m in ((1, 1024), (1, 4096), (1, 16384), (1, 65536), (255, 2048)):
        res["timing"].append(measure(ctx, f"{pairs} pair(s) x {m} records, every list full", *planted_lists(ctx, pairs, m), a.runs, a.rounds))
        print(json.dumps(res["timing"][-1]), flush=True)
    res["accuracy_plane_scenes"] = plane_scenes(ctx, a.rounds)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "scenes"} for k, v in res["accuracy_plane_scenes"].items()}), flush=True)
    res["accuracy_plane_chain"] = plane_chain(ctx, a.rounds)
    print(json.dumps(res["accuracy_plane_chain"]["worst"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

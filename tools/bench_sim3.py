"""A first measurement of frame structure and loop alignment (vslam_frame_world_dev, vslam_sim3_dev).  One run on one box; every
figure is the median of --runs calls after a warm-up call, each kernel through the timing hook in calls of its own.

k_sim3_score has k_res_score's shape - lane = hypothesis, correspondence tiles broadcast from LDS, an integer count - with two
reprojection tests on an 88-byte record where the resection does one on a 48-byte one (80 and 40 bytes staged), so it is held
against k_res_score IN THE SAME RUN at the same (pairs, hypotheses, list length): the resection is timed first and last and the
similarity between; the difference of the resection's two medians is the run-to-run spread the ratio is read against.  Sizes:
1 x 65,536 records, 255 x 2,048 and 2,048 slots x 256, at 512 hypotheses.  Every record is usable on either stage (the resection
call has one pair more: its pair 0 has no correspondences).  Then the whole vslam_sim3_dev call with each of its kernels, and
vslam_frame_world_dev at 255 pairs x 65,536 records against its byte floor at the 6.3 TB/s a float4 copy reaches on this part: 12
bytes read per record and one bit of front_bits, and per index entry 4 bytes of preset and 8 of the atomic's read and write.

  python tools/bench_sim3.py [--runs 10] [--out profiles/sim3_bench.json]
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
HBM_BYTES_PER_S = 6.3e12
K = (800.0, 800.0, 960.0, 540.0)
NH = 512
SIM3_KERNELS = ("k_sim3_corr", "k_sim3_gather", "k_sim3_models", "k_sim3_score", "k_sim3_select", "k_sim3_flags")


def timed(fn, runs):
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
    return round(statistics.median(ms), 4), round(min(ms), 4), round(max(ms), 4)


def kernel_ms(ctx, name, fn, runs):
    """Median over `runs` calls of the time the hook measures for the launches of kernel `name` in one call."""
    fn()
    per_call = []
    for _ in range(runs):
        ctx.kernel_timing_enable(name)
        fn()
        _, ms = ctx.kernel_timing_read()
        per_call.append(ms)
    ctx.kernel_timing_enable(None)
    return round(statistics.median(per_call), 4)


def dev(a, shape, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape).copy()).to(DEV)


def scene(rows, seed):
    """rows scene points in front of the identity camera, and their pixels as octave-1 point records."""
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-4, 4, rows), rng.uniform(-2.5, 2.5, rows), rng.uniform(6, 12, rows)], 1)
    pts = np.zeros(rows, capi.POINT_DTYPE)
    pts["col"], pts["row"] = np.rint(K[0] * X[:, 0] / X[:, 2] + K[2]), np.rint(K[1] * X[:, 1] / X[:, 2] + K[3])
    pts["octave"], pts["level"] = 1, 1
    return X, pts


def score_case(ctx, n_pairs, rows, runs):
    X, pts = scene(rows, rows + n_pairs)
    ident = np.arange(rows, dtype=np.int32)
    rec = np.zeros(rows, capi.MATCH_DTYPE)
    rec["query"] = rec["train"] = ident
    # the similarity: n_pairs frames with the identity camera over the same points, slot p = (p, p), one buffer on both sides
    cams = np.zeros(n_pairs, capi.FRAME_CAM_DTYPE)
    cams["W"], cams["pair"], cams["valid"] = np.eye(3).reshape(9), np.arange(n_pairs), 1
    side = capi.sim3_side(dev(cams, (n_pairs, 28), np.int32), dev(np.tile(ident, (n_pairs, 1)), (n_pairs, rows), np.int32),
                          dev(np.tile(X, (n_pairs, 1, 1)), (n_pairs, rows, 3), np.float64), dev(np.tile(pts, (n_pairs, 1)), (n_pairs, rows, 6), np.int32))
    table = torch.stack([torch.arange(n_pairs, dtype=torch.int32)] * 2, dim=1).contiguous().to(DEV)
    matches, counts = dev(np.tile(rec, (n_pairs, 1)), (n_pairs, rows, 3), np.int32), torch.full((n_pairs,), rows, dtype=torch.int32, device=DEV)
    models, bits = torch.zeros((n_pairs, 34), dtype=torch.int32, device=DEV), torch.zeros((n_pairs, (rows + 63) // 64), dtype=torch.int64, device=DEV)
    sim3 = lambda: ctx.sim3(side, side, table, matches, counts, K, n_hypotheses=NH, seed=1, max_dist2=capi.SIM3_MAX_DIST2, models=models, inlier_bits=bits)
    # the resection over the same points: n_pairs + 1 pairs, x_{j+1} = x_j + t, every record linked, in front and observed
    n = n_pairs + 1
    poses = np.zeros(n, capi.POSE_DTYPE)
    poses["R"], poses["t"], poses["valid"], poses["n_matches"] = np.eye(3).reshape(9), (-0.1, 0.0, 0.0), 1, rows
    r_struct = (dev(poses, (n, 28), np.int32), dev(np.tile(rec, (n, 1)), (n, rows, 3), np.int32), torch.full((n,), rows, dtype=torch.int32, device=DEV),
                dev(np.tile(X, (n, 1, 1)), (n, rows, 3), np.float64), torch.full((n, (rows + 63) // 64), -1, dtype=torch.int64, device=DEV))
    r_train = dev(np.tile(pts, (n, 1)), (n, rows, 6), np.int32)
    r_models = torch.zeros((n, 30), dtype=torch.int32, device=DEV)
    resect = lambda: ctx.resect(*r_struct, rows, r_struct[1], r_struct[2], r_train, K, n_hypotheses=NH, seed=1, max_dist2=4.0, models=r_models)
    first = kernel_ms(ctx, "k_res_score", resect, runs)
    s_ms = {k: kernel_ms(ctx, k, sim3, runs) for k in SIM3_KERNELS}
    last = kernel_ms(ctx, "k_res_score", resect, runs)
    whole = timed(sim3, runs)
    torch.cuda.synchronize()
    got, rgot = models.cpu().numpy().view(capi.SIM3_DTYPE).reshape(-1), r_models.cpu().numpy().view(capi.RESECT_DTYPE).reshape(-1)
    mid = (first + last) / 2
    tests = n_pairs * NH * rows
    return dict(slots=n_pairs, records=rows, hypotheses=NH, k_res_score_first_ms=first, k_res_score_last_ms=last, sim3_kernels_ms=s_ms,
                resection_spread=round(abs(first - last) / mid, 4), k_sim3_score_over_k_res_score=round(s_ms["k_sim3_score"] / mid, 4),
                correspondence_tests_per_s=round(tests / (s_ms["k_sim3_score"] * 1e-3), 0), sim3_dev_call_ms=whole,
                sim3_n_corr=[int(got["n_corr"].min()), int(got["n_corr"].max())], sim3_n_inliers=[int(got["n_inliers"].min()), int(got["n_inliers"].max())],
                resect_n_corr=[int(rgot["n_corr"][1:].min()), int(rgot["n_corr"][1:].max())])


def frame_case(ctx, n_pairs, rows, runs):
    rec = np.zeros(rows, capi.MATCH_DTYPE)
    rec["query"] = rec["train"] = np.random.default_rng(1).permutation(rows)
    poses, chain = np.zeros(n_pairs, capi.POSE_DTYPE), np.zeros(n_pairs, capi.CHAIN_DTYPE)
    poses["R"], poses["t"], poses["valid"] = np.eye(3).reshape(9), (-1.0, 0.0, 0.0), 1
    chain["W"], chain["scale"], chain["valid"] = np.eye(3).reshape(9), 1.0, 1
    t = (dev(poses, (n_pairs, 28), np.int32), dev(np.tile(rec, (n_pairs, 1)), (n_pairs, rows, 3), np.int32), torch.full((n_pairs,), rows, dtype=torch.int32, device=DEV),
         torch.full((n_pairs, (rows + 63) // 64), -1, dtype=torch.int64, device=DEV))
    ch = dev(chain, (n_pairs, 44), np.int32)
    cams, index = torch.zeros((n_pairs + 1, 28), dtype=torch.int32, device=DEV), torch.zeros((n_pairs + 1, rows), dtype=torch.int32, device=DEV)
    call = lambda: ctx.frame_world(*t, rows, ch, cams, index)
    k_index, k_cams, whole = kernel_ms(ctx, "k_frame_index", call, runs), kernel_ms(ctx, "k_frame_cams", call, runs), timed(call, runs)
    records, entries = n_pairs * rows, (n_pairs + 1) * rows
    kernel_bytes = records * 12 + records // 8 + (records + rows) * 8        # the records and their bits; one atomic per record, two for the last pair's
    call_bytes = kernel_bytes + entries * 4                                  # and the preset
    torch.cuda.synchronize()
    linked = int((index >= 0).sum().cpu())
    return dict(pairs=n_pairs, records_per_pair=rows, k_frame_index_ms=k_index, k_frame_cams_ms=k_cams, call_ms=whole, k_frame_index_bytes=kernel_bytes,
                call_bytes=call_bytes, k_frame_index_floor_ms=round(kernel_bytes / HBM_BYTES_PER_S * 1e3, 4), call_floor_ms=round(call_bytes / HBM_BYTES_PER_S * 1e3, 4),
                k_frame_index_of_floor=round(k_index / (kernel_bytes / HBM_BYTES_PER_S * 1e3), 2), call_of_floor=round(whole[0] / (call_bytes / HBM_BYTES_PER_S * 1e3), 2),
                index_entries_set=linked, index_entries=entries)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box; medians of --runs calls", "runs": a.runs, "score": []}
    for n_pairs, rows in ((1, 65536), (255, 2048), (2048, 256)):
        torch.cuda.empty_cache()
        case = score_case(ctx, n_pairs, rows, a.runs)
        res["score"].append(case)
        print(json.dumps(case), flush=True)
    torch.cuda.empty_cache()
    res["frame_world"] = frame_case(ctx, 255, 65536, a.runs)
    print(json.dumps(res["frame_world"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

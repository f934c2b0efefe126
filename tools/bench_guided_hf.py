"""Guided matching under H or F (vslam_match_guided_hf_dev) against guided matching (vslam_match_guided_dev) on the same sets in
the same run: per launch, k_match_guided_hf against k_match_guided through the library's kernel timing hook (HIP events around the
launch; the call launches one form of the kernel per model array it is given, so the figure is the sum of its launches), and the
whole call of each with HIP events around it.  The baseline is measured before and after every new measurement: the two baseline
figures show the spread the comparison has to be read against.  One-pair calls at 1 k / 4 k / 16 k / 64 k rows and 255 pairs at
2 k rows, three pair mixes each: all F (both model arrays given, every pair has an F), all H (every pair's epipolar record is the
gate's "no model", its homography the exact one of a pure rotation) and the two alternating.  2 warm-up calls, the median of --runs
calls.  Every case runs in a child process of its own under a time limit; the first that fails or runs out ends the run.

  python tools/bench_guided_hf.py [--runs 10] [--out profiles/guided_hf_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

CASES = ((1, 1024), (1, 4096), (1, 16384), (1, 65536), (255, 2048))
MIXES = ("all F", "all H", "alternating")
CASE_LIMIT_S = 240


def rotation_points(rng, n, width=1920, height=1080, f=800.0, yaw=0.05):
    """n image points seen before and after a pure yaw -> (query points, train points) int32 [n, 6] at octaves 0 .. 2, and the H of the pair."""
    K = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1.0]])
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    H = K @ R @ np.linalg.inv(K)
    H /= np.linalg.norm(H)
    a = np.stack([rng.uniform(100, width - 100, n), rng.uniform(0, height - 1, n), np.ones(n)], axis=1)
    b = a @ H.T
    b = b[:, :2] / b[:, 2:]
    octave = rng.integers(0, 3, n)
    pts = []
    for xy in (a[:, :2], b):
        p = np.zeros((n, 6), np.int32)
        pitch = 2.0 ** (octave - 1)
        p[:, 0], p[:, 1], p[:, 4], p[:, 5] = np.rint(xy[:, 1] / pitch), np.rint(xy[:, 0] / pitch), octave, 1
        pts.append(p)
    return pts[0], pts[1][rng.permutation(n)], H


def case(index, runs):
    import torch

    from tools.bench_guided import DEV, kernel_ms, planted_points, timed
    from visualslam_amd import capi

    pairs, rows = CASES[index]
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(rows + pairs)
    g = torch.Generator(device=DEV).manual_seed(rows + pairs)
    d = torch.rand((pairs + 1, rows, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((pairs + 1,), rows, dtype=torch.int32, device=DEV)
    fq, ft, F = planted_points(rng, rows)
    hq, ht, H = rotation_points(rng, rows)
    nn = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    matches = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    mc = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    outs = dict(nn=nn, matches=matches, match_counts=mc)
    emodel, hmodel = np.zeros(pairs, capi.EPIPOLAR_DTYPE), np.zeros(pairs, capi.HOMOGRAPHY_DTYPE)
    emodel["F"], hmodel["H"] = F.reshape(9), H.reshape(9)
    exact_f = torch.from_numpy(emodel.view(np.int32).reshape(pairs, 22)).to(DEV)
    results = []
    for mix in MIXES:
        is_h = np.array([mix == "all H" or (mix == "alternating" and j % 2 == 1) for j in range(pairs)])
        qp, tp = np.where(is_h[:, None, None], hq[None], fq[None]), np.where(is_h[:, None, None], ht[None], ft[None])
        qpts, tpts = torch.from_numpy(np.ascontiguousarray(qp)).to(DEV), torch.from_numpy(np.ascontiguousarray(tp)).to(DEV)
        gated = emodel.copy()
        gated["best"][is_h], gated["F"][is_h] = -1, 0.0
        em, hm = (torch.from_numpy(m.view(np.int32).reshape(pairs, -1)).to(DEV) for m in (gated, hmodel))
        Q, T = capi.desc_sets(d[:pairs], counts, None, qpts), capi.desc_sets(d[1:], counts[1:], None, tpts)
        base = lambda: ctx.match_guided(Q, T, exact_f, pairs, 0.64, float("inf"), 4.0, False, **outs)  # every pair under F, whatever the mix
        new = lambda: ctx.match_guided_hf(Q, T, em, hm, pairs, 0.64, float("inf"), 4.0, 4.0, False, **outs)
        out = dict(pairs=pairs, rows=rows, runs=runs, mix=mix, h_pairs=int(is_h.sum()))
        out["k_match_guided_ms"] = [round(kernel_ms(ctx, "k_match_guided", base, runs), 4)]
        out["k_match_guided_hf_ms"] = round(kernel_ms(ctx, "k_match_guided_hf", new, runs, launches=2), 4)
        out["k_match_guided_ms"].append(round(kernel_ms(ctx, "k_match_guided", base, runs), 4))
        out["kernel_ratio"] = round(out["k_match_guided_hf_ms"] / min(out["k_match_guided_ms"]), 3)
        out["guided_call_ms"] = [round(timed(base, runs), 4)]
        out["guided_hf_call_ms"] = round(timed(new, runs), 4)
        found = int((nn.view(pairs * rows, 3)[:, 0] >= 0).sum())
        out.update(accepted=int(mc.sum()), queries_with_a_candidate=found)
        out["guided_call_ms"].append(round(timed(base, runs), 4))
        out["call_ratio"] = round(out["guided_hf_call_ms"] / min(out["guided_call_ms"]), 3)
        if mix == "all F":  # the same call with no homography models: one launch of the search, as vslam_match_guided_dev makes
            only_f = lambda: ctx.match_guided_hf(Q, T, em, None, pairs, 0.64, float("inf"), 4.0, 4.0, False, **outs)
            out["k_match_guided_hf_no_h_ms"] = round(kernel_ms(ctx, "k_match_guided_hf", only_f, runs), 4)
            out["guided_hf_no_h_call_ms"] = round(timed(only_f, runs), 4)
        results.append(out)
    ctx.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--case", type=int, default=-1, help="(internal) run one case in this process and print its JSON")
    a = ap.parse_args()
    if a.case >= 0:
        print("RESULT " + json.dumps(case(a.case, a.runs)), flush=True)
        return 0
    res = {"max_dist2": 4.0, "max_transfer2": 4.0, "cases": []}
    for i in range(len(CASES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", str(i), "--runs", str(a.runs)], capture_output=True, text=True,
                           timeout=CASE_LIMIT_S)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr)
            return 1
        for row in json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:]):
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        import torch

        res["device"] = torch.cuda.get_device_name(0)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

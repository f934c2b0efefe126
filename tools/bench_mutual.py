"""Mutual matching (vslam_match_mutual_dev) against what it replaces, on the same sets in the same run, the three forms taken in
turn in every round:

  fused     one vslam_match_mutual_dev call (k_match_nn2_mutual + k_match_mutual_merge)
  forward   one vslam_match_dev call (k_match_nn2 + k_match_merge): what the cross-check costs on top of
  two       vslam_match_dev(query, train) + vslam_match_dev(train, query): what a user does today for the reverse nearest (the join
            on the host is not counted)

Kernel times through the library's kernel timing hook (HIP events around each launch of one named kernel), whole calls with HIP
events around them.  2 warm-up rounds, then --runs rounds; median, minimum and maximum of each.  The fused kernel is kept if it
takes less time than the two calls by more than the run-to-run spread (max - min) of those two calls: "keeps" per case.
One-pair calls at 1 k / 4 k / 16 k / 64 k rows and 255 pairs at 2 k rows (tools/bench_match.py's shapes).

Quality, from the device through the host entry points: the building crops (the CPU oracle's descriptors) at ratio 0.8 / 0.9 / 0.95
and the 16 planted repeated-structure scenes of tests/guidedref.py at 0.8 - forward and mutual accepted, exact translations /
correct matches kept, train rows claimed by more than one record.

  python tools/bench_mutual.py [--runs 10] [--no-quality] [--out profiles/mutual_bench.json]
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


def stats(ms):
    return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def call_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_ms(ctx, name, fn, launches):
    ctx.kernel_timing_enable(name)
    fn()
    n, total = ctx.kernel_timing_read()
    ctx.kernel_timing_enable(None)
    assert n == launches, (name, n, launches)
    return total


def case(ctx, pairs, rows, runs):
    g = torch.Generator(device=DEV).manual_seed(rows + pairs)
    d = torch.rand((pairs + 1, rows, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((pairs + 1,), rows, dtype=torch.int32, device=DEV)
    nn = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    back = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    rnn = torch.zeros((pairs, rows, 2), dtype=torch.int32, device=DEV)
    matches = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    mc = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:pairs], counts), capi.desc_sets(d[1:], counts[1:])
    forward = lambda: ctx.match(Q, T, pairs, 0.64, False, nn=nn, matches=matches, match_counts=mc)
    swapped = lambda: ctx.match(T, Q, pairs, 0.64, False, nn=back)
    two = lambda: (forward(), swapped())
    fused = lambda: ctx.match_mutual(Q, T, pairs, 0.64, False, nn=nn, rnn=rnn, matches=matches, match_counts=mc)
    forms = {"fused": (fused, (("k_match_nn2_mutual", 1), ("k_match_mutual_merge", 1))),
             "forward": (forward, (("k_match_nn2", 1), ("k_match_merge", 1))),
             "two": (two, (("k_match_nn2", 2), ("k_match_merge", 2)))}
    calls = {k: [] for k in forms}
    kernels = {k: [] for k in forms}
    for r in range(runs + 2):
        for k, (fn, names) in forms.items():  # the three forms in turn, every round
            t_call = call_ms(fn)
            t_kern = sum(kernel_ms(ctx, name, fn, launches) for name, launches in names)
            if r >= 2:
                calls[k].append(t_call), kernels[k].append(t_kern)
    fused()
    torch.cuda.synchronize()
    mutual = int(mc.sum())
    forward()
    torch.cuda.synchronize()
    out = dict(pairs=pairs, rows=rows, runs=runs, accepted_forward=int(mc.sum()), accepted_mutual=mutual,
               kernels_ms={k: stats(v) for k, v in kernels.items()}, calls_ms={k: stats(v) for k, v in calls.items()})
    for what, v in (("kernels", kernels), ("calls", calls)):
        med = {k: statistics.median(x) for k, x in v.items()}
        spread = max(v["two"]) - min(v["two"])
        out[what + "_fused_over_forward"] = round(med["fused"] / med["forward"], 3)
        out[what + "_fused_over_two"] = round(med["fused"] / med["two"], 3)
        out[what + "_two_spread_ms"] = round(spread, 4)
        out[what + "_keeps"] = bool(med["two"] - med["fused"] > spread)
    return out


def claimed(m):
    t, n = np.unique(m["train"], return_counts=True)
    return [int((n > 1).sum()), int(n[n > 1].sum())]


def quality(ctx):
    from tests import guidedref
    from tests.test_gpu_match import building_crops, exact_translations, oracle_chain

    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    crops = []
    for ratio in (0.8, 0.9, 0.95):
        r2 = float(np.float32(ratio) * np.float32(ratio))
        _, fwd, _ = ctx.match_host(qd, td, r2, False, qk, tk)
        _, _, m, _ = ctx.match_mutual_host(qd, td, r2, False, qk, tk)
        ef, em = exact_translations(fwd, qp, tp, 24), exact_translations(m, qp, tp, 24)
        crops.append(dict(ratio=ratio, forward=len(fwd), mutual=len(m), exact_forward=ef, exact_mutual=em, wrong_forward=len(fwd) - ef, wrong_mutual=len(m) - em,
                          multiply_claimed_forward=claimed(fwd), multiply_claimed_mutual=claimed(m)))
    tot = np.zeros(4, np.int64)
    for seed in range(16):
        s = guidedref.repeated_scene(seed)
        _, fwd, _ = ctx.match_host(s["q"], s["t"], 0.64)
        _, _, m, _ = ctx.match_mutual_host(s["q"], s["t"], 0.64)
        tot += (len(fwd), guidedref.correct(fwd, s), len(m), guidedref.correct(m, s))
    f, fc, m, mc = (int(v) for v in tot)
    scenes = dict(scenes=16, ratio=0.8, forward=f, forward_correct=fc, mutual=m, mutual_correct=mc, precision_forward=round(fc / f, 3), precision_mutual=round(mc / m, 3),
                  wrong_removed=round(1 - (m - mc) / (f - fc), 3), correct_removed=round(1 - mc / fc, 3))
    return dict(building_crops=crops, repeated_scenes=scenes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "cases": []}
    for pairs, rows in ((1, 1024), (1, 4096), (1, 16384), (1, 65536), (255, 2048)):
        res["cases"].append(case(ctx, pairs, rows, a.runs))
        print(json.dumps(res["cases"][-1]), flush=True)
    if not a.no_quality:
        res["quality"] = quality(ctx)
        print(json.dumps(res["quality"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

"""A first measurement of loop verification (vslam_match_pairs_dev, vslam_pair_points_dev, vslam_loop_verdict_dev).  One run on one
box; every figure is the median of --runs calls after a warm-up call, each kernel through the timing hook in calls of its own.

The indexed search does the matcher's work plus two table reads per workgroup, so it is held against the matcher ON THE SAME SETS:
the consecutive table {p, p + 1} makes vslam_match_pairs_dev compute exactly what vslam_match_dev(sets, sets + 1, n) computes.  Per
size the matcher is timed first and last and the indexed kernels between: the difference of the matcher's two medians is the
run-to-run spread the ratio is read against.  Sizes: one pair of 65,536 rows, 255 pairs of 2,048 rows, and 2,048 slots of 2,048 rows
(256 frames x 8 candidates).  Then the whole vslam_match_pairs_dev call over the 2,048 slots against the 2,048 one-pair
vslam_match_dev calls it replaces (driven from Python through ctypes, as a caller without the table would), the gather against its
byte floor (per record 12 + 24 + 24 bytes read and 24 + 24 + 12 written, at the 6.3 TB/s a float4 copy reaches on this part), and
the verdict.

  python tools/bench_loop.py [--runs 10] [--out profiles/loop_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from visualslam_amd import capi

DEV = "cuda:0"
HBM_BYTES_PER_S = 6.3e12


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


def search_case(ctx, n_pairs, rows, runs):
    """n_pairs consecutive pairs over n_pairs + 1 full sets of `rows` random descriptor rows."""
    n = n_pairs + 1
    g = torch.Generator(device=DEV).manual_seed(rows + n)
    d = torch.rand((n, rows, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((n,), rows, dtype=torch.int32, device=DEV)
    S, T = capi.desc_sets(d, counts), capi.desc_sets(d[1:], counts[1:])
    table = torch.stack([torch.arange(n_pairs, dtype=torch.int32), torch.arange(1, n, dtype=torch.int32)], dim=1).contiguous().to(DEV)
    nn_a = torch.zeros((n_pairs, rows, 3), dtype=torch.int32, device=DEV)
    nn_b = torch.zeros((n_pairs, rows, 3), dtype=torch.int32, device=DEV)
    match = lambda: ctx.match(S, T, n_pairs, 0.64, False, nn=nn_a)
    pairs = lambda: ctx.match_pairs(S, S, table, n_pairs, 0.64, False, nn=nn_b)
    first = {k: kernel_ms(ctx, k, match, runs) for k in ("k_match_nn2", "k_match_merge")}
    indexed = {k: kernel_ms(ctx, k, pairs, runs) for k in ("k_match_nn2_pairs", "k_match_merge_pairs")}
    last = {k: kernel_ms(ctx, k, match, runs) for k in ("k_match_nn2", "k_match_merge")}
    norms = dict(matcher=kernel_ms(ctx, "k_desc_norms", match, runs), indexed=kernel_ms(ctx, "k_desc_norms", pairs, runs))
    torch.cuda.synchronize()
    equal = bool(torch.equal(nn_a, nn_b))
    m1, m2, ix = sum(first.values()), sum(last.values()), sum(indexed.values())
    mid = (m1 + m2) / 2
    case = dict(pairs=n_pairs, rows=rows, matcher_first_ms=first, indexed_ms=indexed, matcher_last_ms=last, k_desc_norms_ms=norms,
                search_plus_merge_ms=dict(matcher_first=round(m1, 4), indexed=round(ix, 4), matcher_last=round(m2, 4)),
                matcher_spread=round(abs(m1 - m2) / mid, 4), indexed_over_matcher=round(ix / mid, 4),
                inside_spread=bool(min(m1, m2) <= ix <= max(m1, m2) or abs(ix - mid) / mid <= abs(m1 - m2) / mid),
                row_pairs_per_s=round(n_pairs * rows * rows / (indexed["k_match_nn2_pairs"] * 1e-3), 0), outputs_equal=equal)
    return case, (d, counts, S, table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box; medians of --runs calls", "runs": a.runs, "search": []}
    keep = None
    for n_pairs, rows in ((1, 65536), (255, 2048), (2048, 2048)):
        keep = None  # (the previous size's buffers go first)
        torch.cuda.empty_cache()
        case, keep = search_case(ctx, n_pairs, rows, a.runs)
        res["search"].append(case)
        print(json.dumps(case), flush=True)

    # the whole call over the 2,048 slots against the one-pair calls it replaces, on the last size's sets
    d, counts, S, table = keep
    slots, rows, mcap = 2048, 2048, 2048
    matches = torch.zeros((slots, mcap, 3), dtype=torch.int32, device=DEV)
    mcounts = torch.zeros(slots, dtype=torch.int32, device=DEV)
    whole = lambda: ctx.match_pairs(S, S, table, slots, 0.64, False, matches=matches, match_counts=mcounts)
    one = [(capi.desc_sets(d[p:p + 1], counts[p:p + 1]), capi.desc_sets(d[p + 1:p + 2], counts[p + 1:p + 2]), matches[p:p + 1], mcounts[p:p + 1]) for p in range(slots)]

    def singles():
        for q, t, m, c in one:
            ctx.match(q, t, 1, 0.64, False, matches=m, match_counts=c)

    w, s = timed(whole, a.runs), timed(singles, a.runs)
    res["whole_call"] = dict(slots=slots, rows=rows, match_pairs_dev_ms=w, one_pair_match_dev_calls_ms=s, calls_replaced=slots, speedup=round(s[0] / w[0], 2))
    print(json.dumps(res["whole_call"]), flush=True)

    # the gather: every slot with a full list of accepted-looking records (random indices: the worst case for the two 24-byte reads)
    g = torch.Generator(device=DEV).manual_seed(7)
    pts = torch.randint(0, 1000, (slots + 1, rows, 6), generator=g, device=DEV, dtype=torch.int32)
    matches[:, :, 0] = torch.arange(mcap, dtype=torch.int32, device=DEV)[None, :]
    matches[:, :, 1] = torch.randint(0, rows, (slots, mcap), generator=g, device=DEV, dtype=torch.int32)
    mcounts.fill_(mcap)
    qo, to = torch.zeros((slots, mcap, 6), dtype=torch.int32, device=DEV), torch.zeros((slots, mcap, 6), dtype=torch.int32, device=DEV)
    lo = torch.zeros((slots, mcap, 3), dtype=torch.int32, device=DEV)
    gather = lambda: ctx.pair_points(matches, mcounts, table, pts, pts, qo, to, lo)
    g_ms = kernel_ms(ctx, "k_pair_points", gather, a.runs)
    records = slots * mcap
    floor_ms = records * 120 / HBM_BYTES_PER_S * 1e3
    res["gather"] = dict(records=records, bytes_per_record=120, k_pair_points_ms=g_ms, call_ms=timed(gather, a.runs), byte_floor_ms=round(floor_ms, 4),
                         of_floor=round(g_ms / floor_ms, 2), gbytes_per_s=round(records * 120 / (g_ms * 1e-3) / 1e9, 1))
    print(json.dumps(res["gather"]), flush=True)

    # the verdict: one workgroup
    res["verdict"] = []
    for nq, c in ((256, 8), (65535, 8)):
        models = torch.zeros((nq * c, 22), dtype=torch.int32, device=DEV)
        models[:, 18] = 40   # n_matches
        models[:, 19] = torch.randint(0, 41, (nq * c,), generator=g, device=DEV, dtype=torch.int32)  # n_inliers
        tab = torch.stack([torch.arange(nq * c, dtype=torch.int32) // c, torch.arange(nq * c, dtype=torch.int32) % 7], dim=1).contiguous().to(DEV)
        loops, lst, nl = torch.zeros((nq, 5), dtype=torch.int32, device=DEV), torch.zeros(nq, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        verdict = lambda: ctx.loop_verdict(models, tab, nq, c, 7, loops=loops, loop_list=lst, n_loops=nl)
        case = dict(frames=nq, c=c, k_loop_verdict_ms=kernel_ms(ctx, "k_loop_verdict", verdict, a.runs), call_ms=timed(verdict, a.runs), loops=int(nl.cpu()[0]))
        res["verdict"].append(case)
        print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

"""A first measurement of vocabulary training (vslam_vocab_kmeans_dev): --sets sets (256) at the 1080p oriented_cap with noise
content (every set full of random descriptor rows), K = 1024 and K = 4096, the vocabulary sampled from the sets.  HIP events
around a call of one round and a call of --rounds rounds, 2 warm-up calls, the median of --runs calls; each kernel of a one-round
call through the timing hook, in calls of its own.

The round's assignment is the word search as vslam_words_dev enqueues it, so vslam_words_dev is measured IN THE SAME RUN: the
round's assignment kernels should cost what that call's cost.  k_kmeans_block_sums is held against its HBM floor: every assigned
row's 512 bytes read once, at the MI355X's 8 TB/s.  One run on one box.

  python tools/bench_kmeans.py [--runs 10] [--sets 256] [--rounds 4] [--out profiles/kmeans_bench.json]
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
HBM_BYTES_PER_S = 8.0e12
ASSIGN = ("k_desc_norms", "k_words_nn", "k_words_merge")
MEMBERS = ("k_kmeans_count", "k_kmeans_columns", "k_kmeans_scan", "k_kmeans_members")


def timed(fn, runs):
    for _ in range(2):
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
        launches, ms = ctx.kernel_timing_read()
        per_call.append(ms)
    ctx.kernel_timing_enable(None)
    return round(statistics.median(per_call), 4), launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--sets", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    n, cap = a.sets, capi.default_params(1080, 1920, localize=1, orient=1, do_harris=0).oriented_cap
    g = torch.Generator(device=DEV).manual_seed(n)
    d = torch.rand((n, cap, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((n,), cap, dtype=torch.int32, device=DEV)
    S = capi.desc_sets(d, counts)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box", "sets": n, "rows_per_set": cap, "runs": a.runs, "cases": []}
    words = torch.zeros((n, cap), dtype=torch.int32, device=DEV)
    for K in (1024, 4096):
        sampled = torch.zeros((K, 128), dtype=torch.float32, device=DEV)
        vdef = torch.zeros(K, dtype=torch.uint8, device=DEV)
        ctx.vocab_sample(S, sampled, vdef)
        vocab = torch.zeros((K, 128), dtype=torch.float32, device=DEV)
        hist = torch.zeros((n, K), dtype=torch.int32, device=DEV)
        sizes = torch.zeros(K, dtype=torch.int32, device=DEV)
        report = torch.zeros((a.rounds, 4), dtype=torch.int32, device=DEV)
        assign = lambda: ctx.words(S, sampled, vdef, words=words, hist=hist)
        one = lambda: ctx.vocab_kmeans(S, sampled, 1, vdef, vocab=vocab, sizes=sizes, report=report[:1])
        many = lambda: ctx.vocab_kmeans(S, sampled, a.rounds, vdef, vocab=vocab, sizes=sizes, report=report)
        case = {"K": K, "words_ms": timed(assign, a.runs), "kmeans_1_round_ms": timed(one, a.runs), "rounds": a.rounds,
                "kmeans_rounds_ms": timed(many, a.runs), "kernels": {}, "words_call_kernels": {}}
        case["report"] = report.cpu().tolist()
        for name in ASSIGN:
            ms, launches = kernel_ms(ctx, name, assign, a.runs)
            case["words_call_kernels"][name] = {"ms": ms, "launches": launches}
        for name in ASSIGN + ("k_kmeans_init",) + MEMBERS + ("k_kmeans_block_sums", "k_kmeans_update"):
            ms, launches = kernel_ms(ctx, name, one, a.runs)
            case["kernels"][name] = {"ms": ms, "launches": launches}
        k = case["kernels"]
        assigned = int(sizes.sum())
        floor_ms = assigned * 512 / HBM_BYTES_PER_S * 1e3
        s_ms = k["k_kmeans_block_sums"]["ms"]
        case["per_round"] = dict(assignment_ms=round(sum(k[x]["ms"] for x in ASSIGN), 4),
                                 words_call_assignment_ms=round(sum(case["words_call_kernels"][x]["ms"] for x in ASSIGN), 4),
                                 member_list_ms=round(sum(k[x]["ms"] for x in MEMBERS), 4), block_sums_ms=s_ms, update_ms=k["k_kmeans_update"]["ms"])
        case["k_kmeans_block_sums"] = dict(assigned_rows=assigned, bytes=assigned * 512, hbm_floor_ms=round(floor_ms, 4),
                                           fraction_of_hbm_peak=round(floor_ms / s_ms, 3) if s_ms else None)
        case["largest_word"] = int(sizes.max())
        case["empty_words"] = int((sizes == 0).sum())
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

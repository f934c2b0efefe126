"""A first measurement of place recognition (vslam_vocab_sample_dev, vslam_words_dev, vslam_place_dev): --sets sets (256) at the
1080p oriented_cap with noise content (every set full of random descriptor rows), K = 1024 and K = 4096.  HIP events around each
call, 2 warm-up calls, the median of --runs calls; each kernel through the timing hook, in calls of its own.

The word search is the matcher's loop, so its rate is held against the matcher's IN THE SAME RUN: k_words_nn's (row x word) pairs
per second against k_match_nn2's (query x train) pairs per second over --match-pairs consecutive sets of the same descriptors.
k_place_score is held against its LDS-read floor: per four word steps a lane reads three 16-byte operands, and a compute unit's
LDS delivers 256 bytes per clock to ds_read_b128 (MI355X: 256 compute units, 2.4 GHz).  One run on one box.

  python tools/bench_place.py [--runs 10] [--sets 256] [--match-pairs 16] [--out profiles/place_bench.json]
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
CUS, CLOCK_HZ, LDS_B128_BYTES_PER_CLK = 256, 2.4e9, 256


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
    ap.add_argument("--match-pairs", type=int, default=16)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    n, cap = a.sets, capi.default_params(1080, 1920, localize=1, orient=1, do_harris=0).oriented_cap
    g = torch.Generator(device=DEV).manual_seed(n)
    d = torch.rand((n, cap, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((n,), cap, dtype=torch.int32, device=DEV)
    S = capi.desc_sets(d, counts)
    res = {"device": torch.cuda.get_device_name(0), "note": "one run on one box", "sets": n, "rows_per_set": cap, "runs": a.runs, "cases": []}

    # the matcher on the same descriptors, for the comparison
    mp = min(a.match_pairs, n - 1)
    nn = torch.zeros((mp, cap, 3), dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:mp], counts), capi.desc_sets(d[1:mp + 1], counts[1:])
    match = lambda: ctx.match(Q, T, mp, 0.64, False, nn=nn)
    m_ms, _ = kernel_ms(ctx, "k_match_nn2", match, a.runs)
    res["matcher"] = dict(pairs=mp, rows=cap, k_match_nn2_ms=m_ms, row_pairs_per_s=round(mp * cap * cap / (m_ms * 1e-3), 0))
    print(json.dumps(res["matcher"]), flush=True)
    del nn

    words = torch.zeros((n, cap), dtype=torch.int32, device=DEV)
    for K in (1024, 4096):
        vocab = torch.zeros((K, 128), dtype=torch.float32, device=DEV)
        vdef = torch.zeros(K, dtype=torch.uint8, device=DEV)
        hist = torch.zeros((n, K), dtype=torch.int32, device=DEV)
        cands = torch.zeros((n, 3, 3), dtype=torch.int32, device=DEV)
        cc = torch.zeros(n, dtype=torch.int32, device=DEV)
        sample = lambda: ctx.vocab_sample(S, vocab, vdef)
        assign = lambda: ctx.words(S, vocab, vdef, words=words, hist=hist)
        place = lambda: ctx.place(hist, None, min_gap=4, max_candidates=3, num=1, den=5, candidates=cands, cand_counts=cc)
        case = {"K": K, "vocab_sample_ms": timed(sample, a.runs), "words_ms": timed(assign, a.runs), "place_ms": timed(place, a.runs), "kernels": {}}
        for name, fn in (("k_vocab_gather", sample), ("k_desc_norms", assign), ("k_words_nn", assign), ("k_words_merge", assign), ("k_place_df", place),
                         ("k_place_self", place), ("k_place_score", place), ("k_place_top", place)):
            ms, launches = kernel_ms(ctx, name, fn, a.runs)
            case["kernels"][name] = {"ms": ms, "launches": launches}
        w_ms = case["kernels"]["k_words_nn"]["ms"]
        rate = n * cap * K / (w_ms * 1e-3)
        case["k_words_nn"] = dict(row_word_pairs_per_s=round(rate, 0), tflops=round(256 * rate / 1e12, 2),
                                  of_k_match_nn2_rate=round(rate / res["matcher"]["row_pairs_per_s"], 3))
        # the 16 x 16 tiles that run (min_gap 4 on one batch: a tile whose first db frame + 4 is past its last query frame is skipped),
        # every (i, j) of them, K rounded up to the 128-word chunk
        tiles = sum(1 for ti in range((n + 15) // 16) for tj in range((n + 15) // 16) if 16 * tj + 4 <= min(16 * ti + 15, n - 1))
        steps = tiles * 256 * ((K + 127) // 128 * 128)
        floor_ms = steps / 4 * 48 / (CUS * CLOCK_HZ * LDS_B128_BYTES_PER_CLK) * 1e3
        s_ms = case["kernels"]["k_place_score"]["ms"]
        case["k_place_score"] = dict(word_steps=steps, lds_read_floor_ms=round(floor_ms, 4), of_floor=round(s_ms / floor_ms, 2), tiles_run=tiles,
                                     tiles_all=((n + 15) // 16) ** 2)
        case["assigned_rows"] = int(hist.sum())
        case["frames_with_candidates"] = int((cc > 0).sum())
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

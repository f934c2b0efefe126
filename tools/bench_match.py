"""Throughput of descriptor matching (vslam_match_dev): one-pair calls at 1 k / 4 k / 16 k / 64 k rows, 255 pairs at 2 k rows,
and the consecutive-frame matching of bench.py's describe content (every second frame uniform noise) with the step time of
describe alone and of describe + match.  HIP events around each call, 2 warm-up calls, the median of --runs calls.
Rates are 2 * 128 * nq * nt * pairs / time over the rows in use, against the 157.3 TF f32 peak and the 122 TF of an untuned
f32-MFMA GEMM (cdna_hip_programming.md section 3).

  python tools/bench_match.py [--runs 10] [--frames 256] [--out profiles/match_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from visualslam_amd import capi, synth

PEAK_TF, GEMM_TF = 157.3, 122.0
DEV = "cuda:0"


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
    return statistics.median(ms), min(ms), max(ms)


def rate(flop, ms):
    tf = flop / (ms * 1e-3) / 1e12
    return {"tflops": round(tf, 2), "of_f32_peak": round(tf / PEAK_TF, 3), "of_untuned_mfma_gemm": round(tf / GEMM_TF, 3)}


def synthetic_case(ctx, pairs, rows, runs):
    g = torch.Generator(device=DEV).manual_seed(rows + pairs)
    d = torch.rand((pairs + 1, rows, 128), generator=g, device=DEV, dtype=torch.float32).clamp_(max=0.2).mul_(5.0)
    counts = torch.full((pairs + 1,), rows, dtype=torch.int32, device=DEV)
    nn = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    matches = torch.zeros((pairs, rows, 3), dtype=torch.int32, device=DEV)
    mc = torch.zeros(pairs, dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:pairs], counts), capi.desc_sets(d[1:], counts[1:])
    med, lo, hi = timed(lambda: ctx.match(Q, T, pairs, 0.64, False, nn=nn, matches=matches, match_counts=mc), runs)
    return dict(pairs=pairs, rows=rows, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), runs=runs,
                accepted=int(mc.sum()), **rate(2.0 * 128 * rows * rows * pairs, med))


def describe_case(ctx, n, runs):
    rows, cols = 1080, 1920
    p = capi.default_params(rows, cols, localize=1, orient=1, do_harris=0)
    L = capi.batch_layout(p)
    frames = synth.frames_torch(n, rows, cols, stream_id=0, device=DEV, noise_every=2)
    cap = p.oriented_cap
    o = dict(pyramid=torch.empty((n, L.pyramid_frame_bytes), dtype=torch.uint8, device=DEV),
             dog_points=torch.zeros((n, p.dog_cap, 6), dtype=torch.int32, device=DEV), dog_counts=torch.zeros(n, dtype=torch.int32, device=DEV),
             oriented_points=torch.zeros((n, cap, 6), dtype=torch.int32, device=DEV), oriented_counts=torch.zeros(n, dtype=torch.int32, device=DEV),
             descriptors=torch.zeros((n, cap, 128), dtype=torch.float32, device=DEV), descriptor_defined=torch.zeros((n, cap), dtype=torch.uint8, device=DEV))
    matches = torch.zeros((n - 1, cap, 3), dtype=torch.int32, device=DEV)
    mc = torch.zeros(n - 1, dtype=torch.int32, device=DEV)
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    out = {"content": "bench.py's describe content: 1080p camera stream, every second frame uniform noise", "frames": n}
    for same_octave in (0, 1):
        Q, T = capi.desc_sets(d, c, df, pts), capi.desc_sets(d[1:], c[1:], df[1:], pts[1:])
        detect = lambda: ctx.detect_batch(p, frames, **o)
        match = lambda: ctx.match(Q, T, n - 1, 0.64, bool(same_octave), matches=matches, match_counts=mc)
        t_detect = timed(detect, runs)[0]
        t_match = timed(match, runs)[0]
        t_both = timed(lambda: (detect(), match()), runs)[0]
        cnt = c.cpu().clamp(max=cap).double()
        flop = 2.0 * 128 * float((cnt[:-1] * cnt[1:]).sum())
        out["same_octave" if same_octave else "all_octaves"] = dict(
            descriptors_per_step=int(cnt.sum()), accepted_per_step=int(mc.sum()), match_ms=round(t_match, 3), describe_ms=round(t_detect, 3),
            describe_plus_match_ms=round(t_both, 3), describe_frames_per_s=round(n / t_detect * 1e3, 1),
            describe_plus_match_frames_per_s=round(n / t_both * 1e3, 1), full_product=rate(flop, t_match),
            note="full_product counts every row pair; with same_octave most of them are masked in the epilogue, not skipped" if same_octave else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    res = {"device": torch.cuda.get_device_name(0), "f32_peak_tflops": PEAK_TF, "untuned_f32_mfma_gemm_tflops": GEMM_TF, "cases": []}
    for pairs, rows in ((1, 1024), (1, 4096), (1, 16384), (1, 65536), (255, 2048)):
        res["cases"].append(synthetic_case(ctx, pairs, rows, a.runs))
        print(json.dumps(res["cases"][-1]), flush=True)
    if a.frames > 1:
        res["describe"] = describe_case(ctx, a.frames, a.runs)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()

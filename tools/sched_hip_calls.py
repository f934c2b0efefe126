#!/usr/bin/env python3
"""The stream and event calls the library makes around its batch calls, as a sequence: the proof that a change to the
side-stream scheduling (csrc/vslam_sched.cpp) left the order of creation, records and waits alone (queue placement depends
on the order of creation).

  rocprofv3 --hip-trace --output-format csv -d OUT -o parent -- python tools/sched_hip_calls.py run   (VSLAM_LIBRARY = the parent's build)
  rocprofv3 --hip-trace --output-format csv -d OUT -o new -- python tools/sched_hip_calls.py run      (VSLAM_LIBRARY = this build)
  python tools/sched_hip_calls.py compare OUT/parent_hip_api_trace.csv OUT/new_hip_api_trace.csv

run: seven 32 x 120 x 160 batch calls on a context with yielding side streams and the tuner on, then two 64 x 270 x 480 calls
with localize = 1, orient = 1 on a default context; then, for the plan of a chunk (csrc/vslam_batch_plan.h): a 300-frame and a
260-frame 40 x 56 call with localize = 1, orient = 1 (two chunks: both orientation forks, a second chunk with the plan of the
first and one with another), a 320-frame 40 x 56 call (the second chunk's second half waits for ev_chunk), a 300-frame
96 x 160 call on the matrix path in candidates mode (the ev_pack wait of a later chunk) and one single-image Pyramid; each context is closed.  compare: the calls named in CALLS plus
every kernel launch and asynchronous copy (is_enqueue), in trace order - so the interleaving of launches with records and
waits is compared too (function names are compared; handles are not numbered).  Runs of consecutive destroys - a
context's teardown, the tuner's losing pairs - are compared as counts: their internal order is free.
"""
import collections
import csv
import os
import sys

CALLS = ("hipStreamCreateWithPriority", "hipStreamCreateWithFlags", "hipEventCreate", "hipEventCreateWithFlags", "hipEventRecord",
         "hipStreamWaitEvent", "hipEventQuery", "hipEventElapsedTime", "hipEventDestroy", "hipStreamDestroy")


def is_enqueue(f):
    """Kernel launches and asynchronous copies, under whatever name the trace gives them (hipLaunchKernel, hipModuleLaunchKernel,
    hipExtLaunchKernel, ...; hipMemcpyAsync, hipMemcpy2DAsync, hipMemcpyDtoDAsync, ...)."""
    return "LaunchKernel" in f or (f.startswith("hipMemcpy") and f.endswith("Async"))


def run():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    import torch

    from visualslam_amd import capi, synth

    dev = "cuda:0"

    def calls(ctx, n, rows, cols, reps, **pkw):
        p = capi.default_params(rows, cols, **pkw)
        L = capi.batch_layout(p)
        frames = torch.from_numpy(synth.frames_np(n, rows, cols, stream_id=5)).to(dev)
        o = dict(response=torch.empty((n, rows, cols), dtype=torch.float32, device=dev), nms_mask=torch.empty((n, rows, cols), dtype=torch.uint8, device=dev),
                 harris_kps=torch.zeros((n, p.harris_cap, 3), dtype=torch.int32, device=dev), harris_counts=torch.zeros(n, dtype=torch.int32, device=dev),
                 pyramid=torch.empty((n, L.pyramid_frame_bytes), dtype=torch.uint8, device=dev),
                 extrema_bits=torch.zeros((n, max(L.bits_frame_words, 1)), dtype=torch.int64, device=dev),
                 dog_points=torch.zeros((n, p.dog_cap, 6), dtype=torch.int32, device=dev), dog_counts=torch.zeros(n, dtype=torch.int32, device=dev))
        if p.orient:
            o.update(oriented_points=torch.zeros((n, p.oriented_cap, 6), dtype=torch.int32, device=dev), oriented_counts=torch.zeros(n, dtype=torch.int32, device=dev))
        for _ in range(reps):
            ctx.detect_batch(p, frames, **o)
            torch.cuda.synchronize()
        return int(o["dog_counts"].sum())

    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    ctx.set_side_stream_priority(True)
    ctx.tune_side_streams(True)
    a = calls(ctx, 32, 120, 160, 7)
    print("tuner", ctx.side_stream_report(), "watch", ctx.join_watch_report())
    ctx.close()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    b = calls(ctx, 64, 270, 480, 2, localize=1, orient=1)
    small = dict(n_octaves=2, harris_cap=1024, dog_cap=2048, localize=1, orient=1)
    c3 = calls(ctx, 300, 40, 56, 1, **small)
    c4 = calls(ctx, 260, 40, 56, 1, **small)
    c6 = calls(ctx, 320, 40, 56, 1, n_octaves=2, harris_cap=1024, dog_cap=2048)  # a second chunk of 64 frames: upsampled in halves
    ctx.set_matrix_path(True)
    c5 = calls(ctx, 300, 96, 160, 1, n_octaves=3)
    ctx.set_matrix_path(False)
    py = capi.Pyramid(ctx, synth.frame_np(120, 160, kind="noise"), 3)
    py.close()
    ctx.close()
    print("library", capi.LIB_PATH, "dog points", a, b, c3, c4, c6, c5)


def sequence(path):
    rows = [r for r in csv.DictReader(open(path)) if r["Function"] in CALLS or is_enqueue(r["Function"])]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    seq = []
    for r in rows:
        f = r["Function"]
        if f.endswith("Destroy"):
            if not seq or not isinstance(seq[-1], collections.Counter):
                seq.append(collections.Counter())
            seq[-1][f] += 1
        else:
            seq.append(f)
    return seq


def compare(pa, pb):
    a, b = sequence(pa), sequence(pb)
    for name, s in (("parent", a), ("new", b)):
        c = collections.Counter()
        for x in s:
            c.update(x if isinstance(x, collections.Counter) else [x])
        print(name, len(s), "entries;", ", ".join(f"{k} {c[k]}" for k in (*CALLS, *sorted(k for k in c if is_enqueue(k)))))
    plain = lambda s: [x for x in s if not isinstance(x, collections.Counter)]
    same = plain(a) == plain(b)
    print("create / record / wait / query calls, kernel launches and asynchronous copies, in order:", "identical" if same else "DIFFERENT")
    if not same:
        for i, (x, y) in enumerate(zip(plain(a), plain(b))):
            if x != y:
                print("  first difference at entry", i, ":", x, "->", y)
                break
    where = lambda s: [i for i, x in enumerate(s) if isinstance(x, collections.Counter)]
    print("runs of destroys at the same places:", where(a) == where(b))
    for x, y in zip((s for s in a if isinstance(s, collections.Counter)), (s for s in b if isinstance(s, collections.Counter))):
        print("  parent", dict(x), "new", dict(y), "" if x == y else "<- differs")
    return 0 if same and where(a) == where(b) else 1


if __name__ == "__main__":
    sys.exit(run() if sys.argv[1] == "run" else compare(sys.argv[2], sys.argv[3]))

"""bench.py's plain run and its --dump-outputs files: what the timed path computed in its last step, sampled from a fixed
seed so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _fake_outputs(torch, capi, rows, cols, n, n_oct):
    """Output buffers of one batch as a caller allocates them, filled with noise (host tensors)."""
    p = capi.default_params(rows, cols, n_octaves=n_oct)
    L = capi.batch_layout(p)
    g = torch.Generator().manual_seed(7)
    out = dict(
        response=torch.randn((n, rows, cols), generator=g),
        nms_mask=torch.randint(0, 256, (n, rows, cols), dtype=torch.uint8, generator=g),
        harris_kps=torch.randint(0, 1 << 20, (n, p.harris_cap, 3), dtype=torch.int32, generator=g),
        harris_counts=torch.tensor(([p.harris_cap + 3, 5] + [17] * n)[:n], dtype=torch.int32),
        pyramid=torch.randint(0, 256, (n, L.pyramid_frame_bytes), dtype=torch.uint8, generator=g),
        extrema_bits=torch.randint(-(1 << 62), 1 << 62, (n, max(L.bits_frame_words, 1)), dtype=torch.int64, generator=g),
        dog_points=torch.randint(0, 1 << 20, (n, p.dog_cap, 6), dtype=torch.int32, generator=g),
        dog_counts=torch.randint(0, 4000, (n,), dtype=torch.int32, generator=g),
    )
    return p, L, out


def test_dump_outputs_layout_and_determinism(tmp_path):
    torch = pytest.importorskip("torch")
    import bench
    from visualslam_amd import capi

    # 100 x 130: every octave's planes are pitched (260 -> 272, 130 -> 144, 65 -> 80), and two frames are few enough
    # that the samples take every element: the files can be checked element by element
    rows, cols, n, n_oct = 100, 130, 2, 3
    p, L, out = _fake_outputs(torch, capi, rows, cols, n, n_oct)
    bench.dump_outputs(str(tmp_path / "a"), out, p, L)
    bench.dump_outputs(str(tmp_path / "b"), out, p, L)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(k + ".npy" for k in out)
    total = 0
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.array_equal(a, b), f  # same arguments, same elements
        total += a.nbytes
    assert total <= 64 << 20
    load = lambda k: np.load(tmp_path / "a" / (k + ".npy"))
    assert np.array_equal(load("harris_counts"), out["harris_counts"].numpy().astype(np.float64))
    assert np.array_equal(load("response"), out["response"].numpy().reshape(-1))
    assert np.array_equal(load("nms_mask"), out["nms_mask"].numpy().reshape(-1).astype(np.float32))
    # lists: min(count, cap) records of every frame (n <= 4), led by the frame index, list order
    kp = load("harris_kps")
    assert len(kp) == p.harris_cap + 5
    f0 = kp[kp[:, 0] == 0]
    rec = out["harris_kps"][0].numpy().view(capi.KP_DTYPE).reshape(-1)
    assert len(f0) == p.harris_cap and np.array_equal(f0[:, 1], rec["row"].astype(np.float32))
    assert np.array_equal(f0[:, 3], rec["response"])
    dp = load("dog_points")
    rec = out["dog_points"][1, : int(out["dog_counts"][1])].numpy().view(capi.POINT_DTYPE).reshape(-1)
    assert np.array_equal(dp[dp[:, 0] == 1][:, 1:], np.stack([rec[k] for k in ("row", "col", "value", "octave", "level")], 1).astype(np.float32))
    # pyramid: the defined bytes only, in (frame, octave, plane, row, col) order
    pyr = out["pyramid"].numpy()
    want = []
    for f in range(n):
        for o in range(L.n_octaves):
            r, c, pt, off = L.rows[o], L.cols[o], L.pitch[o], L.octave_offset[o]
            assert pt > c
            want.append(pyr[f, off: off + 11 * r * pt].reshape(11, r, pt)[:, :, :c].reshape(-1))
    assert np.array_equal(load("pyramid"), np.concatenate(want).astype(np.float32))
    # candidate masks: every word, the bits past a lattice row's end cleared, as (low, high) halves
    bits = out["extrema_bits"].numpy().view(np.uint64)
    want = []
    for f in range(n):
        for o in range(L.n_octaves):
            lr, lc, lw = L.lat_rows[o], L.lat_cols[o], L.lat_words[o]
            w = bits[f, L.bits_offset[o]: L.bits_offset[o] + 3 * lr * lw].reshape(3, lr, lw)
            u = np.unpackbits(w.view(np.uint8).reshape(3, lr, lw * 8), axis=-1, bitorder="little")
            u[..., lc:] = 0
            want.append(np.packbits(u, axis=-1, bitorder="little").view(np.uint64).reshape(-1))
    assert np.array_equal(load("extrema_bits"), np.concatenate(want).view(np.uint32).reshape(-1, 2).astype(np.float64))


def test_dump_outputs_stays_under_64_mb_at_the_headline_size(tmp_path):
    torch = pytest.importorskip("torch")
    import bench
    from visualslam_amd import capi

    # 1080p with every list at its capacity: the samples and the per-frame record limit bound the files
    p, L, out = _fake_outputs(torch, capi, 1080, 1920, 4, 4)
    out["harris_counts"].fill_(p.harris_cap)
    out["dog_counts"].fill_(p.dog_cap)
    bench.dump_outputs(str(tmp_path), out, p, L)
    assert sum(np.load(tmp_path / f).nbytes for f in os.listdir(tmp_path)) <= 64 << 20


def _line(stdout):
    return json.loads([l for l in stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_bench_is_lean_and_dumps_what_it_computed(tmp_path):
    import oracle
    from visualslam_amd import synth

    rows, cols, n, n_oct, steps = 240, 320, 6, 4, 3
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--frames", str(n), "--rows", str(rows), "--cols", str(cols),
            "--octaves", str(n_oct), "--steps", str(steps), "--warmup", "2"]
    lines = []
    for d in ("a", "b"):
        r = subprocess.run(args + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(_line(r.stdout))
    d = lines[0]
    assert d["steps"] == steps and d["full"] is False and d["ms_per_step"] > 0 and d["value"] > 0
    assert abs(d["value"] - n * steps / (d["ms_per_step"] * steps * 1e-3)) < 1e-6 * d["value"]
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert d[k] is not None, k
    # nothing but the headline ran
    assert d["roofline"] is None and d["modes"] is None and d["two_in_flight"] is None and d["mx_path"] is None
    assert d["cpu_baseline"] is None and "cxx_host" not in d and "config2_harris_only" not in d
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"response.npy", "nms_mask.npy", "harris_kps.npy", "harris_counts.npy", "pyramid.npy", "extrema_bits.npy",
            "dog_points.npy", "dog_counts.npy"} <= set(names)
    for f in names:  # two runs, the same inputs: the same outputs
        a = np.load(tmp_path / "a" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, np.load(tmp_path / "b" / f)), f
    # the files hold what the path computed: counts and lists against the oracle on the same synthetic frames
    frames = synth.frames_np(n, rows, cols, stream_id=0)
    hc, dc = np.load(tmp_path / "a" / "harris_counts.npy"), np.load(tmp_path / "a" / "dog_counts.npy")
    kp, dp = np.load(tmp_path / "a" / "harris_kps.npy"), np.load(tmp_path / "a" / "dog_points.npy")
    sel = np.unique(kp[:, 0]).astype(int)
    assert len(sel) == 4
    for f in sel:
        want_k = oracle.harris_keypoints(oracle.nms2(oracle.harris_response(frames[f]), 5)[0])
        assert hc[f] == len(want_k)
        got = kp[kp[:, 0] == f]
        assert np.array_equal(got[:, 1:3], np.stack([want_k["row"], want_k["col"]], 1).astype(np.float32))
        assert np.array_equal(got[:, 3], want_k["response"])
        pyr = oracle.Pyramid(frames[f], n_oct, 1.6)
        want_p = np.concatenate([pyr.extrema(o, 3, 8)[1] for o in range(n_oct)])
        assert dc[f] == len(want_p)
        got = dp[dp[:, 0] == f]
        assert np.array_equal(got[:, 1:], np.stack([want_p[k] for k in ("row", "col", "value", "octave", "level")], 1).astype(np.float32))

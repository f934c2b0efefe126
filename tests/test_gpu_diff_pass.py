"""The difference-form horizontal pass of octaves 2-3 (k_gauss_h_diff, kernels_hdiff.hip.h) against the CPU oracle: 1080p,
odd sizes, frames narrower than one kernel (reflect-101 over the whole row), the extreme frames of the exactness bound,
and the diagnostics build's dot2 pass (VSLAM_HDIFF=0) equal byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from visualslam_amd import capi, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield ctx, torch
    ctx.close()


def run_pyramid(ctx, torch, frames_np, n_oct):
    n, rows, cols = frames_np.shape
    p = capi.default_params(rows, cols, n_octaves=n_oct)
    L = capi.batch_layout(p)
    dev = "cuda:0"
    o = dict(
        response=torch.empty((n, rows, cols), dtype=torch.float32, device=dev),
        nms_mask=torch.empty((n, rows, cols), dtype=torch.uint8, device=dev),
        harris_kps=torch.zeros((n, p.harris_cap, 3), dtype=torch.int32, device=dev),
        harris_counts=torch.zeros(n, dtype=torch.int32, device=dev),
        pyramid=torch.empty((n, L.pyramid_frame_bytes), dtype=torch.uint8, device=dev),
        dog_points=torch.zeros((n, p.dog_cap, 6), dtype=torch.int32, device=dev),
        dog_counts=torch.zeros(n, dtype=torch.int32, device=dev),
    )
    ctx.detect_batch(p, torch.from_numpy(frames_np).to(dev), **o)
    torch.cuda.synchronize()
    return L, o["pyramid"].cpu().numpy()


def planes(L, block, o):
    """The 11 planes (6 Gaussian, 5 DoG) of octave o of one frame's block, padding cut."""
    r, c, pitch = L.rows[o], L.cols[o], L.pitch[o]
    P = r * pitch
    off = L.octave_offset[o]
    return [block[off + k * P: off + (k + 1) * P].reshape(r, pitch)[:, :c] for k in range(11)]


def check_octaves(L, pyr, frames_np, n_oct, octaves):
    for f in range(len(frames_np)):
        want = oracle.Pyramid(frames_np[f], n_oct, 1.6)
        for o in octaves:
            got = planes(L, pyr[f], o)
            for l in range(6):
                assert (got[l] == want.gauss(o, l)).all(), ("gauss", f, o, l)
            for l in range(5):
                assert (got[6 + l] == want.dog(o, l)).all(), ("dog", f, o, l)
        want.close()


def test_difference_pass_is_dispatched_at_1080p(env):
    ctx, torch = env
    ctx.kernel_timing_enable("k_gauss_h_diff")
    run_pyramid(ctx, torch, synth.frames_np(1, 1080, 1920, stream_id=3), 4)
    launches, ms = ctx.kernel_timing_read()
    ctx.kernel_timing_enable(None)
    assert launches == 2 and ms > 0  # octaves 2 and 3


@pytest.mark.parametrize("rows,cols,n", [(1080, 1920, 2), (541, 961, 3), (1081, 1923, 1)])
def test_octaves_1_to_3_match_oracle(env, rows, cols, n):
    ctx, torch = env
    frames = synth.frames_np(n, rows, cols, stream_id=rows + cols)
    L, pyr = run_pyramid(ctx, torch, frames, 4)
    check_octaves(L, pyr, frames, 4, (1, 2, 3))


@pytest.mark.parametrize("rows,cols", [(120, 200), (64, 90), (37, 41)])
def test_frames_narrower_than_one_kernel(env, rows, cols):
    # octave 2 of a 200-column frame is 100 columns wide against kernels of up to 111 taps, octave 3 50 against 223
    ctx, torch = env
    frames = synth.frames_np(2, rows, cols, stream_id=cols)
    L, pyr = run_pyramid(ctx, torch, frames, 4)
    assert L.cols[3] < 223 // 2
    check_octaves(L, pyr, frames, 4, (2, 3))


@pytest.mark.parametrize("value", [0, 255])
def test_constant_frames_at_the_exactness_bound(env, value):
    # all-255: every row sum is 255 * 256 + 128 = 65408, the largest the bound allows for; all-0: the smallest (128)
    ctx, torch = env
    frames = np.full((2, 541, 961), value, np.uint8)
    L, pyr = run_pyramid(ctx, torch, frames, 4)
    for f in range(2):
        for o in (1, 2, 3):
            got = planes(L, pyr[f], o)
            for l in range(6):
                assert (got[l] == value).all(), (f, o, l)
            for l in range(5):
                assert (got[6 + l] == 0).all(), (f, o, l)
    check_octaves(L, pyr[:1], frames[:1], 4, (2, 3))


_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from visualslam_amd import capi, synth
rows, cols, out = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
frames = synth.frames_np(2, rows, cols, stream_id=11)
frames[1, : rows // 2] = 255
p = capi.default_params(rows, cols, n_octaves=4)
L = capi.batch_layout(p)
pyr = torch.empty((2, L.pyramid_frame_bytes), dtype=torch.uint8, device="cuda:0")
kw = dict(response=torch.empty((2, rows, cols), dtype=torch.float32, device="cuda:0"),
          nms_mask=torch.empty((2, rows, cols), dtype=torch.uint8, device="cuda:0"),
          harris_kps=torch.zeros((2, p.harris_cap, 3), dtype=torch.int32, device="cuda:0"),
          harris_counts=torch.zeros(2, dtype=torch.int32, device="cuda:0"),
          dog_points=torch.zeros((2, p.dog_cap, 6), dtype=torch.int32, device="cuda:0"),
          dog_counts=torch.zeros(2, dtype=torch.int32, device="cuda:0"))
ctx.detect_batch(p, torch.from_numpy(frames).to("cuda:0"), pyramid=pyr, **kw)
torch.cuda.synchronize()
planes = []
for f in range(2):
    for o in range(4):
        r, c, pitch, off = L.rows[o], L.cols[o], L.pitch[o], L.octave_offset[o]
        blk = pyr[f].cpu().numpy()[off: off + 11 * r * pitch].reshape(11, r, pitch)[:, :, :c]
        planes.append(blk.reshape(-1))
np.save(out, np.concatenate(planes))
ctx.close()
"""


@pytest.mark.parametrize("rows,cols", [(1080, 1920), (541, 961)])
def test_diagnostics_build_old_and_new_pass_equal(tmp_path, rows, cols):
    # VSLAM_HDIFF=0 (diagnostics build only) keeps the dot2 pass: every valid byte of the pyramid must be the same
    res = {}
    for tag, extra in (("new", {}), ("old", {"VSLAM_HDIFF": "0"})):
        out = str(tmp_path / f"{tag}.npy")
        env = dict(os.environ, VSLAM_LIBRARY=capi.DIAG_LIB_PATH)
        env.pop("VSLAM_HDIFF", None)
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(rows), str(cols), out], capture_output=True, text=True,
                           timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        res[tag] = np.load(out)
    assert res["new"].shape == res["old"].shape
    assert res["new"].tobytes() == res["old"].tobytes()

"""Octave 1 of the default pyramid through k_pyr_octave with its taps compiled in (PyrCfgConst, kernels_pyramid.hip.h),
byte for byte against the CPU oracle.  Octave 1 has the size of the frame itself, so the frame chooses the tile shape:
272 x 200 runs the 128 x 64 tiles (3 x 4 of them, every one a border tile), 520 x 72 the 256 x 32 tiles (3 x 3, the last
column 8 pixels wide).  Two frames of seeded noise; all 11 planes (six Gaussian, five DoG) of octave 1 are compared, and
octave 0's with them (the table-driven instantiations, which this change must leave alone)."""
import numpy as np
import pytest

import oracle
from visualslam_amd import capi

pytestmark = pytest.mark.gpu

N_OCT = 2
# (cols, rows) of the frame = of octave 1
CASES = [(272, 200), (520, 72)]


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield ctx, torch
    ctx.close()


def planes(L, block, o):
    """The 11 planes (6 Gaussian, 5 DoG) of octave o of one frame's block, padding cut."""
    r, c, pitch = L.rows[o], L.cols[o], L.pitch[o]
    P = r * pitch
    off = L.octave_offset[o]
    return [block[off + k * P: off + (k + 1) * P].reshape(r, pitch)[:, :c] for k in range(11)]


@pytest.mark.parametrize("cols,rows", CASES, ids=[f"{c}x{r}" for c, r in CASES])
def test_octave_1_matches_the_oracle(env, cols, rows):
    ctx, torch = env
    n = 2
    frames = np.random.default_rng(1000 * cols + rows).integers(0, 256, (n, rows, cols), dtype=np.uint8)
    p = capi.default_params(rows, cols, n_octaves=N_OCT)
    L = capi.batch_layout(p)
    assert (L.rows[1], L.cols[1]) == (rows, cols)
    dev = "cuda:0"
    pyr = torch.full((n, L.pyramid_frame_bytes), 0xA5, dtype=torch.uint8, device=dev)
    ctx.kernel_timing_enable("k_pyr_octave@1")
    ctx.detect_batch(p, torch.from_numpy(frames).to(dev), pyramid=pyr)
    torch.cuda.synchronize()
    launches, _ = ctx.kernel_timing_read()
    ctx.kernel_timing_enable(None)
    assert launches == 1, "octave 1 did not run the LDS-tiled octave kernel"
    got_all = pyr.cpu().numpy()
    for f in range(n):
        want = oracle.Pyramid(frames[f], N_OCT, 1.6)
        try:
            for o in (1, 0):
                assert (L.rows[o], L.cols[o]) == tuple(want.sizes[o])
                got = planes(L, got_all[f], o)
                for l in range(6):
                    assert got[l].tobytes() == np.ascontiguousarray(want.gauss(o, l)).tobytes(), ("gauss", f, o, l)
                for l in range(5):
                    assert got[6 + l].tobytes() == np.ascontiguousarray(want.dog(o, l)).tobytes(), ("dog", f, o, l)
        finally:
            want.close()

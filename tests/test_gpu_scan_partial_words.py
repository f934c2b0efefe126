"""The lattice scan of the batch call's plain candidate mode (k_extrema_w3<false>, kernels_aux.hip.h) with the list it feeds,
on lattice rows whose last ballot word is partial.  The scan forms the mask of the lanes that own a site once, on the scalar
unit, from the word's index; takes column -1 of a row (which replicates column 0) through the first site's byte selector
instead of a staged byte; and writes a wave's six words from scalar indices.

Shapes: one octave whose lattice is 3 rows of 190 columns (three words, the last holds 62 sites; the workgroup's fourth wave
owns no word) and of 196 columns (four words, the last holds 4 sites), and one of 27 rows of 196 columns, whose 324 list
words span two chunks of the compaction with a level boundary inside a chunk.  A batch is three frames with unequal counts:
a constant image (every site is a candidate at every level; with min_contrast 0 every site is listed as well, so every
list word is full up to the row's last site), a frame of noise, and a frame that is noise on its left half only.

Checked per frame: the candidate masks against the CPU oracle; the list and its count against the oracle; and both against
vslam_dog_extrema on the same image (the single-image entry point: its own launch of the scan, count -> scan -> scatter
over one frame)."""
import numpy as np
import pytest

import oracle
from visualslam_amd import capi

pytestmark = pytest.mark.gpu

# (frame rows, frame cols) -> octave 0 is twice that; (lattice rows, lattice cols) of octave 0
SHAPES = {190: ((5, 285), (3, 190)), 196: ((5, 294), (3, 196)), "2chunks": ((40, 294), (27, 196))}


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield ctx, torch
    ctx.close()


def batch_frames(rows, cols, seed):
    rng = np.random.default_rng(seed)
    half = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    half[:, cols // 2:] = 93  # noise on the left, constant on the right
    return np.stack([np.full((rows, cols), 93, np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8), half])


@pytest.mark.parametrize("min_contrast", [0, 8])
@pytest.mark.parametrize("shape", list(SHAPES), ids=[str(k) for k in SHAPES])
def test_scan_masks_counts_and_list_order(env, shape, min_contrast):
    ctx, torch = env
    (rows, cols), (lr, lc) = SHAPES[shape]
    frames = batch_frames(rows, cols, 17 * rows + cols)
    n = len(frames)
    p = capi.default_params(rows, cols, n_octaves=1, min_contrast=min_contrast)
    L = capi.batch_layout(p)
    assert (L.lat_rows[0], L.lat_cols[0]) == (lr, lc) and L.lat_words[0] == (lc + 63) // 64
    wpr = L.lat_words[0]
    assert L.bits_frame_words == 3 * lr * wpr
    dev = "cuda:0"
    bits = torch.zeros((n, L.bits_frame_words), dtype=torch.int64, device=dev)
    pts = torch.zeros((n, p.dog_cap, 6), dtype=torch.int32, device=dev)
    cnt = torch.full((n,), -1, dtype=torch.int32, device=dev)
    pyr = torch.zeros((n, L.pyramid_frame_bytes), dtype=torch.uint8, device=dev)
    ctx.kernel_timing_enable("k_extrema_w3@0")
    ctx.detect_batch(p, torch.from_numpy(frames).to(dev), pyramid=pyr, extrema_bits=bits, dog_points=pts, dog_counts=cnt)
    torch.cuda.synchronize()
    launches, _ = ctx.kernel_timing_read()
    ctx.kernel_timing_enable(None)
    assert launches == 1, "octave 0 did not run the lattice scan kernel"
    bits_np = bits.cpu().numpy().view(np.uint64).reshape(n, 3, lr, wpr)
    counts = cnt.cpu().numpy()
    seen = []
    for f in range(n):
        want = oracle.Pyramid(frames[f], 1, 1.6)
        try:
            want_mask, want_pts = want.extrema(0, 3, min_contrast)
        finally:
            want.close()
        got_mask = np.unpackbits(bits_np[f].view(np.uint8), axis=-1, bitorder="little")
        assert (got_mask[..., :lc] == want_mask).all(), ("candidate mask", f)
        assert not got_mask[..., lc:].any(), ("bits past the row's last site", f)
        assert counts[f] == len(want_pts), ("count", f, counts[f], len(want_pts))
        got_pts = pts[f, : len(want_pts)].cpu().numpy().view(capi.POINT_DTYPE).reshape(-1)
        assert got_pts.tobytes() == want_pts.tobytes(), ("list against the oracle", f)
        # the same image through the single-image entry point
        py = ctx.pyramid(frames[f], 1, 1.6)
        prev_mask, prev_pts, prev_n = py.extrema(0, 3, min_contrast, cap=1 << 15)
        assert prev_n == counts[f], ("count against vslam_dog_extrema", f, prev_n, counts[f])
        assert prev_pts.tobytes() == got_pts.tobytes(), ("list order against vslam_dog_extrema", f)
        assert (prev_mask == got_mask[..., :lc]).all(), ("candidate mask against vslam_dog_extrema", f)
        seen.append(int(counts[f]))
    if min_contrast == 0:
        assert seen[0] == 3 * lr * lc, "every site of the constant frame is listed"
    assert len(set(seen)) == n, ("the frames of the batch have unequal counts", seen)

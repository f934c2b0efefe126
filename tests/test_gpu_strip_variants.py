"""Every launch variant of the coarse-octave strip kernels against the CPU oracle.

enqueue_strip_octave (csrc/vslam_hip.hip) asks strip_launch() (csrc/vslam_octave_launch.h) which of the six
k_gauss_h_strip<SH, RI> instantiations, or which k_gauss_h_diff row-pair count, runs an octave of (rows, cols, nf), and over
how many workgroups k_gauss_v_strip splits the six levels.  The rest of the suite runs <4,1> and <4,4> only (small batches);
the batches below are the smallest that select each of the others - the capacity edges (512 / 1024 items per workgroup),
a partial last strip, widths that are no multiple of 8, each step of the rows-per-workgroup ladder - plus every row-pair
count 1..8 and every level split.  Two launch orders come with them: a strip octave 0 of >= 64 frames waits for the second
half's upsample (ev_up2), and a generic octave 0 hands its base to a strip octave through k_resize_nearest_half_v4.

CASES is the contract with tests/test_octave_launch_cpu.py, which asserts on the host that strip_launch() chooses exactly
the variant written here for every octave of every case, and that the table as a whole covers every variant: a change of
the dispatch cannot silently un-cover a kernel.  Here each case is run once and check_frame (tests/test_gpu_batch.py)
compares every Gaussian and DoG plane of every octave, the masks and the lists of the frames named below with the oracle -
the next octave's base is written from inside the strip kernel, so a wrong base shows up one octave later."""
from collections import namedtuple

import numpy as np
import pytest

from visualslam_amd import capi, synth

from tests.test_gpu_batch import check_frame, run_batch

pytestmark = pytest.mark.gpu

# variant of one octave: ("tile",) k_pyr_octave | ("generic",) the one-thread-per-pixel kernels |
# ("dot2", SH, RI, level split) | ("diff", row pairs per workgroup, level split)
TILE, GENERIC = ("tile",), ("generic",)


def dot2(sh, ri, split=1):
    return ("dot2", sh, ri, split)


def diff(npairs, split=1):
    return ("diff", npairs, split)


Case = namedtuple("Case", "id nf rows cols n_octaves sigma0 variants")

# sigma0 1.2 and 2.0: no octave has the widths of a k_pyr_octave configuration or the taps of k_gauss_h_diff, so octave 0
# itself goes through k_gauss_v_strip + k_gauss_h_strip (test_other_sigmas_take_the_dot2_strip_kernels_from_octave_0)
CASES = [
    # 32 x 1024: 128 column groups x 4 row groups = 512 items, exactly what <16,4> holds; its base feeds <8,4>
    Case("16x512-s1.2", 128, 16, 512, 2, 1.2, {0: dot2(16, 4), 1: dot2(8, 4)}),
    # 26 x 502: a partial last strip (10 of 16 rows) and a last column group of 6; 13 x 251: odd in both directions
    Case("13x251-s1.2", 128, 13, 251, 2, 1.2, {0: dot2(16, 4), 1: dot2(8, 4)}),
    # 32 x 960: 960 items of 2 rows (15 whole waves); 32 x 480: 960 items of 1 row
    Case("16x480-s2.0", 128, 16, 480, 2, 2.0, {0: dot2(16, 2), 1: dot2(8, 4)}),
    Case("16x240-s1.2", 128, 16, 240, 2, 1.2, {0: dot2(16, 1), 1: dot2(8, 4)}),
    # the ladder's second and third step at their capacity: 16 x 2048 (256 x 2 items), 8 x 4096 (512 x 1)
    Case("8x1024-s2.0", 128, 8, 1024, 2, 2.0, {0: dot2(8, 4), 1: dot2(4, 4)}),
    Case("4x2048-s1.2", 128, 4, 2048, 2, 1.2, {0: dot2(4, 4), 1: dot2(4, 4)}),
    # 8 x 4100 is too wide for the strip kernels: generic octave 0, k_resize_nearest_half_v4, then <4,4> with 257 items
    Case("4x2050-s1.2", 128, 4, 2050, 2, 1.2, {0: GENERIC, 1: dot2(4, 4)}),
    # the small-launch form, with all six levels of the vertical pass in workgroups of their own
    Case("13x251-s2.0-small", 4, 13, 251, 2, 2.0, {0: dot2(4, 1, 6), 1: dot2(4, 1, 6)}),
    # the automatic octave count's octaves 4 and 5 (kernels of 443 and 885 taps on 8 x 8 and 4 x 4 / 16 x 32 and 8 x 16 images)
    Case("64x64-6oct", 256, 64, 64, 6, 1.6, {0: TILE, 1: TILE, 2: diff(8), 3: diff(8), 4: dot2(16, 1), 5: dot2(16, 1)}),
    Case("128x256-6oct", 128, 128, 256, 6, 1.6, {0: TILE, 1: TILE, 2: diff(8), 3: diff(8, 2), 4: dot2(8, 4, 2), 5: dot2(4, 4, 2)}),
    # the difference form's row pairs per workgroup, 1..7 (8 is above): octaves of 64 and 32 rows, the batch size decides
    Case("128x100-n56", 56, 128, 100, 4, 1.6, {0: TILE, 1: TILE, 2: diff(7, 3), 3: diff(3, 3)}),
    Case("128x100-n48", 48, 128, 100, 4, 1.6, {0: TILE, 1: TILE, 2: diff(6, 6), 3: diff(3, 6)}),
    Case("128x107-n40", 40, 128, 107, 4, 1.6, {0: TILE, 1: TILE, 2: diff(5, 6), 3: diff(2, 6)}),
    Case("128x100-n32", 32, 128, 100, 4, 1.6, {0: TILE, 1: TILE, 2: diff(4, 6), 3: diff(2, 6)}),
    Case("128x93-n4", 4, 128, 93, 4, 1.6, {0: TILE, 1: TILE, 2: diff(1, 6), 3: diff(1, 6)}),
]
BY_ID = {c.id: c for c in CASES}


def case_frames(case):
    """Every frame with a seed of its own; one of uniform noise, one all 255 and one all 0 (the two ends of the u16
    accumulator range: row sums of 255 * 256 + 128 and of 128).  Returns the frames and the ones check_frame looks at."""
    n = case.nf
    frames = synth.frames_np(n, case.rows, case.cols, stream_id=100 + CASES.index(case))
    noise, white, black = 1, n // 2 + 1, n - 2
    assert len({noise, white, black}) == 3
    frames[noise] = synth.frame_np(case.rows, case.cols, frame=noise, stream_id=200 + CASES.index(case), kind="noise")
    frames[white] = 255
    frames[black] = 0
    # first and last; both sides of nf / 2 (from 64 frames on the second half's upsample arrives over ev_up2)
    look = sorted({0, n - 1, max(n // 2 - 1, 0), n // 2, noise, white, black})
    return frames, look


def poison_pyramid(torch, case, **pkw):
    """run_batch takes its pyramid buffer with torch.empty: hand the allocator a block of exactly that size filled with
    0xA5 first, so that a plane element the kernels do not write cannot hold a right answer left by an earlier run."""
    p = capi.default_params(case.rows, case.cols, **pkw)
    L = capi.batch_layout(p)
    junk = torch.full((case.nf, L.pyramid_frame_bytes), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    del junk


def run_case(ctx, torch, case, **pkw):
    frames, look = case_frames(case)
    kw = dict(n_octaves=case.n_octaves, sigma0=case.sigma0, harris_cap=2048, dog_cap=4096, **pkw)
    poison_pyramid(torch, case, **kw)
    p, L, out = run_batch(ctx, torch, frames, **kw)
    for f in look:
        check_frame(p, L, out, f, frames[f], case.n_octaves)
    return p, L, out


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield ctx, torch
    ctx.close()


def launches(ctx, torch, frames, name, **pkw):
    ctx.kernel_timing_enable(name)
    try:
        run_batch(ctx, torch, frames, **pkw)
        return ctx.kernel_timing_read()[0]
    finally:
        ctx.kernel_timing_enable(None)


@pytest.mark.parametrize("sigma0", sorted({c.sigma0 for c in CASES if c.sigma0 != 1.6}))
def test_other_sigmas_take_the_dot2_strip_kernels_from_octave_0(env, sigma0):
    # which kernel family runs an octave is decided by its taps alone (plan_octave), so one small batch per sigma0 shows it
    # for every case with that sigma0: no LDS-tiled kernel, no difference form, both passes of the strip kernels at octave 0
    ctx, torch = env
    frames = synth.frames_np(4, 13, 251, stream_id=99)
    kw = dict(n_octaves=2, sigma0=sigma0, harris_cap=2048, dog_cap=4096)
    for name, want in (("k_gauss_v_strip@0", 1), ("k_gauss_h_strip@0", 1), ("k_gauss_h_strip@1", 1), ("k_gauss_h_diff", 0), ("k_pyr_octave", 0),
                       ("k_blur_h_generic", 0), ("k_resize_nearest_half_v4", 0)):
        assert launches(ctx, torch, frames, name, **kw) == want, (sigma0, name)


def test_generic_octave_hands_its_base_to_a_strip_octave(env):
    ctx, torch = env
    case = BY_ID["4x2050-s1.2"]
    frames, _ = case_frames(case)
    kw = dict(n_octaves=2, sigma0=case.sigma0, harris_cap=2048, dog_cap=4096)
    for name, want in (("k_blur_h_generic@0", 6), ("k_gauss_h_strip@0", 0), ("k_resize_nearest_half_v4", 1), ("k_gauss_h_strip@1", 1)):
        assert launches(ctx, torch, frames, name, **kw) == want, name


def test_default_sigma_deep_octaves_take_both_forms(env):
    # six octaves at sigma0 1.6: octaves 0-1 tiled, 2-3 in difference form, 4-5 through the dot2 strip kernels
    ctx, torch = env
    case = BY_ID["128x256-6oct"]
    frames, _ = case_frames(case)
    kw = dict(n_octaves=6, sigma0=1.6, harris_cap=2048, dog_cap=4096)
    assert launches(ctx, torch, frames, "k_pyr_octave", **kw) >= 2  # (octave 0 of 128 frames in two halves)
    for name, want in (("k_gauss_h_diff", 2), ("k_gauss_h_strip@4", 1), ("k_gauss_h_strip@5", 1), ("k_blur_h_generic", 0)):
        assert launches(ctx, torch, frames, name, **kw) == want, name


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_variant_matches_oracle(env, case):
    ctx, torch = env
    run_case(ctx, torch, case)


def test_partial_strip_case_localized_and_oriented(env):
    # the lists of the later stages are built from the planes the strip kernels wrote, both octaves
    ctx, torch = env
    p, L, out = run_case(ctx, torch, BY_ID["13x251-s1.2"], localize=1, orient=1)
    assert out["dog_counts"].sum() > 0


def test_matrix_path_gives_the_same_bytes_beside_the_strip_octaves(env):
    # the opt-in matrix path takes the octaves it has a configuration for (here 0-3); 4 and 5 stay with <8,4> and <4,4>,
    # now fed by a base the matrix kernel wrote.  Both runs are compared with the oracle, and with each other as bytes.
    ctx, torch = env
    case = BY_ID["128x256-6oct"]
    was = ctx.matrix_path()
    try:
        ctx.set_matrix_path(False)
        p, L, ref = run_case(ctx, torch, case)
        ctx.set_matrix_path(True)
        frames, _ = case_frames(case)
        assert launches(ctx, torch, frames, "k_pyr_octave_mx", n_octaves=6, sigma0=1.6, harris_cap=2048, dog_cap=4096) >= 4
        assert launches(ctx, torch, frames, "k_gauss_h_strip", n_octaves=6, sigma0=1.6, harris_cap=2048, dog_cap=4096) == 2
        p, L, got = run_case(ctx, torch, case)
    finally:
        ctx.set_matrix_path(was)
    valid = L.octave_offset[5] + 11 * L.rows[5] * L.pitch[5]  # the block is rounded up: the tail is never written
    for o in range(6):
        assert L.pitch[o] == L.cols[o]  # (no row padding at 256 columns: whole blocks compare)
    assert got["pyramid"][:, :valid].tobytes() == ref["pyramid"][:, :valid].tobytes()
    for k in ("extrema_bits", "dog_counts", "harris_counts", "response"):
        assert got[k].tobytes() == ref[k].tobytes(), k

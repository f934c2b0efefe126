"""GPU: k_harris_strip (csrc/kernels_harris_strip.hip.h) at its strip seams, segment seams and steady-trip boundaries, bytes-equal
against the oracle: response, 3x3 mask of the 8-bit view, NMS2 map and the keypoint list.

The content (tests/harrisref.py: frame) decides every output: mask pixels, keypoints, responses below 253.5 and at or above 2^31
lie at every seam, and each case asserts that from the oracle (harrisref.coverage) before it compares anything.  The geometry each
case is named for - segment length, rows of the last segment, steady rows, interior strips, any-width form, the right-edge lane's
jedge - is held to csrc/vslam_harris_launch.h and to the restated trip loop by tests/test_harris_launch_cpu.py, without a GPU.

Output sets of a batched case: {response, mask, list} runs the branch-free steady trips on interior strips of an aligned frame,
{mask, list} the same with the response in the library's scratch, {response, mask, nms2, list} the generic trips everywhere.
A buffer that is not requested is passed as null; one that is, is pre-filled with a pattern no output has.
"""
from dataclasses import dataclass

import numpy as np
import pytest

from tests import harrisref as H

pytestmark = pytest.mark.gpu

STEADY, SCRATCH, GENERIC = ("response", "nms_mask", "list"), ("nms_mask", "list"), ("response", "nms_mask", "nms2", "list")
ALONE = (("response",), ("nms2",))
NEAR, COL1 = "NMS2 survivor in [253.5, 254.5)", "NMS2 maximum in column 1"  # content that decides the range test's bound and the column range


@dataclass(frozen=True)
class Case:
    nf: int
    rows: int
    cols: int
    seeds: tuple        # one per distinct frame; frame f has seeds[f % len(seeds)]
    seg: int            # rows per segment ...
    nseg: int
    last_rows: int      # ... and of the last one
    steady_first: int   # rows the steady trips finalise in the first / last segment of an interior strip (aligned form,
    steady_last: int    # output set STEADY); 0 where the case has no interior strip or runs the any-width form
    interior: tuple     # strips that run the straight-line (EDGE = false) code
    anyw: bool          # the any-width form of the kernel
    jedge: int          # pixels of the lane that straddles the right edge (0: the image ends on a lane boundary)
    pad: int = 0        # bytes between frames beyond rows * cols
    ks: tuple = (0.04,)
    sets: tuple = (STEADY, SCRATCH, GENERIC)
    compare: tuple = ()  # frames copied back and compared (default: all)
    extra: tuple = ()    # conditions of harrisref.coverage that only some content meets, and this case's does

    @property
    def id(self):
        return f"{self.nf}x{self.rows}x{self.cols}" + (f"+{self.pad}" if self.pad else "") + ("-k" if len(self.ks) > 1 else "")


# figures: tests/test_harris_launch_cpu.py::test_gpu_case_table_is_what_it_names proves them against the header and the restatement
CASES = [
    # one segment of 15 / 16 rows: one steady trip; 17 = 16 + a 1-row segment
    Case(1, 15, 488, (1,), 15, 1, 15, 6, 6, (1,), False, 0),
    Case(1, 16, 488, (1,), 16, 1, 16, 6, 6, (1,), False, 0, sets=(STEADY, SCRATCH, GENERIC) + ALONE),
    Case(1, 17, 488, (1,), 16, 2, 1, 6, 0, (1,), False, 0),
    # last segment of 5, 6, 7 rows: around one trip
    Case(1, 21, 488, (1,), 16, 2, 5, 12, 0, (1,), False, 0),
    Case(1, 22, 488, (1,), 16, 2, 6, 12, 0, (1,), False, 0),
    Case(1, 23, 488, (1,), 16, 2, 7, 12, 0, (1,), False, 0),
    # rows < 16: seg = rows, no steady trip
    Case(1, 9, 488, (1,), 9, 1, 9, 0, 0, (1,), False, 0),
    # two interior strips, segments 16 / 16 / 1, grid.z > 1
    Case(3, 33, 728, (1, 2, 3), 16, 3, 1, 12, 0, (1, 2), False, 0, extra=(NEAR, COL1)),
    # strip 1 edge (484 aligned, 487 any width) against interior (488: last strip 8 columns; 492)
    Case(2, 35, 484, (1, 2), 16, 3, 3, 0, 0, (), False, 0, extra=(COL1,)),
    Case(2, 35, 487, (1, 2), 16, 3, 3, 0, 0, (), True, 3),
    Case(2, 35, 488, (1, 2), 16, 3, 3, 12, 0, (1,), False, 0, extra=(COL1,)),
    Case(2, 35, 492, (1, 2), 16, 3, 3, 12, 0, (1,), False, 0, extra=(NEAR, COL1)),
    # any width with an interior strip, jedge 1, 2, 3
    Case(2, 33, 489, (2, 3), 16, 3, 1, 0, 0, (1,), True, 1, extra=(NEAR, COL1)),
    Case(2, 33, 490, (1, 2), 16, 3, 1, 0, 0, (1,), True, 2),
    Case(2, 33, 491, (1, 2), 16, 3, 1, 0, 0, (1,), True, 3, extra=(NEAR, COL1)),
    # last strip of 1 .. 9 columns, no interior strip
    Case(2, 19, 241, (6, 7), 16, 2, 3, 0, 0, (), True, 1, extra=(COL1,)),
    Case(2, 19, 243, (1, 2), 16, 2, 3, 0, 0, (), True, 3),
    Case(2, 19, 244, (1, 2), 16, 2, 3, 0, 0, (), False, 0, extra=(COL1,)),
    Case(2, 19, 248, (1, 2), 16, 2, 3, 0, 0, (), False, 0),
    Case(2, 19, 249, (2, 4), 16, 2, 3, 0, 0, (), True, 1, extra=(COL1,)),
    # three interior strips, last strip 8 columns
    Case(2, 19, 968, (1, 2), 16, 2, 3, 6, 0, (1, 2, 3), False, 0),
    # an aligned width through the any-width form (frame stride N + 1), and aligned with a gap (N + 4)
    Case(2, 35, 488, (1, 2), 16, 3, 3, 0, 0, (1,), True, 0, pad=1, extra=(COL1,)),
    Case(2, 35, 488, (1, 2), 16, 3, 3, 12, 0, (1,), False, 0, pad=4, extra=(COL1,)),
    # the clamp at 0 and the keypoint range test at other k
    Case(2, 35, 728, (1, 2), 16, 3, 3, 12, 0, (1, 2), False, 0, ks=(0.0, 0.15, 0.25)),
    # the smallest shapes that leave seg = 16: 16 segments of 17 rows, the last of 2; of 18 rows, the last of 5
    Case(256, 257, 488, (1, 2, 3, 4), 17, 16, 2, 12, 0, (1,), False, 0, compare=(0, 1, 254, 255), extra=(NEAR, COL1)),
    Case(256, 275, 488, (1, 2, 3, 4), 18, 16, 5, 12, 0, (1,), False, 0, compare=(0, 1, 254, 255), extra=(NEAR, COL1)),
]

IMAGE_ROWS = (1, 2, 3, 5, 6, 7, 16, 17, 33)
IMAGE_COLS = (241, 243, 481, 487, 488, 489, 491, 727, 728)
IMAGE_SEED = {1: 1, 2: 1, 3: 1, 5: 2, 6: 6, 7: 4, 16: 19, 17: 85, 33: 2}  # per height: one seed that meets the conditions at all nine widths

FILL_F32, FILL_U8, FILL_I32 = -7.0, 0xAB, -3

_refs = {}


def ref(rows, cols, seed, seg, k=0.04):
    """The oracle's outputs of one generated frame, computed once and left unchanged."""
    key = (rows, cols, seed, seg, k)
    if key not in _refs:
        _refs[key] = H.Ref(H.frame(rows, cols, seed, seg), k)
    return _refs[key]


@pytest.fixture(scope="module")
def gpu():
    import torch

    from visualslam_amd import capi

    capi.build()
    ctx = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield ctx, torch, capi
    ctx.close()


def run_set(gpu, case, frames_dev, k, want):
    """One detect_batch call with exactly the outputs of `want`; the requested buffers as numpy, frames of case.compare only."""
    ctx, torch, capi = gpu
    n, rows, cols = case.nf, case.rows, case.cols
    p = capi.default_params(rows, cols, n_octaves=0, harris_k=k)
    dev = frames_dev.device
    o = {}
    if "response" in want:
        o["response"] = torch.full((n, rows, cols), FILL_F32, dtype=torch.float32, device=dev)
    if "nms_mask" in want:
        o["nms_mask"] = torch.full((n, rows, cols), FILL_U8, dtype=torch.uint8, device=dev)
    if "nms2" in want:
        o["nms2"] = torch.full((n, rows, cols), FILL_F32, dtype=torch.float32, device=dev)
    if "list" in want:
        o["harris_kps"] = torch.full((n, p.harris_cap, 3), FILL_I32, dtype=torch.int32, device=dev)
        o["harris_counts"] = torch.full((n,), FILL_I32, dtype=torch.int32, device=dev)
    ctx.detect_batch(p, frames_dev, **o)
    torch.cuda.synchronize()
    sel = list(case.compare or range(n))
    return p, {name: t[sel].cpu().numpy() for name, t in o.items()}


def compare(case, p, out, want, refs, what):
    from visualslam_amd import capi

    for i, r in enumerate(refs):
        tag = (case.id, what, "frame", i)
        if "response" in want:
            assert out["response"][i].tobytes() == r.R.tobytes(), tag + ("response", np.argwhere(out["response"][i] != r.R)[:4].tolist())
        if "nms_mask" in want:
            assert out["nms_mask"][i].tobytes() == r.mask.tobytes(), tag + ("mask", np.argwhere(out["nms_mask"][i] != r.mask)[:4].tolist())
        if "nms2" in want:
            assert out["nms2"][i].tobytes() == r.nms2.tobytes(), tag + ("nms2", np.argwhere(out["nms2"][i] != r.nms2)[:4].tolist())
        if "list" in want:
            assert len(r.kps) <= p.harris_cap  # cap truncation is test_gpu_batch's
            assert int(out["harris_counts"][i]) == len(r.kps), tag + ("count", int(out["harris_counts"][i]), len(r.kps))
            got = out["harris_kps"][i][: len(r.kps)].copy().view(capi.KP_DTYPE).reshape(-1)
            assert got.tobytes() == r.kps.tobytes(), tag + ("list",)
            assert (out["harris_kps"][i][len(r.kps):] == FILL_I32).all(), tag + ("records past the count were written",)


def assert_coverage(case, refs):
    """Every condition on every distinct frame of the case; the case's `extra` ones on at least one of them."""
    covs = [H.coverage(r, case.seg, H.steady_rows_of(case.rows, case.seg) if case.steady_first + case.steady_last else ()) for r in refs]
    for cov in covs:
        assert all(ok for name, ok in cov.items() if name[0] != "?"), (case.id, [name for name, ok in cov.items() if not ok])
    for name in case.extra:
        assert any(cov["?" + name] for cov in covs), (case.id, name)
    assert len(cov) >= 2 * len(H.seam_cols(case.cols)) + len(case.interior)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_batched_harris_at_the_seams(gpu, case):
    _, torch, _ = gpu
    n, rows, cols = case.nf, case.rows, case.cols
    distinct = [ref(rows, cols, s, case.seg) for s in case.seeds]
    assert_coverage(case, distinct)
    N = rows * cols
    block = np.full(n * (N + case.pad), 0x5A, np.uint8)  # the gap between frames holds bytes no frame has an edge of
    view = np.lib.stride_tricks.as_strided(block, (n, rows, cols), (N + case.pad, cols, 1))
    for f in range(n):
        view[f] = distinct[f % len(distinct)].img
    frames_dev = torch.from_numpy(block).to("cuda:0").as_strided((n, rows, cols), (N + case.pad, cols, 1))
    sel = list(case.compare or range(n))
    for k in case.ks:
        refs = [ref(rows, cols, case.seeds[f % len(case.seeds)], case.seg, k) for f in sel]
        if k == 0.25:  # det <= trace^2 / 4: the clamp at 0 decides every response
            assert all((r.R == 0).all() and len(r.kps) == 0 for r in refs), (case.id, k)
        elif k != 0.04:  # the range test has survivors on both sides at this k too
            surv = np.concatenate([r.nms2[r.nms2 > 0] for r in refs])
            assert (surv < H.KP_LO).any() and ((surv >= H.KP_LO) & (surv < H.TWO31)).any() and (surv >= H.TWO31).any(), (case.id, k)
        for want in case.sets:
            p, out = run_set(gpu, case, frames_dev, k, want)
            assert set(out) == {x for w in want for x in (("harris_kps", "harris_counts") if w == "list" else (w,))}
            compare(case, p, out, want, refs, (k, want))


@pytest.mark.parametrize("rows", IMAGE_ROWS)
def test_per_image_entry_points(gpu, rows):
    # vslam_harris_response_u8 (response alone) and vslam_harris_keypoints_u8 (response + flags): generic trips on every strip
    ctx, _, _ = gpu
    for cols in IMAGE_COLS:
        r = ref(rows, cols, IMAGE_SEED[rows], min(rows, 16))
        # rows >= 16: every condition of the batched cases; 5 .. 7 rows (no room for the high-amplitude tiles): the keypoint ones;
        # below 5 rows the image has no NMS2 row at all
        cov = {name: ok for name, ok in H.coverage(r, 16).items() if (rows >= 16 and name[0] != "?") or (5 <= rows < 16 and name.startswith("keypoint"))}
        assert all(cov.values()) and (rows < 5 or len(cov) >= 4 + len(H.seam_cols(cols))), (rows, cols, [name for name, ok in cov.items() if not ok])
        assert (rows >= 5) == (len(r.kps) > 0)
        got = ctx.harris_response(r.img)
        assert got.tobytes() == r.R.tobytes(), (rows, cols, np.argwhere(got != r.R)[:4].tolist())
        kps, n = ctx.harris_keypoints(r.img)
        assert n == len(r.kps) and kps.tobytes() == r.kps.tobytes(), (rows, cols, n, len(r.kps))

"""The launch geometry of k_harris_strip (csrc/vslam_harris_launch.h) and the kernel's trip loop without a GPU.

Only host arithmetic keeps the kernel's waves inside the image: the segment length decides which rows a wave finalises, the
grid how many waves exist, the flag-word count how large the keypoint-flag buffer is, `aligned` which form may use dword
accesses.  tests/harris_launch_driver.cpp sweeps the header itself; the trip loop inside a segment (which trips are the
branch-free steady ones, which rows they store and prefetch without a bounds test) is restated in tests/harrisref.py and
checked here for every (image height, segment length) the sweep produces; and the case table of
tests/test_gpu_harris_strip.py is held to the geometry each case is named for."""
import os
import shutil
import subprocess

import pytest

from tests import harrisref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")

NFS = (1, 2, 3, 31, 32, 64, 255, 256)


def sweep_cols():
    return sorted(set(range(1, 1001)) | {240 * k + d for k in range(1, 18) for d in range(-1, 10) if 240 * k + d <= 4096})


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("harris_launch") / "driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "harris_launch_driver.cpp"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        out = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        return out.stdout

    return run


@pytest.fixture(scope="module")
def sweep(driver):
    head, *per_rows = driver("sweep").splitlines()
    name, *kv = head.split()
    assert name == "sweep"
    segs = {}
    for line in per_rows:
        a, rows, b, lst = line.split()
        assert (a, b) == ("rows", "seg")
        segs[int(rows)] = [int(s) for s in lst.split(",") if s]
    return dict(x.split("=", 1) for x in kv), segs


def plans(driver, launches):
    """[(nf, rows, cols, frame stride)] -> the header's fields per launch, as ints."""
    out = driver("plan", *[v for l in launches for v in l]).splitlines()
    assert len(out) == len(launches)
    return [{k: int(v) for k, v in (x.split("=", 1) for x in line.split()[1:])} for line in out]


def test_the_launch_header_needs_no_hip():
    src = open(os.path.join(CSRC, "vslam_harris_launch.h")).read()
    assert "#include <hip" not in src and "__global__" not in src and "hipStream_t" not in src and "__device__" not in src
    # ... and states the geometry once: the HIP translation unit and the kernel header have none of their own left
    hip = open(os.path.join(CSRC, "vslam_hip.hip")).read()
    assert "harris_launch(" in hip and "harris_flag_words(" in hip
    for gone in ("want_seg", "12288", "HS_STRIP_W - 1", "fframe % 4"):
        assert gone not in hip, gone
    assert "constexpr int HS_" not in open(os.path.join(CSRC, "kernels_harris_strip.hip.h")).read()


def test_sweep_every_launch_covers_its_image(sweep):
    # rows 1..1200 x cols {1..1000 and 240k - 1 .. 240k + 9 up to 4096} x 8 batch sizes x frame strides N .. N + 4; the driver
    # checks, per launch: 1 <= seg <= rows, nseg * seg >= rows > (nseg - 1) * seg, grid.x * 4 >= nstrips * nseg with no
    # workgroup beyond, flag words == rows * nstrips * 4, aligned iff cols and the frame stride are multiples of 4.
    # `first` names the first violated check and its inputs.
    got, segs = sweep
    assert got["bad"] == "0", got["first"]
    assert int(got["ncols"]) == len(sweep_cols()) and int(got["checked"]) == 1200 * len(sweep_cols()) * len(NFS) * 5
    assert sorted(segs) == list(range(1, 1201)) and all(segs.values())
    assert segs[15] == [15] and segs[16] == [16] and 17 in segs[257] and 18 in segs[275]
    assert max(max(s) for s in segs.values()) > 180  # the sweep reaches long segments too, not only seg = 16


def test_sweep_pinned_plans(driver):
    # values of the code before the geometry moved into the header
    got = plans(driver, [(256, 1080, 1920, 1080 * 1920), (1, 1080, 1920, 1080 * 1920), (256, 600, 868, 600 * 868), (1, 37, 488, 37 * 488 + 1),
                         (64, 2160, 3840, 2160 * 3840)])
    want = [dict(nstrips=8, seg=180, nseg=6, grid_x=12, aligned=1), dict(nstrips=8, seg=16, nseg=68, grid_x=136, aligned=1),
            dict(nstrips=4, seg=50, nseg=12, grid_x=12, aligned=1), dict(nstrips=3, seg=16, nseg=3, grid_x=3, aligned=0),
            dict(nstrips=16, seg=180, nseg=12, grid_x=48, aligned=1)]
    for g, w in zip(got, want):
        assert {k: g[k] for k in w} == w, g


def test_trip_loop_of_every_plan(sweep):
    # for every (rows, seg) of the sweep, every segment: each row finalised exactly once, in order; steady trips finalise only rows
    # in [max(y_begin, 2), min(y_end, rows - 2)) and prefetch only rows in [0, rows) (harrisref.check_segment asserts all of it)
    _, segs = sweep
    pairs = steady_pairs = 0
    for rows, lst in segs.items():
        for seg in lst:
            pairs += 1
            n = sum(H.check_segment(rows, y0, y1) for y0, y1 in H.segments(rows, seg))
            steady_pairs += n > 0
            assert n <= max(rows - 4, 0)
            if seg >= 16 and rows >= 16:
                assert n > 0, (rows, seg)  # a full-length segment always has a steady trip
    assert pairs > 20000 and steady_pairs > 20000


def test_steady_strips_hold_every_lane():
    # steady trips run on interior strips only (edge_strip false), and load and store a dword per lane without a column test:
    # every lane's dword of such a strip lies inside the row, for every width of the sweep - and the kernel's test is tight:
    # a strip it calls an edge strip has a lane that does not
    interior = 0
    for cols in sweep_cols():
        for s in range((cols + H.STRIP_W - 1) // H.STRIP_W):
            assert H.lane_dwords_inside(s, cols) == (not H.edge_strip(s, cols)), (s, cols)
            interior += not H.edge_strip(s, cols)
    assert interior > 1000 and H.edge_strip(1, 487) and not H.edge_strip(1, 488)


def test_gpu_case_table_is_what_it_names(driver):
    from tests.test_gpu_harris_strip import CASES, IMAGE_COLS, IMAGE_ROWS

    got = plans(driver, [(c.nf, c.rows, c.cols, c.rows * c.cols + c.pad) for c in CASES])
    for c, g in zip(CASES, got):
        assert (g["seg"], g["nseg"]) == (c.seg, c.nseg), (c.id, g)
        assert c.rows - (c.nseg - 1) * c.seg == c.last_rows, c.id
        assert tuple(H.interior_strips(c.cols)) == c.interior, c.id
        assert bool(g["aligned"]) == (not c.anyw), (c.id, g)
        assert c.jedge == c.cols % 4 and (c.jedge == 0 or c.anyw), c.id
        segs = H.segments(c.rows, c.seg)
        assert len(segs) == c.nseg
        steady = [H.check_segment(c.rows, y0, y1) if c.interior and not c.anyw else 0 for y0, y1 in segs]
        assert (steady[0], steady[-1]) == (c.steady_first, c.steady_last), (c.id, steady)
        assert g["grid_x"] * 4 >= g["nstrips"] * c.nseg and g["flag_words"] == c.rows * g["nstrips"] * 4
    by = {(c.nf, c.rows, c.cols, c.pad): c for c in CASES}
    assert len(by) == len(CASES)
    # what the table is for: every seam of the kernel has a case
    assert {c.last_rows for c in CASES if c.interior and not c.anyw} >= {1, 2, 3, 5, 6, 7, 9, 15, 16}
    assert {c.seg for c in CASES} >= {9, 15, 16, 17, 18}
    assert {c.jedge for c in CASES if c.anyw and c.interior} == {0, 1, 2, 3} and {c.jedge for c in CASES if c.anyw and not c.interior} == {1, 3}
    assert {c.cols - 240 * ((c.cols - 1) // 240) for c in CASES if not c.interior} >= {1, 3, 4, 7, 8, 9}  # columns of the last strip
    assert any(c.nf > 1 and len(c.interior) > 1 for c in CASES) and any(len(c.interior) == 3 for c in CASES)
    assert by[(2, 35, 488, 1)].anyw and not by[(2, 35, 488, 4)].anyw and not by[(2, 35, 484, 0)].interior and by[(2, 35, 488, 0)].interior
    assert any(c.steady_first == 0 and c.interior and not c.anyw for c in CASES)  # too short for a steady trip
    # the per-image shapes: both sides of the first interior strip, every jedge
    assert {tuple(H.interior_strips(c)) for c in IMAGE_COLS} == {(), (1,), (1, 2)} and {c % 4 for c in IMAGE_COLS} == {0, 1, 3}
    assert set(IMAGE_ROWS) >= {1, 2, 3, 5, 6, 7, 16, 17, 33}


def test_gpu_case_content_meets_its_conditions():
    # what each GPU case asserts before it compares (harrisref.coverage, from the oracle alone), here without a GPU: set mask
    # pixels and keypoints at every seam, responses on both sides of 253.5 and of 2^31, a mask pixel that the 2^31 wrap decides,
    # and all of that in the steady rows where the case has any; the 256-frame cases by their first distinct frame
    import oracle
    from tests.test_gpu_harris_strip import CASES, assert_coverage, ref

    oracle.build()
    for c in CASES:
        assert_coverage(c, [ref(c.rows, c.cols, s, c.seg) for s in (c.seeds if c.nf <= 3 else c.seeds[:2])])

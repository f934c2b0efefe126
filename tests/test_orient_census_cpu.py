"""Coverage floors of tests/test_gpu_orient_steady.py, checked on the CPU: the oracle's lists of every frame that file
compares are put through tests/orientcensus.py, which restates the grid sizes and path conditions of the batched
filterKeypoints / SIFT kernels.  If a change of content (size, seed, block layout) takes records away from a path - the
steady-state loop of a workgroup, a filter form, a change of class between consecutive records - it fails here, not
silently on the GPU.  The measured counts are printed per frame (pytest -s).  Nothing here decides an expected value."""
import functools

import pytest

from tests import orientcensus as oc

NF = oc.STEADY_NF


def census(name, sigma0=1.6):
    return _census(name, sigma0)


@functools.lru_cache(maxsize=None)
def _census(name, sigma0):
    img = oc.steady_frame(name)
    c = oc.census(oc.oracle_lists(img, 4, sigma0), NF)
    print(oc.report("%s %dx%d sigma0 %.1f" % (name, img.shape[0], img.shape[1], sigma0), c))
    return c


def fits(c, caps):
    return c["keypoints"] <= caps["dog_cap"] and c["survivors"] <= caps["oriented_cap"] and c["oriented"] <= caps["oriented_cap"]


def test_grid_formulas():
    assert [oc.gwg(n) for n in (1, 8, 44, 256, 512, 1024)] == [1024, 1024, 186, 32, 16, 16]
    assert [oc.tap_count(1.6, 0, l) for l in (1, 2, 3)] == [25, 31, 39]  # the packed kernel's compiled-in KN
    assert oc.octave_plan(1.6, 0)[0] == "pk" and oc.octave_plan(2.0, 0)[0] == "surv"
    # k_orient_survivors at the default pyramid: patch staged in LDS (octave 1; octave 2 levels 1-2), region without patch
    # (octave 2 level 3), tap by tap (octave 3)
    assert [oc.octave_plan(1.6, o) for o in (1, 2, 3)] == [("surv", {1: "patch", 2: "patch", 3: "patch"}), ("surv", {1: "patch", 2: "patch", 3: "region"}),
                                                          ("surv", {1: "taps", 2: "taps", 3: "taps"})]


@pytest.mark.parametrize("sigma0", [1.6, 1.3])
def test_packed_kernel_frames_reach_the_steady_state(sigma0):
    c = census("noise", sigma0)
    assert fits(c, oc.PACKED_CAPS)
    lv = [c["levels"][0, l] for l in (1, 2, 3)]
    assert all(v["kernel"] == "pk" and v["workgroups"] == 256 for v in lv)
    kns = [v["kn"] for v in lv]
    assert kns == [25, 31, 39] if sigma0 == 1.6 else not set(kns) & {25, 31, 39}  # compiled-in KN / the generic KN = 0
    assert max(v["trips"] for v in lv) >= 4  # >= 769 survivors at 256 workgroups
    for v in lv:
        assert min(v["sh"]) >= 20 and v["border"] >= 20, v
    assert lv[0]["interior_border_changes"] >= 50
    b = census("block4", sigma0)
    assert fits(b, oc.PACKED_CAPS)
    t = [b["levels"][0, l]["trips"] for l in (1, 2, 3)]
    assert t[0] == 1 and max(t[1:]) >= 4, t  # few survivors at level 1 beside many at levels 2-3
    assert b["octaves"][1]["trips"] >= 4 and b["octaves"][1]["interior_border_changes"] >= 50  # k_orient_survivors on octave 1 as well


def test_coarse_octave_frames_reach_every_form_of_k_orient_survivors():
    cs = {name: census(name) for name in oc.COARSE_FRAMES.values()}
    assert all(fits(c, oc.COARSE_CAPS) for c in cs.values())
    for form in ("patch", "region", "taps"):  # in one frame each
        assert max(sum(v["survivors"] for v in c["levels"].values() if v["kernel"] == "surv" and v["form"] == form) for c in cs.values()) >= 10, form
    # the patch form runs for interior survivors only: they, and the change to and from border survivors between trips
    assert max(sum(v["interior"] for v in c["levels"].values() if v["form"] == "patch") for c in cs.values()) >= 50
    assert max(c["octaves"][1]["interior_border_changes"] for c in cs.values()) >= 20
    assert max(c["octaves"][2]["form_changes"] for c in cs.values()) >= 10  # patch <-> region records of one workgroup
    for o in (1, 2):
        assert max(c["octaves"][o]["trips"] for c in cs.values()) >= 2, o
    assert max(c["octaves"][3]["survivors"] for c in cs.values()) >= 20
    for name, c in cs.items():
        fw = c["flag_word"]
        assert fw["obegin"] % 64 and fw["below"] >= 1 and fw["above"] >= 1, (name, fw)  # k_edge_flags: both launches set bits of the shared word
        for o in range(4):  # k_survivor_ranges: a non-empty (octave, level) range in every octave
            assert max(c["levels"][o, l]["survivors"] for l in (1, 2, 3)) >= 1, (name, o)
    # sigma0 = 2.0: octave 0's widest span is past the packed kernel's, k_orient_survivors serves it
    c = census("noise", 2.0)
    assert fits(c, oc.PACKED_CAPS) and c["octaves"][0]["kernel"] == "surv" and c["octaves"][0]["trips"] >= 4


def test_descriptor_kernel_walks_records_of_every_class():
    cs = {name: census(name) for name in oc.COARSE_FRAMES.values()}
    noise = census("noise")
    assert noise["sift"]["trips"] >= 4 and max(c["sift"]["trips"] for c in cs.values()) >= 4
    assert all(oc.tap_count(1.6, o, l) // 2 > oc.SIFT_EXT_R for o in (2, 3) for l in (1, 2, 3))  # octaves 2 and 3: the kt form
    for o in (2, 3):
        assert max(c["octaves"][o]["defined"] for c in cs.values()) >= 20, o
    assert max(c["sift"]["form_changes"] for c in cs.values()) >= 20  # ext <-> kt one stride apart
    assert all(c["sift"]["defined"] == c["sift"]["records"] for c in cs.values())  # square frames: every descriptor defined
    assert noise["sift"]["undefined_to_defined"] >= 50  # landscape: the early return, then a defined record

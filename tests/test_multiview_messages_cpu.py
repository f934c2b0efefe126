"""The messages of the five multi-view argument checks (chain_check_args, resect_check_args, resect_refine_check_args,
tracks_check_args, bundle_check_args in visualslam_amd/csrc/*_plan.h), byte for byte.

The entry points put their stage in front of these strings and callers match on them, so a change to how the plan headers
state a check must leave every one as it was.  tests/multiview_messages_driver.cpp (built with -fsanitize=address,undefined)
takes one valid call per stage, breaks one field of it per case and prints the message; the table below is what the functions
said before their shared checks (check_intrinsics, check_max_dist2, OUT_FITS, OUT_NEEDS in vslam_epipolar_plan.h) were stated
once.  Whole strings are compared, and every distinct message a function can return is in its rows.  The order of the checks is
held by the "first" sections of the *_plan_driver.cpp programs."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")

# stage -> (one broken field, the whole message; None: the call is valid)
WANT = {
    "chain": [
        ("valid", None),
        ("null params", "null argument"),
        ("null out", "null argument"),
        ("struct_size", "out->struct_size is not sizeof(vslam_chain_out)"),
        ("pairs < 0", "0 .. 65535 pairs per call"),
        ("pairs > 65535", "0 .. 65535 pairs per call"),
        ("min_links 0", "min_links must be at least 1"),
        ("null points", "null input"),
        ("match_cap 0", "a capacity is zero"),
        ("null chain", "chain is required"),
        ("chain short", "chain buffer too small"),
        ("map short", "map buffer too small"),
        ("links short", "links buffer too small"),
        ("ratios short", "ratios buffer too small"),
        ("chain alone", None),
    ],
    "resect": [
        ("valid", None),
        ("null params", "null argument"),
        ("null out", "null argument"),
        ("struct_size", "out->struct_size is not sizeof(vslam_resect_out)"),
        ("pairs < 0", "0 .. 65535 pairs per call"),
        ("pairs > 65535", "0 .. 65535 pairs per call"),
        ("hypotheses 0", "1 .. 65535 hypotheses"),
        ("max_dist2 nan", "max_dist2 must be finite and positive"),
        ("max_dist2 zero", "max_dist2 must be finite and positive"),
        ("fx nan", "an intrinsic is not finite"),
        ("cy inf", "an intrinsic is not finite"),
        ("fx zero", "fx and fy must be positive"),
        ("fy negative", "fx and fy must be positive"),
        ("null poses", "null input"),
        ("point_cap 0", "a capacity is zero"),
        ("null obs_counts", "null input"),
        ("train_cap 0", "a capacity is zero"),
        ("null models", "models is required"),
        ("models short", "models buffer too small"),
        ("inlier_bits short", "inlier_bits buffer too small"),
        ("hypotheses short", "hypotheses buffer too small"),
        ("correspondences short", "correspondences buffer too small"),
        ("links short", "links buffer too small"),
    ],
    "resect_refine": [
        ("valid", None),
        ("null params", "null argument"),
        ("null out", "null argument"),
        ("struct_size", "out->struct_size is not sizeof(vslam_resect_refine_out)"),
        ("pairs < 0", "0 .. 65535 pairs per call"),
        ("pairs > 65535", "0 .. 65535 pairs per call"),
        ("rounds 0", "1 .. 8 rounds"),
        ("rounds 9", "1 .. 8 rounds"),
        ("max_dist2 nan", "max_dist2 must be finite and positive"),
        ("max_dist2 zero", "max_dist2 must be finite and positive"),
        ("fx nan", "an intrinsic is not finite"),
        ("cy inf", "an intrinsic is not finite"),
        ("fx zero", "fx and fy must be positive"),
        ("fy negative", "fx and fy must be positive"),
        ("null models_in", "null input"),
        ("obs_cap 0", "a capacity is zero"),
        ("unaligned", "correspondences must be 16-byte aligned"),
        ("unaligned, host", None),
        ("null models", "models is required"),
        ("models short", "models buffer too small"),
        ("info short", "info buffer too small"),
        ("inlier_bits short", "inlier_bits buffer too small"),
        ("models one row behind models_in", "models overlaps models_in without being equal to it"),
    ],
    "tracks": [
        ("valid", None),
        ("null params", "null argument"),
        ("null out", "null argument"),
        ("struct_size", "out->struct_size is not sizeof(vslam_tracks_out)"),
        ("pairs < 0", "0 .. 65535 pairs per call"),
        ("pairs > 65535", "0 .. 65535 pairs per call"),
        ("fx nan", "the intrinsics must be finite"),
        ("cy inf", "the intrinsics must be finite"),
        ("fx zero", "fx and fy must be positive"),
        ("fy negative", "fx and fy must be positive"),
        ("max_dist2 nan", "max_dist2 must be finite and positive"),
        ("max_dist2 zero", "max_dist2 must be finite and positive"),
        ("min_views 1", "min_views must be at least 2"),
        ("null chain", "null input"),
        ("point_cap 0", "a capacity is zero"),
        ("null tracks", "tracks is required"),
        ("tracks short", "tracks buffer too small"),
        ("refs short", "refs buffer too small"),
        ("good_bits short", "good_bits buffer too small"),
        ("summary short", "summary buffer too small"),
    ],
    "bundle": [
        ("valid", None),
        ("null params", "null argument"),
        ("null out", "null argument"),
        ("struct_size", "out->struct_size is not sizeof(vslam_bundle_out)"),
        ("pairs < 0", "0 .. 65535 pairs per call"),
        ("pairs > 65535", "0 .. 65535 pairs per call"),
        ("sweeps 0", "1 .. 64 sweeps"),
        ("sweeps 65", "1 .. 64 sweeps"),
        ("min_views 1", "min_views must be at least 2"),
        ("max_dist2 nan", "max_dist2 must be finite and positive"),
        ("max_dist2 zero", "max_dist2 must be finite and positive"),
        ("fx nan", "the intrinsics must be finite"),
        ("cy inf", "the intrinsics must be finite"),
        ("fx zero", "fx and fy must be positive"),
        ("fy negative", "fx and fy must be positive"),
        ("null refs", "null input"),
        ("match_cap 0", "a capacity is zero"),
        ("null tracks", "tracks is required"),
        ("tracks short", "tracks buffer too small"),
        ("null cams", "cams is required"),
        ("cams short", "cams buffer too small"),
        ("point_info short", "point_info buffer too small"),
        ("member_bits short", "member_bits buffer too small"),
        ("tracks one row behind tracks_in", "tracks overlaps tracks_in without being equal to it"),
    ],
}
PLAN_HEADER = {"chain": "vslam_chain_plan.h", "resect": "vslam_resect_plan.h", "resect_refine": "vslam_resect_refine_plan.h", "tracks": "vslam_tracks_plan.h",
               "bundle": "vslam_bundle_plan.h"}


@pytest.fixture(scope="module")
def said(tmp_path_factory):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("messages") / "multiview_messages_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "multiview_messages_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        stage, case, msg = line.split("|")
        got.setdefault(stage, []).append((case, None if msg == "-" else msg))
    return got


@pytest.mark.parametrize("stage", sorted(WANT))
def test_every_rejection_says_what_it_said(said, stage):
    assert [c for c, _ in said[stage]] == [c for c, _ in WANT[stage]]
    for (case, got), (_, want) in zip(said[stage], WANT[stage]):
        assert got == want, (stage, case, got, want)


@pytest.mark.parametrize("stage", sorted(WANT))
def test_the_table_has_every_message_the_function_can_return(stage):
    """Every string literal a *_check_args of the stage can return - its own, and those of the shared checks it calls - is in the
    stage's rows: a new check cannot land without a row here."""
    def body(name, fn):
        text = open(os.path.join(CSRC, name)).read()
        at = text.index("inline const char* " + fn)
        return text[at:text.index("\n}\n", at)]

    own = body(PLAN_HEADER[stage], stage + "_check_args")
    shared = open(os.path.join(CSRC, "vslam_epipolar_plan.h")).read()
    can = set(re.findall(r'return "([^"]+)"', own)) | set(re.findall(r'check_intrinsics\(prm->K, "([^"]+)"\)', own))
    can |= {f + " buffer too small" for f in re.findall(r"OUT_(?:FITS|NEEDS)\(out, (\w+),", own)} | {f + " is required" for f in re.findall(r"OUT_NEEDS\(out, (\w+),", own)}
    for helper, messages in (("twoview_check_pairs", 1), ("twoview_check_inputs", 2), ("check_max_dist2", 1), ("check_intrinsics", 2)):
        if helper + "(" in own:
            at = shared.index("inline const char* " + helper)
            found = re.findall(r'"([^"]+)"', shared[at:min(shared.index("\n}\n", at), shared.index("; }\n", at))])
            assert len(found) == messages, (helper, found)
            can |= set(found)
    if 'check_intrinsics(prm->K, "' in own:
        can.discard("the intrinsics must be finite")  # (the default wording, replaced by the stage's)
    told = {m for _, m in WANT[stage] if m is not None}
    print(stage, sorted(can))
    assert can == told, (sorted(can - told), sorted(told - can))

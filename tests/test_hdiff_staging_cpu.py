"""The staging bounds of k_gauss_h_diff (csrc/kernels_hdiff.hip.h) without a GPU.  The kernel prefetches the next level's
interior columns into registers while it computes a level and copies the reflect-101 halo inside LDS, each with a fixed
number of items per thread (two interior, one tail, hd_halo_trips() halo) and 16-bit LDS indices; it checks none of that at
run time, so the host arithmetic of csrc/vslam_octave_launch.h that the launch is planned with is swept here over every
width the difference form is used at (up to 4096 columns) and every row-pair count a workgroup can be given.
tests/hdiff_staging_driver.cpp is the host program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("hdiff_staging") / "driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "hdiff_staging_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe), "sweep"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    head, *kv = out.stdout.split()
    assert head == "sweep"
    return dict(x.split("=", 1) for x in kv)


def test_every_width_and_pair_count_fits_the_held_registers(sweep):
    # cols 1..4096 x npairs 1..hd_max_pairs(cols) x both geometries: npairs * ceil(cols/16) <= 256 items, at most two interior
    # items, one tail item and hd_halo_trips() halo items per thread, interior + tail + halo = the columns hd_pw sized the row
    # for, LDS indices below 0xffff; the difference form is offered up to exactly 4096 columns and hdiff_stage_fits holds there.
    # `first` names the first violated check and its inputs.
    assert sweep["bad"] == "0", sweep["first"]
    assert int(sweep["checked"]) > 20_000


def test_the_bounds_are_reached(sweep):
    # two interior items per thread do occur (960 columns x 4 pairs: 480 items), a tail item too, and the halo trips of
    # each geometry are the figure the kernel is instantiated with, no more
    assert sweep["interior"] == "2" and sweep["tail"] == "1"
    assert sweep["halo"] == sweep["trips"]


def test_strip_launch_stays_inside_the_swept_range(sweep):
    # rows x batch sizes: every row-pair count comes back, none above hd_max_pairs(cols)
    assert int(sweep["launches"]) > 500_000 and sweep["npairs"] == "1,2,3,4,5,6,7,8,"


def test_plan_octave_asks_the_bound():
    hip = open(os.path.join(CSRC, "vslam_hip.hip")).read()
    assert "hdiff_fits(cols) && hdiff_stage_fits(cols)" in hip
    # ... and the kernel takes its trip count from the same header
    assert "hd_halo_trips(G::HL, G::rmax)" in open(os.path.join(CSRC, "kernels_hdiff.hip.h")).read()

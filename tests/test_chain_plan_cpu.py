"""The host sizing and the argument checks of the trajectory step (visualslam_amd/csrc/vslam_chain_plan.h) under the sanitizers:
tests/chain_plan_driver.cpp is a stand-alone program that sweeps the capacities and pair counts to their extremes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "chain_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    # match_cap 1 .. 2^32 - 1 (18 values) x point_cap 1 .. 2^32 - 1 (5) x n_pairs 1 .. 65535 (15), 8 checks each
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 18 * 5 * 15 * 8, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 40, rows["args"]
    src = open(os.path.join(CSRC, "vslam_chain_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src

"""The side-stream scheduling policy (csrc/vslam_sched_policy.h) without a GPU: the join watchdog's trials and reverts, the
tuner's order and choice, and the ownership of every stream and event - the paths no GPU test can reach, because a lag
cannot be produced on purpose.  tests/sched_policy_driver.cpp plays the scripts with integers as handles."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("sched") / "driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "visualslam_amd", "csrc"),
                        os.path.join(ROOT, "tests", "sched_policy_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    res = {}
    for line in out.stdout.splitlines():
        name, *kv = line.split()
        res[name] = dict(x.split("=", 1) for x in kv)
    return res


def has(got, **want):
    assert {k: got[k] for k in want} == {k: str(v) for k, v in want.items()}, got


def test_the_policy_header_needs_no_hip():
    src = open(os.path.join(ROOT, "visualslam_amd", "csrc", "vslam_sched_policy.h")).read()
    assert "#include <hip" not in src and "hipStream_t" not in src and "hipEvent_t" not in src


def test_every_handle_is_released_exactly_once(played):
    # at the end of every script, teardown included: no handle left, none released twice, and teardown itself does not
    # touch the pair slots (nothing is decided by comparing handles)
    scripts = [k for k, v in played.items() if "never" in v]
    assert len(scripts) == 18, scripts
    for k in scripts:
        has(played[k], never=0, twice=0, slots_touched=0)
        assert int(played[k]["created"]) >= 7, k


def test_watchdog_scripts(played):
    has(played["s1"], level=1, done=1, trial_from=-1, path="1", pairs_created=1, early=0)  # lags far below 10 %: no trial
    has(played["s2"], level=2, done=1, trial_from=-1, path="12", pairs_created=1)  # 17.0 < 0.99 * 18.0: level 2 is kept
    has(played["s3"], level=1, done=1, trial_from=-1, path="121", pairs_created=1)  # 17.9 >= 17.82: back
    # the ADVICE case: 0 -> 1 kept (19.0 < 19.8), 1 -> 2 not kept (19.5 >= 18.81); both pairs exist and both go at teardown
    has(played["s4"], level=1, done=1, trial_from=-1, path="0121", pairs_created=2, low_prio=2, early=0, never=0, twice=0)
    has(played["s5first"], level=1)  # level 0 on a device without priority levels IS level 1, from the first call
    has(played["s5"], level=1, done=1, path="1", pairs_created=1, low_prio=0)
    has(played["s6trial"], level=2, trial_from=1)
    has(played["s6"], level=1, done=1, trial_from=-1, path="121")  # the fourth change of shape calls the trial off
    has(played["s7"], level=1, done=1, path="1", recorded=0)  # a shape alternating for ever: never a window of three
    # the host RING + 4 calls ahead: four recorded, four skipped, each measurement read once, no slot recorded over
    has(played["s8"], level=1, done=1, recorded=4, read=4, skipped=4, bad_read=0, lag="0.0100")


def test_tuner_scripts(played):
    for name, chosen in (("s9a", 2), ("s9b", 1), ("s9c", 0), ("s9d", 0)):
        # the losing pairs (4 streams) and the 8 events go when the comparison ends; the survivor is the level-0 pair
        has(played[name], tuner_done=1, chosen=chosen, states="0111122", cand1=0, cand2=0, aux_is_level0=1, early=12, pairs_created=3)
    has(played["s10"], tuner_done=1, chosen=0, resets=4, cand1=0, cand2=0, aux_is_level0=1)
    for name in ("s11first0", "s11first1"):
        has(played[name], tuner_done=1)  # nothing to compare at level 1: done at its first call
    has(played["s11"], level=1, done=1, pairs_created=1, recorded=3)  # ... and the watchdog then runs
    has(played["s11pinned"], level=1, done=1, pairs_created=1, recorded=0)
    has(played["seven"], states="0111122", tuner_done=1)


def test_teardown_in_mid_comparison_and_without_a_tuner(played):
    has(played["midfirst"], measured=2, tuner_events=4)
    has(played["mid"], tuner_done=0, cand1=1, cand2=0, pairs_created=2, early=0, never=0, twice=0)
    has(played["plain"], tuner_done=0, pairs_created=2, slots_touched=0, never=0, twice=0)  # (level 0, lag 5 %: the level-1 pair exists too)

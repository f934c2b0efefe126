"""What the cases of tests/limitcases.py are for, held on the CPU: tests/test_gpu_geometry_limits.py runs them on the device, and
here every case is shown to reach the code it was written for - so that a later change of EPI_WANT_WGS, EPI_TILE, a workgroup
size or a planted scene cannot quietly empty it.

The first test asks the plan headers themselves (tests/limits_plan_driver.cpp, built with -fsanitize=address,undefined) for
the grids of every call and asserts, per case, the trips of a score workgroup through its tile loop, the workgroups of the
per-pair kernels, the blocks of the ordered sum and the chunks of the ordered compaction.  The others evaluate every "require"
condition of the GPU file on the restatements' answers alone, and hold the restatements' inlier flags of the L1 winners to the
exact rational predicates (homref.exact_inlier, resectref.exact_inlier) over all their records."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import limitcases as LC
from tests import poseref, refitref, resectrefineref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
K = (800.0, 800.0, 960.0, 540.0)


def ceil_div(a, b):
    return -(-a // b)


def plans(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "limits_plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "limits_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    rows = LC.plan_rows()
    text = "".join("%s %d %d %d %d\n" % row[1:] for row in rows)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(rows)
    got = []
    for row, line in zip(rows, lines):
        assert line.split()[0] == row[1]
        got.append((row, {k: int(v) for k, v in (x.split("=") for x in line.split()[1:])}))
    assert subprocess.run([str(exe)], input="homography 600\n", capture_output=True, text=True, timeout=120).returncode == 2   # a short line
    assert subprocess.run([str(exe)], input="epipolar 600 600 3 64\n", capture_output=True, text=True, timeout=120).returncode == 2
    return got


def test_every_case_reaches_the_trips_workgroups_blocks_and_chunks_it_is_for(tmp_path):
    a, b = LC.CASES["L1"], LC.CASES["L2"]
    seen = set()
    for (case, stage, cap, pcap, n_pairs, H), p in plans(tmp_path):
        seen.add((case, stage))
        records = {"L1": a["records"], "L2": b["cap"], "L3": LC.CASES["L3"]["records"]}[case]
        used_tiles = ceil_div(records, LC.TILE)
        trips = ceil_div(used_tiles, p["nsplit"]) if "nsplit" in p else None
        print(f"{case} {stage}: cap {cap} pairs {n_pairs} H {H}: trips per score workgroup {trips}, pair workgroups {p.get('pair_blocks')}, "
              f"sum blocks {ceil_div(records, LC.SUM_BLOCK)} of {p.get('sum_blocks')}, compaction chunks {ceil_div(records, LC.CHUNK)}; {p}")
        assert p["fwords"] == ceil_div(cap, 64)
        if "tiles" in p:
            assert LC.TILE == 256 and p["tiles"] == ceil_div(cap, LC.TILE) and 1 <= p["nsplit"] <= min(64, p["tiles"])
            assert p["score_blocks"] == ceil_div(H, 256) and p["model_blocks"] == ceil_div(H, 64)
        if "pair_blocks" in p:
            assert p["pair_blocks"] == ceil_div(n_pairs, LC.PAIR_WG)
        if "sum_blocks" in p:
            assert p["sum_blocks"] == ceil_div(cap, LC.SUM_BLOCK)
        if "link_pairs" in p:
            assert p["link_pairs"] == n_pairs - 1
        if case == "L1":
            assert ceil_div(records, LC.CHUNK) >= 3 and ceil_div(min(a["over_count"], cap), LC.CHUNK) == 4     # compaction chunks
            assert ceil_div(records, LC.SUM_BLOCK) >= 10                                                       # blocks of the ordered sum that hold records
            if "sum_blocks" in p:
                assert p["sum_blocks"] == 16 == ceil_div(min(a["over_count"], cap), LC.SUM_BLOCK)
            if "tiles" in p:
                # 157 tiles over 64 splits: two or three trips per score workgroup, the last tile partly filled after full ones
                assert (used_tiles, p["nsplit"], p["tiles"]) == (157, 64, 256) and trips == 3 and used_tiles // p["nsplit"] >= 2
                assert records % LC.TILE == 101 and ceil_div(p["tiles"], p["nsplit"]) == 4
            if stage == "homography":
                assert p["score_blocks"] == (1 if H == 64 else 2)
        if case == "L2":
            if "tiles" in p:
                assert (p["tiles"], p["nsplit"]) == (3, 2) and trips >= 2            # workgroup 0 walks tiles 0 and 2
            if "pair_blocks" in p:
                assert p["pair_blocks"] == 24 >= 2 and n_pairs % LC.PAIR_WG == 28    # a partly filled last workgroup
            if "link_pairs" in p:
                assert p["link_pairs"] == 1499
        if case == "L3":
            assert p["score_blocks"] == 256 and p["model_blocks"] == 1024            # k_hom_select / k_res_select: 256 trips over h
    assert seen >= {("L1", s) for s in ("homography", "pose", "refit", "resect", "resect_refine")}
    assert seen >= {("L2", s) for s in ("homography", "pose", "refit", "resect", "resect_refine", "chain", "tracks")}
    assert seen >= {("L3", "homography"), ("L3", "resect")}
    # the workgroup sizes this file and the table assume are the headers'
    src = {name: open(os.path.join(CSRC, name)).read() for name in os.listdir(CSRC) if name.endswith("_plan.h")}
    for name, text in (("vslam_epipolar_plan.h", "EPI_TILE = 256"), ("vslam_epipolar_plan.h", "EPI_MAX_SPLIT = 64"), ("vslam_pose_plan.h", "POSE_PAIR_WG = 64"),
                       ("vslam_refit_plan.h", "REFIT_PAIR_WG = 64"), ("vslam_refit_plan.h", "REFIT_WG * REFIT_PER_LANE;  // 4096"),
                       ("vslam_homography_plan.h", "HOM_PAIR_WG = 64"), ("vslam_resect_refine_plan.h", "RR_PAIR_WG = 64")):
        assert text in src[name], (name, text)


# ---- L1

def cut_inside_chunk_1(flags):
    """The inlier_cap of the cut run: 5 records into chunk 1's share of the list -> (cut, inliers per chunk)."""
    per = LC.per_chunk(flags, 3)
    cut = int(per[0]) + LC.CASES["L1"]["cut_extra"]
    assert flags.sum() >= 0.5 * len(flags) and (per > 0).all(), (int(flags.sum()), per)      # require: 50 % inliers, some in every chunk
    assert per[0] < cut < per[0] + per[1]                                                     # require: the cut falls strictly inside chunk 1
    return cut, per


@pytest.mark.parametrize("H", LC.CASES["L1"]["hypotheses"])
def test_l1_homography_requirements(H):
    model, flags, _ = LC.l1_homography_restated(H)
    cut, per = cut_inside_chunk_1(flags)
    print("L1 homography H", H, "winner", int(model["best"][0]), "inliers", int(flags.sum()), per, "cut", cut)
    assert int(model["best"][0]) >= 0 and len(flags) == 40037
    if H == 64:
        assert (int(model["best"][0]), int(flags.sum()), per.tolist()) == (31, 27216, [11173, 11100, 4943])
    epi = LC.l1_epipolar_model("homography")[0]
    assert int(epi["best"][0]) >= 0 and int(epi["n_inliers"][0]) > 0                           # require: the verdict has something to judge


def test_l1_pose_and_refit_requirements():
    c = LC.CASES["L1"]
    pair, (model, flags) = LC.l1_epipolar_pair(), LC.l1_epipolar_model("epipolar")
    assert int(model["best"][0]) >= 0 and flags.sum() >= 0.5 * len(flags)
    pose = poseref.pose(model, *pair, K)[0]
    assert int(pose["best"][0]) >= 0 and int(pose["n_front"][0]) >= 0.5 * c["records"]
    _, info, rflags, _ = refitref.refit(model, *pair, c["rounds"], c["max_dist2"])
    cut, per = cut_inside_chunk_1(rflags)
    print("L1 refit", info, per, "cut", cut)
    assert int(info["accepted"][0]) >= 1 and int(info["n_before"][0]) > 8                       # require: the sums are taken, and a round is kept


def test_l1_resect_and_refine_requirements():
    c = LC.CASES["L1"]
    n = c["records"]
    caps = c["res_caps"]
    assert len(set(caps.values())) == 4
    models, links, corrs, flags, _ = LC.l1_resect_want(False)
    for j in (1, 2):
        usable = np.isin(np.arange(n), corrs[j]["b"])
        dropped = LC.per_chunk(~usable, 3)
        print("L1 resect pair", j, models[j], "dropped per chunk", dropped, "inliers per chunk", LC.per_chunk(flags[j], 3))
        assert int(models["best"][j]) >= 0 and int(models["n_obs"][j]) == n
        assert int(models["n_corr"][j]) < n and (dropped > 0).all() and dropped.sum() == n - int(models["n_corr"][j])   # require: the compaction is no copy, in any chunk
        assert ceil_div(int(models["n_corr"][j]), LC.SUM_BLOCK) >= 10                      # require: the refinement sums ten blocks
        assert flags[j].sum() >= 0.5 * n and (LC.per_chunk(flags[j], 3) > 0).all()
        assert (links[j][-40:] == -1).all() and (links[j] >= 0).sum() > int(models["n_corr"][j])    # the points past point_cap; links that the train side then drops
    assert int(models["best"][0]) == -1 and int(models["n_corr"][0]) == 0
    over = LC.l1_resect_want(True)[0]
    assert (over["n_obs"] == caps["obs_cap"]).all() and (over["n_corr"][1:] > 3 * LC.CHUNK).all() and (over["best"][1:] >= 0).all()   # four chunks
    for is_over in (False, True):
        m, cs, cap, Kk = LC.l1_refine_inputs(is_over)
        _, info, bits = rr.refine(m, rr.dense(cs, cap), c["refine_rounds"], c["max_dist2"], Kk, cap)
        print("L1 refine", "over" if is_over else "full", info)
        assert int(info["stop"][0]) == 5 and (info["accepted"][1:] >= 1).all() and (info["n_after"][1:] >= 0.5 * n).all()
        if is_over:
            assert (info["n_after"][1:] <= cap).all() and (info["n_before"][1:] > 3 * LC.CHUNK).all()


# ---- L2

def test_l2_trajectory_requirements():
    c = LC.CASES["L2"]
    d = LC.l2_resect_inputs()
    models, _, corrs, _, _ = LC.l2_resect_want()
    has = models["best"] >= 0
    print("L2 resect: models", int(has.sum()), "past pair 64", int(has[64:].sum()))
    assert has[64:].sum() >= 0.5 * (c["pairs"] - 64) and has[:64].any() and has[1472:].any()      # require: at least half the pairs past 64 have a model
    nc = models["n_corr"]
    assert (nc > 512).any() and (nc == 512).any() and (nc == 513).any() and (nc[64:] == 4).any()   # require: both sides of the second trip's boundary
    assert (models["best"][[8, 101, 102, 901]] == -1).all()                                        # after a pair without a pose
    _, info, _ = rr.refine(models, rr.dense(corrs, c["cap"]), c["refine_rounds"], c["max_dist2"], d["K"], c["cap"])
    stops = {int(s) for s in info["stop"][64:]}
    assert stops >= {1, 4, 5} and (info["accepted"][64:] >= 1).sum() >= 0.5 * (c["pairs"] - 64), stops
    chain = LC.l2_chain_want()[0]
    assert sorted(set(chain["segment"].tolist())) == [0, 7, 8, 100, 101, 102, 900, 901]               # four breaks
    summary = LC.l2_tracks_want()[4]
    print("L2 tracks: heads", int(summary["n_heads"].sum()), "good", int(summary["n_good"].sum()), "max_views", int(summary["max_views"].max()))
    assert summary["max_views"].max() >= 256 and summary["n_good"].sum() >= 0.5 * summary["n_heads"].sum()   # require: long paths that triangulate


def test_l2_list_requirements():
    c = LC.CASES["L2"]
    counts = LC.l2_counts()
    for at in c["planted_at"]:
        assert counts[at:at + 6].tolist() == list(c["planted_counts"])
    assert c["planted_at"][0] + 6 <= 64 <= c["planted_at"][1] and c["planted_at"][2] >= (c["pairs"] // 64) * 64
    assert (counts > 512).any() and (counts == 512).any()                      # require: the boundary of the second trip
    judged, gated, flags = LC.l2_homography_want()
    deg = judged["degenerate"][64:]
    has = judged["best"][64:] >= 0
    print("L2 lists: homography models past pair 64", int(has.sum()), "degenerate", int(deg.sum()), "gated models left", int((gated["best"][64:] >= 0).sum()))
    assert has.sum() >= 0.5 * len(has) and (deg == 0).any() and (deg == 1).any()          # require: every verdict value past pair 64
    assert (np.array([f.sum() for f in flags]) > c["inlier_cap"]).any()                    # require: lists that are cut
    pairs, epi = LC.l2_lists()
    assert (gated["best"][64:] >= 0).sum() >= 100 and (epi["best"][64:] >= 0).sum() >= 0.5 * len(has)
    # pose and refit start from the ungated records, so most pairs past 64 do work
    posed = sum(int(poseref.pose(epi[j:j + 1], *pairs[j], K)[0]["best"][0]) >= 0 for j in range(64, c["pairs"]))
    stops = np.bincount([int(refitref.refit(epi[j:j + 1], *pairs[j], c["rounds"], c["max_dist2"])[1]["stop"][0]) for j in range(64, c["pairs"])], minlength=6)
    print("L2 lists: poses past pair 64", posed, "refit stops", stops)
    assert posed >= 0.5 * len(has) and stops[[0, 4]].sum() >= 0.5 * len(has) and stops[5] > 0 and stops[1] > 0


# ---- L3

@pytest.mark.parametrize("max_dist2", LC.CASES["L3"]["max_dist2"])
def test_l3_requirements(max_dist2):
    from tests import homref, resectref

    c = LC.CASES["L3"]
    H, seed = c["hypotheses"], c["seed"]
    last = high = False
    for j, pair in enumerate(LC.l3_homography_pairs()):
        model, _, hyps = homref.ransac(*pair, H, seed, max_dist2, pair=j)
        lv, hw = LC.l3_require(max_dist2, int(model["best"][0]), int(model["n_inliers"][0]), hyps, 4)
        last, high = last or lv, high or hw
    assert last and (high or max_dist2 != 0.25)
    models, _, _, _, hyps = resectref.run(LC.l3_resect_inputs(), H, seed, max_dist2)
    last = high = False
    for j in (1, 2):
        lv, hw = LC.l3_require(max_dist2, int(models["best"][j]), int(models["n_inliers"][j]), hyps[j], 0)
        last, high = last or lv, high or hw
    assert last and (high or max_dist2 != 0.25)


# ---- L4

def test_l4_restated_flags_of_the_l1_winners_against_the_exact_predicates():
    model, flags, _ = LC.l1_homography_restated(LC.L4_HYPOTHESES)
    total = np.array(LC.l4_check(flags, LC.l4_homography_exact()))
    print(f"L4 homography restatement: {total[0]} records, {total[1]} exempt, {total[2]} disagreeing")
    assert total[0] == 40037 and total[2] == 0 and total[1] <= 0.01 * total[0]
    rflags = LC.l1_resect_want(False)[3]
    for j in LC.L4_RESECT_PAIRS:
        total = np.array(LC.l4_check(rflags[j], LC.l4_resect_exact(j)))
        print(f"L4 resect restatement, pair {j}: {total[0]} records, {total[1]} exempt, {total[2]} disagreeing")
        assert total[0] > 36864 and total[2] == 0 and total[1] <= 0.01 * total[0]

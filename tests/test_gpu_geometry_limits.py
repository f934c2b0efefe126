"""The stages from homography to tracks on the GPU at list capacity and past 64 pairs per call (vslam_homography_dev,
vslam_pose_dev, vslam_refit_dev, vslam_resect_dev, vslam_resect_refine_dev, vslam_chain_dev, vslam_tracks_dev; include/vslam.h):
bytes-equal against each stage's restatement through the stage's own Call class, like the stage files, but over the cases of
tests/limitcases.py -

L1  one pair of 40037 records under capacity 65536: a score workgroup takes two or three trips through its tile loop and ends
    on a tile of 101 records, the ordered compaction has three chunks, the ordered sum ten blocks; then the same with
    inlier_cap cut to 5 records inside chunk 1 (where the stage has one), and with a count above the capacity (65536 records,
    256 tiles, four chunks, sixteen blocks);
L2  1500 pairs in one call: 24 workgroups of every per-pair kernel, the last with 28 pairs, three record tiles dealt to two
    score workgroups, four breaks in the trajectory and tracks of up to 799 views; and a call that starts at pair 1000;
L3  65535 hypotheses under a seed that wraps, at three values of max_dist2;
L4  the device's own inlier bits of the L1 winners against the exact rational predicates, no restatement in between.

tests/test_geometry_limits_cpu.py shows on the CPU that every case reaches what it is for, and evaluates the "require"
conditions on the restatements alone; the ones that bear on a comparison are repeated here."""
import numpy as np
import pytest

from tests import limitcases as LC
from tests import chainref
from tests import test_gpu_chain as TCH, test_gpu_pose as TP, test_gpu_refit as TF, test_gpu_resect as TR, test_gpu_resect_refine as TRR, test_gpu_tracks as TT
from tests.test_geometry_limits_cpu import cut_inside_chunk_1
from tests.test_gpu_homography import Call, env  # noqa: F401 (env: the module's fixture)
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
L1, L2, L3 = LC.CASES["L1"], LC.CASES["L2"], LC.CASES["L3"]
_WANT = {}


def once(key, make):
    """The restatement's answer under `key`, computed once: the full run and the cut run of a stage read the same records."""
    if key not in _WANT:
        _WANT[key] = make()
    return _WANT[key]


class HomographyCall(Call):
    key = None

    def want(self, j, seed, max_dist2=4.0, pair=None):
        return once(("homography", self.key, j, seed, max_dist2, pair), lambda: Call.want(self, j, seed, max_dist2, pair))


class RefitCall(TF.Call):
    key = None

    def want(self, j, rounds=4, max_dist2=4.0):
        return once(("refit", self.key, j, rounds, max_dist2), lambda: TF.Call.want(self, j, rounds, max_dist2))


def unpacked(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


# ---- L1. one pair at the detector's capacity

@pytest.mark.parametrize("run", ["full", "cut", "over"])
@pytest.mark.parametrize("H", L1["hypotheses"])  # 300: two score blocks, the second partly filled
def test_l1_homography_at_capacity(env, H, run):
    ctx, torch = env
    pair, cap, seed = LC.l1_homography_pair(), L1["cap"], L1["hom_seed"]
    cut, _ = cut_inside_chunk_1(LC.l1_homography_restated(H)[1])          # require: 50 % inliers, some in every chunk, the cut inside chunk 1
    call = HomographyCall(torch, [pair], cap, cap, H, inlier_cap=cut if run == "cut" else cap, counts=[L1["over_count"]] if run == "over" else None,
                          epi=LC.l1_epipolar_model("homography")[0].copy())
    call.key = (H, run == "over")
    got = call.run(ctx, torch, seed=seed, max_dist2=L1["max_dist2"])
    model, flags, _ = call.check(got, 0, seed=seed, max_dist2=L1["max_dist2"])
    call.check_rows_past_the_call(got)
    assert int(model["n_matches"][0]) == len(flags) == (cap if run == "over" else L1["records"]) and int(model["best"][0]) >= 0
    assert int(model["n_epipolar"][0]) > 0                                # the verdict had an epipolar model to judge


@pytest.mark.parametrize("run", ["full", "over"])
def test_l1_pose_at_capacity(env, run):
    ctx, torch = env
    pair, cap = LC.l1_epipolar_pair(), L1["cap"]
    call = TP.Call(torch, [(LC.l1_epipolar_model("epipolar")[0],) + pair], cap, cap, counts=[L1["over_count"]] if run == "over" else None)
    got = call.run(ctx, torch)
    pose, _, flags, X = call.check(got, 0)
    call.check_rows_past_the_call(got)
    assert int(pose["n_matches"][0]) == len(X) == (cap if run == "over" else L1["records"]) and int(pose["best"][0]) >= 0
    assert flags[:L1["records"]].sum() >= 0.5 * L1["records"]


@pytest.mark.parametrize("run", ["full", "cut", "over"])
def test_l1_refit_at_capacity(env, run):
    ctx, torch = env
    pair, cap, model = LC.l1_epipolar_pair(), L1["cap"], LC.l1_epipolar_model("epipolar")[0]
    tight = RefitCall(torch, [(model,) + pair], cap, cap)
    tight.key = False
    cut, _ = cut_inside_chunk_1(tight.want(0, L1["rounds"], L1["max_dist2"])[2])
    call = RefitCall(torch, [(model,) + pair], cap, cap, counts=[L1["over_count"]] if run == "over" else None, inlier_cap=cut if run == "cut" else None)
    call.key = run == "over"
    got = call.run(ctx, torch, rounds=L1["rounds"], max_dist2=L1["max_dist2"])
    _, info, flags = call.check(got, 0, rounds=L1["rounds"], max_dist2=L1["max_dist2"])
    call.check_rows_past_the_call(got)
    assert len(flags) == (cap if run == "over" else L1["records"]) and int(info["n_before"]) > 0.5 * L1["records"] and int(info["accepted"]) >= 1


@pytest.mark.parametrize("run", ["full", "over"])
def test_l1_resect_at_capacity_under_four_different_capacities(env, run):
    ctx, torch = env
    over = run == "over"
    call = TR.Call(torch, LC.l1_resect_inputs(over), L1["res_hypotheses"])
    assert {call.cap, call.ocap, call.tcap, call.d["point_cap"]} == set(L1["res_caps"].values()) and len(set(L1["res_caps"].values())) == 4
    want = LC.l1_resect_want(over)
    models = want[0]
    # require: a winner, the usable records fewer than the records (the compaction is no copy), three chunks - four in the over run
    assert (models["best"][1:] >= 0).all() and (models["n_corr"][1:] < models["n_obs"][1:]).all()
    assert (models["n_corr"][1:] > (3 if over else 2) * LC.CHUNK).all() and (models["n_inliers"][1:] >= 0.5 * L1["records"]).all()
    call.check(call.run(ctx, torch, seed=L1["res_seed"], max_dist2=L1["max_dist2"]), want)


@pytest.mark.parametrize("run", ["full", "over"])
def test_l1_resect_refine_over_the_resections_answer(env, run):
    ctx, torch = env
    models, corrs, cap, K = LC.l1_refine_inputs(run == "over")
    call = TRR.Call(torch, models, corrs, cap, K)
    want = call.want(L1["refine_rounds"], L1["max_dist2"])
    info = want[1]
    assert (info["accepted"][1:] >= 1).all() and (info["n_before"][1:] > (3 if run == "over" else 1) * LC.CHUNK).all()    # require: sums over ten (sixteen) blocks are kept
    call.check(call.run(ctx, torch, L1["refine_rounds"], L1["max_dist2"]), want)


# ---- L2. 1500 pairs in one call

def equal_from(part, full, s, names, skip=0):
    """A call over the pairs s .. gives the records of the whole call, from its pair `skip` on."""
    n = L2["pairs"]
    for k in names:
        assert part[k][skip:n - s].tobytes() == full[k][s + skip:n].tobytes(), k


def test_l2_resect_1500_pairs_and_a_call_that_starts_at_pair_1000(env):
    ctx, torch = env
    d, want, seed, s = LC.l2_resect_inputs(), LC.l2_resect_want(), L2["res_seed"], L2["sub_call"]
    has = want[0]["best"] >= 0
    assert has[64:].sum() >= 0.5 * (L2["pairs"] - 64) and has[1472:].any()           # require: models past pair 64, and in the last workgroup
    call = TR.Call(torch, d, L2["hypotheses"])
    full = call.run(ctx, torch, seed=seed, max_dist2=L2["max_dist2"])
    call.check(full, want)
    # a second call that starts at pair s, its seed advanced by s: pairs s + 1 .. give the same records (pair s is its pair 0)
    part = TR.Call(torch, d, L2["hypotheses"]).run(ctx, torch, seed=seed + s, first=s, max_dist2=L2["max_dist2"])
    for k in TR.OUTS:
        assert part[k][s + 1:].tobytes() == full[k][s + 1:].tobytes(), k
        assert (part[k][:s] == TR.SENT).all(), k
    first = part["models"][s].view(capi.RESECT_DTYPE)[0]
    assert int(first["best"]) == -1 and int(first["n_corr"]) == 0 and int(first["n_obs"]) == int(want[0]["n_obs"][s])


def test_l2_resect_refine_1500_pairs_and_a_call_over_the_last_500(env):
    ctx, torch = env
    models, _, corrs, _, _ = LC.l2_resect_want()
    K, s = LC.l2_resect_inputs()["K"], L2["sub_call"]
    call = TRR.Call(torch, models, corrs, L2["cap"], K)
    want = call.want(L2["refine_rounds"], L2["max_dist2"])
    assert {int(v) for v in want[1]["stop"][64:]} >= {1, 4, 5} and (want[1]["accepted"][64:] >= 1).sum() >= 0.5 * (L2["pairs"] - 64)   # require
    full = call.run(ctx, torch, L2["refine_rounds"], L2["max_dist2"])
    call.check(full, want)
    part = TRR.Call(torch, models[s:], corrs[s:], L2["cap"], K).run(ctx, torch, L2["refine_rounds"], L2["max_dist2"])
    equal_from(part, full, s, ("models", "info", "inlier_bits"))


class Trajectory:
    """The structure side of the planted trajectory from pair `first` on, with the attributes tests/test_gpu_chain.py's and
    tests/test_gpu_tracks.py's Call read from their Inputs."""

    def __init__(self, first=0):
        d = LC.l2_resect_inputs()
        self.n, self.pcap, self.cap = L2["pairs"] - first, d["point_cap"], L2["cap"]
        self.words = (self.cap + 63) // 64
        self.poses, self.matches, self.counts = d["poses"][first:], d["matches"][first:], d["match_counts"][first:]
        self.points, self.bits = d["points"][first:], d["front_bits"][first:]
        self.chain, self.frames = LC.l2_chain_want()[0], LC.l2_frames()


def test_l2_chain_1500_pairs_and_a_call_over_the_last_500(env):
    ctx, torch = env
    want = LC.l2_chain_want()
    assert sorted(set(want[0]["segment"].tolist())) == [0, 7, 8, 100, 101, 102, 900, 901]        # require: four breaks
    call = TCH.Call(torch, Trajectory())
    call.check(call.run(ctx, torch, L2["min_links"]), want)
    # a call that starts at pair s is a trajectory of its own: against the restatement over the same 500 pairs
    sub = Trajectory(L2["sub_call"])
    call = TCH.Call(torch, sub)
    call.check(call.run(ctx, torch, L2["min_links"]), chainref.chain(sub.poses, sub.matches, sub.counts, sub.points, sub.bits, sub.pcap, L2["min_links"]))


def test_l2_tracks_of_up_to_799_views(env):
    ctx, torch = env
    want = LC.l2_tracks_want()
    summary = want[4]
    assert summary["max_views"].max() >= 256 and summary["n_good"].sum() >= 0.5 * summary["n_heads"].sum()    # require: long paths that triangulate
    call = TT.Call(torch, Trajectory())
    call.check(call.run(ctx, torch, L2["max_dist2"], L2["min_views"]), want)


def l2_model_pairs():
    pairs, epi = LC.l2_lists()
    return [(epi[j:j + 1],) + pairs[j] for j in range(L2["pairs"])]


def test_l2_homography_1500_pairs_and_a_call_that_starts_at_pair_1000(env):
    ctx, torch = env
    (pairs, epi), seed, s = LC.l2_lists(), L2["hom_seed"], L2["sub_call"]
    judged, gated, _ = LC.l2_homography_want()
    deg = judged["degenerate"][64:]
    assert (deg == 0).any() and (deg == 1).any() and (judged["best"][64:] >= 0).sum() >= 0.5 * len(deg)       # require: every verdict past pair 64
    make = lambda ps, e: Call(torch, ps, L2["cap"], L2["point_cap"], L2["hypotheses"], inlier_cap=L2["inlier_cap"], epi=e.copy())
    call = make(pairs, epi)
    full = call.run(ctx, torch, seed=seed, max_dist2=L2["max_dist2"])
    call.check_rows_past_the_call(full)
    for j in range(L2["pairs"]):
        call.check(full, j, seed=seed, max_dist2=L2["max_dist2"])
    n = L2["pairs"]
    assert full["models"][:n].tobytes() == judged.tobytes() and full["gated_models"][:n].tobytes() == gated.tobytes()
    part = make(pairs[s:], epi[s:]).run(ctx, torch, seed=seed + s, max_dist2=L2["max_dist2"])   # pair 0 of a call with seed + s samples like pair s
    equal_from(part, full, s, full.keys())


def test_l2_pose_1500_pairs_and_a_call_over_the_last_500(env):
    ctx, torch = env
    pairs, s = l2_model_pairs(), L2["sub_call"]
    call = TP.Call(torch, pairs, L2["cap"], L2["point_cap"])
    full = call.run(ctx, torch)
    call.check_rows_past_the_call(full)
    posed = sum(int(call.check(full, j)[0]["best"][0]) >= 0 for j in range(L2["pairs"]))
    assert posed >= 0.5 * L2["pairs"]
    part = TP.Call(torch, pairs[s:], L2["cap"], L2["point_cap"]).run(ctx, torch)
    equal_from(part, full, s, full.keys())


def test_l2_refit_1500_pairs_and_a_call_over_the_last_500(env):
    ctx, torch = env
    pairs, s = l2_model_pairs(), L2["sub_call"]
    make = lambda ps: TF.Call(torch, ps, L2["cap"], L2["point_cap"], inlier_cap=L2["inlier_cap"])
    call = make(pairs)
    full = call.run(ctx, torch, rounds=L2["rounds"], max_dist2=L2["max_dist2"])
    call.check_rows_past_the_call(full)
    stops = np.bincount([int(call.check(full, j, rounds=L2["rounds"], max_dist2=L2["max_dist2"])[1]["stop"]) for j in range(64, L2["pairs"])], minlength=6)
    assert stops[[0, 4]].sum() >= 0.5 * (L2["pairs"] - 64) and stops[1] > 0 and stops[5] > 0          # require: work past pair 64, and pairs that stop at once
    part = make(pairs[s:]).run(ctx, torch, rounds=L2["rounds"], max_dist2=L2["max_dist2"])
    equal_from(part, full, s, full.keys())


# ---- L3. hypothesis and seed limits

@pytest.mark.parametrize("max_dist2", L3["max_dist2"])
def test_l3_homography_65535_hypotheses_and_a_seed_that_wraps(env, max_dist2):
    ctx, torch = env
    H, seed = L3["hypotheses"], L3["seed"]   # pair j hashes seed + j: 2^32 - 1, 0, 1
    call = Call(torch, LC.l3_homography_pairs(), L3["records"], L3["records"], H)
    got = call.run(ctx, torch, seed=seed, max_dist2=max_dist2)
    last = high = False
    for j in range(L3["pairs"]):
        model, _, hyps = call.check(got, j, seed=seed, max_dist2=max_dist2)
        lv, hw = LC.l3_require(max_dist2, int(model["best"][0]), int(model["n_inliers"][0]), hyps, 4)   # require: the tie the value is for
        last, high = last or lv, high or hw
    call.check_rows_past_the_call(got)
    assert last                               # require: hypothesis 65534, the last one, is valid for some pair
    assert high or max_dist2 != 0.25          # require: a winner that needs all 16 bits of the selection key's h field


@pytest.mark.parametrize("max_dist2", L3["max_dist2"])
def test_l3_resect_65535_hypotheses_and_a_seed_that_wraps(env, max_dist2):
    ctx, torch = env
    H, seed = L3["hypotheses"], L3["seed"]
    call = TR.Call(torch, LC.l3_resect_inputs(), H)
    want = call.want(seed, max_dist2)
    models, hyps = want[0], want[4]
    last = high = False
    for j in range(1, L3["pairs"]):
        lv, hw = LC.l3_require(max_dist2, int(models["best"][j]), int(models["n_inliers"][j]), hyps[j], 0)
        last, high = last or lv, high or hw
    assert last and (high or max_dist2 != 0.25)
    call.check(call.run(ctx, torch, seed=seed, max_dist2=max_dist2), want)


# ---- L4. the device against exact rational arithmetic, no restatement in between

def test_l4_device_homography_inlier_bits_against_the_exact_transfer_predicates(env):
    ctx, torch = env
    n = L1["records"]
    # the exact predicates are evaluated under the restatement's winner: the device's must be the same doubles
    want = LC.l1_homography_restated(LC.L4_HYPOTHESES)[0]
    call = Call(torch, [LC.l1_homography_pair()], L1["cap"], L1["cap"], LC.L4_HYPOTHESES)
    got = call.run(ctx, torch, seed=L1["hom_seed"], max_dist2=L1["max_dist2"])
    g = got["models"][0].view(capi.HOMOGRAPHY_DTYPE)[0]
    assert g["H"].tobytes() == want["H"][0].tobytes() and g["G"].tobytes() == want["G"][0].tobytes() and int(g["best"]) >= 0
    bits = unpacked(got["inlier_bits"][0], n)
    assert int(g["n_inliers"]) == int(bits.sum()) >= 0.5 * n
    total = np.array(LC.l4_check(bits, LC.l4_homography_exact()))
    print(f"L4 homography device: {total[0]} records, {total[1]} exempt, {total[2]} disagreeing")
    assert total[0] == n and total[2] == 0 and total[1] <= 0.01 * total[0]


@pytest.mark.parametrize("j", LC.L4_RESECT_PAIRS)
def test_l4_device_resect_inlier_bits_against_the_exact_reprojection_predicate(env, j):
    ctx, torch = env
    n = L1["records"]
    models = LC.l1_resect_want(False)[0]
    call = TR.Call(torch, LC.l1_resect_inputs(False), L1["res_hypotheses"])
    got = call.run(ctx, torch, seed=L1["res_seed"], max_dist2=L1["max_dist2"])
    g = got["models"][j].view(capi.RESECT_DTYPE)[0]
    assert g["R"].tobytes() == models["R"][j].tobytes() and g["t"].tobytes() == models["t"][j].tobytes() and int(g["best"]) >= 0
    bits = unpacked(got["inlier_bits"][j], n)
    assert int(g["n_inliers"]) == int(bits.sum()) >= 0.5 * n
    total = np.array(LC.l4_check(bits, LC.l4_resect_exact(j)))
    print(f"L4 resect device, pair {j}: {total[0]} records, {total[1]} exempt, {total[2]} disagreeing")
    assert total[0] == int(g["n_corr"]) and total[2] == 0 and total[1] <= 0.01 * total[0]

"""Two-view geometry on the GPU at the detector's capacity and at the limits of its parameters (vslam_epipolar_dev,
include/vslam.h): bytes-equal against tests/epiref.py like tests/test_gpu_epipolar.py, but with records in three 16384-record chunks of the
ordered list (four at the 65536 capacity, in the run whose count exceeds it) and 64 record splits per pair, 65535 hypotheses, a seed that wraps, max_dist2 from 4 * 2^-1074 to 1e300, octaves
up to 31, negative coordinates, samples that cannot give a model, and 1500 pairs in one call.  The last test compares the
device's own inlier bits with the Sampson inequality in exact rational arithmetic (epiref.exact_inlier), with no restatement
in between.

Every "require" comment marks a condition on the input, evaluated on the restatement's answer alone: the case only
exercises what it is for while it holds."""
import functools

import numpy as np
import pytest

from tests import epiref
from tests.test_gpu_epipolar import Call, env, make_pair  # noqa: F401 (env: the module's fixture)
from tests.test_match_epipolar_exact_cpu import check_flags_against_exact
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
CHUNK = 16384  # match records per workgroup of the count -> scan -> scatter kernels: 256 flag words of 64 records


def winner(got, j=0):
    return got["models"][j].view(capi.EPIPOLAR_DTYPE).reshape(-1)[0]


# ---- D1. a pair at capacity

@functools.lru_cache(maxsize=None)
def large_scene():
    mt, qp, tp, _ = epiref.planted_scene(5, n=40037)
    for a in (mt, qp, tp):
        a.setflags(write=False)
    return mt, qp, tp


@pytest.mark.parametrize("H", [64, 300])  # 300: two score blocks, the second partly filled
def test_d1_40037_records_three_chunks_four_at_capacity_and_64_record_splits(env, H):
    ctx, torch = env
    pair, cap, seed = large_scene(), 65536, 5
    _, flags, _ = epiref.ransac(*pair, H, seed, 4.0)
    per_chunk = np.bincount(np.flatnonzero(flags) // CHUNK, minlength=3)
    assert flags.sum() >= 0.5 * len(flags) and (per_chunk > 0).all(), (int(flags.sum()), per_chunk)  # require: 50 % inliers, some in every chunk
    cut = int(per_chunk[0]) + 5  # the cut falls inside chunk 1
    assert per_chunk[0] < cut < per_chunk[0] + per_chunk[1]
    for inlier_cap, counts in ((cap, None), (cut, None), (cap, [100000])):  # the last: min(count, cap) = 65536 records, 256 tiles
        call = Call(torch, [pair], cap, cap, H, inlier_cap=inlier_cap, counts=counts)
        got = call.run(ctx, torch, seed=seed)
        model, _, _ = call.check(got, 0, seed=seed)
        call.check_rows_past_the_call(got)
        assert int(model["n_matches"][0]) == (40037 if counts is None else cap) and int(model["best"][0]) >= 0


# ---- D2. hypothesis and seed limits

@pytest.mark.parametrize("max_dist2,scene", [(1e300, 20), (1e-300, 20), (0.25, 22)])  # the scenes: chosen so that the requirements below hold
def test_d2_65535_hypotheses_and_a_seed_that_wraps(env, max_dist2, scene):
    ctx, torch = env
    H, seed = 65535, 0xFFFFFFFF  # pair j hashes seed + j: 2^32 - 1, 0, 1
    pairs = [epiref.planted_scene(scene + j, n=64, outliers=0.0)[:3] for j in range(3)]
    call = Call(torch, pairs, 64, 64, H)
    got = call.run(ctx, torch, seed=seed, max_dist2=max_dist2)
    last_valid, high_winner = False, False
    for j in range(3):
        model, flags, hyps = call.check(got, j, seed=seed, max_dist2=max_dist2)
        first = int(np.flatnonzero(hyps["valid"])[0])
        last_valid |= bool(hyps["valid"][H - 1])
        high_winner |= int(model["best"][0]) >= 32768
        # require: a tie of all valid hypotheses - at 64 inliers or at none - so the winner is the lowest valid h
        if max_dist2 == 1e300:
            assert (hyps["inliers"][hyps["valid"] == 1] == 64).all() and int(model["best"][0]) == first and flags.all()
        if max_dist2 == 1e-300:
            assert not hyps["inliers"].any() and int(model["best"][0]) == first and int(model["n_inliers"][0]) == 0
        assert winner(got, j)["best"] == model["best"][0] and int(model["n_valid"][0]) > H // 2
    call.check_rows_past_the_call(got)
    assert last_valid                      # require: hypothesis 65534, the last one, is valid for some pair
    if max_dist2 == 0.25:
        assert high_winner                 # require: a winner that needs all 16 bits of the selection key's h field


# ---- D3. coordinate range

def scene_one():
    return tuple(a.copy() for a in epiref.planted_scene(1)[:3])


@pytest.mark.parametrize("shift", [20, 29])
def test_d3_octaves_up_to_31(env, shift):
    ctx, torch = env
    mt, qp, tp = scene_one()
    qp["octave"] += shift
    tp["octave"] += shift
    n = len(mt)
    # three more records, copies of records 0 .. 2: one at octave 31 (trusted), one at 32 and one at -1 (not trusted)
    qp, tp, mt = np.concatenate([qp, qp[mt["query"][:3]]]), np.concatenate([tp, tp[mt["train"][:3]]]), np.concatenate([mt, mt[:3]])
    mt["query"][n:], mt["train"][n:] = np.arange(n, n + 3), np.arange(n, n + 3)
    qp["octave"][n], tp["octave"][n] = 31, 31
    qp["octave"][n + 1] = 32
    tp["octave"][n + 2] = -1
    max_dist2 = 4.0 * 4.0 ** shift
    call = Call(torch, [(mt, qp, tp)], n + 3, n + 3, 512)
    got = call.run(ctx, torch, seed=1, max_dist2=max_dist2)
    model, flags, _ = call.check(got, 0, seed=1, max_dist2=max_dist2)
    call.check_rows_past_the_call(got)
    xy = epiref.coords(mt, qp, tp)
    print("octaves +", shift, ": n_valid", int(model["n_valid"][0]), "inliers", int(flags.sum()), "largest coordinate of the shifted scene", np.abs(xy[:n]).max())
    assert int(model["n_valid"][0]) > 0 and flags.sum() >= 200            # require
    assert not np.isnan(xy[n]).any() and np.isnan(xy[n + 1:]).all() and not flags[n + 1:].any()


def test_d3_negative_coordinates(env):
    ctx, torch = env
    mt, qp, tp = scene_one()
    qp["padding"] += 3000
    call = Call(torch, [(mt, qp, tp)], len(mt), len(mt), 512)
    got = call.run(ctx, torch, seed=1)
    model, flags, _ = call.check(got, 0, seed=1)
    xy = epiref.coords(mt, qp, tp)
    call.check_rows_past_the_call(got)
    print("negative coordinates: n_valid", int(model["n_valid"][0]), "inliers", int(flags.sum()))
    assert (xy[:, 0] < 0).mean() > 0.5 and (xy[:, 1] < 0).mean() > 0.5 and int(model["n_valid"][0]) > 256 and flags.sum() >= 16   # require


@pytest.mark.parametrize("max_dist2", [1e-12, 4 * 2.0 ** -1074])
def test_d3_tiny_max_dist2(env, max_dist2):
    ctx, torch = env
    assert max_dist2 > 0.0
    pair = scene_one()
    call = Call(torch, [pair], len(pair[0]), len(pair[0]), 512)
    got = call.run(ctx, torch, seed=1, max_dist2=max_dist2)
    model, _, _ = call.check(got, 0, seed=1, max_dist2=max_dist2)
    call.check_rows_past_the_call(got)
    assert int(model["n_valid"][0]) > 256 and int(model["best"][0]) >= 0     # require


# ---- D4. samples that give no model

@pytest.mark.parametrize("kind", ["collinear", "coincident"])
def test_d4_degenerate_pairs(env, kind):
    ctx, torch = env
    mt, qp, tp, _ = epiref.planted_scene(40, n=64, outliers=0.0)
    qp["octave"], qp["padding"], qp["row"] = 1, 0, 100   # every query point on the row y = 100: three columns of the 8 x 9 matrix are zero
    if kind == "coincident":
        qp["col"] = 200                                  # every query point the same: the mean distance d is 0
    H = 128
    call = Call(torch, [(mt, qp, tp)], 64, 64, H)
    got = call.run(ctx, torch, seed=3)
    model, flags, hyps = call.check(got, 0, seed=3)
    call.check_rows_past_the_call(got)
    # require: no hypothesis gives a model
    assert int(model["n_valid"][0]) == 0 and int(model["best"][0]) == -1 and not hyps["valid"].any() and not flags.any()
    g = winner(got)
    assert int(g["best"]) == -1 and int(g["n_valid"]) == 0 and int(g["n_matches"]) == 64 and not g["F"].any()


# ---- D5. many small pairs

def test_d5_1500_small_pairs_in_one_call(env):
    ctx, torch = env
    rng = np.random.default_rng(105)
    n, cap = 1500, 24
    pairs = [make_pair(3000 + j, int(rng.integers(0, cap + 1)), specials=(j % 3 == 0)) for j in range(n)]
    call = Call(torch, pairs, cap, cap + 3, 16, inlier_cap=4)
    got = call.run(ctx, torch, seed=9)
    call.check_rows_past_the_call(got)
    models = [call.check(got, j, seed=9)[0] for j in range(n)]
    best = np.array([int(m["best"][0]) for m in models])
    inl = np.array([int(m["n_inliers"][0]) for m in models])
    assert (best == -1).any() and (best > 0).any() and (inl > 4).any()  # require: pairs without a model, later winners, lists that are cut


# ---- C3. the device against exact rational arithmetic, no restatement in between

def test_c3_device_inlier_bits_against_the_exact_sampson_predicate(env):
    ctx, torch = env
    pairs = [epiref.planted_scene(seed)[:3] for seed in (1, 2, 3, 4)]
    call = Call(torch, pairs, 300, 300, 512)
    got = call.run(ctx, torch, seed=1)
    total = np.zeros(3, np.int64)
    for j, (mt, qp, tp) in enumerate(pairs):
        g = winner(got, j)
        bits = np.unpackbits(got["inlier_bits"][j].view(np.uint8), bitorder="little")[:300].astype(bool)
        assert int(g["best"]) >= 0 and int(g["n_inliers"]) == int(bits.sum()) > 100
        total += check_flags_against_exact(g["F"], epiref.coords(mt, qp, tp), bits, 4.0)
    print(f"C3 device: {total[0]} records, {total[1]} exempt, {total[2]} disagreeing")
    assert total[2] == 0 and total[1] <= 0.01 * total[0]

"""Guided matching under H or F on the GPU (vslam_match_guided_hf_dev / vslam_match_guided_hf_host, include/vslam.h): every
comparison is bytes-equal against the CPU restatement in tests/guidedhfref.py - every nn row, every match record, every count, and
the sentinels past every count.  Most sets carry their points on the exact fixtures of tests/test_guided_hf_cpu.py and
tests/test_guided_cpu.py, where window and band membership are decided by construction."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import guidedhfref, guidedref, homref, matchref
from tests.test_gpu_guided import SENT, side_to_device
from tests.test_guided_cpu import BAND2, EXACT_F, identity_sets, lattice_points
from tests.test_guided_hf_cpu import (EXACT_H, HAND, HORIZON_H, WINDOW2, build_cxx_driver, check_scene_conditions, figures_of, scene_chain,
                                      with_entry, xy_points)
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_OK, E_NO = guidedref.model_record(EXACT_F), guidedref.model_record(EXACT_F, best=-1)
H_OK, H_NO = guidedhfref.homography_record(EXACT_H), guidedhfref.homography_record(EXACT_H, best=-1)
H_NEG = guidedhfref.homography_record(tuple(-v for v in EXACT_H))  # the same projected position with p2 = -1 everywhere: no row is in window


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def pair(q, t, q_points, t_points, emodel=None, hmodel=None, q_defined=None, t_defined=None, q_count=None, t_count=None):
    """One pair of a call.  emodel / hmodel None: the call passes no such array (then none of its pairs may have one).
    *_count: the count the device is given (default: the number of rows; above the capacity it is clamped)."""
    return dict(q=np.asarray(q, np.float32).reshape(-1, 128), t=np.asarray(t, np.float32).reshape(-1, 128), q_points=q_points, t_points=t_points,
                emodel=emodel, hmodel=hmodel, q_defined=q_defined, t_defined=t_defined, q_count=q_count, t_count=t_count)


def models_to_device(torch, pairs, key, words):
    given = [p[key] is not None for p in pairs]
    assert all(given) or not any(given), "a model array is there for every pair of a call or for none"
    if not given[0]:
        return None
    return torch.from_numpy(np.concatenate([p[key] for p in pairs]).view(np.int32).reshape(len(pairs), words)).to(DEV)


PRM = dict(ratio2=0.64, max_desc_dist2=np.inf, max_dist2=BAND2, max_transfer2=WINDOW2, same_octave=False)


def run_dev(ctx, torch, pairs, qcap, tcap, match_cap=None, with_defined=True, only=("nn", "matches", "match_counts"), n_pairs=None, **prm):
    """One vslam_match_guided_hf_dev call over `pairs` -> (nn, matches, counts) as numpy, sentinel-filled where nothing was written."""
    n = len(pairs)
    Q, kq = side_to_device(torch, pairs, "q", qcap, with_defined)
    T, kt = side_to_device(torch, pairs, "t", tcap, with_defined)
    em, hm = models_to_device(torch, pairs, "emodel", 22), models_to_device(torch, pairs, "hmodel", 42)
    match_cap = qcap if match_cap is None else match_cap
    outs = dict(nn=torch.full((n, qcap, 3), SENT, dtype=torch.int32, device=DEV), matches=torch.full((n, match_cap, 3), SENT, dtype=torch.int32, device=DEV),
                match_counts=torch.full((n,), SENT, dtype=torch.int32, device=DEV))
    ctx.match_guided_hf(Q, T, em, hm, n if n_pairs is None else n_pairs, **dict(PRM, **prm), **{k: v for k, v in outs.items() if k in only})
    torch.cuda.synchronize()
    return tuple(outs[k].cpu().numpy() for k in ("nn", "matches", "match_counts"))


def restated(p, qcap, tcap, **prm):
    nq = min(len(p["q"]) if p["q_count"] is None else p["q_count"], qcap, len(p["q"]))
    nt = min(len(p["t"]) if p["t_count"] is None else p["t_count"], tcap, len(p["t"]))
    cut = lambda a, k: None if a is None else np.asarray(a)[:k]
    return guidedhfref.guided_hf(p["q"][:nq], p["t"][:nt], p["q_points"][:nq], p["t_points"][:nt], p["emodel"], p["hmodel"],
                                 q_defined=cut(p["q_defined"], nq), t_defined=cut(p["t_defined"], nt), **dict(PRM, **prm))


def check_pair(got, j, p, qcap, tcap, match_cap=None, **prm):
    nn, matches, counts = got
    match_cap = qcap if match_cap is None else match_cap
    wnn, wm = restated(p, qcap, tcap, **prm)
    nq = len(wnn)
    diff = (nn[j, :nq].view(np.uint8).reshape(nq, 12) != wnn.view(np.uint8).reshape(nq, 12)).any(axis=1)
    assert not diff.any(), ("nn", j, int(diff.sum()), nq, np.flatnonzero(diff)[:8], nn[j, :nq].view(capi.NN2_DTYPE).reshape(-1)[diff][:4], wnn[diff][:4])
    assert (nn[j, nq:] == SENT).all(), "nn rows past the count were written"
    assert counts[j] == len(wm), ("match_counts", j, int(counts[j]), len(wm))
    m = min(len(wm), match_cap)
    assert matches[j, :m].tobytes() == wm[:m].tobytes(), ("matches", j)
    assert (matches[j, m:] == SENT).all(), "matches past the count were written"
    return wnn, wm


# ---- the hand-made sets of the CPU file, on the device

def test_hand_made_sets_equal_the_restatement(env):
    ctx, torch = env
    groups = {}
    for name, (case, _, _) in HAND.items():
        prm = {k: case[k] for k in ("ratio2", "max_desc_dist2", "max_dist2", "max_transfer2", "same_octave") if k in case}
        key = (tuple(sorted(prm.items())), case["epipolar_model"] is None, case["homography_model"] is None)
        groups.setdefault(key, []).append((name, pair(case["q"], case["t"], case["q_points"], case["t_points"], case["epipolar_model"],
                                                      case["homography_model"], case["q_defined"], case["t_defined"])))
    assert len(groups) >= 5
    for (key, _, _), members in groups.items():
        prm = dict(key)
        pairs = [p for _, p in members]
        got = run_dev(ctx, torch, pairs, 5, 6, **prm)
        for j, (name, p) in enumerate(members):
            wnn, wm = check_pair(got, j, p, 5, 6, **prm)
            want_nn, want_acc = HAND[name][1], HAND[name][2]
            assert [tuple(r) for r in wnn.tolist()] == [tuple(float(v) if i else v for i, v in enumerate(r)) for r in want_nn] and list(wm["query"]) == want_acc


# ---- seams

KIND_MODELS = ((E_OK, H_OK), (E_NO, H_OK), (E_NO, H_NO))  # pair j of a call has kind j mod 3: F (H is there too and loses), H, NONE


def fixture_pair(rng, nq, nt, kind, hostile_points=False, span=12):
    """Crafted descriptors (a quarter of the query rows exact copies of train rows, a quarter near copies) with points on both exact
    fixtures at once: x and y in 0 .. span - 0.5, a quarter of the rows octave-0 points on half pixels - so rows exactly 2 pixels
    and (1.5, 1) pixels from a predicted position, and exactly 2 and 1.5 pixels from a query's line, occur all over -, a few rows
    undefined.  A window holds about 8 % of the train rows, a band about 30 %."""
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq, t)

    def pts(n):
        octave = np.where(rng.random(n) < 0.25, 0, rng.integers(1, 3, n))
        pitch = 2.0 ** (octave - 1)
        p = lattice_points(np.floor(rng.uniform(0, span, n) / pitch) * pitch, octave, np.floor(rng.uniform(0, span, n) / pitch) * pitch,
                           padding=int(rng.integers(0, 2)))
        if hostile_points and n >= 8:
            p["octave"][1], p["octave"][5] = 32, -1
            p["col"][2], p["row"][3], p["col"][6], p["padding"][6] = 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1
        return p

    qdf, tdf = (rng.random(nq) > 0.05).astype(np.uint8), (rng.random(nt) > 0.05).astype(np.uint8)
    return pair(q, t, pts(nq), pts(nt), *KIND_MODELS[kind], qdf, tdf)


SEAM_NQ, SEAM_NT = (1, 127, 128, 129, 257), (1, 31, 32, 33, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def seam_pairs():
    rng = np.random.default_rng(4177)
    return [fixture_pair(rng, nq, nt, j % 3) for j, (nq, nt) in enumerate((a, b) for a in SEAM_NQ for b in SEAM_NT)]


def test_seams_forty_unequal_pairs_of_three_kinds_in_one_call_and_the_call_repeated(env, seam_pairs):
    """Every (nq, nt) of the tile seams - 128 query rows per workgroup, 64 train rows per tile, 32 per MFMA block - as one pair of
    a 40-pair call in which the kinds F, H and NONE alternate, capacities above every count; the same call again gives the same
    bytes.  Then the call with an absolute bound that lies among the distances of the near copies, so that it cuts the lists."""
    ctx, torch = env
    got = run_dev(ctx, torch, seam_pairs, 260, 131, match_cap=300)
    accepted, with_nn = [0, 0, 0], [0, 0, 0]
    for j, p in enumerate(seam_pairs):
        wnn, wm = check_pair(got, j, p, 260, 131, match_cap=300)
        accepted[j % 3] += len(wm)
        with_nn[j % 3] += int((wnn["index"] >= 0).sum())
    assert accepted[0] > 150 and accepted[1] > 150 and with_nn[0] > 600 and with_nn[1] > 300 and accepted[2] == with_nn[2] == 0, (accepted, with_nn)
    again = run_dev(ctx, torch, seam_pairs, 260, 131, match_cap=300)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    bounded = run_dev(ctx, torch, seam_pairs, 260, 131, match_cap=300, max_desc_dist2=0.05)
    kept = sum(len(check_pair(bounded, j, p, 260, 131, match_cap=300, max_desc_dist2=0.05)[1]) for j, p in enumerate(seam_pairs))
    assert 50 < kept < sum(accepted) - 50 and bounded[0].tobytes() == got[0].tobytes()  # the bound changes the lists, never nn


@pytest.mark.parametrize("same_octave", [False, True])
def test_seams_one_pair_per_call_counts_above_the_capacities_and_a_cut_list(env, seam_pairs, same_octave):
    ctx, torch = env
    sizes = []
    for k in (0, 10, 15, 19, 31, 39, 37):  # kinds F H F H H F H: (1, 1), (127, 32), (127, 129), (128, 33), (129, 129), (257, 129), (257, 64)
        p = dict(seam_pairs[k], q_count=100000, t_count=2 ** 31 - 1)
        if k % 3 == 1 and k != 31:
            p["emodel"] = None  # H applies to every pair of a call without epipolar models
        nq, nt = len(p["q"]), len(p["t"])
        qcap, tcap = max(nq - 1, 1), max(nt - 2, 1)  # min(count, cap) rows are used: the last rows are not
        got = run_dev(ctx, torch, [p], qcap, tcap, match_cap=7, same_octave=same_octave)
        sizes.append(len(check_pair(got, 0, p, qcap, tcap, match_cap=7, same_octave=same_octave)[1]))
    assert sizes[-1] > 7 and sizes[-2] > 7, sizes  # the largest of either kind: the total is reported, the list is cut
    p = dict(seam_pairs[37], hmodel=H_NEG)  # p2 < 0 for every query row: the position is the same, the window is empty
    got = run_dev(ctx, torch, [p], 257, 64, same_octave=same_octave)
    wnn, wm = check_pair(got, 0, p, 257, 64, same_octave=same_octave)
    assert len(wm) == 0 and (wnn["index"] == -1).all()


def test_train_tiles_dealt_to_sixteen_splits_unevenly_under_h(env):
    """nt = 64 * 17 + 5: 18 train tiles over 16 workgroups per query tile, tiles 16 and 17 (the short one) going to splits 0 and 1.
    Query 0: the window's nearest in tile 0 (split 0), its second nearest in tile 1 (split 1), the global nearest - an exact copy, out
    of window - in tile 2 (split 2).  Query 1: a tie across tiles 3 and 5, an out-of-window copy before them.  Query 2: the nearest is
    the very last row, in the short tile."""
    ctx, torch = env
    rng = np.random.default_rng(1193)
    nt, nq = 64 * 17 + 5, 5
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq)
    qxy = np.array([(10, 10), (40, 10), (70, 10), (10, 10), (200, 200)], np.float64)
    txy = np.full((nt, 2), 400.0)
    txy[:, 0] += np.arange(nt) % 50
    near = lambda row, s: np.abs(row + rng.normal(0, s, 128)).astype(np.float32)
    t[2 * 64 + 9] = q[0]
    t[10], t[64 + 6] = near(q[0], 0.02), near(q[0], 0.06)
    txy[10], txy[64 + 6] = (13, 8), (14, 8)
    t[[7, 3 * 64 + 1, 5 * 64 + 63]] = near(q[1], 0.03)
    txy[3 * 64 + 1], txy[5 * 64 + 63] = (43, 8), (43, 9)
    t[nt - 1], t[16 * 64] = near(q[2], 0.02), near(q[2], 0.2)
    txy[nt - 1], txy[16 * 64] = (73, 8), (72, 8)
    fill = rng.choice(np.arange(6 * 64, 16 * 64), 60, replace=False)
    txy[fill] = np.array([(13, 8), (12, 9), (43, 8), (44.5, 9), (73, 8), (75, 8)])[rng.integers(0, 6, 60)]
    octave = np.where((txy % 1 == 0).all(axis=1), 1, 0)
    p = pair(q, t, xy_points(qxy), xy_points(txy, octave), None, H_OK)
    got = run_dev(ctx, torch, [p], nq, nt)
    wnn, wm = check_pair(got, 0, p, nq, nt)
    assert wnn["index"][0] == 10 and wnn["second_dist2"][0] == matchref.d2(q[0], t[64 + 6]) and matchref.match(q, t)[0]["index"][0] == 2 * 64 + 9
    assert wnn["index"][1] == 3 * 64 + 1 and wnn["dist2"][1] == wnn["second_dist2"][1] and 1 not in wm["query"]
    assert wnn["index"][2] == nt - 1 and wnn["index"][4] == -1


# ---- window content

def windowed_pair(seed=300, nq=300, nt=300, sites=16):
    """Train row j sits at site j % sites of a row of sites 8 pixels apart - the rows of one site exactly 2 pixels off it (out of every
    window), those of another (1.5, 1) off (octave-0 points, in) -, and each query row is put, by its index mod 5, where H predicts a
    site that does not hold its unguided nearest (0, 1), the site of its unguided nearest (2, 3), a site without any train row (4,
    every other one) or a site with a single train row (4, the rest)."""
    rng = np.random.default_rng(seed)
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq, t)
    site = np.arange(nt) % sites
    txy = np.stack([8.0 * site + 20, np.full(nt, 40.0)], axis=1)
    txy[5::16] += (2.0, 0.0)
    txy[9::16] += (1.5, 1.0)
    txy[nt - 1] = (8.0 * (sites + 1) + 20, 40.0)  # the single row of its site
    order = np.argsort(matchref.d2_all(q, t), axis=1, kind="stable")
    px = np.zeros(nq)
    for i in range(nq):
        k = i % 5
        px[i] = 8.0 * ((site[order[i, 0]] + 1) % sites) if k < 2 else 8.0 * site[order[i, 0]] if k < 4 else 8.0 * (sites + 1 + (i // 5) % 2)
    qxy = np.stack([px + 20 - EXACT_H[2], np.full(nq, 40.0 - EXACT_H[5])], axis=1)
    return pair(q, t, xy_points(qxy), xy_points(txy, np.where((txy % 1 == 0).all(axis=1), 1, 0)), E_NO, H_OK)


def test_window_content_winners_seconds_lone_candidates_and_empty_windows(env):
    ctx, torch = env
    p = windowed_pair()
    unn, um = matchref.match(p["q"], p["t"])
    win = guidedhfref.window(p["hmodel"], p["q_points"], p["t_points"], WINDOW2)
    nq = len(p["q"])
    order = np.argsort(matchref.d2_all(p["q"], p["t"]), axis=1, kind="stable")
    first_out = ~win[np.arange(nq), order[:, 0]]
    assert first_out.sum() > nq / 3, first_out.sum()  # the unguided nearest is out of window for over a third of the queries
    assert (win.sum(axis=1) == 1).sum() >= 20 and (win.sum(axis=1) == 0).sum() >= 20
    qxy, txy = guidedref.rows_xy(p["q_points"]), guidedref.rows_xy(p["t_points"])
    d2 = (qxy[:, None, 0] + EXACT_H[2] - txy[None, :, 0]) ** 2 + (qxy[:, None, 1] + EXACT_H[5] - txy[None, :, 1]) ** 2
    assert (d2 == 4.0).sum() > 100 and not win[d2 == 4.0].any() and (d2 == 3.25).sum() > 100 and win[d2 == 3.25].all()
    for prm in (dict(), dict(max_desc_dist2=1.0), dict(ratio2=0.36, max_desc_dist2=0.5)):
        got = run_dev(ctx, torch, [p], 300, 300, **prm)
        wnn, wm = check_pair(got, 0, p, 300, 300, **prm)
        # an ignored mask changes the answer: the restatement differs from the matcher's in winners and in the accepted list
        assert (wnn["index"] != unn["index"]).sum() >= nq / 3 and set(wm["query"]) != set(um["query"])
    behind = dict(p, hmodel=H_NEG)
    wnn, wm = check_pair(run_dev(ctx, torch, [behind], 300, 300), 0, behind, 300, 300)
    assert len(wm) == 0 and (wnn["index"] == -1).all()


# ---- hostile values

@pytest.mark.parametrize("block", ["overflow", "partial_specials", "subnormals"])
def test_hostile_descriptor_rows(env, block):
    from tests import test_gpu_match_limits as ML

    ctx, torch = env
    rng = np.random.default_rng(515)
    q, t = getattr(ML, "block_" + block)(rng, 140, 150)
    q[3], t[4] = -0.0, np.nan
    for kind in (0, 1):
        p = dict(fixture_pair(rng, 140, 150, kind), q=q, t=t)
        got = run_dev(ctx, torch, [p], 140, 150)
        check_pair(got, 0, p, 140, 150)
        got = run_dev(ctx, torch, [p], 140, 150, with_defined=False)  # `defined` NULL
        check_pair(got, 0, dict(p, q_defined=None, t_defined=None), 140, 150)
    if block == "overflow":
        assert np.isneginf(matchref.d2_all(q, t)).any()


def test_hostile_homographies_and_points(env):
    ctx, torch = env
    rng = np.random.default_rng(616)
    s, c = scene_chain(2, "plane")
    good = c["hmodel"]

    def model(edit):
        m = good.copy()
        edit(m["H"][0])
        return m

    def set_to(i, v):
        return lambda Hm: Hm.__setitem__(i, v)

    models = [good, model(set_to(4, np.nan)), model(set_to(2, np.inf)), model(set_to(7, -np.inf)), model(lambda Hm: Hm.__imul__(2.0 ** 300)),
              model(lambda Hm: Hm.__imul__(2.0 ** -300)), model(lambda Hm: Hm.__imul__(0.0)), model(set_to(0, 2.0 ** 300)), model(set_to(8, 2.0 ** -300)),
              model(lambda Hm: Hm.__imul__(-1.0)), model(set_to(8, 2.0 ** 300)), model(set_to(6, np.nan))]
    pairs = [pair(s["q"], s["t"], s["qp"], s["tp"], c["gated"], m) for m in models]
    hp = fixture_pair(rng, 150, 140, 1, hostile_points=True)     # octave 32 / -1 and int32-extreme row / col / padding on both sides
    horizon = guidedhfref.homography_record(with_entry(with_entry(HORIZON_H, 7, -1.0), 8, 6.0))  # p2 = 6 - y: through the fixture's 12 rows
    pairs += [hp, dict(hp, hmodel=good), dict(hp, hmodel=models[4]), dict(hp, hmodel=horizon)]
    got = run_dev(ctx, torch, pairs, 600, 600, max_transfer2=4.0)
    found = [int((check_pair(got, j, p, 600, 600, max_transfer2=4.0)[0]["index"] >= 0).sum()) for j, p in enumerate(pairs)]
    # a power of two scales both sides of the test; a negated, zero or NaN H has no row in window
    assert found[0] > 300 and found[4] == found[0] == found[5] and found[1] == found[6] == found[9] == found[11] == 0, found
    nn = got[0][12].view(capi.NN2_DTYPE).reshape(-1)
    assert (nn["index"][[1, 5]] == -1).all() and not np.isin(nn["index"][:150], [1, 5]).any()
    qy = guidedref.rows_xy(hp["q_points"])[:, 1]
    below = got[0][15].view(capi.NN2_DTYPE).reshape(-1)["index"][:150][qy >= 6.0]
    assert found[15] > 0 and len(below) > 30 and (below == -1).all()  # on and below the horizon: nothing


# ---- calls

def test_no_pairs_each_optional_output_alone_and_the_rejections(env):
    ctx, torch = env
    rng = np.random.default_rng(66)
    p = fixture_pair(rng, 150, 140, 1)
    want = run_dev(ctx, torch, [p], 160, 150, match_cap=5)
    _, wm = check_pair(want, 0, p, 160, 150, match_cap=5)
    assert len(wm) > 5
    names = ("nn", "matches", "match_counts")
    for only in (("nn",), ("match_counts",), ("matches", "match_counts"), ("nn", "match_counts")):
        got = run_dev(ctx, torch, [p], 160, 150, match_cap=5, only=only)
        for k, g, w in zip(names, got, want):
            assert g.tobytes() == w.tobytes() if k in only else (g == SENT).all(), (only, k)
    got = run_dev(ctx, torch, [p], 160, 150, n_pairs=0)
    assert all((g == SENT).all() for g in got)
    Q, kq = side_to_device(torch, [p], "q", 160, True)
    T, kt = side_to_device(torch, [p], "t", 150, True)
    em, hm = models_to_device(torch, [p], "emodel", 22), models_to_device(torch, [p], "hmodel", 42)
    nn = torch.zeros((1, 160, 3), dtype=torch.int32, device=DEV)
    with pytest.raises(capi.VslamError):
        ctx.match_guided_hf(Q, T, em, hm, 1, nn=torch.zeros((1, 159, 3), dtype=torch.int32, device=DEV))  # undersized
    with pytest.raises(capi.VslamError):
        ctx.match_guided_hf(Q, T, em, hm, 1, matches=torch.zeros((1, 5, 3), dtype=torch.int32, device=DEV))  # matches without match_counts
    with pytest.raises(capi.VslamError):
        ctx.match_guided_hf(Q, capi.desc_sets(kt[0], kt[1], kt[2]), em, hm, 1, nn=nn)  # no points
    with pytest.raises(capi.VslamError):
        ctx.match_guided_hf(Q, T, em, hm, 1, max_transfer2=0.0, nn=nn)
    with pytest.raises(capi.VslamError):
        ctx.match_guided_hf(Q, T, em, None, 1, max_dist2=float("nan"), nn=nn)
    with pytest.raises(ValueError):
        ctx.match_guided_hf(Q, T, None, None, 1, nn=nn)
    with pytest.raises(ValueError):
        ctx.match_guided_hf(Q, T, em, hm[:, :41].contiguous(), 1, nn=nn)  # fewer than 168 bytes per pair
    ctx.match_guided_hf(Q, T, em, None, 1, max_transfer2=float("nan"), nn=nn)  # not looked at without homography models
    # the result depends neither on the f32-fused switch nor on the matrix-path switch
    ctx.set_f32_fused(True)
    ctx.set_matrix_path(True)
    got = run_dev(ctx, torch, [p], 160, 150, match_cap=5)
    ctx.set_f32_fused(False)
    ctx.set_matrix_path(False)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("same_octave", [False, True])
def test_identities_on_the_device_against_the_guided_call_and_the_matcher(env, same_octave):
    """(a) without homography models the call gives vslam_match_guided_dev's own bytes; (b) under the exact H with everything in
    window it gives vslam_match_dev's."""
    ctx, torch = env
    q, t, qp, tp, model = identity_sets()
    Q, kq = side_to_device(torch, [dict(q=q, q_defined=None, q_points=qp, q_count=None)], "q", 1003, True)
    T, kt = side_to_device(torch, [dict(t=t, t_defined=None, t_points=tp, t_count=None)], "t", 780, True)
    fresh = lambda: dict(nn=torch.full((1, 1003, 3), SENT, dtype=torch.int32, device=DEV), matches=torch.full((1, 1003, 3), SENT, dtype=torch.int32, device=DEV),
                         match_counts=torch.full((1,), SENT, dtype=torch.int32, device=DEV))
    same = lambda a, b: all(a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes() for k in a)
    models = torch.from_numpy(model.view(np.int32).reshape(1, 22)).to(DEV)
    for md in (4.0, 1e300):
        a, b = fresh(), fresh()
        ctx.match_guided(Q, T, models, 1, 0.64, np.inf, md, same_octave, **a)
        ctx.match_guided_hf(Q, T, models, None, 1, 0.64, np.inf, md, float("nan"), same_octave, **b)
        torch.cuda.synchronize()
        assert same(a, b) and int(a["match_counts"][0]) > 0
    a, b = fresh(), fresh()
    ctx.match(Q, T, 1, 0.64, same_octave, **a)
    ctx.match_guided_hf(Q, T, None, torch.from_numpy(H_OK.view(np.int32).reshape(1, 42)).to(DEV), 1, 0.64, np.inf, 4.0, 1e300, same_octave, **b)
    torch.cuda.synchronize()
    assert same(a, b) and int(a["match_counts"][0]) > 100
    p = pair(q, t, qp, tp, None, H_OK)
    check_pair(tuple(b[k].cpu().numpy() for k in ("nn", "matches", "match_counts")), 0, p, 1003, 780, max_transfer2=1e300, same_octave=same_octave)


# ---- higher layers

def test_host_entry_point(env):
    ctx, torch = env
    p = windowed_pair(7, 150, 140)
    for models, prm in (((E_NO, H_OK), dict()), ((None, H_OK), dict(max_desc_dist2=1.0, same_octave=True)), ((E_OK, H_OK), dict()), ((E_OK, None), dict()),
                        ((E_NO, H_NO), dict()), ((None, H_NEG), dict())):
        pm = dict(p, emodel=models[0], hmodel=models[1])
        wnn, wm = restated(pm, 150, 140, **prm)
        nn, m, total = ctx.match_guided_hf_host(p["q"], p["t"], p["q_points"], p["t_points"], models[0], models[1], **dict(PRM, **prm))
        assert nn.tobytes() == wnn.tobytes() and m.tobytes() == wm.tobytes() and total == len(wm) and (total > 5 or models[0] is E_OK or models[1] is not H_OK)
        nn, m, total = ctx.match_guided_hf_host(p["q"], p["t"], p["q_points"], p["t_points"], models[0], models[1], match_cap=5, **dict(PRM, **prm))
        assert m.tobytes() == wm[:5].tobytes() and total == len(wm)
    nn, m, total = ctx.match_guided_hf_host(np.zeros((0, 128), np.float32), p["t"], p["q_points"][:0], p["t_points"], None, H_OK)
    assert len(nn) == 0 and total == 0
    nn, m, total = ctx.match_guided_hf_host(p["q"], np.zeros((0, 128), np.float32), p["q_points"], p["t_points"][:0], None, H_OK)
    assert (nn["index"] == -1).all() and np.isinf(nn["dist2"]).all() and total == 0


def test_cxx_wrapper_equals_the_restatement(env, tmp_path):
    p = windowed_pair(8, 150, 140)
    src, dst = tmp_path / "pair.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([150, 140], np.uint64).tobytes() + E_OK.tobytes() + H_OK.tobytes() + p["q"].tobytes() + p["t"].tobytes() + p["q_points"].tobytes() +
                p["t_points"].tobytes())
    exe = build_cxx_driver(tmp_path)
    for which, bound in (("h", "inf"), ("h", "1.0"), ("fh", "inf"), ("f", "inf")):
        r = subprocess.run([exe, str(src), which, "0.64", bound, repr(BAND2), repr(WINDOW2), "0", str(dst)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        raw = dst.read_bytes()
        pm = dict(p, emodel=E_OK if "f" in which else None, hmodel=H_OK if "h" in which else None)
        wnn, wm = restated(pm, 150, 140, max_desc_dist2=float(bound))
        k = int(np.frombuffer(raw[:8], np.uint64)[0])
        assert k == 150 and raw[8:8 + 12 * k] == wnn.tobytes()
        rest = raw[8 + 12 * k:]
        assert int(np.frombuffer(rest[:8], np.uint64)[0]) == len(wm) > (5 if which == "h" else 0) and rest[8:] == wm.tobytes()


def device_chain(ctx, torch, d, c, df, pts, cap, bound=np.inf, ratio2=0.64, max_transfer2=4.0):
    """match -> epipolar -> homography with the gate -> guided under (gated F, H) -> homography on that list, over two device sets,
    nothing downloaded in between -> dict of every list and model as numpy."""
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:1], c[:1], df[:1], pts[:1]), capi.desc_sets(d[1:], c[1:], df[1:], pts[1:])
    m0, c0, emod, hmod, gated = z(1, cap, 3), z(1), z(1, 22), z(1, 42), z(1, 22)
    ctx.match(Q, T, 1, 0.64, False, matches=m0, match_counts=c0)
    ctx.epipolar(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, models=emod)
    ctx.homography(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, epipolar_models=emod, models=hmod, gated_models=gated)
    nn1, m1, c1, hmod1 = z(1, cap, 3), z(1, cap, 3), z(1), z(1, 42)
    ctx.match_guided_hf(Q, T, gated, hmod, 1, ratio2, bound, 4.0, max_transfer2, False, nn=nn1, matches=m1, match_counts=c1)
    ctx.homography(m1, c1, pts[:1], pts[1:], 1, 512, 1, 4.0, models=hmod1)
    torch.cuda.synchronize()
    rec = lambda t, n, dt: t.cpu().numpy()[0, :n].copy().view(dt).reshape(-1)
    whole = lambda t, dt: t.cpu().numpy().view(dt).reshape(-1)
    return dict(m0=rec(m0, int(c0[0]), capi.MATCH_DTYPE), emodel=whole(emod, capi.EPIPOLAR_DTYPE), hmodel=whole(hmod, capi.HOMOGRAPHY_DTYPE),
                gated=whole(gated, capi.EPIPOLAR_DTYPE), m1=rec(m1, int(c1[0]), capi.MATCH_DTYPE), nn1=rec(nn1, cap, capi.NN2_DTYPE),
                hmodel1=whole(hmod1, capi.HOMOGRAPHY_DTYPE))


def test_match_executable_reports_the_guided_h_counts_of_the_python_path(env, tmp_path):
    from tests.test_gpu_match import building_crops, detect

    ctx, torch = env
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(building_crops()):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    p, o = detect(ctx, torch, np.stack(building_crops()))
    args = (o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"], p.oriented_cap)
    plain = json.loads(subprocess.run([exe, "--epipolar", "--homography", paths[0], paths[1], "3"], capture_output=True, text=True,
                                      timeout=300).stdout.strip().splitlines()[-1])
    new = ("guided_hf_kind", "guided_hf_matches", "guided_hf_h_inliers")
    assert not any(k in plain for k in new)
    squared = float(np.float32(0.8) * np.float32(0.8))  # the executable squares the ratio it is given in f32
    for opt, bound, ratio2, t2 in ((["--guided-h"], np.inf, 0.64, 4.0), (["--guided-h", "9.0,0.8,0.25"], 0.25, squared, 9.0)):
        r = subprocess.run([exe, "--epipolar", "--homography", *opt, paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        rep = json.loads(r.stdout.strip().splitlines()[-1])
        c = device_chain(ctx, torch, *args, bound=bound, ratio2=ratio2, max_transfer2=t2)
        assert rep["accepted"] == len(c["m0"]) and rep["homography"]["n_inliers"] == int(c["hmodel"]["n_inliers"][0])
        assert rep["homography"]["degenerate"] == 1 and rep["guided_hf_kind"] == "H" and int(c["gated"]["best"][0]) < 0
        assert (rep["guided_hf_matches"], rep["guided_hf_h_inliers"]) == (len(c["m1"]), int(c["hmodel1"]["n_inliers"][0])), (rep, len(c["m1"]))
        assert {k: v for k, v in rep.items() if k not in new + ("ms",)} == {k: v for k, v in plain.items() if k != "ms"}
        assert len(c["m1"]) > 300


# ---- end to end on the device

@pytest.mark.parametrize("kind,seed", [("plane", 5), ("rotation", 6)])
def test_end_to_end_degenerate_scene_equals_the_chain_of_restatements(env, kind, seed):
    ctx, torch = env
    s, w = scene_chain(seed, kind)
    n = len(s["q"])
    d = torch.from_numpy(np.stack([s["q"], s["t"]])).to(DEV)
    c = torch.full((2,), n, dtype=torch.int32, device=DEV)
    df = torch.ones((2, n), dtype=torch.uint8, device=DEV)
    pts = torch.from_numpy(np.stack([s["qp"], s["tp"]]).view(np.int32).reshape(2, n, 6)).to(DEV)
    lists = {}
    for bound, key in ((np.inf, "m1"), (1.0, "m2")):
        g = device_chain(ctx, torch, d, c, df, pts, n, bound=bound)
        for k in ("m0", "emodel", "hmodel", "gated"):
            assert g[k].tobytes() == w[k].tobytes(), k
        assert g["m1"].tobytes() == w[key].tobytes() and g["nn1"].tobytes() == w["nn1"].tobytes()
        assert g["hmodel1"].tobytes() == homref.ransac(w[key], s["qp"], s["tp"], 512, 1, 4.0)[0].tobytes()
        lists[key] = g["m1"]
    f = figures_of(s, g["m0"], lists["m1"], lists["m2"])
    print("device,", kind, seed, f, "H inliers of the guided list", int(g["hmodel1"]["n_inliers"][0]))
    assert int(g["gated"]["best"][0]) == -1 and int(g["hmodel"]["degenerate"][0]) == 1
    check_scene_conditions(f)

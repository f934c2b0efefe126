"""Guided matching on the GPU (vslam_match_guided_dev / vslam_match_guided_host, include/vslam.h): every comparison is
bytes-equal against the CPU restatement in tests/guidedref.py - every nn row, every match record, every count, and the sentinels
past every count.  Most sets carry their points on the exact-F fixture of tests/test_guided_cpu.py, where a row is in band iff
its y is within 2 pixels of the query's: band membership is then decided by construction."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import epiref, guidedref, matchref
from tests.test_guided_cpu import BAND2, EXACT_F, HAND, build_cxx_driver, check_scene_conditions, identity_sets, lattice_points
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def pair(q, t, q_points, t_points, model, q_defined=None, t_defined=None, q_count=None, t_count=None):
    """One pair of a call.  *_count: the count the device is given (default: the number of rows; above the capacity it is clamped)."""
    return dict(q=np.asarray(q, np.float32).reshape(-1, 128), t=np.asarray(t, np.float32).reshape(-1, 128), q_points=q_points, t_points=t_points, model=model,
                q_defined=q_defined, t_defined=t_defined, q_count=q_count, t_count=t_count)


def side_to_device(torch, pairs, side, cap, with_defined):
    n = len(pairs)
    desc = np.full((n, cap, 128), 3.5, np.float32)
    defined = np.ones((n, cap), np.uint8)
    points = np.zeros((n, cap), capi.POINT_DTYPE)
    points["octave"] = 1
    counts = np.zeros(n, np.int32)
    for j, p in enumerate(pairs):
        d, df, pt, cnt = p[side], p[side + "_defined"], p[side + "_points"], p[side + "_count"]
        m = min(len(d), cap)
        desc[j, :m], points[j, :m] = d[:m], pt[:m]
        if df is not None:
            defined[j, :m] = np.asarray(df, np.uint8)[:m]
        counts[j] = len(d) if cnt is None else cnt
    t = [torch.from_numpy(a).to(DEV) for a in (desc, counts, defined, points.view(np.int32).reshape(n, cap, 6))]
    return capi.desc_sets(t[0], t[1], t[2] if with_defined else None, t[3]), t


def run_dev(ctx, torch, pairs, qcap, tcap, match_cap=None, with_defined=True, only=("nn", "matches", "match_counts"), n_pairs=None, **prm):
    """One vslam_match_guided_dev call over `pairs` -> (nn, matches, counts) as numpy, sentinel-filled where nothing was written."""
    n = len(pairs)
    Q, kq = side_to_device(torch, pairs, "q", qcap, with_defined)
    T, kt = side_to_device(torch, pairs, "t", tcap, with_defined)
    models = torch.from_numpy(np.concatenate([p["model"] for p in pairs]).view(np.int32).reshape(n, 22)).to(DEV)
    match_cap = qcap if match_cap is None else match_cap
    outs = dict(nn=torch.full((n, qcap, 3), SENT, dtype=torch.int32, device=DEV), matches=torch.full((n, match_cap, 3), SENT, dtype=torch.int32, device=DEV),
                match_counts=torch.full((n,), SENT, dtype=torch.int32, device=DEV))
    prm.setdefault("max_dist2", BAND2)
    ctx.match_guided(Q, T, models, n if n_pairs is None else n_pairs, prm.get("ratio2", 0.64), prm.get("max_desc_dist2", np.inf), prm["max_dist2"],
                     prm.get("same_octave", False), **{k: v for k, v in outs.items() if k in only})
    torch.cuda.synchronize()
    return tuple(outs[k].cpu().numpy() for k in ("nn", "matches", "match_counts"))


def restated(p, qcap, tcap, **prm):
    prm.setdefault("max_dist2", BAND2)
    nq = min(len(p["q"]) if p["q_count"] is None else p["q_count"], qcap, len(p["q"]))
    nt = min(len(p["t"]) if p["t_count"] is None else p["t_count"], tcap, len(p["t"]))
    cut = lambda a, k: None if a is None else np.asarray(a)[:k]
    return guidedref.guided(p["q"][:nq], p["t"][:nt], p["q_points"][:nq], p["t_points"][:nt], p["model"], q_defined=cut(p["q_defined"], nq),
                            t_defined=cut(p["t_defined"], nt), **prm)


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
        prm = {k: case[k] for k in ("ratio2", "max_desc_dist2", "max_dist2", "same_octave") if k in case}
        groups.setdefault(tuple(sorted(prm.items())), []).append((name, pair(case["q"], case["t"], case["q_points"], case["t_points"], case["model"],
                                                                             case["q_defined"], case["t_defined"])))
    assert len(groups) >= 4
    for key, members in groups.items():
        prm = dict(key)
        pairs = [p for _, p in members]
        got = run_dev(ctx, torch, pairs, 5, 6, **prm)
        for j, (name, p) in enumerate(members):
            wnn, wm = check_pair(got, j, p, 5, 6, **prm)
            want_nn, want_acc = HAND[name][1], HAND[name][2]
            assert [tuple(r) for r in wnn.tolist()] == [tuple(float(v) if i else v for i, v in enumerate(r)) for r in want_nn] and list(wm["query"]) == want_acc


# ---- seams

def fixture_pair(rng, nq, nt, hostile_points=False):
    """Crafted descriptors (a quarter of the query rows exact copies of train rows, a quarter near copies) with points on the exact-F
    fixture: y in 0 .. 11.5, a quarter of the rows octave-0 points on half pixels - so rows exactly 2 pixels and 1.5 pixels from a
    query occur all over -, a few rows undefined."""
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq, t)

    def pts(n):
        octave = np.where(rng.random(n) < 0.25, 0, rng.integers(1, 3, n))
        pitch = 2.0 ** (octave - 1)
        y = np.floor(rng.uniform(0, 12, n) / pitch) * pitch
        p = lattice_points(y, octave, np.floor(rng.uniform(0, 1900, n) / pitch) * pitch, padding=int(rng.integers(0, 2)))
        if hostile_points and n >= 8:
            p["octave"][1], p["octave"][5] = 32, -1
            p["col"][2], p["row"][3], p["col"][6], p["padding"][6] = 2 ** 31 - 1, -2 ** 31, -2 ** 31, 2 ** 31 - 1
        return p

    qdf, tdf = (rng.random(nq) > 0.05).astype(np.uint8), (rng.random(nt) > 0.05).astype(np.uint8)
    return pair(q, t, pts(nq), pts(nt), guidedref.model_record(EXACT_F), qdf, tdf)


SEAM_NQ, SEAM_NT = (1, 127, 128, 129, 257), (1, 31, 32, 33, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def seam_pairs():
    rng = np.random.default_rng(4077)
    return [fixture_pair(rng, nq, nt) for nq in SEAM_NQ for nt in SEAM_NT]


def test_seams_forty_unequal_pairs_in_one_call_and_the_call_repeated(env, seam_pairs):
    """Every (nq, nt) of the tile seams - 128 query rows per workgroup, 64 train rows per tile, 32 per MFMA block - as one pair of
    a 40-pair call, capacities above every count; the same call again gives the same bytes.  Then the call with an absolute bound
    that lies among the distances of the near copies (sigma 0.02 over 128 entries: d2 about 0.05), so that it cuts the lists."""
    ctx, torch = env
    got = run_dev(ctx, torch, seam_pairs, 260, 131, match_cap=300)
    accepted = with_nn = 0
    for j, p in enumerate(seam_pairs):
        wnn, wm = check_pair(got, j, p, 260, 131, match_cap=300)
        accepted, with_nn = accepted + len(wm), with_nn + int((wnn["index"] >= 0).sum())
    assert accepted > 500 and with_nn > 2000
    again = run_dev(ctx, torch, seam_pairs, 260, 131, match_cap=300)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    bounded = run_dev(ctx, torch, seam_pairs, 260, 131, match_cap=300, max_desc_dist2=0.05)
    kept = sum(len(check_pair(bounded, j, p, 260, 131, match_cap=300, max_desc_dist2=0.05)[1]) for j, p in enumerate(seam_pairs))
    assert 100 < kept < accepted - 100 and bounded[0].tobytes() == got[0].tobytes()  # the bound changes the lists, never nn


@pytest.mark.parametrize("same_octave", [False, True])
def test_seams_one_pair_per_call_counts_above_the_capacities_and_a_cut_list(env, seam_pairs, same_octave):
    ctx, torch = env
    for k in (0, 9, 15, 20, 31, 39):  # (1, 1), (127, 31), (127, 129), (128, 63), (129, 129), (257, 129)
        p = dict(seam_pairs[k], q_count=100000, t_count=2 ** 31 - 1)
        nq, nt = len(p["q"]), len(p["t"])
        qcap, tcap = max(nq - 1, 1), max(nt - 2, 1)  # min(count, cap) rows are used: the last rows are not
        got = run_dev(ctx, torch, [p], qcap, tcap, match_cap=7, same_octave=same_octave)
        _, wm = check_pair(got, 0, p, qcap, tcap, match_cap=7, same_octave=same_octave)
        assert k < 39 or len(wm) > 7  # the largest: the total is reported, the list is cut


def test_train_tiles_dealt_to_sixteen_splits_unevenly(env):
    """nt = 64 * 17 + 5: 18 train tiles over 16 workgroups per query tile, tiles 16 and 17 (the short one) going to splits 0 and 1.
    Query 0: the band's nearest in tile 0 (split 0), its second nearest in tile 1 (split 1), the global nearest - an exact copy, out
    of band - in tile 2 (split 2).  Query 1: a tie across tiles 3 and 5, out-of-band copies before them.  Query 2: the nearest is
    the very last row, in the short tile."""
    ctx, torch = env
    rng = np.random.default_rng(1093)
    nt, nq = 64 * 17 + 5, 5
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq)
    ty = np.full(nt, 100.0)
    near = lambda row, s: np.abs(row + rng.normal(0, s, 128)).astype(np.float32)
    t[2 * 64 + 9] = q[0]
    t[10], t[64 + 6] = near(q[0], 0.02), near(q[0], 0.06)
    ty[[10, 64 + 6]] = 10.0
    t[[7, 3 * 64 + 1, 5 * 64 + 63]] = near(q[1], 0.03)
    ty[[3 * 64 + 1, 5 * 64 + 63]] = 21.0
    t[nt - 1], t[16 * 64] = near(q[2], 0.02), near(q[2], 0.2)
    ty[[nt - 1, 16 * 64]] = 29.0
    ty[rng.choice(np.arange(6 * 64, 16 * 64), 60, replace=False)] = rng.choice([10.0, 12.0, 21.0, 19.5, 29.0, 30.5], 60)
    octave = np.where(ty % 1 == 0, 1, 0)
    p = pair(q, t, lattice_points([10.0, 21.0, 29.0, 10.0, 55.0]), lattice_points(ty, octave), guidedref.model_record(EXACT_F))
    got = run_dev(ctx, torch, [p], nq, nt)
    wnn, wm = check_pair(got, 0, p, nq, nt)
    assert wnn["index"][0] == 10 and wnn["second_dist2"][0] == matchref.d2(q[0], t[64 + 6]) and matchref.match(q, t)[0]["index"][0] == 2 * 64 + 9
    assert wnn["index"][1] == 3 * 64 + 1 and wnn["dist2"][1] == wnn["second_dist2"][1] and 1 not in wm["query"]
    assert wnn["index"][2] == nt - 1 and wnn["index"][4] == -1


# ---- band content

def banded_pair(seed=300, nq=300, nt=300, groups=16):
    """Train row j lies on line y = 4 * (j % groups) - the rows of one line 2 pixels off it (out of every band), those of another
    1.5 pixels off (octave-0 points, in) -, and each query row is put, by its index mod 5, on a line that does not hold its
    unguided nearest (0, 1), on the pixel row of its unguided nearest (2, 3: the unguided second nearest is then elsewhere unless it
    shares the line), on a line without any train row (4, every other one) or on a line with a single train row (4, the rest)."""
    rng = np.random.default_rng(seed)
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq, t)
    line = np.arange(nt) % groups
    ty = 4.0 * line
    ty[5::16] += 2.0
    ty[9::16] += 1.5
    ty[nt - 1] = 4.0 * (groups + 1)  # the single row of its line
    order = np.argsort(matchref.d2_all(q, t), axis=1, kind="stable")
    qy = np.zeros(nq)
    for i in range(nq):
        k = i % 5
        qy[i] = 4.0 * ((line[order[i, 0]] + 1) % groups) if k < 2 else np.floor(ty[order[i, 0]]) if k < 4 else 4.0 * (groups + 1 + (i // 5) % 2)
    return pair(q, t, lattice_points(qy), lattice_points(ty, np.where(ty % 1 == 0, 1, 0)), guidedref.model_record(EXACT_F))


def test_band_content_winners_seconds_lone_candidates_and_empty_bands(env):
    ctx, torch = env
    p = banded_pair()
    unn, um = matchref.match(p["q"], p["t"])
    band = guidedref.band(p["model"], p["q_points"], p["t_points"], BAND2)
    nq = len(p["q"])
    order = np.argsort(matchref.d2_all(p["q"], p["t"]), axis=1, kind="stable")
    first_out = ~band[np.arange(nq), order[:, 0]]
    second_out = band[np.arange(nq), order[:, 0]] & ~band[np.arange(nq), order[:, 1]]
    assert first_out.sum() >= nq / 3 and second_out.sum() >= nq / 3, (first_out.sum(), second_out.sum())
    assert (band.sum(axis=1) == 1).sum() >= 20 and (band.sum(axis=1) == 0).sum() >= 20
    dy = np.abs(guidedref.rows_xy(p["q_points"])[:, None, 1] - guidedref.rows_xy(p["t_points"])[None, :, 1])
    assert (dy == 2.0).sum() > 100 and not band[dy == 2.0].any() and (dy == 1.5).sum() > 100 and band[dy == 1.5].all()
    for prm in (dict(), dict(max_desc_dist2=1.0), dict(ratio2=0.36, max_desc_dist2=0.5)):
        got = run_dev(ctx, torch, [p], 300, 300, **prm)
        wnn, wm = check_pair(got, 0, p, 300, 300, **prm)
        # an ignored mask changes the answer: the restatement differs from the matcher's in winners and in the accepted list
        assert (wnn["index"] != unn["index"]).sum() >= nq / 3 and set(wm["query"]) != set(um["query"])


# ---- hostile values

@pytest.mark.parametrize("block", ["overflow", "partial_specials", "subnormals"])
def test_hostile_descriptor_rows(env, block):
    from tests import test_gpu_match_limits as ML

    ctx, torch = env
    rng = np.random.default_rng(515)
    q, t = getattr(ML, "block_" + block)(rng, 140, 150)
    q[3], t[4] = -0.0, np.nan
    base = fixture_pair(rng, 140, 150)
    p = dict(base, q=q, t=t)
    got = run_dev(ctx, torch, [p], 140, 150)
    wnn, _ = check_pair(got, 0, p, 140, 150)
    if block == "overflow":
        assert np.isneginf(matchref.d2_all(q, t)).any()
    got = run_dev(ctx, torch, [p], 140, 150, with_defined=False)  # `defined` NULL
    check_pair(got, 0, dict(p, q_defined=None, t_defined=None), 140, 150)


def test_hostile_models_and_points(env):
    ctx, torch = env
    rng = np.random.default_rng(616)
    s = guidedref.repeated_scene(2)
    good = epiref.ransac(matchref.match(s["q"], s["t"])[1], s["qp"], s["tp"], 256, 1, 4.0)[0]

    def model(edit):
        m = good.copy()
        edit(m["F"][0])
        return m

    def set_to(i, v):
        return lambda F: F.__setitem__(i, v)

    models = [good, model(set_to(4, np.nan)), model(set_to(2, np.inf)), model(set_to(7, -np.inf)), model(lambda F: F.__imul__(2.0 ** 300)),
              model(lambda F: F.__imul__(2.0 ** -300)), model(lambda F: F.__imul__(0.0)), model(set_to(0, 2.0 ** 300)), model(set_to(8, 2.0 ** -300))]
    pairs = [pair(s["q"], s["t"], s["qp"], s["tp"], m) for m in models]
    hp = fixture_pair(rng, 150, 140, hostile_points=True)     # octave 32 / -1 and int32-extreme row / col / padding on both sides
    pairs += [hp, dict(hp, model=good), dict(hp, model=models[4])]
    got = run_dev(ctx, torch, pairs, 600, 600, max_dist2=4.0)
    found = [int((check_pair(got, j, p, 600, 600, max_dist2=4.0)[0]["index"] >= 0).sum()) for j, p in enumerate(pairs)]
    assert found[0] > 400 and found[1] == 0 and found[6] == 0 and found[4] == found[0], found  # a power of two scales both sides of the test
    nn = got[0][9].view(capi.NN2_DTYPE).reshape(-1)
    assert (nn["index"][[1, 5]] == -1).all() and not np.isin(nn["index"][:150], [1, 5]).any()


# ---- calls

def test_a_pair_without_a_model_in_the_middle_of_a_call(env):
    ctx, torch = env
    rng = np.random.default_rng(55)
    pairs = [fixture_pair(rng, 130, 70) for _ in range(5)]
    pairs[2]["model"] = guidedref.model_record(EXACT_F, best=-1)
    got = run_dev(ctx, torch, pairs, 130, 70)
    for j, p in enumerate(pairs):
        wnn, wm = check_pair(got, j, p, 130, 70)
        assert (len(wm) == 0 and (wnn["index"] == -1).all()) if j == 2 else len(wm) > 10


def test_no_pairs_and_each_optional_output_alone(env):
    ctx, torch = env
    rng = np.random.default_rng(66)
    p = fixture_pair(rng, 150, 140)
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
    models = torch.from_numpy(p["model"].view(np.int32).reshape(1, 22)).to(DEV)
    nn = torch.zeros((1, 160, 3), dtype=torch.int32, device=DEV)
    with pytest.raises(capi.VslamError):
        ctx.match_guided(Q, T, models, 1, nn=torch.zeros((1, 159, 3), dtype=torch.int32, device=DEV))  # undersized
    with pytest.raises(capi.VslamError):
        ctx.match_guided(Q, T, models, 1, matches=torch.zeros((1, 5, 3), dtype=torch.int32, device=DEV))  # matches without match_counts
    with pytest.raises(capi.VslamError):
        ctx.match_guided(Q, capi.desc_sets(kt[0], kt[1], kt[2]), models, 1, nn=nn)  # no points
    with pytest.raises(capi.VslamError):
        ctx.match_guided(Q, T, models, 1, max_desc_dist2=0.0, nn=nn)
    # the result depends neither on the f32-fused switch nor on the matrix-path switch
    ctx.set_f32_fused(True)
    ctx.set_matrix_path(True)
    got = run_dev(ctx, torch, [p], 160, 150, match_cap=5)
    ctx.set_f32_fused(False)
    ctx.set_matrix_path(False)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("same_octave", [False, True])
def test_identity_a_on_the_device_everything_in_band_is_vslam_match_dev(env, same_octave):
    ctx, torch = env
    q, t, qp, tp, model = identity_sets()
    p = pair(q, t, qp, tp, model)
    got = run_dev(ctx, torch, [p], 1003, 780, max_dist2=1e300, same_octave=same_octave)
    Q, kq = side_to_device(torch, [p], "q", 1003, True)
    T, kt = side_to_device(torch, [p], "t", 780, True)
    nn = torch.full((1, 1003, 3), SENT, dtype=torch.int32, device=DEV)
    matches = torch.full((1, 1003, 3), SENT, dtype=torch.int32, device=DEV)
    counts = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
    ctx.match(Q, T, 1, 0.64, same_octave, nn=nn, matches=matches, match_counts=counts)
    torch.cuda.synchronize()
    for g, w in zip(got, (nn, matches, counts)):
        assert g.tobytes() == w.cpu().numpy().tobytes()
    assert int(counts[0]) > 100
    check_pair(got, 0, p, 1003, 780, max_dist2=1e300, same_octave=same_octave)


# ---- higher layers

def test_host_entry_point(env):
    ctx, torch = env
    p = banded_pair(7, 150, 140)
    for prm in (dict(), dict(max_desc_dist2=1.0, same_octave=True)):
        wnn, wm = restated(p, 150, 140, **prm)
        nn, m, total = ctx.match_guided_host(p["q"], p["t"], p["q_points"], p["t_points"], p["model"], max_dist2=BAND2, **prm)
        assert nn.tobytes() == wnn.tobytes() and m.tobytes() == wm.tobytes() and total == len(wm) > 5
        nn, m, total = ctx.match_guided_host(p["q"], p["t"], p["q_points"], p["t_points"], p["model"], max_dist2=BAND2, match_cap=5, **prm)
        assert m.tobytes() == wm[:5].tobytes() and total == len(wm)
    nn, m, total = ctx.match_guided_host(np.zeros((0, 128), np.float32), p["t"], p["q_points"][:0], p["t_points"], p["model"])
    assert len(nn) == 0 and total == 0
    nn, m, total = ctx.match_guided_host(p["q"], np.zeros((0, 128), np.float32), p["q_points"], p["t_points"][:0], p["model"])
    assert (nn["index"] == -1).all() and np.isinf(nn["dist2"]).all() and total == 0


def test_cxx_wrapper_equals_the_restatement(env, tmp_path):
    p = banded_pair(8, 150, 140)
    src, dst = tmp_path / "pair.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([150, 140], np.uint64).tobytes() + p["model"].tobytes() + p["q"].tobytes() + p["t"].tobytes() + p["q_points"].tobytes() +
                p["t_points"].tobytes())
    exe = build_cxx_driver(tmp_path)
    for bound in ("inf", "1.0"):
        r = subprocess.run([exe, str(src), "0.64", bound, repr(BAND2), "0", str(dst)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        raw = dst.read_bytes()
        wnn, wm = restated(p, 150, 140, max_desc_dist2=float(bound))
        k = int(np.frombuffer(raw[:8], np.uint64)[0])
        assert k == 150 and raw[8:8 + 12 * k] == wnn.tobytes()
        rest = raw[8 + 12 * k:]
        assert int(np.frombuffer(rest[:8], np.uint64)[0]) == len(wm) > 5 and rest[8:] == wm.tobytes()


def device_chain(ctx, torch, d, c, df, pts, cap, bound=np.inf, ratio2=0.64):
    """match -> epipolar -> guided -> epipolar on the guided list over two device sets, nothing downloaded in between ->
    (first list, first model, guided list, guided nn, second model) as numpy."""
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:1], c[:1], df[:1], pts[:1]), capi.desc_sets(d[1:], c[1:], df[1:], pts[1:])
    m0, c0, mod0 = z(1, cap, 3), z(1), z(1, 22)
    ctx.match(Q, T, 1, 0.64, False, matches=m0, match_counts=c0)
    ctx.epipolar(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, models=mod0)
    nn1, m1, c1, mod1 = z(1, cap, 3), z(1, cap, 3), z(1), z(1, 22)
    ctx.match_guided(Q, T, mod0, 1, ratio2, bound, 4.0, False, nn=nn1, matches=m1, match_counts=c1)
    ctx.epipolar(m1, c1, pts[:1], pts[1:], 1, 512, 1, 4.0, models=mod1)
    torch.cuda.synchronize()
    rec = lambda t, n, dt: t.cpu().numpy()[0, :n].copy().view(dt).reshape(-1)
    return (rec(m0, int(c0[0]), capi.MATCH_DTYPE), mod0.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1), rec(m1, int(c1[0]), capi.MATCH_DTYPE),
            nn1.cpu().numpy()[0].copy().view(capi.NN2_DTYPE).reshape(-1), mod1.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1))


def test_match_executable_reports_the_guided_counts_of_the_python_path(env, tmp_path):
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
    plain = json.loads(subprocess.run([exe, "--epipolar", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1])
    assert "guided_matches" not in plain and "guided_inliers" not in plain
    squared = float(np.float32(0.8) * np.float32(0.8))  # the executable squares the ratio it is given in f32
    for opt, bound, ratio2 in ((["--guided"], np.inf, 0.64), (["--guided", "4.0,0.8,0.25"], 0.25, squared)):
        r = subprocess.run([exe, "--epipolar", *opt, paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        rep = json.loads(r.stdout.strip().splitlines()[-1])
        m0, mod0, m1, _, mod1 = device_chain(ctx, torch, *args, bound=bound, ratio2=ratio2)
        assert rep["accepted"] == len(m0) and rep["epipolar"]["n_inliers"] == int(mod0["n_inliers"][0])
        assert (rep["guided_matches"], rep["guided_inliers"]) == (len(m1), int(mod1["n_inliers"][0])), (rep, len(m1))
        assert {k: v for k, v in rep.items() if k not in ("guided_matches", "guided_inliers", "ms")} == {k: v for k, v in plain.items() if k != "ms"}
        assert len(m1) > 300


# ---- end to end on the device

def test_end_to_end_repeated_structure_scene_equals_the_chain_of_restatements(env):
    ctx, torch = env
    s = guidedref.repeated_scene(5)
    n = len(s["q"])
    d = torch.from_numpy(np.stack([s["q"], s["t"]])).to(DEV)
    c = torch.full((2,), n, dtype=torch.int32, device=DEV)
    df = torch.ones((2, n), dtype=torch.uint8, device=DEV)
    pts = torch.from_numpy(np.stack([s["qp"], s["tp"]]).view(np.int32).reshape(2, n, 6)).to(DEV)
    _, w0 = matchref.match(s["q"], s["t"], 0.64)
    wmod0 = epiref.ransac(w0, s["qp"], s["tp"], 512, 1, 4.0)[0]
    figures = dict(planted=int(s["planted"].sum()), unguided_correct=guidedref.correct(w0, s))
    for bound in (np.inf, 1.0):
        m0, mod0, m1, nn1, mod1 = device_chain(ctx, torch, d, c, df, pts, n, bound=bound)
        wnn1, w1 = guidedref.guided(s["q"], s["t"], s["qp"], s["tp"], wmod0, 0.64, bound, 4.0)
        wmod1 = epiref.ransac(w1, s["qp"], s["tp"], 512, 1, 4.0)[0]
        assert m0.tobytes() == w0.tobytes() and mod0.tobytes() == wmod0.tobytes()
        assert nn1.tobytes() == wnn1.tobytes() and m1.tobytes() == w1.tobytes() and mod1.tobytes() == wmod1.tobytes()
        if bound == np.inf:
            figures.update(guided=len(m1), guided_correct=guidedref.correct(m1, s))
        else:
            figures.update(bounded=len(m1), bounded_correct=guidedref.correct(m1, s))
    print("device, scene 5:", figures, "inliers of the second model", int(mod1["n_inliers"][0]))
    check_scene_conditions(figures)

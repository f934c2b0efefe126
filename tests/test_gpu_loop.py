"""Loop verification on the GPU (vslam_loop_pairs_dev, vslam_match_pairs_dev / _host, vslam_pair_points_dev, vslam_loop_verdict_dev /
_host; include/vslam.h): every comparison is bytes-equal against the CPU restatement in tests/loopref.py, and sentinels stay intact
in every row the section leaves untouched."""
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import epiref, loopref, matchref, placeref
from tests.test_gpu_match import detect, sets_to_device
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


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def table_of(rows):
    return np.array(rows, capi.SET_PAIR_DTYPE)


def records(t, dtype, shape):
    return t.cpu().numpy().view(dtype).reshape(shape)


def sent(torch, *shape):
    return torch.full(shape, SENT, dtype=torch.int32, device=DEV)


def run_pairs(ctx, torch, S, keep, table, cap, same_octave=False, match_cap=None, want=("nn", "matches", "match_counts"), T=None, ratio2=0.64):
    """-> (nn [n, cap] NN2_DTYPE, matches [n, match_cap] MATCH_DTYPE, match_counts [n] int32), sentinel-filled before the call."""
    n = len(table)
    mc = cap if match_cap is None else match_cap
    o = dict(nn=sent(torch, n, cap, 3), matches=sent(torch, n, mc, 3), match_counts=sent(torch, n))
    ctx.match_pairs(S, S if T is None else T, dev(torch, table.view(np.int32).reshape(-1, 2)), n, ratio2, same_octave, **{k: v for k, v in o.items() if k in want})
    torch.cuda.synchronize()
    return records(o["nn"], capi.NN2_DTYPE, (n, cap)), records(o["matches"], capi.MATCH_DTYPE, (n, mc)), o["match_counts"].cpu().numpy()


def want_pairs(keep, table, cap, same_octave=False, match_cap=None, with_defined=True, ratio2=0.64):
    """The restatement over the tensors behind a DescSets (sets_to_device's desc, counts, defined, points), sentinels where nothing is written."""
    desc, counts, defined, points = (t.cpu().numpy() for t in keep)
    n = len(table)
    mc = cap if match_cap is None else match_cap
    nn = np.full((n, cap, 3), SENT, np.int32).view(capi.NN2_DTYPE).reshape(n, cap)
    matches = np.full((n, mc, 3), SENT, np.int32).view(capi.MATCH_DTYPE).reshape(n, mc)
    pts = points.view(capi.POINT_DTYPE).reshape(points.shape[:2])
    cnt = loopref.match_pairs(desc, counts.astype(np.int64), desc, counts.astype(np.int64), table, nn, matches, ratio2, same_octave,
                              defined if with_defined else None, defined if with_defined else None, pts if same_octave else None, pts if same_octave else None)
    return nn, matches, cnt.astype(np.int32)


def same(got, want):
    for name, a, b in zip(("nn", "matches", "match_counts"), got, want):
        assert a.tobytes() == b.tobytes(), (name, np.flatnonzero((a.reshape(len(a), -1).view(np.int32) != b.reshape(len(b), -1).view(np.int32)).any(axis=1))[:8])


# ---- the seams

CAP = 320
SEAM_COUNTS = (0, 1, 63, 64, 65, 127, 129, 300, 100000)  # the last: a count above the capacity, CAP rows in use
# both roles for every set; a set against itself; a pair and its reverse; set 7 as the query of three slots; the empty slots: {-1, -1}, a set index
# equal to the number of sets on either side, and a negative index beside a valid one
SEAM_TABLE = table_of([(7, 8), (8, 7), (7, 7), (7, 5), (0, 3), (3, 0), (-1, -1), (1, 2), (9, 4), (2, 6), (4, 9), (6, 1), (5, -2), (8, 8)])


@functools.lru_cache(maxsize=None)
def seam_sets():
    rng = np.random.default_rng(320)
    base = matchref.crafted(rng, 64)
    sets = []
    for k, m in enumerate(SEAM_COUNTS):
        rows = min(m, CAP + 40)  # (the set with the count above the capacity has more rows than the capacity too)
        d = matchref.crafted(rng, rows, base)
        sets.append((d, (rng.random(rows) < 0.9).astype(np.uint8) if k % 2 else None, rng.integers(0, 3, rows).astype(np.int32), m))
    return sets


@pytest.mark.parametrize("same_octave", [False, True])
def test_seam_counts_in_both_roles_and_untouched_rows(env, same_octave):
    ctx, torch = env
    S, keep = sets_to_device(torch, seam_sets(), CAP, True)
    got = run_pairs(ctx, torch, S, keep, SEAM_TABLE, CAP, same_octave, match_cap=40)
    want = want_pairs(keep, SEAM_TABLE, CAP, same_octave, match_cap=40)
    same(got, want)
    nn, matches, counts = got
    for p in (6, 8, 10, 12):  # the empty slots: a count of 0, every row untouched
        assert counts[p] == 0 and (nn[p].view(np.int32) == SENT).all() and (matches[p].view(np.int32) == SENT).all()
    assert (nn[4].view(np.int32) == SENT).all() and counts[4] == 0                    # a query set without rows
    assert (nn[5, :64]["index"] == -1).all() and (nn[5, 64:].view(np.int32) == SENT).all() and counts[5] == 0  # a train set without rows
    assert (nn[0, 300:].view(np.int32) == SENT).all() and (nn[1]["index"] >= 0).sum() > 200
    assert counts.max() > 40 and (matches[int(counts.argmax())].view(np.int32) != SENT).all()  # the list is cut at match_cap, the total is not
    assert (nn[2, :300]["dist2"][nn[2, :300]["index"] >= 0] <= 0).all()   # a set against itself: every defined row finds a row at distance 0 or below


@pytest.mark.parametrize("same_octave", [False, True])
def test_the_consecutive_table_is_vslam_match_dev_byte_for_byte(env, same_octave):
    ctx, torch = env
    S, keep = sets_to_device(torch, seam_sets(), CAP, True)
    n = len(SEAM_COUNTS)
    table = table_of([(p, p + 1) for p in range(n - 1)])
    got = run_pairs(ctx, torch, S, keep, table, CAP, same_octave, match_cap=50)
    d, c, df, pts = keep
    nn, matches, counts = sent(torch, n - 1, CAP, 3), sent(torch, n - 1, 50, 3), sent(torch, n - 1)
    ctx.match(S, capi.desc_sets(d[1:], c[1:], df[1:], pts[1:]), n - 1, 0.64, same_octave, nn=nn, matches=matches, match_counts=counts)
    torch.cuda.synchronize()
    same(got, (records(nn, capi.NN2_DTYPE, (n - 1, CAP)), records(matches, capi.MATCH_DTYPE, (n - 1, 50)), counts.cpu().numpy()))
    assert got[2].max() > 50  # (a list is cut at match_cap)


# ---- ties, hostile rows, table order

def test_ties_inside_a_tile_across_tiles_and_across_splits_at_two_split_counts(env):
    ctx, torch = env
    rng = np.random.default_rng(1100)
    cap = 1100  # 18 train tiles, 9 query tiles: one slot is dealt to 16 workgroups per query tile, 40 slots to 6 (vslam_match_plan.h)
    t = matchref.crafted(rng, cap)
    q = matchref.crafted(rng, 500, t)
    # train rows 5 == 6 (one tile), 70 == 200 == 1094 (tiles 1, 3 and 17), 1099 == 64 (the last tile and tile 1)
    t[6], t[200], t[1094], t[1099] = t[5], t[70], t[70], t[64]
    q[0], q[1], q[2] = t[5], t[70], t[64]
    sets = [(q, None, None, 500), (t, None, None, cap)]
    S, keep = sets_to_device(torch, sets, cap, False)
    one = run_pairs(ctx, torch, S, keep, table_of([(0, 1)]), cap)
    same(one, want_pairs(keep, table_of([(0, 1)]), cap))
    assert one[0][0, :3]["index"].tolist() == [5, 70, 64] and (one[0][0, :3]["dist2"] == 0).all() and (one[0][0, :3]["second_dist2"] == 0).all()
    forty = table_of([(1, 0) if p % 2 else (0, 0) for p in range(40)])
    forty[37] = (0, 1)
    many = run_pairs(ctx, torch, S, keep, forty, cap)
    for a, b in zip(many, one):
        assert a[37].tobytes() == b[0].tobytes()
    assert many[1][36].tobytes() != many[1][37].tobytes()


def hostile_sets(rng):
    f = np.finfo(np.float32)
    out = []
    for side in range(2):
        d = matchref.crafted(rng, 150, signed=True)
        d[1] = np.nan
        d[2, 17] = np.nan
        d[3, 5] = np.inf
        d[4, 9] = -np.inf
        d[5] = 2.0 ** 59.75   # n(row) is about 2^126.5: the sum of two such norms is finite, barely
        d[6] = d[5]
        d[7] = f.tiny / 4   # subnormals
        d[8, ::2] = f.tiny / 2
        d[9] = 0.0
        out.append(d)
    out[1][10:40] = out[0][20:50]
    return out


def test_hostile_rows_on_either_side_defined_bytes_of_zero_and_no_defined(env):
    ctx, torch = env
    rng = np.random.default_rng(127)
    a, b = hostile_sets(rng)
    da, db = np.ones(150, np.uint8), np.ones(150, np.uint8)
    da[[0, 3, 149]], db[[5, 11, 12, 64]] = 0, 0
    sets = [(a, da, None, 150), (b, db, None, 150), (a, None, None, 150)]
    S, keep = sets_to_device(torch, sets, 150, False)
    table = table_of([(0, 1), (1, 0), (2, 1), (1, 2), (0, 0)])
    got = run_pairs(ctx, torch, S, keep, table, 150)
    same(got, want_pairs(keep, table, 150))
    nn = got[0]
    assert (nn[0, [0, 3, 149]]["index"] == -1).all() and nn[0, 1]["index"] == -1 and nn[2, 3]["index"] == -1  # undefined, all-NaN and inf rows find nothing
    assert 11 not in nn[0]["index"] and 12 not in nn[0]["index"] and (nn[0, 21:23]["index"] >= 0).all()       # a skipped train row is never a neighbour
    # defined == NULL: every row of every set is defined
    d, c, _, _ = keep
    S0 = capi.desc_sets(d, c)
    got0 = run_pairs(ctx, torch, S0, keep, table, 150)
    same(got0, want_pairs(keep, table, 150, with_defined=False))
    assert got0[0][0, 21]["index"] == 11 and got0[0][0, 21]["dist2"] == 0


def test_a_scrambled_table_against_forty_one_slot_calls(env):
    ctx, torch = env
    rng = np.random.default_rng(40)
    base = matchref.crafted(rng, 64)
    rows = [int(v) for v in rng.integers(20, 140, 10)]
    sets = [(matchref.crafted(rng, m, base), None, None, m) for m in rows]
    S, keep = sets_to_device(torch, sets, 140, False)
    table = table_of([(int(a), int(b)) for a, b in zip(rng.integers(0, 10, 40), rng.integers(0, 10, 40))])
    assert len({tuple(p) for p in table.tolist()}) > 30 and (table["query_set"] != table["train_set"]).sum() > 30
    got = run_pairs(ctx, torch, S, keep, table, 140)
    same(got, want_pairs(keep, table, 140))
    for p in range(40):
        one = run_pairs(ctx, torch, S, keep, table[p:p + 1], 140)
        for a, b in zip(got, one):
            assert a[p].tobytes() == b[0].tobytes(), p


def test_each_optional_output_alone_and_two_buffers(env):
    ctx, torch = env
    S, keep = sets_to_device(torch, seam_sets(), CAP, True)
    want = want_pairs(keep, SEAM_TABLE, CAP, match_cap=40)
    for asked in (("nn",), ("match_counts",), ("matches", "match_counts")):
        got = run_pairs(ctx, torch, S, keep, SEAM_TABLE, CAP, match_cap=40, want=asked)
        for name, a, b in zip(("nn", "matches", "match_counts"), got, want):
            assert a.tobytes() == b.tobytes() if name in asked else (a.view(np.int32) == SENT).all(), (asked, name)
    # the train side in a buffer of its own, with another capacity and another number of sets
    rng = np.random.default_rng(9)
    tsets = [(matchref.crafted(rng, m, seam_sets()[7][0]), None, None, m) for m in (70, 0, 130)]
    T, keept = sets_to_device(torch, tsets, 130, False)
    table = table_of([(7, 2), (8, 0), (3, 3), (2, 1), (9, 0), (1, 2)])
    got = run_pairs(ctx, torch, S, keep, table, CAP, T=T)
    q, t = [x.cpu().numpy() for x in keep], [x.cpu().numpy() for x in keept]
    nn = np.full((6, CAP, 3), SENT, np.int32).view(capi.NN2_DTYPE).reshape(6, CAP)
    matches = np.full((6, CAP, 3), SENT, np.int32).view(capi.MATCH_DTYPE).reshape(6, CAP)
    cnt = loopref.match_pairs(q[0], q[1].astype(np.int64), t[0], t[1].astype(np.int64), table, nn, matches, 0.64, False, q[2], t[2])
    same(got, (nn, matches, cnt.astype(np.int32)))
    assert cnt[2] == 0 and cnt[4] == 0 and (nn[2].view(np.int32) == SENT).all() and cnt[0] > 0  # train set 3 of 3 and query set 9 of 9 are empty slots


# ---- the gather

def test_gather_counts_of_0_1_cap_and_above_and_hostile_indices(env):
    ctx, torch = env
    rng = np.random.default_rng(24)
    n_sets, cap, mcap = 4, 90, 33
    points = rng.integers(-5, 500, (n_sets, cap, 6)).astype(np.int32)
    tpoints = rng.integers(-5, 500, (3, 70, 6)).astype(np.int32)
    table = table_of([(0, 1), (3, 2), (-1, -1), (1, 0), (2, 2), (0, 3), (3, 0), (260, 1)])
    counts = np.array([0, 1, 20, mcap, 100000, 9, 300, 5], np.int32)
    matches = np.zeros((len(table), mcap), capi.MATCH_DTYPE)
    matches["query"], matches["train"] = rng.integers(0, cap, matches.shape), rng.integers(0, 70, matches.shape)
    matches["dist2"] = rng.random(matches.shape).astype(np.float32)
    matches[3, 4]["query"], matches[3, 5]["train"], matches[3, 6]["query"], matches[3, 7]["train"] = cap, 70, -1, -2 ** 31  # at the capacity and far past it
    matches[4, 0]["dist2"] = np.nan
    qo, to, lo = sent(torch, len(table), mcap, 6), sent(torch, len(table), mcap, 6), sent(torch, len(table), mcap, 3)
    ctx.pair_points(dev(torch, matches.view(np.int32).reshape(len(table), mcap, 3)), dev(torch, counts), dev(torch, table.view(np.int32).reshape(-1, 2)),
                    dev(torch, points), dev(torch, tpoints), qo, to, lo)
    torch.cuda.synchronize()
    wq = np.full((len(table), mcap, 6), SENT, np.int32).view(capi.POINT_DTYPE).reshape(len(table), mcap)
    wt, wl = wq.copy(), np.full((len(table), mcap, 3), SENT, np.int32).view(capi.MATCH_DTYPE).reshape(len(table), mcap)
    loopref.gather(matches, counts.astype(np.int64), table, points.view(capi.POINT_DTYPE).reshape(n_sets, cap), tpoints.view(capi.POINT_DTYPE).reshape(3, 70), wq, wt, wl)
    assert qo.cpu().numpy().tobytes() == wq.tobytes() and to.cpu().numpy().tobytes() == wt.tobytes() and lo.cpu().numpy().tobytes() == wl.tobytes()
    for p in (0, 2, 5, 7):  # a count of 0, {-1, -1}, train set 3 of 3, query set 260 of 4: nothing of the slot is written
        assert (wq[p].view(np.int32) == SENT).all() and (wl[p].view(np.int32) == SENT).all()
    assert (wq[1, 1:].view(np.int32) == SENT).all() and (wq[1, :1].view(np.int32) != SENT).any() and (wl[4].view(np.int32) != SENT).all()
    assert wq[3, 4].tobytes() == wt[3, 5].tobytes() == wq[3, 6].tobytes() == wt[3, 7].tobytes() == b"\xff" * 24


def test_epipolar_on_the_gathered_lists_is_epipolar_on_the_pair_s_own_lists(env):
    ctx, torch = env
    scenes = [epiref.planted_scene(s, n=100 + 30 * s) for s in range(4)]
    cap = 200
    matches = np.zeros((4, cap), capi.MATCH_DTYPE)
    counts = np.zeros(4, np.int32)
    qsets, tsets = np.zeros((4, cap), capi.POINT_DTYPE), np.zeros((4, cap), capi.POINT_DTYPE)
    for s, (m, qp, tp, _) in enumerate(scenes):
        matches[s, : len(m)], counts[s] = m, len(m)
        qsets[s, : len(qp)], tsets[s, : len(tp)] = qp, tp
    matches[2, 3]["query"] = cap  # a hostile record: untrusted on both routes
    as_t = lambda a, w: dev(torch, a.view(np.int32).reshape(a.shape + (w,)))
    tm, tc, tq, tt = as_t(matches, 3), dev(torch, counts), as_t(qsets, 6), as_t(tsets, 6)

    def epipolar(m, q, t):
        models = torch.zeros(4 * 88, dtype=torch.uint8, device=DEV)
        bits = torch.zeros((4, (cap + 63) // 64), dtype=torch.int64, device=DEV)
        ctx.epipolar(m, tc, q, t, 4, n_hypotheses=256, seed=5, max_dist2=4.0, models=models, inlier_bits=bits)
        torch.cuda.synchronize()
        return models.cpu().numpy().view(capi.EPIPOLAR_DTYPE), bits.cpu().numpy()

    direct = epipolar(tm, tq, tt)
    # the same four pairs as the slots of a table in the SAME order (the slot index is the pair index of the sampler): query sets 0 .. 3 of one buffer,
    # train sets 0 .. 3 of another
    table = table_of([(s, s) for s in range(4)])
    qo, to, lo = sent(torch, 4, cap, 6), sent(torch, 4, cap, 6), sent(torch, 4, cap, 3)
    ctx.pair_points(tm, tc, dev(torch, table.view(np.int32).reshape(-1, 2)), tq, tt, qo, to, lo)
    gathered = epipolar(lo, qo, to)
    assert gathered[0].tobytes() == direct[0].tobytes() and gathered[1].tobytes() == direct[1].tobytes()
    assert (direct[0]["best"] >= 0).all() and (direct[0]["n_inliers"] >= 8).all()
    want, flags = loopref.models_of(records(lo, capi.MATCH_DTYPE, (4, cap)), counts, records(qo, capi.POINT_DTYPE, (4, cap)), records(to, capi.POINT_DTYPE, (4, cap)),
                                    table, 4, 4, 256, 5, 4.0)
    assert gathered[0].tobytes() == want.tobytes()
    for s in range(4):
        assert gathered[1][s, : (counts[s] + 63) // 64].tobytes() == epiref.bits(flags[s], (counts[s] + 63) // 64).tobytes()


# ---- the verdict and the table

def run_verdict(ctx, torch, case, want=("loops", "loop_list", "n_loops")):
    nq = case["nq"]
    o = dict(loops=sent(torch, nq, 5), loop_list=sent(torch, nq), n_loops=sent(torch, 1))
    ctx.loop_verdict(dev(torch, case["models"].view(np.uint8)), dev(torch, case["pairs"].view(np.int32).reshape(-1, 2)), nq, case["c"], case["n_train_sets"],
                     case["min_inliers"], case["num"], case["den"], **{k: v for k, v in o.items() if k in want})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def check_verdict(got, case, want=("loops", "loop_list", "n_loops")):
    loops, lst, n = loopref.verdict(**case, loop_list=np.full(case["nq"], SENT, np.int32))
    ref = dict(loops=loops, loop_list=lst, n_loops=np.array([n], np.int32))
    for k in ("loops", "loop_list", "n_loops"):
        assert got[k].tobytes() == ref[k].tobytes() if k in want else (got[k] == SENT).all(), k
    return ref


@pytest.mark.parametrize("name", sorted(loopref.verdict_cases()))
def test_verdict_rule_cases(env, name):
    ctx, torch = env
    case = loopref.verdict_cases()[name]
    check_verdict(run_verdict(ctx, torch, case), case)


@pytest.mark.parametrize("nq", [1, 64, 65, 300])
@pytest.mark.parametrize("c", [1, 3, 8])
def test_verdict_frames_past_one_wave_and_one_workgroup(env, nq, c):
    ctx, torch = env
    case = loopref.random_verdict_case(nq * 10 + c, nq, c, 40)
    ref = check_verdict(run_verdict(ctx, torch, case), case)
    if nq >= 64:
        assert 0 < ref["n_loops"][0] < nq
    for asked in (("loops",), ("n_loops",), ("loop_list", "n_loops")):
        check_verdict(run_verdict(ctx, torch, case, asked), case, asked)
    loops, lst, n = ctx.loop_verdict_host(case["models"], case["pairs"], c, 40, case["min_inliers"], case["num"], case["den"], fill=SENT)
    assert loops.tobytes() == ref["loops"].tobytes() and lst.tobytes() == ref["loop_list"].tobytes() and n == ref["n_loops"][0]


@pytest.mark.parametrize("name", sorted(loopref.table_cases()))
def test_table_rule_cases(env, name):
    ctx, torch = env
    case = loopref.table_cases()[name]
    cands = case["candidates"]
    nq, c = cands.shape
    pairs = sent(torch, nq * c, 2)
    ctx.loop_pairs(dev(torch, cands.view(np.int32).reshape(nq, c, 3)), dev(torch, np.array(case["cand_counts"], np.int32)), pairs, case["db_first"], case["nd"])
    torch.cuda.synchronize()
    assert pairs.cpu().numpy().tobytes() == loopref.pairs_table(**case).tobytes()


# ---- the whole chain

def chain_on_device(ctx, torch, d, c, df, pts, cands, counts, n_slots_per_frame, match_cap, params, ransac):
    """candidates -> table -> match -> gather -> F -> verdict over one batch searched in itself; nothing comes down in between."""
    n = d.shape[0]
    slots = n * n_slots_per_frame
    pairs = sent(torch, slots, 2)
    matches, mcounts = sent(torch, slots, match_cap, 3), sent(torch, slots)
    qo, to, lo = sent(torch, slots, match_cap, 6), sent(torch, slots, match_cap, 6), sent(torch, slots, match_cap, 3)
    models = torch.zeros(slots * 88, dtype=torch.uint8, device=DEV)
    loops, lst, nl = sent(torch, n, 5), sent(torch, n), sent(torch, 1)
    S = capi.desc_sets(d, c, df, pts)
    ctx.loop_pairs(cands, counts, pairs)
    ctx.match_pairs(S, S, pairs, matches=matches, match_counts=mcounts)
    ctx.pair_points(matches, mcounts, pairs, pts, pts, qo, to, lo)
    ctx.epipolar(lo, mcounts, qo, to, slots, models=models, **ransac)
    ctx.loop_verdict(models, pairs, n, n_slots_per_frame, n, *params, loops=loops, loop_list=lst, n_loops=nl)
    torch.cuda.synchronize()
    return dict(pairs=records(pairs, capi.SET_PAIR_DTYPE, (slots,)), match_counts=mcounts.cpu().numpy(), matches=records(matches, capi.MATCH_DTYPE, (slots, match_cap)),
                models=models.cpu().numpy().view(capi.EPIPOLAR_DTYPE), loops=records(loops, capi.LOOP_DTYPE, (n,)), loop_list=lst.cpu().numpy(), n_loops=int(nl.cpu()[0]))


def test_seventeen_crops_end_to_end_the_host_twins_the_cxx_wrapper_and_the_place_executable(env, tmp_path):
    from tests.test_loop_cpu import LOOPS_AT_DEFAULT, LOOSE, RANSAC, build_cxx_driver
    from tests.test_place_cpu import VOCAB_FRAMES, crop_sequence

    ctx, torch = env
    crops = crop_sequence()
    n, K, C8 = len(crops), 256, 8
    shapes = sorted({img.shape for img in crops})
    outs = [(idx, *detect(ctx, torch, np.stack([crops[f] for f in idx]))) for idx in ([f for f in range(n) if crops[f].shape == sh] for sh in shapes)]
    cap = max(p.oriented_cap for _, p, _ in outs)
    d = torch.zeros((n, cap, 128), dtype=torch.float32, device=DEV)
    c = torch.zeros(n, dtype=torch.int32, device=DEV)
    df = torch.zeros((n, cap), dtype=torch.uint8, device=DEV)
    pts = torch.zeros((n, cap, 6), dtype=torch.int32, device=DEV)
    for idx, p, o in outs:
        at = torch.tensor(idx, device=DEV)
        d[at, : p.oriented_cap], c[at], df[at, : p.oriented_cap], pts[at, : p.oriented_cap] = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    rows = int(c.max())
    d, df, pts, cap = d[:, :rows].contiguous(), df[:, :rows].contiguous(), pts[:, :rows].contiguous(), rows  # (the restatement's matcher walks every row below the capacity)
    S = capi.desc_sets(d, c, df)
    vocab, vdef = torch.zeros((K, 128), dtype=torch.float32, device=DEV), torch.zeros(K, dtype=torch.uint8, device=DEV)
    hist = sent(torch, n, K)
    cands, counts = sent(torch, n, C8, 3), sent(torch, n)
    V = VOCAB_FRAMES
    params = (capi.Context.LOOP_MIN_INLIERS, capi.Context.LOOP_NUM, capi.Context.LOOP_DEN)
    ctx.vocab_sample(capi.desc_sets(d[:V], c[:V], df[:V]), vocab, vdef)
    ctx.words(S, vocab, vdef, hist=hist)
    ctx.place(hist, None, min_gap=4, max_candidates=C8, num=LOOSE[0], den=LOOSE[1], candidates=cands, cand_counts=counts)  # the loosened threshold
    got = chain_on_device(ctx, torch, d, c, df, pts, cands, counts, C8, cap, params, RANSAC)
    # the restatement over what the device detected
    hd, hc, hdf, hp = d.cpu().numpy(), c.cpu().numpy().astype(np.int64), df.cpu().numpy(), pts.cpu().numpy().view(capi.POINT_DTYPE).reshape(n, cap)
    hcands, hcounts = records(cands, capi.PLACE_CAND_DTYPE, (n, C8)), counts.cpu().numpy()
    ref = placeref.place(hist.cpu().numpy().view(np.uint32), None, min_gap=4, max_candidates=C8, num=LOOSE[0], den=LOOSE[1], fill=SENT)
    assert hcands.tobytes() == ref["candidates"].tobytes() and hcounts.tobytes() == ref["cand_counts"].tobytes()
    want = loopref.verify(hd, hc, hdf, hp, hcands, hcounts, 0, RANSAC["n_hypotheses"], RANSAC["seed"], RANSAC["max_dist2"], *params)
    assert got["pairs"].tobytes() == want["pairs"].tobytes() and (got["pairs"]["query_set"] >= 0).sum() == 22
    used = [p for p in range(n * C8) if got["pairs"][p]["query_set"] >= 0]
    assert got["match_counts"].tobytes() == want["match_counts"].astype(np.int32).tobytes()
    for p in used:
        k = want["match_counts"][p]
        assert got["matches"][p, :k].tobytes() == want["matches"][p, :k].tobytes() and (got["matches"][p, k:].view(np.int32) == SENT).all(), p
    assert got["models"].tobytes() == want["models"].tobytes()
    assert got["loops"].tobytes() == want["loops"].tobytes() and got["n_loops"] == want["n_loops"] == 3
    assert got["loop_list"][:3].tolist() == [12, 13, 14] and (got["loop_list"][3:] == SENT).all()
    # ... which are the loops the CPU test recorded from the oracle's descriptors
    loops = {int(l["query_set"]): (int(l["train_set"]), int(l["slot"]), int(l["n_matches"]), int(l["n_inliers"])) for l in got["loops"] if l["slot"] >= 0}
    assert loops == LOOPS_AT_DEFAULT
    # the host twins: the matcher over the table, the verdict over the models
    hnn = np.full((n * C8, cap, 3), SENT, np.int32).view(capi.NN2_DTYPE).reshape(n * C8, cap)
    hm = np.full((n * C8, cap, 3), SENT, np.int32).view(capi.MATCH_DTYPE).reshape(n * C8, cap)
    _, hm, hmc = ctx.match_pairs_host(hd, hc, hd, None, want["pairs"], query_defined=hdf, train_defined=hdf, nn=hnn, matches=hm)
    assert hm.tobytes() == got["matches"].tobytes() and hmc.tobytes() == want["match_counts"].tobytes()
    assert (hnn[0].view(np.int32) == SENT).all() and (hnn[96, : hc[12]]["index"] >= -1).all() and (hnn[96, hc[12]:].view(np.int32) == SENT).all()
    hl, hlst, hn = ctx.loop_verdict_host(want["models"], want["pairs"], C8, n, *params, fill=SENT)
    assert hl.tobytes() == got["loops"].tobytes() and hlst.tobytes() == got["loop_list"].tobytes() and hn == 3
    # vslam::verifyLoops on the same frames and candidates (the C++ mirror squares its ratio of 0.8 in f32: 0.64000005, not 0.64)
    want = loopref.verify(hd, hc, hdf, hp, hcands, hcounts, 0, RANSAC["n_hypotheses"], RANSAC["seed"], RANSAC["max_dist2"], *params,
                          ratio2=float(np.float32(0.8) * np.float32(0.8)))
    exe = build_cxx_driver(tmp_path)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<9Q", n, cap, C8, 0, *params, RANSAC["n_hypotheses"], RANSAC["seed"]) + hc.astype(np.uint32).tobytes() + hd.tobytes() + hdf.tobytes() +
                    hp.tobytes() + hcounts.astype(np.uint32).tobytes() + hcands.tobytes())
    r = subprocess.run([exe, "verify", str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    per_slot = b"".join(struct.pack("<I", int(k)) + want["matches"][p, :k].tobytes() for p, k in enumerate(want["match_counts"]))
    assert dst.read_bytes() == want["pairs"].tobytes() + per_slot + want["models"].tobytes() + want["loops"].tobytes() + struct.pack("<I", 3) + want["loop_list"][:3].tobytes()
    # Place --verify on the same images
    place = os.path.join(ROOT, "visualslam_amd", "bin", "Place")
    paths = []
    for k, img in enumerate(crops):
        paths.append(str(tmp_path / f"crop{k:02d}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([place, "--words", "256", "--gap", "4", "--candidates", "8", "--threshold", "%d/%d" % LOOSE, "--octaves", "3", "--vocab-frames", str(V), "--verify",
                        str(params[0])] + paths, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["loops"] == [[int(l["train_set"]), int(l["slot"]), int(l["n_matches"]), int(l["n_inliers"])] for l in want["loops"]]
    assert rep["verified"] == [[[int(want["models"][i * C8 + r][k]) for k in ("n_matches", "n_inliers", "best")] for r in range(hcounts[i])] for i in range(n)]


def test_the_table_of_a_real_place_output_with_its_own_offsets(env):
    ctx, torch = env
    rng = np.random.default_rng(77)
    K, nq, nd = 300, 37, 50
    hd = (rng.integers(1, 9, (nd, K)) * (rng.random((nd, K)) < 0.2)).astype(np.int32)
    hq = (rng.integers(1, 9, (nq, K)) * (rng.random((nq, K)) < 0.2)).astype(np.int32)
    hq[::3] = hd[5:5 + len(hq[::3])]
    cands, counts = sent(torch, nq, 5, 3), sent(torch, nq)
    ctx.place(dev(torch, hq), dev(torch, hd), q_first=106, db_first=100, min_gap=4, max_candidates=5, num=1, den=10, candidates=cands, cand_counts=counts)
    pairs = sent(torch, nq * 5, 2)
    ctx.loop_pairs(cands, counts, pairs, db_first=100, nd=nd)   # the slots past a count hold sentinel bytes: they are not read
    short = sent(torch, nq * 5, 2)
    ctx.loop_pairs(cands, counts, short, db_first=100, nd=20)   # a database cut short: the frames at and past db_first + 20 fall out
    torch.cuda.synchronize()
    hcands, hcounts = records(cands, capi.PLACE_CAND_DTYPE, (nq, 5)), counts.cpu().numpy()
    assert hcounts.max() == 5 and hcounts.min() < 5
    assert pairs.cpu().numpy().tobytes() == loopref.pairs_table(hcands, hcounts, 100, nd).tobytes()
    assert short.cpu().numpy().tobytes() == loopref.pairs_table(hcands, hcounts, 100, 20).tobytes()
    got, cut = records(pairs, capi.SET_PAIR_DTYPE, (nq * 5,)), records(short, capi.SET_PAIR_DTYPE, (nq * 5,))
    assert (got["train_set"] >= 20).sum() > 0 and (cut["train_set"] >= 20).sum() == 0 and (cut["query_set"] >= 0).sum() < (got["query_set"] >= 0).sum()

"""Mutual matching on the GPU (vslam_match_mutual_dev / vslam_match_mutual_host, include/vslam.h): every comparison is bytes-equal
against the CPU restatement in tests/mutualref.py - nn, rnn, the mutual list and its totals - over outputs that were filled with a
sentinel first, so that the rows a call must leave alone are checked too.

Every "require" comment marks a condition on the input, evaluated on the restatement's answer alone: the case only exercises
what it is for while it holds."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from tests import epiref, matchref, mutualref
from tests.test_gpu_match import SENT, building_crops, detect, env, exact_translations, make_pair, oracle_chain, sets_to_device  # noqa: F401 (env: fixture)
from tests.test_gpu_match_limits import block_near_copies, block_overflow
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_dev(ctx, torch, qsets, tsets, qcap, tcap, ratio2=0.64, same_octave=False, match_cap=None, only=("nn", "rnn", "matches", "match_counts")):
    """-> (nn [n, qcap, 3], rnn [n, tcap, 2], matches [n, match_cap, 3], counts [n]) as int32, SENT where nothing was written."""
    n = len(qsets)
    Q, keepq = sets_to_device(torch, qsets, qcap, same_octave)
    T, keept = sets_to_device(torch, tsets, tcap, same_octave)
    match_cap = qcap if match_cap is None else match_cap
    out = dict(nn=torch.full((n, qcap, 3), SENT, dtype=torch.int32, device=DEV), rnn=torch.full((n, tcap, 2), SENT, dtype=torch.int32, device=DEV),
               matches=torch.full((n, match_cap, 3), SENT, dtype=torch.int32, device=DEV), match_counts=torch.full((n,), SENT, dtype=torch.int32, device=DEV))
    ctx.match_mutual(Q, T, n, ratio2, same_octave, **{k: v for k, v in out.items() if k in only})
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in ("nn", "rnn", "matches", "match_counts"))


def reference(qs, ts, qcap, tcap, ratio2=0.64, same_octave=False):
    (qd, qdf, qoc, qcnt), (td, tdf, toc, tcnt) = qs, ts
    nq, nt = min(qcnt, qcap), min(tcnt, tcap)
    cut = lambda a, n: None if a is None else a[:n]
    return mutualref.mutual(qd[:nq], td[:nt], ratio2, same_octave, cut(qdf, nq), cut(tdf, nt), cut(qoc, nq), cut(toc, nt))


def check_pair(got, j, qs, ts, qcap, tcap, ratio2=0.64, same_octave=False, match_cap=None):
    nn, rnn, matches, counts = got
    match_cap = qcap if match_cap is None else match_cap
    wnn, wrnn, wm = reference(qs, ts, qcap, tcap, ratio2, same_octave)
    nq, nt = len(wnn), len(wrnn)
    assert nn[j, :nq].tobytes() == wnn.tobytes(), ("nn", j)
    assert (nn[j, nq:] == SENT).all(), "nn rows past the count were written"
    bad = np.flatnonzero((rnn[j, :nt].view(np.uint8).reshape(nt, 8) != wrnn.view(np.uint8).reshape(nt, 8)).any(axis=1))
    assert len(bad) == 0, ("rnn", j, bad[:5], rnn[j, bad[:5]].copy().view(capi.RNN_DTYPE), wrnn[bad[:5]])
    assert (rnn[j, nt:] == SENT).all(), "rnn rows past the train count were written"
    assert counts[j] == len(wm), ("match_counts", j, int(counts[j]), len(wm))
    m = min(len(wm), match_cap)
    assert matches[j, :m].tobytes() == wm[:m].tobytes(), ("matches", j)
    assert (matches[j, m:] == SENT).all(), "matches past the count were written"
    return wnn, wrnn, wm


def make_pair_m(rng, nq, nt, octaves=False, specials=True):
    """make_pair's sets (duplicates, a NaN row and an undefined row on each side, an exact copy; train row 2 undefined where query 6
    is its copy) and, for the reverse side, a train row whose best candidate is the undefined query row 4."""
    qs, ts = make_pair(rng, nq, nt, octaves, specials)
    if specials and nt >= 8 and nq >= 8:
        ts[0][6] = qs[0][4]
        if octaves:
            ts[2][6] = qs[2][4]
    return qs, ts


SIZES = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 63), (65, 127), (127, 129), (129, 65), (257, 130), (1000, 777)]


@pytest.mark.parametrize("same_octave", [False, True])
@pytest.mark.parametrize("nq,nt", SIZES)
def test_crafted_sets_match_the_restatement(env, nq, nt, same_octave):
    ctx, torch = env
    rng = np.random.default_rng(1000 * nq + nt)
    qs, ts = make_pair_m(rng, nq, nt, octaves=same_octave)
    qcap, tcap = max(nq, 1) + 3, max(nt, 1) + 2
    got = run_dev(ctx, torch, [qs], [ts], qcap, tcap, same_octave=same_octave)
    wnn, wrnn, wm = check_pair(got, 0, qs, ts, qcap, tcap, 0.64, same_octave)
    assert len(np.unique(wm["train"])) == len(wm)
    if nq >= 8 and nt >= 8:
        # require: the undefined and the NaN rows get nothing and are nobody's reverse nearest, even where they would be the best
        assert wrnn["index"][2] == -1 and np.isposinf(wrnn["dist2"][2]) and wrnn["index"][3] == -1
        assert not np.isin(wrnn["index"], [4, 5]).any() and wrnn["index"][6] != 4
        if not same_octave:
            assert wrnn["index"][1] == 0 and wrnn["dist2"][1] == 0.0 and wrnn["index"][4] == 7 and 7 in wm["query"]


# positions of identical query rows -> where the tie is decided: 3 & 8 in one lane's 16 rows, 3 & 7 between the halves of a wave,
# 3 & 35 between waves (LDS), 3 & 131 and 3 & 259 between workgroups (the atomic); then four at once
TIES = [(3, 8), (3, 7), (3, 35), (3, 131), (3, 259), (3, 7, 35, 131), (3, 8, 131, 259)]


def test_reverse_ties_at_every_merge_level_keep_the_lowest_query(env):
    ctx, torch = env
    rng = np.random.default_rng(21)
    nq, nt, trow = 300, 70, 37
    qsets, tsets, want = [], [], []
    for rows in TIES:
        for lower_undefined in (False, True):
            td = matchref.crafted(rng, nt)
            qd = matchref.crafted(rng, nq)
            qd[list(rows)] = td[trow]
            qdf = np.ones(nq, np.uint8)
            if lower_undefined:
                qdf[rows[0]] = 0
            qsets.append((qd, qdf, None, nq)), tsets.append((td, None, None, nt)), want.append(rows[1] if lower_undefined else rows[0])
    got = run_dev(ctx, torch, qsets, tsets, nq + 5, nt + 3)
    for j, w in enumerate(want):
        _, wrnn, _ = check_pair(got, j, qsets[j], tsets[j], nq + 5, nt + 3)
        assert wrnn["index"][trow] == w and wrnn["dist2"][trow] == 0.0, (j, wrnn[trow], w)  # require: the tie is the row's minimum


def test_clamped_tail_rows_past_the_count_take_no_part(env):
    """nq = 130: the second query tile holds rows 128 and 129, and 126 clamped copies of row 129 beside them."""
    ctx, torch = env
    rng = np.random.default_rng(22)
    nq, nt, qcap = 130, 70, 256
    pairs = []
    for last_undefined in (False, True):
        td = matchref.crafted(rng, nt)
        qd = matchref.crafted(rng, qcap)        # the capacity holds real rows past the count, `defined` bytes of 1 past it
        td[10] = qd[129]
        td[11] = qd[200]                        # a row past the count would be the best
        qdf = np.ones(qcap, np.uint8)
        qdf[129] = 0 if last_undefined else 1   # undefined: a phantom copy of it, read with a `defined` byte past the count, would win
        pairs.append(((qd, qdf, None, nq), (td, None, None, nt)))
    qsets, tsets = [p[0] for p in pairs], [p[1] for p in pairs]
    got = run_dev(ctx, torch, qsets, tsets, qcap, nt + 2)
    for j in (0, 1):
        _, wrnn, _ = check_pair(got, j, qsets[j], tsets[j], qcap, nt + 2)
        assert (got[1][j, :nt, 0] < nq).all()
        # require: row 129 is the reverse nearest where it is defined, and some other row in use where it is not
        assert (wrnn["index"][10] == 129 and wrnn["dist2"][10] == 0.0) if j == 0 else (0 <= wrnn["index"][10] < 129 and wrnn["dist2"][10] > 0.0)
        assert 0 <= wrnn["index"][11] < nq and wrnn["dist2"][11] > 0.0


def test_negative_minus_inf_and_plus_inf_distances(env):
    ctx, torch = env
    rng = np.random.default_rng(3)
    nq = nt = 300
    q1, t1 = block_near_copies(rng, nq, nt)
    q2, t2 = block_overflow(rng, nq, nt)
    qsets, tsets = [(q1, None, None, len(q1)), (q2, None, None, len(q2))], [(t1, None, None, len(t1)), (t2, None, None, len(t2))]
    qcap, tcap = nq + 3, 2 * nt + 2
    got = run_dev(ctx, torch, qsets, tsets, qcap, tcap)
    _, wrnn, wm = check_pair(got, 0, qsets[0], tsets[0], qcap, tcap)
    assert (wrnn["dist2"] < 0).sum() >= 20 and len(wm) > 0                                    # require: negative reverse minima
    _, wrnn, wm = check_pair(got, 1, qsets[1], tsets[1], qcap, tcap)
    neginf = np.flatnonzero(np.isneginf(wrnn["dist2"]))
    assert len(neginf) >= 1 and np.isin(neginf, wm["train"]).any()                            # require: a -inf that wins and is mutual
    assert not np.isnan(wrnn["dist2"]).any() and ((wrnn["index"] >= 0) == (wrnn["dist2"] < np.inf)).all()
    assert (wrnn["index"] == -1).any()                                                        # require: rows whose every distance is +inf or NaN
    # a train row of an octave no query has
    qs, ts = make_pair_m(np.random.default_rng(4), 140, 150, octaves=True)
    ts[2][20] = 7
    got = run_dev(ctx, torch, [qs], [ts], 143, 152, same_octave=True)
    _, wrnn, _ = check_pair(got, 0, qs, ts, 143, 152, 0.64, True)
    assert wrnn["index"][20] == -1 and np.isposinf(wrnn["dist2"][20])


def test_sixteen_splits_and_a_reverse_winner_in_another_query_tile(env):
    """One pair of 3 query tiles and 33 train tiles: ceil(2048 / 3) workgroups per tile are wanted, 16 are the most."""
    ctx, torch = env
    rng = np.random.default_rng(23)
    nq, nt = 300, 2100
    td = matchref.crafted(rng, nt)
    qd = matchref.crafted(rng, nq, td)
    for trow, (near, exact) in {500: (10, 200), 1999: (290, 5), 64 * 16 + 1: (130, 131)}.items():
        td[trow] = matchref.crafted(rng, 1)[0]
        qd[exact] = td[trow]
        qd[near] = np.abs(td[trow] + rng.normal(0, 0.01, 128)).astype(np.float32)
    qs, ts = (qd, None, None, nq), (td, None, None, nt)
    got = run_dev(ctx, torch, [qs], [ts], nq + 4, nt + 12)
    wnn, wrnn, wm = check_pair(got, 0, qs, ts, nq + 4, nt + 12)
    # require: the forward winner of `near` is the train row whose reverse winner is `exact`, in another query tile for two of them
    assert (wnn["index"][[10, 290, 130]] == [500, 1999, 1025]).all() and (wrnn["index"][[500, 1999, 1025]] == [200, 5, 131]).all()
    assert not np.isin([10, 290, 130], wm["query"]).any() and np.isin([200, 5, 131], wm["query"]).all()
    again = run_dev(ctx, torch, [qs], [ts], nq + 4, nt + 12)  # the atomics decide between workgroups: two runs, the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_forty_unequal_pairs_in_one_call(env):
    ctx, torch = env
    rng = np.random.default_rng(40)
    n, qcap, tcap = 40, 150, 170
    sizes = [(int(rng.integers(1, qcap + 1)), int(rng.integers(1, tcap + 1))) for _ in range(n)]
    sizes[0], sizes[1], sizes[2], sizes[39] = (0, 90), (90, 0), (0, 0), (qcap, tcap)
    pairs = [make_pair_m(rng, a, b, octaves=True, specials=(j % 3 == 0)) for j, (a, b) in enumerate(sizes)]
    for j in (5, 6):  # counts above the capacity: min(count, cap) rows are used
        (qd, qdf, qoc, _), (td, tdf, toc, _) = make_pair_m(rng, qcap + 40, tcap + 30, octaves=True)
        pairs[j] = ((qd, qdf, qoc, 100000), (td, tdf, toc, 4000 + j))
    qsets, tsets = [p[0] for p in pairs], [p[1] for p in pairs]
    for same_octave in (False, True):
        got = run_dev(ctx, torch, qsets, tsets, qcap, tcap, same_octave=same_octave, match_cap=32)
        totals = [len(check_pair(got, j, qsets[j], tsets[j], qcap, tcap, 0.64, same_octave, 32)[2]) for j in range(n)]
        assert min(totals) == 0 and max(totals) > 32  # require: empty lists and lists that are cut
        # no pair reads its neighbour's table: each pair alone gives the same bytes
        for j in (1, 2, 5, 20):
            one = run_dev(ctx, torch, qsets[j:j + 1], tsets[j:j + 1], qcap, tcap, same_octave=same_octave, match_cap=32)
            assert all(w[j].tobytes() == o[0].tobytes() for w, o in zip(got, one)), j


def test_two_calls_in_a_row_the_reverse_table_is_reset(env):
    ctx, torch = env
    rng = np.random.default_rng(24)
    nq, nt = 200, 180
    td = matchref.crafted(rng, nt)
    first = ((np.concatenate([td, td[:nq - nt]]), None, None, nq), (td, None, None, nt))  # every train row has an exact copy: d2 = 0 everywhere
    td2 = matchref.crafted(rng, nt)
    second = ((matchref.crafted(rng, nq), None, None, nq), (td2, None, None, nt))         # nothing in common: every minimum is far above 0
    got1 = run_dev(ctx, torch, [first[0]], [first[1]], nq, nt)
    got2 = run_dev(ctx, torch, [second[0]], [second[1]], nq, nt)
    _, w1, _ = check_pair(got1, 0, first[0], first[1], nq, nt)
    _, w2, _ = check_pair(got2, 0, second[0], second[1], nq, nt)
    assert (w1["dist2"] == 0.0).all() and (w2["dist2"] > 1.0).all()  # require: a table left over from the first call would win everywhere


def test_small_match_cap_and_each_optional_output_alone(env):
    ctx, torch = env
    qs, ts = make_pair_m(np.random.default_rng(25), 260, 300, octaves=True)
    whole = run_dev(ctx, torch, [qs], [ts], 263, 302)
    _, _, wm = check_pair(whole, 0, qs, ts, 263, 302)
    cut = run_dev(ctx, torch, [qs], [ts], 263, 302, match_cap=17)
    check_pair(cut, 0, qs, ts, 263, 302, match_cap=17)
    assert len(wm) > 17  # require: the total is reported, the list is cut
    for only in (("nn",), ("rnn",), ("match_counts",), ("matches", "match_counts"), ("rnn", "match_counts")):
        got = run_dev(ctx, torch, [qs], [ts], 263, 302, only=only)
        for k, name in enumerate(("nn", "rnn", "matches", "match_counts")):
            assert got[k].tobytes() == whole[k].tobytes() if name in only else (got[k] == SENT).all(), (only, name)
    Q, _kq = sets_to_device(torch, [qs], 263, False)
    T, _kt = sets_to_device(torch, [ts], 302, False)
    with pytest.raises(capi.VslamError, match="match_mutual: rnn buffer too small"):
        ctx.match_mutual(Q, T, 1, rnn=torch.zeros((1, 301, 2), dtype=torch.int32, device=DEV))
    with pytest.raises(capi.VslamError, match="match_mutual: same_octave needs the points of both sets"):
        ctx.match_mutual(Q, T, 1, same_octave=True, rnn=torch.zeros((1, 302, 2), dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("same_octave", [False, True])
def test_identities_on_the_device_forward_is_the_matcher_reverse_is_the_swapped_matcher(env, same_octave):
    ctx, torch = env
    nq, nt, qcap, tcap = 1000, 777, 1003, 779
    qs, ts = make_pair_m(np.random.default_rng(26), nq, nt, octaves=True)
    Q, _kq = sets_to_device(torch, [qs], qcap, True)
    T, _kt = sets_to_device(torch, [ts], tcap, True)
    nn = torch.full((1, qcap, 3), SENT, dtype=torch.int32, device=DEV)
    rnn = torch.full((1, tcap, 2), SENT, dtype=torch.int32, device=DEV)
    matches = torch.full((1, qcap, 3), SENT, dtype=torch.int32, device=DEV)
    counts = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
    ctx.match_mutual(Q, T, 1, 0.64, same_octave, nn=nn, rnn=rnn, matches=matches, match_counts=counts)
    fnn = torch.full((1, qcap, 3), SENT, dtype=torch.int32, device=DEV)
    fm = torch.full((1, qcap, 3), SENT, dtype=torch.int32, device=DEV)
    fc = torch.full((1,), SENT, dtype=torch.int32, device=DEV)
    ctx.match(Q, T, 1, 0.64, same_octave, nn=fnn, matches=fm, match_counts=fc)
    bnn = torch.full((1, tcap, 3), SENT, dtype=torch.int32, device=DEV)
    ctx.match(T, Q, 1, 0.64, same_octave, nn=bnn)
    torch.cuda.synchronize()
    assert torch.equal(nn, fnn)
    assert torch.equal(rnn, bnn[:, :, :2])
    # ... and the list is the join of the two on the host
    f = fm.cpu().numpy()[0, :int(fc[0])].copy().view(capi.MATCH_DTYPE).reshape(-1)
    back = bnn.cpu().numpy()[0, :nt, 0]
    want = f[back[f["train"]] == f["query"]]
    assert int(counts[0]) == len(want) and matches.cpu().numpy()[0, :len(want)].tobytes() == want.tobytes() and 100 < len(want) < len(f)


def test_host_entry_point(env):
    ctx, torch = env
    (qd, qdf, qoc, nq), (td, tdf, toc, nt) = make_pair_m(np.random.default_rng(27), 150, 140, octaves=True)
    qp, tp = np.zeros(nq, capi.POINT_DTYPE), np.zeros(nt, capi.POINT_DTYPE)
    qp["octave"], tp["octave"] = qoc, toc
    for same_octave in (False, True):
        wnn, wrnn, wm = mutualref.mutual(qd, td, 0.64, same_octave, qdf, tdf, qoc, toc)
        nn, rnn, m, total = ctx.match_mutual_host(qd, td, 0.64, same_octave, qdf, tdf, qp, tp)
        assert nn.tobytes() == wnn.tobytes() and rnn.tobytes() == wrnn.tobytes() and m.tobytes() == wm.tobytes() and total == len(wm)
        nn, rnn, m, total = ctx.match_mutual_host(qd, td, 0.64, same_octave, qdf, tdf, qp, tp, match_cap=5)
        assert m.tobytes() == wm[:5].tobytes() and total == len(wm) > 5
    nn, rnn, m, total = ctx.match_mutual_host(np.zeros((0, 128), np.float32), td)
    assert len(nn) == 0 and total == 0 and (rnn["index"] == -1).all() and np.isposinf(rnn["dist2"]).all()
    nn, rnn, m, total = ctx.match_mutual_host(qd, np.zeros((0, 128), np.float32))
    assert (nn["index"] == -1).all() and np.isposinf(nn["dist2"]).all() and len(rnn) == 0 and total == 0


def test_cxx_wrapper_match_mutual(env, tmp_path):
    from tests.test_mutual_cpu import build_cxx_driver

    (qd, qdf, _, nq), (td, tdf, _, nt) = make_pair_m(np.random.default_rng(28), 200, 170)
    exe = build_cxx_driver(tmp_path)
    src, dst = tmp_path / "pair.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nq, nt], np.uint64).tobytes() + qd.tobytes() + td.tobytes() + qdf.tobytes() + tdf.tobytes())
    r = subprocess.run([exe, str(src), "0.8", str(dst)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    wnn, wrnn, wm = mutualref.mutual(qd, td, float(np.float32(0.8) * np.float32(0.8)), False, qdf, tdf)
    raw = open(dst, "rb").read()
    at = 0
    for want, size in ((wnn, 12), (wrnn, 8), (wm, 12)):
        k = int(np.frombuffer(raw, np.uint64, 1, at)[0])
        assert k == len(want) and raw[at + 8:at + 8 + k * size] == want.tobytes()
        at += 8 + k * size
    assert at == len(raw) and len(wm) > 50


@functools.lru_cache(maxsize=None)
def crops_cpu_chain():
    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    return (qp, tp) + mutualref.mutual(qd, td, 0.64, False, qk, tk)


def test_building_crops_end_to_end_detect_mutual_epipolar(env):
    ctx, torch = env
    qp, tp, wnn, wrnn, wm = crops_cpu_chain()
    assert (len(wm), exact_translations(wm, qp, tp, 24), mutualref.multiply_claimed(wm)) == (717, 710, (0, 0))  # the CPU chain alone
    model, flags, _ = epiref.ransac(wm, qp, tp, 512, 1, 4.0)
    # the device chain: detect -> mutual -> epipolar, nothing downloaded in between
    p, o = detect(ctx, torch, np.stack(building_crops()))
    cap = p.oriented_cap
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    nn = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    rnn = torch.zeros((1, cap, 2), dtype=torch.int32, device=DEV)
    matches = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.match_mutual(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, nn=nn, rnn=rnn, matches=matches,
                     match_counts=counts)
    models = torch.zeros((1, 22), dtype=torch.int32, device=DEV)
    inliers = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    icounts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models, inliers=inliers, inlier_counts=icounts)
    torch.cuda.synchronize()
    hc = c.cpu().numpy()
    assert (int(hc[0]), int(hc[1])) == (len(qp), len(tp))
    gm = matches.cpu().numpy()[0, :int(counts[0])].copy().view(capi.MATCH_DTYPE).reshape(-1)
    hp = pts.cpu().numpy().view(capi.POINT_DTYPE).reshape(2, cap)
    got = (len(gm), exact_translations(gm, hp[0], hp[1], 24), mutualref.multiply_claimed(gm))
    print("building crops: mutual accepted, exact translations, multiply claimed: gpu", got)
    assert got == (717, 710, (0, 0))
    assert gm.tobytes() == wm.tobytes() and nn.cpu().numpy()[0, :hc[0]].tobytes() == wnn.tobytes() and rnn.cpu().numpy()[0, :hc[1]].tobytes() == wrnn.tobytes()
    ge = models.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1)[0]
    gi = inliers.cpu().numpy()[0, :int(icounts[0])].copy().view(capi.MATCH_DTYPE).reshape(-1)
    assert ge.tobytes() == model[0].tobytes() and gi.tobytes() == wm[flags].tobytes() and int(ge["n_inliers"]) == int(flags.sum()) >= 710


def test_match_executable_with_mutual_reports_the_counts_of_the_python_path(env, tmp_path):
    ctx, torch = env
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(building_crops()):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--mutual", "--epipolar", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    p, o = detect(ctx, torch, np.stack(building_crops()))
    cap = p.oriented_cap
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    matches = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.match_mutual(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, matches=matches, match_counts=counts)
    models = torch.zeros((1, 22), dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models)
    torch.cuda.synchronize()
    gm = models.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1)[0]
    assert rep["mutual"] is True and rep["accepted"] == int(counts[0]) == 717
    e = rep["epipolar"]
    assert (e["n_inliers"], e["best"], e["n_valid"]) == (int(gm["n_inliers"]), int(gm["best"]), int(gm["n_valid"]))
    assert np.array(e["F"], np.float64).tobytes() == gm["F"].tobytes()
    r = subprocess.run([exe, paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)  # without the switch: the forward list, no "mutual"
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert "mutual" not in rep and rep["accepted"] == 730

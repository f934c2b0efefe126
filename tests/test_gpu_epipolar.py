"""Two-view geometry on the GPU (vslam_epipolar_dev / vslam_epipolar_host, include/vslam.h): every comparison is bytes-equal
against the CPU restatement of the arithmetic in tests/epiref.py - models, inlier_bits, inliers, inlier_counts and every
hypotheses row."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import epiref, matchref
from tests.test_gpu_match import building_crops, detect, oracle_chain
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def make_pair(seed, m, specials=True):
    """(matches [m], query points, train points): a planted scene (octaves 0 .. 2 and paddings 0 / 1 mixed); with `specials` two
    records share a train point and one record points past the query capacity."""
    mt, qp, tp, _ = epiref.planted_scene(seed, n=max(m, 8))
    mt = mt[:m].copy()
    if specials and m >= 9:
        mt["train"][1] = mt["train"][0]
        mt["query"][2] = len(qp) + 1000
    return mt, qp, tp


class Call:
    """One vslam_epipolar_dev call over host-side pairs: the padded arrays that go to the device, and the outputs pre-filled with
    a sentinel.  counts: what match_counts holds (default: each pair's record count)."""

    def __init__(self, torch, pairs, match_cap, pcap, H, inlier_cap=None, counts=None):
        n = len(pairs)
        self.n, self.match_cap, self.pcap, self.H = n, match_cap, pcap, H
        self.inlier_cap = match_cap if inlier_cap is None else inlier_cap
        rng = np.random.default_rng(n * 1000 + match_cap)
        self.matches = np.zeros((n, match_cap), capi.MATCH_DTYPE)
        self.matches["query"], self.matches["train"] = rng.integers(0, pcap, (n, match_cap)), rng.integers(0, pcap, (n, match_cap))  # past the counts: plausible records
        self.qp, self.tp = np.zeros((n, pcap), capi.POINT_DTYPE), np.zeros((n, pcap), capi.POINT_DTYPE)
        self.counts = np.zeros(n, np.int32)
        for j, (mt, qp, tp) in enumerate(pairs):
            k = min(len(mt), match_cap)
            self.matches[j, :k] = mt[:k]
            self.qp[j, :len(qp)], self.tp[j, :len(tp)] = qp, tp
            self.counts[j] = len(mt) if counts is None else counts[j]
        dev = lambda a, shape: torch.from_numpy(a.view(np.int32).reshape(shape)).to(DEV)
        self.d_in = (dev(self.matches, (n, match_cap, 3)), torch.from_numpy(self.counts).to(DEV), dev(self.qp, (n, pcap, 6)), dev(self.tp, (n, pcap, 6)))
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.fwords = (match_cap + 63) // 64
        # one row more than the call writes, everywhere: it keeps the sentinel
        self.out = dict(models=full((n + 1, 22), torch.int32), inlier_bits=full((n + 1, self.fwords), torch.int64),
                        inliers=full((n + 1, self.inlier_cap, 3), torch.int32), inlier_counts=full((n + 1,), torch.int32),
                        hypotheses=full((n + 1, H, 20), torch.int32))

    def run(self, ctx, torch, seed, max_dist2=4.0, only=None):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        ctx.epipolar(*self.d_in, n_pairs=self.n, n_hypotheses=self.H, seed=seed, max_dist2=max_dist2, **outs)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def want(self, j, seed, max_dist2=4.0, pair=None):
        """The restatement's answer for pair j: (model, flags, hypotheses, the records considered)."""
        k = min(int(self.counts[j]), self.match_cap)
        rec = self.matches[j, :k]
        model, flags, hyps = epiref.ransac(rec, self.qp[j], self.tp[j], self.H, seed, max_dist2, pair=j if pair is None else pair)
        return model, flags, hyps, rec

    def check(self, got, j, seed, max_dist2=4.0, pair=None):
        model, flags, hyps, rec = self.want(j, seed, max_dist2, pair)
        k = len(rec)
        gh = got["hypotheses"][j].view(capi.EPIPOLAR_HYP_DTYPE).reshape(-1)
        stage = [h for h in range(self.H) if gh[h].tobytes() != hyps[h].tobytes()]
        assert not stage, ("hypotheses", j, len(stage), stage[:4], gh[stage[0]], hyps[stage[0]])
        assert got["models"][j].tobytes() == model.tobytes(), ("models", j, got["models"][j].view(capi.EPIPOLAR_DTYPE), model)
        used = (k + 63) // 64
        assert got["inlier_bits"][j, :used].tobytes() == epiref.bits(flags, used).tobytes(), ("inlier_bits", j)
        assert (got["inlier_bits"][j, used:] == SENT).all(), "inlier_bits words past the count were written"
        inl = rec[flags]
        assert int(got["inlier_counts"][j]) == len(inl) == int(model["n_inliers"][0]), ("inlier_counts", j, int(got["inlier_counts"][j]), len(inl))
        c = min(len(inl), self.inlier_cap)
        assert got["inliers"][j, :c].tobytes() == inl[:c].tobytes(), ("inliers", j)
        assert (got["inliers"][j, c:] == SENT).all(), "inlier records past the count were written"
        return model, flags, hyps

    def check_rows_past_the_call(self, got):
        for name in ("models", "inlier_bits", "inliers", "inlier_counts", "hypotheses"):
            assert (got[name][self.n] == SENT).all(), name + ": the row past n_pairs was written"


@pytest.mark.parametrize("H", [1, 64, 65, 512])
@pytest.mark.parametrize("m", [0, 7, 8, 9, 63, 64, 65, 300, 1000])
def test_planted_pairs_equal_the_restatement(env, m, H):
    ctx, torch = env
    pair = make_pair(100 + m, m)
    call = Call(torch, [pair], max(m, 1) + 3, len(pair[1]) + 3, H)
    got = call.run(ctx, torch, seed=m + H)
    model, flags, hyps = call.check(got, 0, seed=m + H)
    call.check_rows_past_the_call(got)
    assert int(model["n_matches"][0]) == m
    if m < 8:
        assert int(model["best"][0]) == -1 and not hyps["valid"].any()
    if m >= 9:
        assert not flags[2]                                     # the record that points past the query capacity
    if m >= 300 and H == 512:
        assert int(model["best"][0]) >= 0 and int(model["n_inliers"][0]) > 0.55 * m   # 70 % planted


def test_counts_above_cap_and_a_small_inlier_cap(env):
    ctx, torch = env
    pair = make_pair(11, 300)
    call = Call(torch, [pair], 200, 303, 128, inlier_cap=17, counts=[100000])  # min(count, cap) records are considered
    got = call.run(ctx, torch, seed=5)
    model, flags, _ = call.check(got, 0, seed=5)
    assert int(model["n_matches"][0]) == 200 and int(got["inlier_counts"][0]) > 17  # the total is reported, the list is cut
    call.check_rows_past_the_call(got)


def test_forty_unequal_pairs_in_one_call_equal_forty_calls(env):
    ctx, torch = env
    rng = np.random.default_rng(40)
    pairs = [make_pair(200 + j, int(rng.integers(0, 301)), specials=(j % 3 == 0)) for j in range(40)]
    pairs[5], pairs[6] = make_pair(205, 7), make_pair(206, 0)
    call = Call(torch, pairs, 300, 310, 96, inlier_cap=64)
    whole = call.run(ctx, torch, seed=77)
    again = Call(torch, pairs, 300, 310, 96, inlier_cap=64).run(ctx, torch, seed=77)  # two runs of one call: byte-identical
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    call.check_rows_past_the_call(whole)
    for j in range(40):
        one = Call(torch, pairs[j:j + 1], 300, 310, 96, inlier_cap=64)
        got = one.run(ctx, torch, seed=77 + j)
        for k in whole:
            assert whole[k][j].tobytes() == got[k][0].tobytes(), (k, j)
    for j in (0, 5, 6, 21, 39):
        call.check(whole, j, seed=77)


def translation_pair(seed, n=730, wrong=20, shift=24):
    """An exact translation by `shift` pixels over mixed octaves, `wrong` of the train points replaced by random ones: the
    8-point matrix of a pure translation has rank 6, so most samples run out of pivots."""
    rng = np.random.default_rng(seed)
    octave = rng.integers(0, 3, n).astype(np.int32)
    qp, tp = np.zeros(n, capi.POINT_DTYPE), np.zeros(n, capi.POINT_DTYPE)
    qp["col"], qp["row"] = rng.integers(60, 1100, n) >> octave, rng.integers(60, 1100, n) >> octave
    qp["octave"] = tp["octave"] = octave
    tp["col"], tp["row"] = qp["col"] - ((2 * shift) >> octave), qp["row"] - ((2 * shift) >> octave)
    bad = rng.choice(n, wrong, replace=False)
    tp["col"][bad], tp["row"][bad] = rng.integers(0, 1100, wrong) >> octave[bad], rng.integers(0, 1100, wrong) >> octave[bad]
    mt = np.zeros(n, capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(n)
    true = np.ones(n, bool)
    true[bad] = False
    return (mt, qp, tp), true


def test_degenerate_pair_an_exact_translation(env):
    ctx, torch = env
    pair, true = translation_pair(4)
    call = Call(torch, [pair], 730, 730, 512)
    got = call.run(ctx, torch, seed=1)
    model, flags, hyps = call.check(got, 0, seed=1)
    print("translation: n_valid", int(model["n_valid"][0]), "inliers", int(model["n_inliers"][0]), "true found", int((flags & true).sum()))
    assert 0 < int(model["n_valid"][0]) < 512 and flags[true].all()           # the restatement
    gm = got["models"][0].view(capi.EPIPOLAR_DTYPE).reshape(-1)[0]
    gbits = np.unpackbits(got["inlier_bits"][0].view(np.uint8), bitorder="little")[:730].astype(bool)
    assert 0 < int(gm["n_valid"]) < 512 and gbits[true].all()                 # the GPU


def exact_translation_mask(m, qp, tp, shift):
    q, t = qp[m["query"]], tp[m["train"]]
    s = (2 * shift) >> q["octave"]
    return ((q["octave"] == t["octave"]) & (q["level"] == t["level"]) & (q["value"] == t["value"]) & (q["row"] - t["row"] == s) &
            (q["col"] - t["col"] == s))


def test_building_crops_end_to_end_like_the_cpu_chain(env):
    ctx, torch = env
    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    _, wm = matchref.match(qd, td, 0.64, False, qk, tk)
    exact = exact_translation_mask(wm, qp, tp, 24)
    model, flags, _ = epiref.ransac(wm, qp, tp, 512, 1, 4.0)
    assert (len(wm), int(exact.sum())) == (730, 710)
    print("building crops, CPU chain: n_valid", int(model["n_valid"][0]), "inliers", int(flags.sum()), "exact among them", int((flags & exact).sum()))
    assert flags[exact].all() and int(flags.sum()) == 719                # the CPU chain alone: every exact translation is an inlier
    # the device chain: detect -> match -> epipolar, nothing downloaded in between
    p, o = detect(ctx, torch, np.stack([a, b]))
    cap = p.oriented_cap
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    matches = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.match(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, matches=matches, match_counts=counts)
    models = torch.zeros((1, 22), dtype=torch.int32, device=DEV)
    inliers = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    icounts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models, inliers=inliers, inlier_counts=icounts)
    torch.cuda.synchronize()
    gm = models.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1)[0]
    gi = inliers.cpu().numpy()[0, :int(icounts[0])].copy().view(capi.MATCH_DTYPE).reshape(-1)
    assert gm.tobytes() == model[0].tobytes(), (gm, model[0])
    assert gi.tobytes() == wm[flags].tobytes()
    hp = pts.cpu().numpy().view(capi.POINT_DTYPE).reshape(2, cap)
    assert int(exact_translation_mask(gi, hp[0], hp[1], 24).sum()) == 710  # every exact-translation match is in the inlier list


def test_host_entry_point_and_optional_outputs(env):
    ctx, torch = env
    mt, qp, tp = make_pair(31, 300)
    model, flags, hyps = epiref.ransac(mt, qp, tp, 96, 9, 4.0)
    gm, bits, inl, total, gh = ctx.epipolar_host(mt, qp, tp, 96, 9, 4.0, want_hypotheses=True)
    assert gm.tobytes() == model[0].tobytes() and bits.tobytes() == epiref.bits(flags, 5).tobytes()
    assert inl.tobytes() == mt[flags].tobytes() and total == int(flags.sum()) and gh.tobytes() == hyps.tobytes()
    gm, bits, inl, total, gh = ctx.epipolar_host(mt, qp, tp, 96, 9, 4.0, inlier_cap=5)
    assert inl.tobytes() == mt[flags][:5].tobytes() and total == int(flags.sum()) and gh is None
    gm, bits, inl, total, gh = ctx.epipolar_host(mt, qp, tp, 96, 9, 4.0, want_bits=False, want_inliers=False)
    assert gm.tobytes() == model[0].tobytes() and bits is None and inl is None and total is None
    gm, bits, inl, total, gh = ctx.epipolar_host(mt[:0], qp, tp, 96, 9, 4.0)     # no records
    assert int(gm["best"]) == -1 and int(gm["n_matches"]) == 0 and total == 0 and len(bits) == 0
    # each optional output of the device entry alone, and none of them
    call = Call(torch, [(mt, qp, tp)], 303, 303, 96)
    want = call.run(ctx, torch, seed=9)
    call.check(want, 0, seed=9)
    for only in (("models",), ("models", "inlier_bits"), ("models", "inlier_counts"), ("models", "inliers", "inlier_counts"), ("models", "hypotheses")):
        alone = Call(torch, [(mt, qp, tp)], 303, 303, 96)
        got = alone.run(ctx, torch, seed=9, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == want[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    with pytest.raises(capi.VslamError):
        ctx.epipolar(*call.d_in, n_pairs=1, models=call.out["models"], inliers=call.out["inliers"])  # inliers without inlier_counts
    with pytest.raises(capi.VslamError):
        ctx.epipolar(*call.d_in, n_pairs=1, models=torch.zeros(21, dtype=torch.int32, device=DEV))  # undersized
    # the result depends neither on the f32-fused switch nor on the matrix-path switch
    ctx.set_f32_fused(True)
    ctx.set_matrix_path(True)
    got = Call(torch, [(mt, qp, tp)], 303, 303, 96).run(ctx, torch, seed=9)
    ctx.set_f32_fused(False)
    ctx.set_matrix_path(False)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_match_executable_reports_the_epipolar_counts_of_the_python_path(env, tmp_path):
    ctx, torch = env
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(building_crops()):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--epipolar", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    p, o = detect(ctx, torch, np.stack(building_crops()))
    cap = p.oriented_cap
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    matches = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.match(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, matches=matches, match_counts=counts)
    models = torch.zeros((1, 22), dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models)
    torch.cuda.synchronize()
    gm = models.cpu().numpy().view(capi.EPIPOLAR_DTYPE).reshape(-1)[0]
    assert rep["accepted"] == int(counts[0])
    e = rep["epipolar"]
    assert (e["n_inliers"], e["best"], e["n_valid"]) == (int(gm["n_inliers"]), int(gm["best"]), int(gm["n_valid"]))
    assert np.array(e["F"], np.float64).tobytes() == gm["F"].tobytes()   # printed with 17 significant digits: the same doubles

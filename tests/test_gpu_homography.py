"""Homography and the degeneracy verdict on the GPU (vslam_homography_dev / vslam_homography_host, include/vslam.h): every
comparison is bytes-equal against the CPU restatement of the arithmetic in tests/homref.py - models with their verdict,
inlier_bits, inliers, inlier_counts, every hypotheses row and the gated epipolar models - with sentinels intact past every
count."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import chainref, epiref, homref, matchref, poseref
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SENT = -77
OUTS = ("models", "inlier_bits", "inliers", "inlier_counts", "hypotheses", "gated_models")


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def make_pair(seed, m, specials=True, kind=None):
    """(matches [m], query points, train points): a planted scene of homref (the kind follows the seed unless given); with
    `specials` two records share a train point and one record points past the query capacity."""
    mt, qp, tp, _ = homref.planted_scene(seed, n=max(m, 8), kind=kind or homref.KINDS[seed % 3])
    mt = mt[:m].copy()
    if specials and m >= 9:
        mt["train"][1] = mt["train"][0]
        mt["query"][2] = len(qp) + 1000
    return mt, qp, tp


def epipolar_records(pairs, H, seed, d2=4.0):
    """The restatement's epipolar model of every pair, as the [n] EPIPOLAR_DTYPE array vslam_epipolar_dev would have written."""
    out = np.zeros(len(pairs), capi.EPIPOLAR_DTYPE)
    for j, (mt, qp, tp) in enumerate(pairs):
        out[j] = epiref.ransac(mt, qp, tp, H, seed, d2, pair=j)[0][0]
    return out


class Call:
    """One vslam_homography_dev call over host-side pairs: the padded arrays that go to the device, and the outputs pre-filled
    with a sentinel.  counts: what match_counts holds (default: each pair's record count).  epi: [n] EPIPOLAR_DTYPE or None."""

    def __init__(self, torch, pairs, match_cap, pcap, H, inlier_cap=None, counts=None, epi=None, verdict=(1, 2, 16)):
        n = len(pairs)
        self.n, self.match_cap, self.pcap, self.H, self.verdict = n, match_cap, pcap, H, verdict
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
        self.epi = None if epi is None else np.ascontiguousarray(epi, dtype=capi.EPIPOLAR_DTYPE).reshape(n)
        self.d_epi = None if epi is None else dev(self.epi, (n, 22))
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.fwords = (match_cap + 63) // 64
        # one row more than the call writes, everywhere: it keeps the sentinel
        self.out = dict(models=full((n + 1, 42), torch.int32), inlier_bits=full((n + 1, self.fwords), torch.int64),
                        inliers=full((n + 1, self.inlier_cap, 3), torch.int32), inlier_counts=full((n + 1,), torch.int32),
                        hypotheses=full((n + 1, H, 38), torch.int32), gated_models=full((n + 1, 22), torch.int32))

    def run(self, ctx, torch, seed, max_dist2=4.0, only=None, gated_in_place=False):
        outs = {k: v for k, v in self.out.items() if (only is None or k in only) and (k != "gated_models" or self.epi is not None)}
        if gated_in_place:
            outs["gated_models"] = self.d_epi
        num, den, mi = self.verdict
        ctx.homography(*self.d_in, n_pairs=self.n, n_hypotheses=self.H, seed=seed, max_dist2=max_dist2, degenerate_num=num, degenerate_den=den,
                       min_inliers=mi, epipolar_models=self.d_epi, **outs)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        if gated_in_place:
            got["gated_models"] = np.concatenate([self.d_epi.cpu().numpy(), got["gated_models"][self.n:]])
        return got

    def want(self, j, seed, max_dist2=4.0, pair=None):
        """The restatement's answer for pair j: (model with its verdict, flags, hypotheses, the records considered, gated record or None)."""
        k = min(int(self.counts[j]), self.match_cap)
        rec = self.matches[j, :k]
        model, flags, hyps = homref.ransac(rec, self.qp[j], self.tp[j], self.H, seed, max_dist2, pair=j if pair is None else pair)
        model = homref.verdict(model, None if self.epi is None else self.epi[j:j + 1], *self.verdict)
        return model, flags, hyps, rec, None if self.epi is None else homref.gate(self.epi[j:j + 1], model)

    def check(self, got, j, seed, max_dist2=4.0, pair=None):
        model, flags, hyps, rec, gated = self.want(j, seed, max_dist2, pair)
        k = len(rec)
        gh = got["hypotheses"][j].view(capi.HOMOGRAPHY_HYP_DTYPE).reshape(-1)
        stage = [h for h in range(self.H) if gh[h].tobytes() != hyps[h].tobytes()]
        assert not stage, ("hypotheses", j, len(stage), stage[:4], gh[stage[0]], hyps[stage[0]])
        assert got["models"][j].tobytes() == model.tobytes(), ("models", j, got["models"][j].view(capi.HOMOGRAPHY_DTYPE), model)
        used = (k + 63) // 64
        assert got["inlier_bits"][j, :used].tobytes() == epiref.bits(flags, used).tobytes(), ("inlier_bits", j)
        assert (got["inlier_bits"][j, used:] == SENT).all(), "inlier_bits words past the count were written"
        inl = rec[flags]
        assert int(got["inlier_counts"][j]) == len(inl) == int(model["n_inliers"][0]), ("inlier_counts", j, int(got["inlier_counts"][j]), len(inl))
        c = min(len(inl), self.inlier_cap)
        assert got["inliers"][j, :c].tobytes() == inl[:c].tobytes(), ("inliers", j)
        assert (got["inliers"][j, c:] == SENT).all(), "inlier records past the count were written"
        if gated is None:
            assert (got["gated_models"][j] == SENT).all()
        else:
            assert got["gated_models"][j].tobytes() == gated.tobytes(), ("gated_models", j, got["gated_models"][j].view(capi.EPIPOLAR_DTYPE), gated)
        return model, flags, hyps

    def check_rows_past_the_call(self, got):
        for name in OUTS:
            assert (got[name][self.n] == SENT).all(), name + ": the row past n_pairs was written"


@pytest.mark.parametrize("H", [1, 64, 65, 256, 257])
@pytest.mark.parametrize("m", [0, 3, 4, 5, 63, 64, 65, 255, 256, 257, 513])
def test_planted_pairs_equal_the_restatement(env, m, H):
    """The model workgroup (64), the score workgroup and the record tile (256) and their seams, each at a tight capacity and at
    one where the plan deals the record tiles to several workgroups per hypothesis block."""
    ctx, torch = env
    pair = make_pair(100 + m, m)
    epi = epipolar_records([pair], 64, 3)
    for cap in (max(m, 1) + 3, 1100):  # 1100: five record tiles, dealt to five workgroups per hypothesis block
        call = Call(torch, [pair], cap, len(pair[1]) + 3, H, epi=epi)
        got = call.run(ctx, torch, seed=m + H)
        model, flags, hyps = call.check(got, 0, seed=m + H)
        call.check_rows_past_the_call(got)
        assert int(model["n_matches"][0]) == m
        if m < 4:
            assert int(model["best"][0]) == -1 and not hyps["valid"].any() and int(model["degenerate"][0]) == 0
        if m >= 9:
            assert not flags[2]                                     # the record that points past the query capacity
    if m >= 255 and H >= 256 and (100 + m) % 3 != 0:
        assert int(model["best"][0]) >= 0 and int(model["n_inliers"][0]) > 0.55 * m   # 70 % planted on a plane / under a rotation


def test_counts_above_cap_and_a_small_inlier_cap(env):
    ctx, torch = env
    pair = make_pair(11, 300, kind="plane")
    call = Call(torch, [pair], 200, 303, 128, inlier_cap=17, counts=[100000])  # min(count, cap) records are considered
    got = call.run(ctx, torch, seed=5)
    model, flags, _ = call.check(got, 0, seed=5)
    assert int(model["n_matches"][0]) == 200 and int(got["inlier_counts"][0]) > 17  # the total is reported, the list is cut
    call.check_rows_past_the_call(got)


# ---- hostile fixtures

def lattice_pair(xq, xt, octave=1):
    """Records 0 .. n - 1 between lattice points given as integer (col, row) arrays at one octave."""
    n = len(xq)
    qp, tp = np.zeros(n, capi.POINT_DTYPE), np.zeros(n, capi.POINT_DTYPE)
    qp["col"], qp["row"], tp["col"], tp["row"] = xq[:, 0], xq[:, 1], xt[:, 0], xt[:, 1]
    qp["octave"] = tp["octave"] = octave
    mt = np.zeros(n, capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(n)
    return mt, qp, tp


def translation_pair(seed, n=730, wrong=20, shift=24):
    """An exact translation by `shift` pixels over mixed octaves, `wrong` of the train points replaced by random ones (the
    construction of tests/test_gpu_epipolar.py): F is degenerate here, H is the model."""
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


def hostile_pairs():
    rng = np.random.default_rng(7)
    out = {}
    # every record at one point: d == 0 on both sides
    out["one point"] = lattice_pair(np.full((40, 2), 100), np.full((40, 2), 90))
    # three of every four sample points collinear: all records but one on a line
    x = np.arange(40)
    q = np.stack([10 + 7 * x, 20 + 3 * x], axis=1)
    q[17] = (400, 31)
    out["collinear"] = lattice_pair(q, q + 5)
    # exactly 4 records, a proper quadrilateral under a scaling
    q = np.array([[10, 10], [200, 20], [220, 240], [30, 210]])
    out["four"] = lattice_pair(q, 2 * q + 3)
    # records that are not trusted interleaved: every other record has an octave past 31 on one side, or an index past a capacity
    mt, qp, tp = make_pair(5, 200, specials=False, kind="plane")
    qp, tp, mt = qp.copy(), tp.copy(), mt.copy()
    qp["octave"][mt["query"][0::4]] = 32
    tp["octave"][mt["train"][2::8]] = -1
    mt["train"][6::8] = len(tp) + 5
    out["untrusted"] = (mt, qp, tp)
    # records past the query capacity, among them the whole head of the list
    mt, qp, tp = make_pair(6, 150, specials=False, kind="rotation")
    mt = mt.copy()
    mt["query"][:40] = np.arange(40) + len(qp) + 3
    mt["query"][77] = -1
    out["past the capacity"] = (mt, qp, tp)
    # octave-31 coordinates: the pitch is 2^30
    q = rng.integers(-2000, 2000, (60, 2))
    mt, qp, tp = lattice_pair(q, q + 3, octave=31)
    qp["octave"][::5] = tp["octave"][::5] = 30
    qp["col"][::5] *= 2; qp["row"][::5] *= 2; tp["col"][::5] = qp["col"][::5] + 6; tp["row"][::5] = qp["row"][::5] + 6
    out["octave 31"] = (mt, qp, tp)
    # a planted H whose third coordinate p2 = x / 100 - 1 changes sign inside the image: records on both sides of the horizon
    # x = 100, and one on it (p2 == 0 exactly, its train point arbitrary)
    xq = np.stack([rng.integers(0, 400, 120), rng.integers(0, 300, 120)], axis=1)
    xq[:3] = [[100, 50], [101, 10], [99, 200]]
    p2 = xq[:, 0] / 100.0 - 1.0
    xt = np.where(p2[:, None] != 0, np.rint(xq / np.where(p2 == 0, 1, p2)[:, None]), 0).astype(np.int64)
    out["horizon"] = lattice_pair(xq, xt)
    out["translation"] = translation_pair(4)[0]
    return out


def test_hostile_fixtures_equal_the_restatement(env):
    ctx, torch = env
    pairs = hostile_pairs()
    names = list(pairs)
    seen = {}
    for name in names:
        mt, qp, tp = pairs[name]
        epi = epipolar_records([pairs[name]], 64, 2)
        call = Call(torch, [pairs[name]], len(mt) + 5, max(len(qp), len(tp)) + 2, 128, epi=epi)
        got = call.run(ctx, torch, seed=3)
        seen[name] = call.check(got, 0, seed=3)
        call.check_rows_past_the_call(got)
    model, flags, hyps = seen["one point"]
    assert int(model["best"][0]) == -1 and int(model["n_valid"][0]) == 0 and not model["H"].any()
    model, flags, hyps = seen["four"]
    assert int(model["best"][0]) >= 0 and flags.all() and int(model["n_valid"][0]) > 0
    assert np.abs(model["H"][0].reshape(3, 3) / model["H"][0][8] - [[2, 0, 3], [0, 2, 3], [0, 0, 1]]).max() < 1e-9
    model, flags, hyps = seen["untrusted"]
    mt, qp, tp = pairs["untrusted"]
    assert not flags[0::4].any() and not flags[6::8].any() and flags.any()
    assert 0 < int(model["n_valid"][0]) < 128                         # a sample with an untrusted record is invalid
    model, flags, hyps = seen["past the capacity"]
    assert not flags[:40].any() and not flags[77] and flags.any()
    model, flags, hyps = seen["octave 31"]
    assert int(model["best"][0]) >= 0 and flags.sum() >= 48             # the translation, at a pitch of 2^30
    model, flags, hyps = seen["horizon"]
    xq = pairs["horizon"][1]["col"].astype(np.int64)
    assert int(model["best"][0]) >= 0 and not flags[0]                  # the record on the horizon is nobody's inlier
    side = xq[flags] > 100
    assert flags.sum() >= 30 and (side.all() or not side.any())         # the inliers lie on one side of the horizon
    model, flags, hyps = seen["translation"]
    assert flags[translation_pair(4)[1]].all() and int(model["degenerate"][0]) == 1


def test_forty_unequal_pairs_in_one_call_equal_forty_calls(env):
    ctx, torch = env
    rng = np.random.default_rng(40)
    pairs = [make_pair(200 + j, int(rng.integers(0, 301)), specials=(j % 3 == 0)) for j in range(40)]
    pairs[5], pairs[6] = make_pair(205, 3), make_pair(206, 0)
    epi = epipolar_records(pairs, 96, 77)
    epi["best"][7], epi["best"][8] = -1, -1
    make = lambda ps, e: Call(torch, ps, 300, 310, 96, inlier_cap=64, epi=e)
    call = make(pairs, epi)
    whole = call.run(ctx, torch, seed=77)
    again = make(pairs, epi).run(ctx, torch, seed=77)  # two runs of one call: byte-identical
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    call.check_rows_past_the_call(whole)
    for j in range(40):
        got = make(pairs[j:j + 1], epi[j:j + 1]).run(ctx, torch, seed=77 + j)   # pair 0 of a call with seed + j samples like pair j
        for k in whole:
            assert whole[k][j].tobytes() == got[k][0].tobytes(), (k, j)
        call.check(whole, j, seed=77, pair=j)
    deg = whole["models"].view(capi.HOMOGRAPHY_DTYPE).reshape(-1)[:40]["degenerate"]
    assert deg.any() and not deg.all() and not deg[[5, 6, 7, 8]].any()


def test_each_optional_output_alone_and_the_gate_in_place(env):
    ctx, torch = env
    pair = make_pair(31, 300, kind="plane")
    epi = epipolar_records([pair], 96, 9)
    call = Call(torch, [pair], 303, 303, 96, epi=epi)
    want = call.run(ctx, torch, seed=9)
    model, _, _ = call.check(want, 0, seed=9)
    assert int(model["degenerate"][0]) == 1
    for only in (("models",), ("models", "inlier_bits"), ("models", "inlier_counts"), ("models", "inliers", "inlier_counts"), ("models", "hypotheses"),
                 ("models", "gated_models")):
        alone = Call(torch, [pair], 303, 303, 96, epi=epi)
        got = alone.run(ctx, torch, seed=9, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == want[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    # without epipolar models: no verdict, and nothing else changes
    bare = Call(torch, [pair], 303, 303, 96)
    got = bare.run(ctx, torch, seed=9)
    bare.check(got, 0, seed=9)
    gm = got["models"][0].view(capi.HOMOGRAPHY_DTYPE)[0]
    assert int(gm["degenerate"]) == 0 and int(gm["n_epipolar"]) == 0 and gm["H"].tobytes() == model["H"][0].tobytes()
    # the gate written onto the epipolar models themselves
    inplace = Call(torch, [pair], 303, 303, 96, epi=epi)
    got = inplace.run(ctx, torch, seed=9, gated_in_place=True)
    assert got["gated_models"][0].tobytes() == want["gated_models"][0].tobytes() and got["models"].tobytes() == want["models"].tobytes()
    with pytest.raises(capi.VslamError):
        ctx.homography(*call.d_in, n_pairs=1, models=call.out["models"], inliers=call.out["inliers"])  # inliers without inlier_counts
    with pytest.raises(capi.VslamError):
        ctx.homography(*call.d_in, n_pairs=1, models=torch.zeros(41, dtype=torch.int32, device=DEV))  # undersized
    with pytest.raises(capi.VslamError):
        ctx.homography(*call.d_in, n_pairs=1, models=call.out["models"], gated_models=call.out["gated_models"])  # the gate without epipolar models
    # the result depends neither on the f32-fused switch nor on the matrix-path switch
    ctx.set_f32_fused(True)
    ctx.set_matrix_path(True)
    got = Call(torch, [pair], 303, 303, 96, epi=epi).run(ctx, torch, seed=9)
    ctx.set_f32_fused(False)
    ctx.set_matrix_path(False)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_verdict_boundaries_on_the_device(env):
    ctx, torch = env
    pair = make_pair(32, 200, kind="rotation")
    nh = int(homref.ransac(*pair, 64, 4, 4.0)[0]["n_inliers"][0])
    assert 16 < nh < 200
    B = 2 ** 32 - 1
    cases = [  # (epipolar n_inliers, epipolar best), (num, den, min_inliers) -> degenerate
        ((100, 3), (nh, 100, 16), 1),           # the product equal
        ((101, 3), (nh, 100, 16), 0),           # ... and one short
        ((nh, 3), (1, 2, nh), 1),               # min_inliers equal
        ((nh, 3), (1, 2, nh + 1), 0),           # ... and one above
        ((nh, 3), (B, B, 0), 1),                # den near 2^32: the products need 64 bits
        ((nh + 1, 3), (B, B, 0), 0),
        ((nh + 1, 3), (2 ** 31, 2 ** 31 + 1, 0), 0),
        ((B, 0), (1, B, 0), int(nh >= 1)),
        ((B, 0), (nh + 1, B, 0), 0),
        ((nh, -1), (1, 2, 16), 0),              # no epipolar model
        ((0, 5), (0, 1, 0), 1),
    ]
    for (ne, eb), vd, want in cases:
        epi = np.zeros(1, capi.EPIPOLAR_DTYPE)
        epi["F"], epi["n_matches"], epi["n_inliers"], epi["best"], epi["n_valid"] = np.arange(9) + 1.0, 200, ne, eb, 33
        call = Call(torch, [pair], 203, 203, 64, epi=epi, verdict=vd)
        got = call.run(ctx, torch, seed=4)
        model, _, _ = call.check(got, 0, seed=4)
        gm = got["models"][0].view(capi.HOMOGRAPHY_DTYPE)[0]
        gg = got["gated_models"][0].view(capi.EPIPOLAR_DTYPE)[0]
        assert int(gm["degenerate"]) == want == int(model["degenerate"][0]), ((ne, eb), vd)
        assert int(gm["n_epipolar"]) == (ne if eb >= 0 else 0)
        if want:
            assert (int(gg["best"]), int(gg["n_inliers"]), int(gg["n_matches"]), int(gg["n_valid"])) == (-1, 0, 200, 33) and not gg["F"].any()
        else:
            assert gg.tobytes() == epi[0].tobytes()


def test_host_entry_point_equals_the_python_path(env):
    ctx, torch = env
    mt, qp, tp = make_pair(31, 300, kind="plane")
    model, flags, hyps = homref.ransac(mt, qp, tp, 96, 9, 4.0)
    epi = epipolar_records([(mt, qp, tp)], 96, 9)
    judged = homref.verdict(model, epi)
    gm, bits, inl, total, gh, gated = ctx.homography_host(mt, qp, tp, 96, 9, 4.0, epipolar_model=epi, want_hypotheses=True)
    assert gm.tobytes() == judged[0].tobytes() and bits.tobytes() == epiref.bits(flags, 5).tobytes()
    assert inl.tobytes() == mt[flags].tobytes() and total == int(flags.sum()) and gh.tobytes() == hyps.tobytes()
    assert gated.tobytes() == homref.gate(epi, judged)[0].tobytes() and int(gated["best"]) == -1
    gm, bits, inl, total, gh, gated = ctx.homography_host(mt, qp, tp, 96, 9, 4.0, inlier_cap=5)
    assert gm.tobytes() == model[0].tobytes() and inl.tobytes() == mt[flags][:5].tobytes() and total == int(flags.sum()) and gh is None and gated is None
    gm, bits, inl, total, gh, gated = ctx.homography_host(mt, qp, tp, 96, 9, 4.0, want_bits=False, want_inliers=False)
    assert gm.tobytes() == model[0].tobytes() and bits is None and inl is None and total is None
    gm, bits, inl, total, gh, gated = ctx.homography_host(mt[:0], qp, tp, 96, 9, 4.0)     # no records
    assert int(gm["best"]) == -1 and int(gm["n_matches"]) == 0 and total == 0 and len(bits) == 0


def test_cxx_wrapper_equals_the_python_path(env, tmp_path):
    """vslam::findHomography through a small driver: the same bytes."""
    mt, qp, tp = make_pair(31, 300, kind="plane")
    model, flags, _ = homref.ransac(mt, qp, tp, 96, 9, 4.0)
    epi = epipolar_records([(mt, qp, tp)], 96, 9)
    judged = homref.verdict(model, epi)
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    archive = os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a")
    assert os.path.exists(archive), "visualslam_amd/bin/libvslam_cxx.a is missing: __graft_entry__.build() builds it"
    exe = str(tmp_path / "homography_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "homography_cxx_driver.cpp"), archive,
                        "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = tmp_path / "pair.bin"
    with open(blob, "wb") as f:
        f.write(np.array([len(mt), len(qp), len(tp)], np.uint64).tobytes() + epi.tobytes() + mt.tobytes() + qp.tobytes() + tp.tobytes())
    r = subprocess.run([exe, str(blob), "96", "9", "4.0", "1", "2", "16", str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = open(tmp_path / "out.bin", "rb").read()
    assert out[:168] == judged[0].tobytes() and out[168:256] == homref.gate(epi, judged)[0].tobytes()
    assert out[256:] == np.array([int(flags.sum())], np.uint64).tobytes() + mt[flags].tobytes()


def test_match_executable_reports_the_homography_of_the_python_path(env, tmp_path):
    from tests.test_gpu_match import building_crops, oracle_chain

    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    _, wm = matchref.match(qd, td, 0.64, False, qk, tk)
    em, eflags, _ = epiref.ransac(wm, qp, tp, 512, 1, 4.0)
    hm, _, _ = homref.ransac(wm, qp, tp, 512, 1, 4.0)
    judged = homref.verdict(hm, em)[0]
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate((a, b)):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--epipolar", "--homography", "--refit", "4", "--pose", "800,800,288,288", paths[0], paths[1], "3"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    h = rep["homography"]
    assert (h["n_inliers"], h["best"], h["n_valid"], h["n_epipolar"], h["degenerate"]) == (int(judged["n_inliers"]), int(judged["best"]), int(judged["n_valid"]),
                                                                                         int(judged["n_epipolar"]), 1)
    assert np.array(h["H"], np.float64).tobytes() == judged["H"].tobytes()                  # 17 significant digits: the same doubles
    assert rep["epipolar"]["n_inliers"] == int(eflags.sum())
    # the steps after it read the gated model: the refit copies "no model" through, the pose stage gives no pose
    assert (rep["refit"]["stop"], rep["refit"]["n_after"], rep["refit"]["accepted"]) == (5, 0, 0) and not any(rep["refit"]["F"])
    assert (rep["pose"]["best"], rep["pose"]["valid"], rep["pose"]["n_front"]) == (-1, 0, 0)
    # without --homography nothing changes
    r = subprocess.run([exe, "--epipolar", "--pose", "800,800,288,288", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "homography" not in json.loads(r.stdout.strip().splitlines()[-1])


def test_building_crops_end_to_end_like_the_cpu_chain(env):
    """detect -> match -> epipolar -> homography -> pose on the gated models -> chain on the device, nothing downloaded in
    between, against the CPU chain of the restatements: the crops are a pure translation, the verdict says so, the pose stage
    gives the pair no pose and the chain starts a segment."""
    from tests.test_gpu_match import building_crops, detect, oracle_chain

    ctx, torch = env
    K = (800.0, 800.0, 288.0, 288.0)
    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    _, wm = matchref.match(qd, td, 0.64, False, qk, tk)
    em, eflags, _ = epiref.ransac(wm, qp, tp, 512, 1, 4.0)
    hm, hflags, _ = homref.ransac(wm, qp, tp, 512, 1, 4.0)
    judged = homref.verdict(hm, em)
    gated = homref.gate(em, judged)
    inl = wm[eflags]
    pose, _, front, X = poseref.pose(gated, inl, qp, tp, K)
    assert int(judged["degenerate"][0]) == 1 and int(pose["best"][0]) == -1 and X is None
    # the device chain
    p, o = detect(ctx, torch, np.stack([a, b]))
    cap = p.oriented_cap
    words = (cap + 63) // 64
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    matches, counts = z((1, cap, 3), torch.int32), z((1,), torch.int32)
    ctx.match(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, matches=matches, match_counts=counts)
    models, inliers, icounts = z((1, 22), torch.int32), z((1, cap, 3), torch.int32), z((1,), torch.int32)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models, inliers=inliers, inlier_counts=icounts)
    hmodels, hcounts, dgated = z((1, 42), torch.int32), z((1,), torch.int32), z((1, 22), torch.int32)
    ctx.homography(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, 1, 2, 16, epipolar_models=models, models=hmodels, inlier_counts=hcounts,
                   gated_models=dgated)
    dposes, dX, fb = z((1, 28), torch.int32), z((1, cap, 3), torch.float64), z((1, words), torch.int64)
    ctx.pose(dgated, inliers, icounts, pts[:1], pts[1:], K, poses=dposes, points=dX, front_bits=fb)
    full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
    out = dict(chain=full((2, 44), torch.int32))
    ctx.chain(dposes, inliers, icounts, dX, fb, cap, 16, n_pairs=1, **out)
    torch.cuda.synchronize()
    assert hmodels.cpu().numpy().tobytes() == judged.tobytes(), (hmodels.cpu().numpy().view(capi.HOMOGRAPHY_DTYPE), judged)
    assert int(hcounts[0]) == int(hflags.sum()) == 715
    assert models.cpu().numpy().tobytes() == em.tobytes() and dgated.cpu().numpy().tobytes() == gated.tobytes()
    assert dposes.cpu().numpy().tobytes() == pose.tobytes()
    k = len(inl)
    hmt, hbits = np.zeros((1, cap), capi.MATCH_DTYPE), np.zeros((1, words), np.uint64)
    hmt[0, :k] = inl
    want = chainref.chain(pose, hmt, np.array([k], np.uint32), np.zeros((1, cap, 3)), hbits, cap, 16)[0]
    got = out["chain"].cpu().numpy()
    assert got[:1].tobytes() == want.tobytes() and (got[1] == SENT).all()
    gc = got[:1].view(capi.CHAIN_DTYPE).reshape(-1)[0]
    assert (int(gc["valid"]), int(gc["linked"]), int(gc["segment"])) == (0, 0, 0)   # no pose: the pair stands alone in the trajectory

"""Pose from homography on the GPU (vslam_hpose_dev / vslam_hpose_host, include/vslam.h): every comparison is bytes-equal
against the CPU restatement of the arithmetic in tests/hposeref.py - info, all four candidates with their counts, the poses,
every point row and every ballot word - and every output carries sentinels: past every count, past the call, and across every
pair the call does not select."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import chainref, epiref, homref, hposeref
from tests.test_hpose_cpu import build_cxx_driver, ratio_boundaries
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77
K = hposeref.K_PLANTED
_MODELS = {}


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def planted_model(kind="plane"):
    """One homography of the planted cameras over the planted plane, or of the planted pure rotation (every planted_scene of a kind
    has the same cameras and the same plane), found once; judged degenerate."""
    if kind not in _MODELS:
        m, qp, tp, _ = homref.planted_scene(1, 300, kind)
        model = homref.ransac(m, qp, tp, 512, 7, 4.0)[0]
        model["degenerate"] = 1
        _MODELS[kind] = model
    return _MODELS[kind].copy()


def make_pair(seed, m, kind="plane", specials=True):
    """(matches [m], query points, train points) of a planted scene (octaves 0 .. 2 and paddings 0 / 1 mixed, 30 % wrong matches);
    with `specials`, from three records on, two share a train point and one points past the query capacity."""
    mt, qp, tp, _ = homref.planted_scene(seed, max(m, 8), kind)
    mt = mt[:m].copy()
    if specials and m >= 3:
        mt["train"][1] = mt["train"][0]
        mt["query"][2] = len(qp) + 1000
    return mt, qp, tp


class Call:
    """One vslam_hpose_dev call over host-side pairs (model [1], matches, query points, train points): the padded arrays that go
    to the device, and the outputs pre-filled with a sentinel, one row more than the call writes.  counts: what match_counts
    holds (default: each pair's record count); priors: [n] POSE_DTYPE or None."""

    def __init__(self, torch, pairs, match_cap, pcap, counts=None, priors=None):
        n = len(pairs)
        self.n, self.match_cap, self.pcap = n, match_cap, pcap
        rng = np.random.default_rng(n * 1000 + match_cap)
        self.matches = np.zeros((n, match_cap), capi.MATCH_DTYPE)
        self.matches["query"], self.matches["train"] = rng.integers(0, pcap, (n, match_cap)), rng.integers(0, pcap, (n, match_cap))  # past the counts: plausible records
        self.qp, self.tp = np.zeros((n, pcap), capi.POINT_DTYPE), np.zeros((n, pcap), capi.POINT_DTYPE)
        self.models = np.zeros(n, capi.HOMOGRAPHY_DTYPE)
        self.counts = np.zeros(n, np.int32)
        self.priors = priors
        for j, (model, mt, qp, tp) in enumerate(pairs):
            k = min(len(mt), match_cap)
            self.models[j] = np.asarray(model).reshape(-1)[0]
            self.matches[j, :k] = mt[:k]
            self.qp[j, :len(qp)], self.tp[j, :len(tp)] = qp, tp
            self.counts[j] = len(mt) if counts is None else counts[j]
        dev = lambda a, shape: torch.from_numpy(a.view(np.int32).reshape(shape)).to(DEV)
        self.d_in = (dev(self.models, (n, 42)), dev(self.matches, (n, match_cap, 3)), torch.from_numpy(self.counts).to(DEV), dev(self.qp, (n, pcap, 6)),
                     dev(self.tp, (n, pcap, 6)))
        self.d_priors = None if priors is None else dev(np.ascontiguousarray(priors), (n, 28))
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.fwords = (match_cap + 63) // 64
        self.out = dict(poses=full((n + 1, 28), torch.int32), info=full((n + 1, 36), torch.int32), candidates=full((n + 1, 4 * 32), torch.int32),
                        points=full((n + 1, match_cap, 3), torch.int64), front_bits=full((n + 1, self.fwords), torch.int64))

    def run(self, ctx, torch, intrinsics=K, only=None, **prm):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        ctx.hpose(*self.d_in, intrinsics, n_pairs=self.n, priors=self.d_priors, **prm, **outs)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def check(self, got, j, intrinsics=K, only_degenerate=True, **prm):
        """Pair j of `got` against the restatement; -> (info, cands, pose, flags, X), or None for a pair that is not selected."""
        k = min(int(self.counts[j]), self.match_cap)
        used = (k + 63) // 64
        if not hposeref.selected(self.models[j], only_degenerate):
            assert (got["poses"][j] == SENT).all() and (got["points"][j] == SENT).all() and (got["front_bits"][j] == SENT).all(), ("not selected", j)
            assert not got["info"][j].any() and not got["candidates"][j].any(), ("not selected", j)
            return None
        prior = None if self.priors is None else self.priors[j]
        info, cands, pose, flags, X = hposeref.pair(self.models[j], self.matches[j, :k], self.qp[j], self.tp[j], intrinsics, prior=prior, **prm)
        gc = got["candidates"][j].view(capi.HPOSE_CAND_DTYPE).reshape(-1)
        for c in range(4):
            assert gc[c].tobytes() == cands[c].tobytes(), ("candidates", j, c, gc[c], cands[c])
        assert got["info"][j].tobytes() == info.tobytes(), ("info", j, got["info"][j].view(capi.HPOSE_DTYPE), info)
        assert got["poses"][j].tobytes() == pose.tobytes(), ("poses", j, got["poses"][j].view(capi.POSE_DTYPE), pose)
        assert got["front_bits"][j, :used].tobytes() == epiref.bits(flags, used).tobytes(), ("front_bits", j)
        assert (got["front_bits"][j, used:] == SENT).all(), "front_bits words past the count were written"
        rows = 0
        if X is not None:
            rows = k
            bad = [i for i in range(k) if got["points"][j, i].tobytes() != X[i].tobytes()]
            assert not bad, ("points", j, len(bad), bad[:4], got["points"][j, bad[0]].view(np.float64), X[bad[0]])
        assert (got["points"][j, rows:] == SENT).all(), "point rows past the count (or of a pair without a pose) were written"
        return info, cands, pose, flags, X

    def check_rows_past_the_call(self, got):
        for name in self.out:
            assert (got[name][self.n] == SENT).all(), name + ": the row past n_pairs was written"


# ---- seams: the waves and the 256-record workgroups of the vote, and the words of front_bits

@pytest.mark.parametrize("m", [0, 1, 3, 4, 63, 64, 65, 255, 256, 257, 513])
def test_planted_planes_equal_the_restatement_at_the_seams(env, m):
    ctx, torch = env
    mt, qp, tp = make_pair(100 + m, m)
    if m >= 64:                       # an untrusted record on the seam: its point's octave is out of range
        qp = qp.copy()
        qp["octave"][mt["query"][m - 1 if m % 64 else 63]] = 40
    for cap in (max(m, 1), 1100):
        call = Call(torch, [(planted_model(), mt, qp, tp)], cap, len(qp) + 3)
        got = call.run(ctx, torch)
        info, cands, pose, flags, X = call.check(got, 0)
        call.check_rows_past_the_call(got)
        assert int(info["kind"][0]) == capi.HPOSE_PLANE and int(info["n_matches"][0]) == m
        if m >= 3 and X is not None:
            assert not flags[2] and np.isnan(X[2]).all()     # the record that points past the query capacity
        if m >= 63:
            assert int(pose["best"][0]) >= 0 and int(info["ambiguous"][0]) == 0 and int(pose["n_front"][0]) > 0.5 * m   # 70 % planted


def test_counts_above_cap(env):
    ctx, torch = env
    mt, qp, tp = make_pair(11, 300)
    call = Call(torch, [(planted_model(), mt, qp, tp)], 200, 303, counts=[100000])  # min(count, cap) records are considered
    got = call.run(ctx, torch)
    info, _, pose, _, X = call.check(got, 0)
    assert int(pose["n_matches"][0]) == 200 and int(info["n_matches"][0]) == 200 and len(X) == 200
    call.check_rows_past_the_call(got)


# ---- many pairs

def forty_pairs():
    """40 unequal pairs: planes, rotations (every fifth), and by hand a pair without records, one without a homography, one with H
    = 0 (NONE though selected), two that are not degenerate, and the ambiguous narrow plane."""
    rng = np.random.default_rng(40)
    pairs = []
    for j in range(40):
        m = int(rng.integers(0, 301))
        kind = "rotation" if j % 5 == 4 else "plane"
        pairs.append((planted_model(kind),) + make_pair(200 + j, m, kind, specials=j % 3 == 0))
    pairs[6] = (planted_model(),) + make_pair(206, 0)
    none = planted_model()
    none["best"] = -1
    pairs[9] = (none,) + make_pair(209, 130, specials=False)
    zero = planted_model()
    zero["H"], zero["G"] = 0.0, 0.0
    pairs[12] = (zero,) + make_pair(212, 70, specials=False)
    for j in (15, 31):
        general = planted_model()
        general["degenerate"] = 0
        pairs[j] = (general,) + pairs[j][1:]
    narrow = hposeref.narrow_plane()
    pairs[20] = (narrow[0], narrow[1], narrow[2], narrow[3])
    return pairs


@pytest.mark.parametrize("only_degenerate", [True, False])
def test_forty_unequal_pairs_in_one_call_equal_forty_calls(env, only_degenerate):
    ctx, torch = env
    pairs = forty_pairs()
    pcap = 1010
    call = Call(torch, pairs, 300, pcap)
    whole = call.run(ctx, torch, only_degenerate=only_degenerate)
    again = Call(torch, pairs, 300, pcap).run(ctx, torch, only_degenerate=only_degenerate)  # two runs of one call: byte-identical
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    call.check_rows_past_the_call(whole)
    kinds = []
    for j in range(40):
        got = Call(torch, pairs[j:j + 1], 300, pcap).run(ctx, torch, only_degenerate=only_degenerate)
        for k in whole:
            assert whole[k][j].tobytes() == got[k][0].tobytes(), (k, j)
        r = call.check(whole, j, only_degenerate=only_degenerate)
        kinds.append(None if r is None else (int(r[0]["kind"][0]), int(r[0]["ambiguous"][0]), int(r[2]["best"][0])))
    assert kinds[9] is None and (kinds[15] is None) == only_degenerate and (kinds[31] is None) == only_degenerate
    assert kinds[12] == (capi.HPOSE_NONE, 0, -1) and kinds[20] == (capi.HPOSE_PLANE, 1, -1) and kinds[6][2] == -1
    assert kinds[4][0] == capi.HPOSE_ROTATION and kinds[0][0] == capi.HPOSE_PLANE and kinds[0][2] >= 0
    p12 = whole["poses"][12].view(capi.POSE_DTYPE)[0]
    assert int(p12["best"]) == -1 and int(p12["valid"]) == 0 and int(p12["n_matches"]) == 70
    assert (whole["front_bits"][12, :2] == 0).all() and (whole["front_bits"][12, 2:] == SENT).all()


def test_the_holes_of_the_gate_are_filled_in_place_after_pose_dev(env):
    """The intended use: vslam_pose_dev over the gated models writes poses, points and front_bits on the device, vslam_hpose_dev
    fills the degenerate pairs into the same tensors, and the pairs F explains keep every byte."""
    ctx, torch = env
    n, cap = 6, 300
    lists, hom, epi = [], np.zeros(n, capi.HOMOGRAPHY_DTYPE), np.zeros(n, capi.EPIPOLAR_DTYPE)
    for j in range(n):
        kind = "plane" if j % 2 else "general"
        m, qp, tp, _ = homref.planted_scene(300 + j, cap, kind)
        lists.append((m, qp, tp))
        epi[j] = epiref.ransac(m, qp, tp, 512, 1, 4.0, pair=j)[0][0]
        hom[j] = homref.ransac(m, qp, tp, 512, 7, 4.0, pair=j)[0][0]
    hom = homref.verdict(hom, epi)
    gated = homref.gate(epi, hom)
    assert hom["degenerate"].tolist() == [0, 1, 0, 1, 0, 1]
    call = Call(torch, [(hom[j],) + lists[j] for j in range(n)], cap, cap)
    dgated = torch.from_numpy(gated.view(np.int32).reshape(n, 22)).to(DEV)
    outs = {k: call.out[k] for k in ("poses", "points", "front_bits")}
    ctx.pose(dgated, *call.d_in[1:], K, n_pairs=n, **outs)
    torch.cuda.synchronize()
    before = {k: v.cpu().numpy() for k, v in outs.items()}
    got = call.run(ctx, torch)
    for j in range(n):
        if j % 2 == 0:
            assert all(got[k][j].tobytes() == before[k][j].tobytes() for k in before), j
            assert before["poses"][j].view(capi.POSE_DTYPE)[0]["best"] >= 0 and not got["info"][j].any()
        else:
            assert before["poses"][j].view(capi.POSE_DTYPE)[0]["best"] == -1
            info, cands, pose, flags, X = hposeref.pair(hom[j], *lists[j], K)
            assert got["info"][j].tobytes() == info.tobytes() and got["poses"][j].tobytes() == pose.tobytes() and int(pose["best"][0]) >= 0
            assert got["points"][j].tobytes() == X.tobytes() and got["front_bits"][j].tobytes() == epiref.bits(flags, call.fwords).tobytes()
    call.check_rows_past_the_call(got)


# ---- hostile values

HOSTILE_NAMES = (["H zero", "H nan", "H inf", "H identity", "spread equal to min_spread", "spread one ulp below min_spread"] +
                 [f"intrinsic {pos} = {v:g}" for pos in range(4) for v in (1e-300, 1e300)] + ["octave 31", "a record on the horizon"] + list(hposeref.UNDERFLOW_A))
_HOSTILE = {}


def hostile_cases():
    """name -> ((model, matches, query points, train points), parameters), built at the first use (never at collection)."""
    if _HOSTILE:
        return _HOSTILE
    plane = make_pair(51, 130, specials=False)
    ident = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    cases = {}
    for name, fill in (("H zero", 0.0), ("H nan", np.nan), ("H inf", np.inf)):
        mod = planted_model()
        mod["H"], mod["G"] = fill, fill
        cases[name] = ((mod,) + plane, {})
    eye = hposeref.model_record(np.eye(3))                                  # K I K^-1 normalised: spread 0, R = I up to rounding
    cases["H identity"] = ((eye,) + plane, {})
    spread = float(hposeref.pair(planted_model()[0], *plane, K)[0]["spread"][0])
    cases["spread equal to min_spread"] = ((planted_model(),) + plane, dict(min_spread=spread))
    cases["spread one ulp below min_spread"] = ((planted_model(),) + plane, dict(min_spread=float(np.nextafter(spread, 1.0))))
    for pos in range(4):
        for v in (1e-300, 1e300):
            Kh = list(K)
            Kh[pos] = v
            cases[f"intrinsic {pos} = {v:g}"] = ((planted_model(),) + plane, dict(intrinsics=tuple(Kh)))
    far = tuple(a.copy() for a in plane)                                     # octave-31 coordinates: 2^30 pixels per unit
    far[1]["octave"][far[0]["query"][:40]] = 31
    far[2]["octave"][far[0]["train"][40:80]] = 31
    cases["octave 31"] = ((planted_model(),) + far, {})
    # a record on H's horizon: the third row of H vanishes at the pixel (1200, 500) exactly
    hor = planted_model()
    H = hor["H"][0].reshape(3, 3).copy()
    H[2] = [1.0 / 1024, 0.0, -1200.0 / 1024]
    hor["H"][0] = H.ravel()
    pts = tuple(a.copy() for a in plane)
    q0 = pts[0]["query"][0]
    pts[1]["col"][q0], pts[1]["row"][q0], pts[1]["octave"][q0], pts[1]["padding"][q0] = 1200, 500, 1, 0
    cases["a record on the horizon"] = ((hor,) + pts, {})
    for name in hposeref.UNDERFLOW_A:                                        # T = A n - R n cancels to zero exactly inside a PLANE pair
        cases[name] = (hposeref.underflow_pair(name), dict(intrinsics=(1.0, 1.0, 0.0, 0.0), min_spread=hposeref.UNDERFLOW_MIN_SPREAD))
    assert list(cases) == HOSTILE_NAMES
    _HOSTILE.update(cases)
    return _HOSTILE


@pytest.mark.parametrize("name", HOSTILE_NAMES)
def test_hostile_values_equal_the_restatement(env, name):
    ctx, torch = env
    pair, prm = hostile_cases()[name]
    call = Call(torch, [pair], 130, 133)
    kw = dict(prm)
    intrinsics = kw.pop("intrinsics", K)
    got = call.run(ctx, torch, intrinsics=intrinsics, **kw)
    info, cands, pose, flags, X = call.check(got, 0, intrinsics=intrinsics, **kw)
    call.check_rows_past_the_call(got)
    kind = int(info["kind"][0])
    if name in ("H zero", "H nan", "H inf"):
        assert kind == capi.HPOSE_NONE and not got["info"][0].any() and int(pose["best"][0]) == -1 and int(pose["n_matches"][0]) == 130
    if name == "H identity":
        assert kind == capi.HPOSE_ROTATION and float(info["spread"][0]) < 1e-12 and np.abs(info["R"][0] - np.eye(3).ravel()).max() < 1e-12
    if name == "spread equal to min_spread":
        assert kind == capi.HPOSE_PLANE and int(pose["best"][0]) >= 0
    if name == "spread one ulp below min_spread":
        assert kind == capi.HPOSE_ROTATION and int(pose["best"][0]) == -1
    if name in hposeref.UNDERFLOW_A:            # the zero half of "zero or not finite": one sign's candidates are invalid and never voted for
        valid = hposeref.UNDERFLOW_A[name][1]
        assert kind == capi.HPOSE_PLANE and cands["valid"].tolist() == valid and all(int(f) == 0 for f, v in zip(cands["front"], valid) if not v)
        assert (int(cands["front"].max()) > 0) == any(valid) and all(not cands[c].tobytes().strip(b"\0") for c in range(4) if not valid[c])
    # every NaN written is the quiet NaN
    for k, dt, fields in (("info", capi.HPOSE_DTYPE, ("R", "n", "inv_d", "spread")), ("candidates", capi.HPOSE_CAND_DTYPE, ("R", "t", "n")),
                          ("poses", capi.POSE_DTYPE, ("R", "t"))):
        rec = got[k][0].view(dt)
        for f in fields:
            v = np.ascontiguousarray(rec[f]).reshape(-1)
            assert (v.view(np.uint64)[np.isnan(v)] == 0x7FF8000000000000).all(), (k, f)


def test_the_ambiguity_rule_and_the_prior_on_the_device(env):
    ctx, torch = env
    narrow = hposeref.narrow_plane()
    pair = narrow[:4]
    base = hposeref.pair(narrow[0][0], *narrow[1:4], K)
    priors = np.zeros(6, capi.POSE_DTYPE)
    priors["R"][0], priors["best"][0] = narrow[4].ravel(), 0                 # the planted rotation
    priors["R"][1], priors["best"][1] = base[1]["R"][2], 2                    # the twin's
    priors["R"][2], priors["best"][2] = narrow[4].ravel(), -1                 # a prior without a pose
    priors["R"][3], priors["best"][3] = 0.0, 0                                # an exact tie of the two scores
    priors["R"][4], priors["best"][4] = np.nan, 0                             # NaN in R
    priors["R"][5], priors["best"][5] = narrow[4].ravel(), 1
    priors["R"][5][4] = np.nan
    call = Call(torch, [pair] * 6, 64, 64, priors=priors)
    got = call.run(ctx, torch)
    best = [int(call.check(got, j)[2]["best"][0]) for j in range(6)]
    assert best == [1, 2, -1, 1, 1, 1]
    call.check_rows_past_the_call(got)
    free = Call(torch, [pair], 64, 64)                                       # priors = NULL
    assert int(free.check(free.run(ctx, torch), 0)[2]["best"][0]) == -1
    # the boundaries of the ratio on a planted plane: products equal, one short, den near 2^32
    plane = (planted_model(),) + make_pair(1, 300, specials=False)
    info = hposeref.pair(plane[0][0], *plane[1:], K)[0]
    for num, den, want in ratio_boundaries(int(info["front"][0]), int(info["front_runner"][0])):
        c = Call(torch, [plane], 300, 300)
        r = c.check(c.run(ctx, torch, ambiguous_num=num, ambiguous_den=den), 0, num=num, den=den)
        assert int(r[0]["ambiguous"][0]) == want, (num, den)


# ---- interfaces

def test_each_optional_output_alone_the_host_entry_point_and_bad_arguments(env):
    ctx, torch = env
    pairs = [(planted_model(),) + make_pair(31, 300), (planted_model("rotation"),) + make_pair(32, 120, "rotation")]
    general = planted_model()
    general["degenerate"] = 0
    pairs.append((general,) + make_pair(33, 200))
    call = Call(torch, pairs, 303, 303)
    want = call.run(ctx, torch)
    for j in range(3):
        call.check(want, j)
    for only in (("poses", "info"), ("poses", "info", "candidates"), ("poses", "info", "points"), ("poses", "info", "front_bits")):
        got = Call(torch, pairs, 303, 303).run(ctx, torch, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == want[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    # the host entry point: the same bytes, and what the call leaves untouched keeps the caller's
    n, cap = 3, 303
    poses = np.frombuffer(np.full(n * 28, SENT, np.int32).tobytes(), capi.POSE_DTYPE).copy()
    pts, bits = np.full((n, cap, 3), SENT, np.int64), np.full((n, call.fwords), SENT, np.int64)
    info, cands = ctx.hpose_host(call.models, call.matches, call.counts, call.qp, call.tp, K, poses, points=pts.view(np.float64),
                                 front_bits=bits.view(np.uint64), want_candidates=True)
    assert info.tobytes() == want["info"][:n].tobytes() and cands.tobytes() == want["candidates"][:n].tobytes()
    assert poses.tobytes() == want["poses"][:n].tobytes() and pts.tobytes() == want["points"][:n].tobytes() and bits.tobytes() == want["front_bits"][:n].tobytes()
    with pytest.raises(capi.VslamError):
        ctx.hpose(*call.d_in, K, n_pairs=3, poses=call.out["poses"], info=torch.zeros(3 * 36 - 1, dtype=torch.int32, device=DEV))  # undersized
    for bad in (dict(min_spread=0.0), dict(max_dist2=float("nan")), dict(ambiguous_den=0)):
        with pytest.raises(capi.VslamError):
            ctx.hpose(*call.d_in, K, n_pairs=3, poses=call.out["poses"], info=call.out["info"], **bad)
    torch.cuda.synchronize()
    assert call.out["poses"].cpu().numpy().tobytes() == want["poses"].tobytes()   # a refused call writes nothing
    none = Call(torch, pairs, 303, 303)
    ctx.hpose(*none.d_in, K, n_pairs=0, **none.out)                              # no pairs: nothing is written
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == SENT).all() for v in none.out.values())


def cxx_pair_file(path, model, gated_pose, prior, mt, qp, tp):
    with open(path, "wb") as f:
        f.write(np.array([len(mt), len(qp), len(tp), 0 if prior is None else 1], np.uint64).tobytes() + np.asarray(model).tobytes() + gated_pose.tobytes() +
                (np.zeros(1, capi.POSE_DTYPE) if prior is None else np.asarray(prior)).tobytes() + mt.tobytes() + qp.tobytes() + tp.tobytes())


def test_cxx_wrapper_equals_the_restatement(env, tmp_path):
    """vslam::poseFromHomography through tests/hpose_cxx_driver.cpp: a planted plane, the ambiguous pair with and without a prior,
    a rotation, an empty list, and a pair that is not selected (its pose comes back as it went in)."""
    exe = build_cxx_driver(tmp_path)
    src, dst = tmp_path / "pair.bin", tmp_path / "out.bin"
    narrow = hposeref.narrow_plane()
    prior = np.zeros(1, capi.POSE_DTYPE)
    prior["R"][0], prior["best"] = narrow[4].ravel(), 0
    general = planted_model()
    general["degenerate"] = 0
    cases = [((planted_model(),) + make_pair(61, 200), None, 1), (narrow[:4], None, 1), (narrow[:4], prior, 1),
             ((planted_model("rotation"),) + make_pair(62, 90, "rotation"), None, 1), ((planted_model(),) + make_pair(63, 0), None, 1),
             ((general,) + make_pair(64, 100), None, 1), ((general,) + make_pair(64, 100), None, 0)]
    for (model, mt, qp, tp), pr, only in cases:
        m, words = len(mt), (len(mt) + 63) // 64
        gated = np.zeros(1, capi.POSE_DTYPE)
        gated["n_matches"], gated["best"], gated["valid"] = m, -1, 0
        cxx_pair_file(src, model, gated, pr, mt, qp, tp)
        r = subprocess.run([exe, str(src)] + [repr(v) for v in K] + [repr(capi.HPOSE_MIN_SPREAD), "9", "10", str(only), str(dst)], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
        raw = dst.read_bytes()
        ginfo, gcand, gpose, rest = raw[:144], raw[144:144 + 512], raw[656:768], raw[768:]
        npts = int(np.frombuffer(rest[:8], np.uint64)[0])
        gpts, rest = rest[8:8 + 8 * npts], rest[8 + 8 * npts:]
        nbits = int(np.frombuffer(rest[:8], np.uint64)[0])
        gbits = rest[8:]
        assert nbits == words and len(gbits) == 8 * words
        if not hposeref.selected(model, bool(only)):
            assert ginfo == bytes(144) and gcand == bytes(512) and gpose == gated.tobytes() and npts == 0 and gbits == bytes(8 * words)
            continue
        info, cands, pose, flags, X = hposeref.pair(model, mt, qp, tp, K, prior=pr)
        assert ginfo == info.tobytes() and gcand == cands.tobytes() and gpose == pose.tobytes()
        assert gbits == epiref.bits(flags, words).tobytes() and gpts == (b"" if X is None else X.tobytes())


def test_match_executable_prints_the_hpose_object(env):
    """Match --epipolar --homography --pose ... --hpose on two frames of the synthetic stream: the JSON line carries an "hpose" object
    whose fields are consistent with the "homography" and "pose" objects beside it."""
    capi.build()
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "visualslam_amd", "cxx")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Match")
    r = subprocess.run([exe, "--epipolar", "--homography", "--pose", "800,800,128,96", "--hpose", "256x192", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    hp, hom, pose = out["hpose"], out["homography"], out["pose"]
    assert set(hp) == {"kind", "best", "ambiguous", "n_support", "front", "front_runner", "pose_best", "pose_n_front"}
    selected = hom["best"] >= 0 and hom["degenerate"] == 1
    if not selected:                                             # the pose relativePose gave is left as it was
        assert hp["kind"] == capi.HPOSE_NONE and hp["n_support"] == 0 and hp["pose_best"] == pose["best"] and hp["pose_n_front"] == pose["n_front"]
    else:
        assert pose["best"] == -1 and hp["kind"] in (capi.HPOSE_NONE, capi.HPOSE_PLANE, capi.HPOSE_ROTATION) and hp["front_runner"] <= hp["front"] <= hp["n_support"]
        assert (hp["pose_best"] >= 0) == (hp["kind"] == capi.HPOSE_PLANE and hp["best"] >= 0 and not hp["ambiguous"])
        assert hp["pose_n_front"] <= hp["front"]
    r = subprocess.run([exe, "--epipolar", "--pose", "800,800,128,96", "--hpose", "256x192", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0                                     # --hpose needs --homography: the switch is not taken and the argument is no frame


def test_the_plane_scene_chains_into_one_segment_on_the_device(env):
    """The five-frame plane scene end to end on the device: vslam_pose_dev over the gated models, vslam_hpose_dev into the same
    tensors, vslam_chain_dev - bytes-equal to the CPU chain of the restatements, one segment of four linked pairs."""
    ctx, torch = env
    n = 300
    d = hposeref.plane_chain_inputs(3, n)
    poses, pts, bits = d["poses"].copy(), d["points"].copy(), d["bits"].copy()
    hposeref.fill(d["models"], d["matches"], d["counts"], d["query"], d["train"], K, poses, pts, bits)
    want = chainref.chain(poses, d["matches"], d["counts"], pts, bits, n, 16)[0]
    assert want["segment"].tolist() == [0, 0, 0, 0] and want["linked"].tolist() == [0, 1, 1, 1] and want["valid"].all()
    dev = lambda a, shape: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(shape)).to(DEV)
    words = (n + 63) // 64
    lists = (dev(d["matches"], (4, n, 3)), torch.from_numpy(d["counts"].astype(np.int32)).to(DEV), dev(d["query"], (4, n, 6)), dev(d["train"], (4, n, 6)))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    dposes, X, fb = z((4, 28), torch.int32), z((4, n, 3), torch.float64), z((4, words), torch.int64)
    ctx.pose(dev(d["gated"], (4, 22)), *lists, K, poses=dposes, points=X, front_bits=fb)
    dchain = z((4, 44), torch.int32)
    ctx.chain(dposes, lists[0], lists[1], X, fb, n, 16, chain=dchain)
    torch.cuda.synchronize()
    before = dchain.cpu().numpy().view(capi.CHAIN_DTYPE).reshape(-1)
    assert before["valid"].tolist() == [0, 0, 0, 0] and before["segment"].tolist() == [0, 1, 2, 3]
    ctx.hpose(dev(d["models"], (4, 42)), *lists, K, poses=dposes, info=z((4, 36), torch.int32), points=X, front_bits=fb)
    ctx.chain(dposes, lists[0], lists[1], X, fb, n, 16, chain=dchain)
    torch.cuda.synchronize()
    assert dposes.cpu().numpy().tobytes() == poses.tobytes() and fb.cpu().numpy().tobytes() == bits.tobytes() and X.cpu().numpy().tobytes() == pts.tobytes()
    assert dchain.cpu().numpy().tobytes() == want.tobytes(), (dchain.cpu().numpy().view(capi.CHAIN_DTYPE), want)


# ---- limits

def test_a_list_at_capacity(env):
    """40037 records under capacity 65536 (tests/limitcases.py's shape): 157 workgroups of the vote, the last one partial."""
    ctx, torch = env
    m = 40037
    mt, qp, tp = make_pair(77, m, specials=True)
    call = Call(torch, [(planted_model(), mt, qp, tp)], 65536, m + 5)
    got = call.run(ctx, torch)
    info, _, pose, _, _ = call.check(got, 0)
    call.check_rows_past_the_call(got)
    assert int(info["n_matches"][0]) == m and int(pose["best"][0]) >= 0 and int(info["n_support"][0]) > 0.6 * m


def test_1500_pairs_in_one_call(env):
    """Past 64 pairs per k_hpose_candidates workgroup and past 1024: 24 workgroups of pairs, the last one partial."""
    ctx, torch = env
    base = [(planted_model("rotation" if j % 7 == 3 else "plane"),) + make_pair(400 + j, 40 + 3 * j, "rotation" if j % 7 == 3 else "plane", specials=False)
            for j in range(12)]
    pairs = [base[j % 12] for j in range(1500)]
    skip = planted_model()
    skip["degenerate"] = 0
    pairs[1000] = (skip,) + base[0][1:]
    call = Call(torch, pairs, 80, 88)
    got = call.run(ctx, torch)
    call.check_rows_past_the_call(got)
    for j in range(12):
        call.check(got, j)
    assert call.check(got, 1000) is None
    for j in range(12, 1500):
        if j != 1000:
            assert all(got[k][j].tobytes() == got[k][j % 12].tobytes() for k in got), j

"""Relative pose and triangulation on the GPU (vslam_pose_dev / vslam_pose_host, include/vslam.h): every comparison is
bytes-equal against the CPU restatement of the arithmetic in tests/poseref.py - poses, all four candidates with their counts,
every point row and every ballot word."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import epiref, matchref, poseref
from tests.test_gpu_epipolar import make_pair
from tests.test_gpu_match import building_crops, detect, oracle_chain
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
K = (800.0, 800.0, 960.0, 540.0)
_MODEL = []


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def planted_model():
    """One fundamental matrix of the planted two-camera geometry (every planted_scene has the same two cameras), found once."""
    if not _MODEL:
        m, qp, tp, _ = epiref.planted_scene(1, 300)
        _MODEL.append(epiref.ransac(m, qp, tp, 512, 1, 4.0)[0])
    return _MODEL[0].copy()


def special_pair(seed, m):
    """make_pair's planted records; from three records on, two share a train point and one points past the query capacity."""
    mt, qp, tp = make_pair(seed, m, specials=False)
    if m >= 3:
        mt["train"][1] = mt["train"][0]
        mt["query"][2] = len(qp) + 1000
    return mt, qp, tp


class Call:
    """One vslam_pose_dev call over host-side pairs (model [1], matches, query points, train points): the padded arrays that go
    to the device, and the outputs pre-filled with a sentinel, one row more than the call writes.  counts: what match_counts
    holds (default: each pair's record count)."""

    def __init__(self, torch, pairs, match_cap, pcap, counts=None):
        n = len(pairs)
        self.n, self.match_cap, self.pcap = n, match_cap, pcap
        rng = np.random.default_rng(n * 1000 + match_cap)
        self.matches = np.zeros((n, match_cap), capi.MATCH_DTYPE)
        self.matches["query"], self.matches["train"] = rng.integers(0, pcap, (n, match_cap)), rng.integers(0, pcap, (n, match_cap))  # past the counts: plausible records
        self.qp, self.tp = np.zeros((n, pcap), capi.POINT_DTYPE), np.zeros((n, pcap), capi.POINT_DTYPE)
        self.models = np.zeros(n, capi.EPIPOLAR_DTYPE)
        self.counts = np.zeros(n, np.int32)
        for j, (model, mt, qp, tp) in enumerate(pairs):
            k = min(len(mt), match_cap)
            self.models[j] = np.asarray(model).reshape(-1)[0]
            self.matches[j, :k] = mt[:k]
            self.qp[j, :len(qp)], self.tp[j, :len(tp)] = qp, tp
            self.counts[j] = len(mt) if counts is None else counts[j]
        dev = lambda a, shape: torch.from_numpy(a.view(np.int32).reshape(shape)).to(DEV)
        self.d_in = (dev(self.models, (n, 22)), dev(self.matches, (n, match_cap, 3)), torch.from_numpy(self.counts).to(DEV), dev(self.qp, (n, pcap, 6)),
                     dev(self.tp, (n, pcap, 6)))
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.fwords = (match_cap + 63) // 64
        self.out = dict(poses=full((n + 1, 28), torch.int32), candidates=full((n + 1, 4 * 26), torch.int32),
                        points=full((n + 1, match_cap, 3), torch.int64), front_bits=full((n + 1, self.fwords), torch.int64))

    def run(self, ctx, torch, intrinsics=K, only=None):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        ctx.pose(*self.d_in, intrinsics, n_pairs=self.n, **outs)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def want(self, j, intrinsics=K):
        k = min(int(self.counts[j]), self.match_cap)
        return poseref.pose(self.models[j:j + 1], self.matches[j, :k], self.qp[j], self.tp[j], intrinsics) + (k,)

    def check(self, got, j, intrinsics=K):
        pose, cands, flags, X, k = self.want(j, intrinsics)
        gc = got["candidates"][j].view(capi.POSE_CAND_DTYPE).reshape(-1)
        for c in range(4):
            assert gc[c].tobytes() == cands[c].tobytes(), ("candidates", j, c, gc[c], cands[c])
        assert got["poses"][j].tobytes() == pose.tobytes(), ("poses", j, got["poses"][j].view(capi.POSE_DTYPE), pose)
        used = (k + 63) // 64
        assert got["front_bits"][j, :used].tobytes() == epiref.bits(flags, used).tobytes(), ("front_bits", j)
        assert (got["front_bits"][j, used:] == SENT).all(), "front_bits words past the count were written"
        rows = 0
        if X is not None:
            rows = k
            bad = [i for i in range(k) if got["points"][j, i].tobytes() != X[i].tobytes()]
            assert not bad, ("points", j, len(bad), bad[:4], got["points"][j, bad[0]].view(np.float64), X[bad[0]])
        assert (got["points"][j, rows:] == SENT).all(), "point rows past the count (or of a pair without a winner) were written"
        return pose, cands, flags, X

    def check_rows_past_the_call(self, got):
        for name in self.out:
            assert (got[name][self.n] == SENT).all(), name + ": the row past n_pairs was written"


@pytest.mark.parametrize("m", [0, 1, 7, 8, 63, 64, 65, 255, 256, 257, 300, 1000])
def test_planted_pairs_equal_the_restatement(env, m):
    ctx, torch = env
    mt, qp, tp = special_pair(100 + m, m)
    call = Call(torch, [(planted_model(), mt, qp, tp)], max(m, 1) + 3, len(qp) + 3)
    got = call.run(ctx, torch)
    pose, cands, flags, X = call.check(got, 0)
    call.check_rows_past_the_call(got)
    assert int(pose["n_matches"][0]) == m and int(pose["valid"][0]) == 1
    if m >= 3:
        assert not flags[2] and (X is None or np.isnan(X[2]).all())     # the record that points past the query capacity
    if m >= 63:
        assert int(pose["best"][0]) >= 0 and int(pose["n_front"][0]) > 0.5 * m   # 70 % planted


def test_counts_above_cap(env):
    ctx, torch = env
    mt, qp, tp = special_pair(11, 300)
    call = Call(torch, [(planted_model(), mt, qp, tp)], 200, 303, counts=[100000])  # min(count, cap) records are considered
    got = call.run(ctx, torch)
    pose, _, _, X = call.check(got, 0)
    assert int(pose["n_matches"][0]) == 200 and len(X) == 200
    call.check_rows_past_the_call(got)


def forty_pairs():
    rng = np.random.default_rng(40)
    pairs = []
    for j in range(40):
        m = int(rng.integers(0, 301))
        pairs.append((planted_model(),) + (special_pair(200 + j, m) if j % 3 == 0 else make_pair(200 + j, m, specials=False)))
    pairs[6] = (planted_model(),) + make_pair(206, 0)
    none = planted_model()
    none["best"] = -1                                                     # a pair without a model: F is not looked at
    pairs[9] = (none,) + make_pair(209, 130, specials=False)
    return pairs


def test_forty_unequal_pairs_in_one_call_equal_forty_calls(env):
    ctx, torch = env
    pairs = forty_pairs()
    call = Call(torch, pairs, 300, 310)
    whole = call.run(ctx, torch)
    again = Call(torch, pairs, 300, 310).run(ctx, torch)  # two runs of one call: byte-identical
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    call.check_rows_past_the_call(whole)
    for j in range(40):
        got = Call(torch, pairs[j:j + 1], 300, 310).run(ctx, torch)
        for k in whole:
            assert whole[k][j].tobytes() == got[k][0].tobytes(), (k, j)
    for j in (0, 5, 6, 9, 21, 39):
        call.check(whole, j)
    p9 = whole["poses"][9].view(capi.POSE_DTYPE)[0]
    assert int(p9["best"]) == -1 and int(p9["valid"]) == 0 and int(p9["n_matches"]) == 130
    assert (whole["front_bits"][9, :3] == 0).all() and (whole["front_bits"][9, 3:] == SENT).all() and (whole["points"][9] == SENT).all()
    p6 = whole["poses"][6].view(capi.POSE_DTYPE)[0]
    assert int(p6["best"]) == -1 and int(p6["valid"]) == 1 and int(p6["n_matches"]) == 0 and (whole["front_bits"][6] == SENT).all()


def test_each_optional_output_alone_and_bad_arguments(env):
    ctx, torch = env
    pair = (planted_model(),) + special_pair(31, 300)
    call = Call(torch, [pair], 303, 303)
    want = call.run(ctx, torch)
    call.check(want, 0)
    for only in (("poses",), ("poses", "candidates"), ("poses", "points"), ("poses", "front_bits")):
        got = Call(torch, [pair], 303, 303).run(ctx, torch, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == want[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    with pytest.raises(capi.VslamError):
        ctx.pose(*call.d_in, K, n_pairs=1, poses=torch.zeros(27, dtype=torch.int32, device=DEV))  # undersized
    for fx in (0.0, -800.0):
        with pytest.raises(capi.VslamError):
            ctx.pose(*call.d_in, (fx, 800.0, 960.0, 540.0), n_pairs=1, poses=call.out["poses"])
    torch.cuda.synchronize()
    assert call.out["poses"].cpu().numpy().tobytes() == want["poses"].tobytes()   # a refused call writes nothing


def translation_records(n_good, n_same):
    """Lattice records at octave 1 (pitch 1): n_good points moved by whole pixels along x - the exact images of a camera moved
    along x with K = identity - then n_same records that are identical in both frames."""
    rng = np.random.default_rng(5)
    n = n_good + n_same
    qp, tp = np.zeros(n, capi.POINT_DTYPE), np.zeros(n, capi.POINT_DTYPE)
    qp["octave"] = tp["octave"] = 1
    qp["col"], qp["row"] = rng.integers(-40, 40, n), rng.integers(-40, 40, n)
    tp["col"], tp["row"] = qp["col"], qp["row"]
    tp["col"][:n_good] += rng.integers(1, 9, n_good)
    mt = np.zeros(n, capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(n)
    return mt, qp, tp


def test_hostile_values_equal_the_restatement(env):
    ctx, torch = env
    mt, qp, tp = special_pair(77, 200)
    good = planted_model()
    nanF, zeroF = good.copy(), good.copy()
    nanF["F"][0, 4] = np.nan
    zeroF["F"][0] = 0.0
    call = Call(torch, [(nanF, mt, qp, tp), (zeroF, mt, qp, tp), (good, mt, qp, tp)], 203, 203)
    got = call.run(ctx, torch)
    for j in range(3):
        pose = call.check(got, j)[0]
        assert int(pose["valid"][0]) == (1 if j == 2 else 0)
    call.check_rows_past_the_call(got)
    # intrinsics at both ends of the exponent range, in every position
    for intr in ((1e-300, 1e-300, 960.0, 540.0), (1e300, 1e300, 960.0, 540.0), (1e-300, 800.0, 960.0, 540.0), (800.0, 1e300, 960.0, 540.0),
                 (800.0, 800.0, 1e300, -1e300), (800.0, 800.0, 1e-300, 1e-300), (1e-300, 1e-300, 1e300, 1e300), (1e300, 1e300, 1e-300, -1e-300)):
        one = Call(torch, [(good, mt, qp, tp)], 203, 203)
        one.check(one.run(ctx, torch, intr), 0, intr)
    # K = identity, a camera moved along x: E = [e0]x exactly, one of the two rotations is the identity exactly, and a record that
    # is identical in both frames has a == b there: det == 0 and n1 == n2 == 0, X = 0 / 0
    ident = (1.0, 1.0, 0.0, 0.0)
    E = good.copy()
    E["F"][0] = [0, 0, 0, 0, 0, -1, 0, 1, 0]
    same = translation_records(0, 150)            # every record identical in both frames
    mixed = translation_records(16, 150)          # ... and behind 16 records that give the identity rotation a winning vote
    call = Call(torch, [(E,) + same, (E,) + mixed], 170, 170)
    got = call.run(ctx, torch, ident)
    call.check(got, 0, ident)
    pose, cands, flags, X = call.check(got, 1, ident)
    assert int(pose["best"][0]) >= 0 and int(pose["n_front"][0]) == 16 and flags[:16].all() and not flags[16:].any()
    assert np.isnan(X[16:]).all() and np.isfinite(X[:16]).all()
    assert (got["points"][1, 16:166] == 0x7FF8000000000000).all()        # the canonical quiet NaN
    # octave 31: coordinates of 2^30 times the lattice index
    mt, qp, tp = special_pair(78, 100)
    qp["octave"], tp["octave"] = 31, 31
    call = Call(torch, [(good, mt, qp, tp)], 103, 103)
    call.check(call.run(ctx, torch), 0)


def test_host_entry_point_and_the_context_switches(env):
    ctx, torch = env
    model = planted_model()
    mt, qp, tp = special_pair(31, 300)
    pose, cands, flags, X = poseref.pose(model, mt, qp, tp, K)
    gp, gc, gx, gb = ctx.pose_host(model, mt, qp, tp, K)
    assert gp.tobytes() == pose[0].tobytes() and gc.tobytes() == cands.tobytes() and gx.tobytes() == X.tobytes()
    assert gb.tobytes() == epiref.bits(flags, 5).tobytes()
    gp, gc, gx, gb = ctx.pose_host(model, mt, qp, tp, K, want_candidates=False, want_points=False, want_bits=False)
    assert gp.tobytes() == pose[0].tobytes() and gc is None and gx is None and gb is None
    gp, gc, gx, gb = ctx.pose_host(model, mt[:0], qp, tp, K)             # no records: candidates, no winner
    assert int(gp["best"]) == -1 and int(gp["valid"]) == 1 and int(gp["n_matches"]) == 0 and gx is None and len(gb) == 0
    assert gc.tobytes() == poseref.candidates(model["F"][0], K).tobytes()
    # the device path gives the same bytes, whatever the f32-fused and the matrix-path switches say
    call = Call(torch, [(model, mt, qp, tp)], 303, 303)
    want = call.run(ctx, torch)
    call.check(want, 0)
    assert want["poses"][0].tobytes() == pose.tobytes()
    ctx.set_f32_fused(True)
    ctx.set_matrix_path(True)
    got = Call(torch, [(model, mt, qp, tp)], 303, 303).run(ctx, torch)
    hp = ctx.pose_host(model, mt, qp, tp, K)[0]
    ctx.set_f32_fused(False)
    ctx.set_matrix_path(False)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want) and hp.tobytes() == pose[0].tobytes()


def device_chain(ctx, torch):
    """detect -> match -> epipolar -> pose on the building crops, nothing downloaded in between; -> (pose, inlier count, points,
    bits) as numpy."""
    p, o = detect(ctx, torch, np.stack(building_crops()))
    cap = p.oriented_cap
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    matches = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.match(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, matches=matches, match_counts=counts)
    models = torch.zeros((1, 22), dtype=torch.int32, device=DEV)
    inliers = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    icounts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models, inliers=inliers, inlier_counts=icounts)
    poses = torch.zeros((1, 28), dtype=torch.int32, device=DEV)
    X = torch.full((1, cap, 3), SENT, dtype=torch.int64, device=DEV)
    bits = torch.full((1, (cap + 63) // 64), SENT, dtype=torch.int64, device=DEV)
    ctx.pose(models, inliers, icounts, pts[:1], pts[1:], K, poses=poses, points=X, front_bits=bits)
    torch.cuda.synchronize()
    return poses.cpu().numpy().view(capi.POSE_DTYPE).reshape(-1)[0], int(icounts[0]), X.cpu().numpy()[0], bits.cpu().numpy()[0]


def test_building_crops_end_to_end_like_the_cpu_chain(env):
    ctx, torch = env
    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    _, wm = matchref.match(qd, td, 0.64, False, qk, tk)
    model, flags, _ = epiref.ransac(wm, qp, tp, 512, 1, 4.0)
    inl = wm[flags]
    pose, cands, front, X = poseref.pose(model, inl, qp, tp, K)
    print("building crops, CPU chain: inliers", len(inl), "best", int(pose["best"][0]), "front", int(pose["n_front"][0]), "candidates", list(cands["front"]))
    gp, k, gx, gb = device_chain(ctx, torch)
    assert k == len(inl) == 719
    assert gp.tobytes() == pose[0].tobytes(), (gp, pose[0])
    used = (k + 63) // 64
    assert gb[:used].tobytes() == epiref.bits(front, used).tobytes() and (gb[used:] == SENT).all()
    if X is None:
        assert (gx == SENT).all()
    else:
        assert gx[:k].tobytes() == X.tobytes() and (gx[k:] == SENT).all()


def test_match_executable_reports_the_pose_of_the_python_path(env, tmp_path):
    ctx, torch = env
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(building_crops()):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--epipolar", "--pose", "800,800,960,540", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    gp, k, _, _ = device_chain(ctx, torch)
    e = rep["pose"]
    assert rep["epipolar"]["n_inliers"] == k == e["n_matches"]
    assert (e["n_front"], e["best"], e["valid"]) == (int(gp["n_front"]), int(gp["best"]), int(gp["valid"]))
    assert np.array(e["R"], np.float64).tobytes() == gp["R"].tobytes() and np.array(e["t"], np.float64).tobytes() == gp["t"].tobytes()   # 17 significant digits: the same doubles

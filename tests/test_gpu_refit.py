"""Least-squares refit of the fundamental matrix on the GPU (vslam_refit_dev / vslam_refit_host, include/vslam.h): every
comparison is bytes-equal against the CPU restatement of the arithmetic in tests/refitref.py - models, info records, every
ballot word, the inlier list and its total -, with sentinels intact past every count."""
import os
import subprocess

import numpy as np
import pytest

from tests import epiref, matchref, poseref, refitref
from tests.test_gpu_match import building_crops, detect, oracle_chain
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
K = (800.0, 800.0, 960.0, 540.0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


class Call:
    """One vslam_refit_dev call over host-side pairs (model [1], matches, query points, train points): the padded arrays that go
    to the device, and the outputs pre-filled with a sentinel, one row more than the call writes.  counts: what match_counts
    holds (default: each pair's record count)."""

    def __init__(self, torch, pairs, match_cap, pcap, counts=None, inlier_cap=None):
        n = len(pairs)
        self.n, self.match_cap, self.pcap = n, match_cap, pcap
        self.inlier_cap = match_cap if inlier_cap is None else inlier_cap
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
        self.out = dict(models=full((n + 1, 22), torch.int32), info=full((n + 1, 4), torch.int32), inlier_bits=full((n + 1, self.fwords), torch.int64),
                        inliers=full((n + 1, self.inlier_cap, 3), torch.int32), inlier_counts=full((n + 1,), torch.int32))

    def run(self, ctx, torch, rounds=4, max_dist2=4.0, only=None, in_place=False):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        if in_place:
            outs["models"] = self.d_in[0]
        ctx.refit(*self.d_in, n_pairs=self.n, rounds=rounds, max_dist2=max_dist2, **outs)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        if in_place:
            got["models"] = np.concatenate([self.d_in[0].cpu().numpy(), got["models"][self.n:]])
        return got

    def want(self, j, rounds=4, max_dist2=4.0):
        k = min(int(self.counts[j]), self.match_cap)
        return refitref.refit(self.models[j:j + 1], self.matches[j, :k], self.qp[j], self.tp[j], rounds, max_dist2)[:3] + (k,)

    def check(self, got, j, rounds=4, max_dist2=4.0):
        model, info, flags, k = self.want(j, rounds, max_dist2)
        assert got["models"][j].tobytes() == model.tobytes(), ("models", j, got["models"][j].view(capi.EPIPOLAR_DTYPE), model)
        assert got["info"][j].tobytes() == info.tobytes(), ("info", j, got["info"][j].view(capi.REFIT_DTYPE), info)
        used = (k + 63) // 64
        assert got["inlier_bits"][j, :used].tobytes() == epiref.bits(flags, used).tobytes(), ("inlier_bits", j)
        assert (got["inlier_bits"][j, used:] == SENT).all(), "inlier_bits words past the count were written"
        total = int(flags.sum())
        assert int(got["inlier_counts"][j]) == total, ("inlier_counts", j)
        rows = min(total, self.inlier_cap)
        assert got["inliers"][j, :rows].tobytes() == self.matches[j, :k][flags][:rows].tobytes(), ("inliers", j)
        assert (got["inliers"][j, rows:] == SENT).all(), "inlier rows past the total were written"
        return model, info[0], flags

    def check_rows_past_the_call(self, got):
        for name in self.out:
            assert (got[name][self.n] == SENT).all(), name + ": the row past n_pairs was written"


@pytest.mark.parametrize("m", [0, 7, 8, 9, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_seams_equal_the_restatement_at_two_capacities(env, m):
    """One pair at every seam of the ordered sum (slot, wave, block, more than one block), non-members and untrusted records
    interleaved; the same list under two capacities gives the same bytes: the sum depends on m and the terms only."""
    ctx, torch = env
    mt, qp, tp = refitref.seam_pair(100 + m, m)
    model = refitref.planted_model()
    outs = []
    for cap in (max(m, 1) + 3, max(m, 1) + 4096 + 77):
        call = Call(torch, [(model, mt, qp, tp)], cap, len(qp) + 3)
        got = call.run(ctx, torch)
        want, info, flags = call.check(got, 0)
        call.check_rows_past_the_call(got)
        outs.append((got["models"][0].tobytes(), got["info"][0].tobytes()))
    assert outs[0] == outs[1]
    assert int(want["n_matches"][0]) == int(model["n_matches"][0])            # copied from the input, like best and n_valid
    if m >= 63:
        assert 8 <= int(info["n_before"]) < m and int(info["n_after"]) >= int(info["n_before"]) and int(info["stop"]) in (0, 4)
    if m < 8:
        assert int(info["stop"]) == 1


def test_counts_above_cap(env):
    ctx, torch = env
    mt, qp, tp = refitref.seam_pair(11, 300)
    call = Call(torch, [(refitref.planted_model(), mt, qp, tp)], 200, 303, counts=[100000], inlier_cap=50)  # min(count, cap) records are considered
    got = call.run(ctx, torch)
    model, info, flags = call.check(got, 0)
    assert len(flags) == 200 and int(flags.sum()) > 50    # the total exceeds inlier_cap
    call.check_rows_past_the_call(got)


def test_hostile_values_reach_every_stop(env):
    """All members at one point (d == 0), best < 0, a NaN F, a zero F, exactly 8 members, a refit with fewer inliers, records past
    the query capacity, octave-31 coordinates.  The stops seen are 0, 1, 2, 4, 5: no input reaches stop 3 (the argument is in
    tests/test_refit_cpu.py, test_hostile_fixtures_stop_where_they_must)."""
    ctx, torch = env
    seen = set()
    for name, model, mt, qp, tp, d2, want in refitref.hostile_fixtures():
        call = Call(torch, [(model, mt, qp, tp)], len(mt) + 5, max(len(qp), len(tp)) + 2)
        got = call.run(ctx, torch, max_dist2=d2)
        _, info, flags = call.check(got, 0, max_dist2=d2)
        call.check_rows_past_the_call(got)
        assert want is None or int(info["stop"]) == want, (name, info)
        seen.add(int(info["stop"]))
        if name == "no model":
            assert got["models"][0].tobytes() == np.asarray(model).tobytes()
        if name == "exactly eight":
            assert int(info["n_before"]) == 8
    assert seen == {0, 1, 2, 4, 5}


def forty_pairs():
    rng = np.random.default_rng(40)
    pairs = []
    for j in range(40):
        m = int(rng.integers(0, 301))
        pairs.append((refitref.planted_model(),) + refitref.seam_pair(200 + j, m))
    pairs[6] = (refitref.planted_model(),) + refitref.seam_pair(206, 0)
    none = refitref.planted_model()
    none["best"] = -1
    pairs[9] = (none,) + refitref.seam_pair(209, 130)
    pairs[12] = refitref.one_point_pair()
    mt, qp, tp = refitref.seam_pair(213, 5000)                                  # one pair with two blocks among the short ones
    pairs[13] = (refitref.planted_model(), mt, qp[:300], tp[:300])              # ... most of its records past the capacities
    return pairs


def test_forty_unequal_pairs_in_one_call_equal_forty_calls(env):
    ctx, torch = env
    pairs = forty_pairs()
    call = Call(torch, pairs, 5000, 310)
    whole = call.run(ctx, torch)
    again = Call(torch, pairs, 5000, 310).run(ctx, torch)  # two runs of one call: byte-identical
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    call.check_rows_past_the_call(whole)
    for j in range(40):
        got = Call(torch, pairs[j:j + 1], 5000, 310).run(ctx, torch)
        for k in whole:
            assert whole[k][j].tobytes() == got[k][0].tobytes(), (k, j)
    stops = [int(call.check(whole, j)[1]["stop"]) for j in range(40)]
    assert stops[9] == 5 and stops[6] == 1 and stops[12] == 2 and stops[0] in (0, 4)


@pytest.mark.parametrize("rounds", [1, 2, 8])
def test_rounds(env, rounds):
    ctx, torch = env
    m8, q8, t8, _ = epiref.planted_scene(8, 1000)
    pairs = [(refitref.planted_model(),) + refitref.seam_pair(31, 300), (epiref.ransac(m8, q8, t8, 512, 8, 4.0)[0], m8, q8, t8)]
    call = Call(torch, pairs, 1003, 1003)
    got = call.run(ctx, torch, rounds=rounds)
    info = [call.check(got, j, rounds=rounds)[1] for j in range(2)]
    assert int(info[0]["accepted"]) <= rounds and int(info[1]["stop"]) == 4 and int(info[1]["accepted"]) == 0


def test_each_optional_output_alone_in_place_and_bad_arguments(env):
    ctx, torch = env
    pair = (refitref.planted_model(),) + refitref.seam_pair(31, 300)
    call = Call(torch, [pair], 303, 303)
    want = call.run(ctx, torch)
    call.check(want, 0)
    for only in (("models",), ("models", "info"), ("models", "inlier_bits"), ("models", "inlier_counts"), ("models", "inliers", "inlier_counts")):
        got = Call(torch, [pair], 303, 303).run(ctx, torch, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == want[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    # models aliased onto the input
    alias = Call(torch, [pair], 303, 303)
    got = alias.run(ctx, torch, in_place=True)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    with pytest.raises(capi.VslamError):
        ctx.refit(*call.d_in, n_pairs=1, models=torch.zeros(21, dtype=torch.int32, device=DEV))  # undersized
    for rounds, d2 in ((0, 4.0), (9, 4.0), (4, 0.0), (4, float("nan"))):
        with pytest.raises(capi.VslamError):
            ctx.refit(*call.d_in, n_pairs=1, rounds=rounds, max_dist2=d2, models=call.out["models"])
    torch.cuda.synchronize()
    assert call.out["models"].cpu().numpy().tobytes() == want["models"].tobytes()   # a refused call writes nothing


def test_host_entry_point_and_the_cxx_wrapper(env, tmp_path):
    ctx, torch = env
    model = refitref.planted_model()
    mt, qp, tp = refitref.seam_pair(31, 300)
    want, info, flags, _ = refitref.refit(model, mt, qp, tp, 4, 4.0)
    gm, gi, gb, gl, total = ctx.refit_host(model, mt, qp, tp, 4, 4.0)
    assert gm.tobytes() == want[0].tobytes() and gi.tobytes() == info[0].tobytes() and gb.tobytes() == epiref.bits(flags, 5).tobytes()
    assert total == int(flags.sum()) and gl.tobytes() == mt[flags].tobytes()
    gm, gi, gb, gl, total = ctx.refit_host(model, mt, qp, tp, 4, 4.0, want_bits=False, want_inliers=False)
    assert gm.tobytes() == want[0].tobytes() and gb is None and gl is None and total is None
    gm, gi, gb, gl, total = ctx.refit_host(model, mt[:0], qp, tp, 4, 4.0)            # no records: fewer than 8 members
    assert int(gi["stop"]) == 1 and int(gi["n_before"]) == 0 and total == 0 and gm["F"].tobytes() == model["F"][0].tobytes()
    # the C++ wrapper (vslam::refitFundamental) through a small driver: the same bytes
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    archive = os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a")
    assert os.path.exists(archive), "visualslam_amd/bin/libvslam_cxx.a is missing: __graft_entry__.build() builds it"
    exe = str(tmp_path / "refit_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "refit_cxx_driver.cpp"), archive,
                        "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = tmp_path / "pair.bin"
    with open(blob, "wb") as f:
        f.write(np.array([len(mt), len(qp), len(tp)], np.uint64).tobytes() + np.asarray(model).tobytes() + mt.tobytes() + qp.tobytes() + tp.tobytes())
    r = subprocess.run([exe, str(blob), "4", "4.0", str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = open(tmp_path / "out.bin", "rb").read()
    assert out[:88] == want[0].tobytes() and out[88:104] == info[0].tobytes()
    assert out[104:] == np.array([int(flags.sum())], np.uint64).tobytes() + mt[flags].tobytes()


@pytest.fixture(scope="module")
def cpu_chain():
    """The building crops through the restatements, once: match -> RANSAC -> refit (4 rounds) -> pose."""
    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    _, wm = matchref.match(qd, td, 0.64, False, qk, tk)
    model, flags, _ = epiref.ransac(wm, qp, tp, 512, 1, 4.0)
    refit, info, rflags, _ = refitref.refit(model, wm, qp, tp, 4, 4.0)
    pose = poseref.pose(refit, wm[rflags], qp, tp, K)[0]
    print("building crops, CPU chain: inliers", int(flags.sum()), "->", int(rflags.sum()), "info", info[0], "front", int(pose["n_front"][0]))
    return wm, flags, refit, info, rflags, pose


def test_building_crops_end_to_end_like_the_cpu_chain(env, cpu_chain):
    """detect -> match -> epipolar -> refit -> pose on the device, nothing downloaded in between, against the chain of the
    restatements."""
    ctx, torch = env
    wm, flags, refit, info, rflags, pose = cpu_chain
    p, o = detect(ctx, torch, np.stack(building_crops()))
    cap = p.oriented_cap
    d, c, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    matches = torch.zeros((1, cap, 3), dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.match(capi.desc_sets(d[:1], c[:1], df[:1]), capi.desc_sets(d[1:], c[1:], df[1:]), 1, 0.64, False, matches=matches, match_counts=counts)
    models = torch.zeros((1, 22), dtype=torch.int32, device=DEV)
    ctx.epipolar(matches, counts, pts[:1], pts[1:], 1, 512, 1, 4.0, models=models)
    rinfo = torch.zeros((1, 4), dtype=torch.int32, device=DEV)
    inliers = torch.full((1, cap, 3), SENT, dtype=torch.int32, device=DEV)
    icounts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.refit(models, matches, counts, pts[:1], pts[1:], 1, 4, 4.0, models=models, info=rinfo, inliers=inliers, inlier_counts=icounts)  # in place
    poses = torch.zeros((1, 28), dtype=torch.int32, device=DEV)
    ctx.pose(models, inliers, icounts, pts[:1], pts[1:], K, poses=poses)
    torch.cuda.synchronize()
    k = int(icounts[0])
    assert models.cpu().numpy().tobytes() == refit.tobytes() and rinfo.cpu().numpy().tobytes() == info.tobytes()
    assert k == int(rflags.sum()) >= int(flags.sum())
    gi = inliers.cpu().numpy()[0]
    assert gi[:k].tobytes() == wm[rflags].tobytes() and (gi[k:] == SENT).all()
    assert poses.cpu().numpy().tobytes() == pose.tobytes()


def test_match_executable_reports_the_refit_of_the_python_path(env, cpu_chain, tmp_path):
    import json

    wm, flags, refit, info, rflags, pose = cpu_chain
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(building_crops()):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--epipolar", "--refit", "4", "--pose", "800,800,960,540", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    e, i = rep["refit"], info[0]
    assert (e["rounds"], e["n_before"], e["n_after"], e["accepted"], e["stop"]) == (4, int(i["n_before"]), int(i["n_after"]), int(i["accepted"]), int(i["stop"]))
    assert np.array(e["F"], np.float64).tobytes() == refit["F"][0].tobytes()                    # 17 significant digits: the same doubles
    assert rep["epipolar"]["n_inliers"] == int(flags.sum()) and rep["pose"]["n_matches"] == int(rflags.sum())
    assert np.array(rep["pose"]["R"], np.float64).tobytes() == pose["R"][0].tobytes() and np.array(rep["pose"]["t"], np.float64).tobytes() == pose["t"][0].tobytes()
    bad = subprocess.run([exe, "--epipolar", "--refit", "9", "64x48"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "1 .. 8" in bad.stderr

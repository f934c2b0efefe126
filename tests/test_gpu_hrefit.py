"""Least-squares refit of the homography on the GPU (vslam_hrefit_dev / vslam_hrefit_host, include/vslam.h): every comparison is
bytes-equal against the CPU restatement of the arithmetic in tests/hrefitref.py - models with the verdict, info records, every
ballot word, the inlier list and its total, the gate -, with sentinels intact past every count."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import epiref, guidedhfref, homref, hposeref, hrefitref, matchref, poseref
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
K = hposeref.K_PLANTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


class Call:
    """One vslam_hrefit_dev call over host-side pairs (model [1], matches, query points, train points): the padded arrays that go
    to the device, and the outputs pre-filled with a sentinel, one row more than the call writes.  counts: what match_counts
    holds (default: each pair's record count); epi: the EPIPOLAR_DTYPE records of the verdict, or None."""

    def __init__(self, torch, pairs, match_cap, pcap, counts=None, inlier_cap=None, epi=None):
        n = len(pairs)
        self.n, self.match_cap, self.pcap = n, match_cap, pcap
        self.inlier_cap = match_cap if inlier_cap is None else inlier_cap
        rng = np.random.default_rng(n * 1000 + match_cap)
        self.matches = np.zeros((n, match_cap), capi.MATCH_DTYPE)
        self.matches["query"], self.matches["train"] = rng.integers(0, pcap, (n, match_cap)), rng.integers(0, pcap, (n, match_cap))  # past the counts: plausible records
        self.qp, self.tp = np.zeros((n, pcap), capi.POINT_DTYPE), np.zeros((n, pcap), capi.POINT_DTYPE)
        self.models = np.zeros(n, capi.HOMOGRAPHY_DTYPE)
        self.counts = np.zeros(n, np.int32)
        self.epi = None if epi is None else np.ascontiguousarray(epi, dtype=capi.EPIPOLAR_DTYPE).reshape(n).copy()
        for j, (model, mt, qp, tp) in enumerate(pairs):
            k = min(len(mt), match_cap)
            self.models[j] = np.asarray(model).reshape(-1)[0]
            self.matches[j, :k] = mt[:k]
            self.qp[j, :len(qp)], self.tp[j, :len(tp)] = qp, tp
            self.counts[j] = len(mt) if counts is None else counts[j]
        dev = lambda a, shape: torch.from_numpy(a.view(np.int32).reshape(shape)).to(DEV)
        self.d_in = (dev(self.models, (n, 42)), dev(self.matches, (n, match_cap, 3)), torch.from_numpy(self.counts).to(DEV), dev(self.qp, (n, pcap, 6)),
                     dev(self.tp, (n, pcap, 6)))
        self.d_epi = None if self.epi is None else dev(self.epi, (n, 22))
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.fwords = (match_cap + 63) // 64
        self.out = dict(models=full((n + 1, 42), torch.int32), info=full((n + 1, 4), torch.int32), inlier_bits=full((n + 1, self.fwords), torch.int64),
                        inliers=full((n + 1, self.inlier_cap, 3), torch.int32), inlier_counts=full((n + 1,), torch.int32))
        if self.epi is not None:
            self.out["gated_models"] = full((n + 1, 22), torch.int32)

    def run(self, ctx, torch, rounds=4, max_dist2=4.0, only=None, in_place=False, gate_in_place=False, **verdict):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        if in_place:
            outs["models"] = self.d_in[0]
        if gate_in_place:
            outs["gated_models"] = self.d_epi
        ctx.hrefit(*self.d_in, n_pairs=self.n, rounds=rounds, max_dist2=max_dist2, epipolar_models=self.d_epi, **verdict, **outs)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        if in_place:
            got["models"] = np.concatenate([self.d_in[0].cpu().numpy(), got["models"][self.n:]])
        if gate_in_place:
            got["gated_models"] = np.concatenate([self.d_epi.cpu().numpy(), got["gated_models"][self.n:]])
        return got

    def want(self, j, rounds=4, max_dist2=4.0, **verdict):
        k = min(int(self.counts[j]), self.match_cap)
        epi = None if self.epi is None else self.epi[j:j + 1]
        return hrefitref.hrefit(self.models[j:j + 1], self.matches[j, :k], self.qp[j], self.tp[j], rounds, max_dist2, epipolar=epi, **verdict)[:3] + (k,)

    def check(self, got, j, rounds=4, max_dist2=4.0, **verdict):
        model, info, flags, k = self.want(j, rounds, max_dist2, **verdict)
        assert got["models"][j].tobytes() == model.tobytes(), ("models", j, got["models"][j].view(capi.HOMOGRAPHY_DTYPE), model)
        assert got["info"][j].tobytes() == info.tobytes(), ("info", j, got["info"][j].view(capi.HREFIT_DTYPE), info)
        used = (k + 63) // 64
        assert got["inlier_bits"][j, :used].tobytes() == epiref.bits(flags, used).tobytes(), ("inlier_bits", j)
        assert (got["inlier_bits"][j, used:] == SENT).all(), "inlier_bits words past the count were written"
        total = int(flags.sum())
        assert int(got["inlier_counts"][j]) == total, ("inlier_counts", j)
        rows = min(total, self.inlier_cap)
        assert got["inliers"][j, :rows].tobytes() == self.matches[j, :k][flags][:rows].tobytes(), ("inliers", j)
        assert (got["inliers"][j, rows:] == SENT).all(), "inlier rows past the total were written"
        if self.epi is not None:
            assert got["gated_models"][j].tobytes() == homref.gate(self.epi[j:j + 1], model).tobytes(), ("gated_models", j)
        return model, info[0], flags

    def check_rows_past_the_call(self, got):
        for name in self.out:
            assert (got[name][self.n] == SENT).all(), name + ": the row past n_pairs was written"


@pytest.mark.parametrize("m", [0, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193])
def test_seams_equal_the_restatement_at_two_capacities(env, m):
    """One pair at every seam of the ordered sum (slot, wave, block, more than one block) and at the 4-member floor, non-members
    and untrusted records interleaved; the same list under two capacities gives the same bytes: the sum depends on m and the
    terms only."""
    ctx, torch = env
    mt, qp, tp = hrefitref.seam_pair(100 + m, m)
    model = hrefitref.planted_model()
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
        assert 4 <= int(info["n_before"]) < m and int(info["n_after"]) >= int(info["n_before"]) and int(info["stop"]) in (0, 4)
    if m <= 3:
        assert int(info["stop"]) == 1


def test_counts_above_cap(env):
    ctx, torch = env
    mt, qp, tp = hrefitref.seam_pair(11, 300)
    call = Call(torch, [(hrefitref.planted_model(), mt, qp, tp)], 200, 303, counts=[100000], inlier_cap=50)  # min(count, cap) records are considered
    got = call.run(ctx, torch)
    model, info, flags = call.check(got, 0)
    assert len(flags) == 200 and int(flags.sum()) > 50    # the total exceeds inlier_cap
    call.check_rows_past_the_call(got)


def test_hostile_values_reach_every_stop(env):
    """Three members, all members at one point (d == 0), members on one line, best < 0, a NaN H, a zero H, exactly 4 members, a
    refit with fewer inliers, records past the query capacity, exact data, octave-31 coordinates: the stops 0 .. 5, each where
    the restatement has it."""
    ctx, torch = env
    seen = set()
    for name, model, mt, qp, tp, d2, want in hrefitref.hostile_fixtures():
        call = Call(torch, [(model, mt, qp, tp)], len(mt) + 5, max(len(qp), len(tp)) + 2)
        got = call.run(ctx, torch, max_dist2=d2)
        _, info, flags = call.check(got, 0, max_dist2=d2)
        call.check_rows_past_the_call(got)
        assert want is None or int(info["stop"]) == want, (name, info)
        seen.add(int(info["stop"]))
        if name == "no model":
            assert got["models"][0].tobytes() == np.asarray(model).tobytes()
        if name == "exactly four":
            assert int(info["n_before"]) == 4 and int(info["stop"]) != 1
        if name in ("one line", "nan H", "zero H"):
            assert int(info["stop"]) != 0
        if name == "exact":
            assert int(info["n_after"]) == len(mt)
    assert seen == {0, 1, 2, 3, 4, 5}


def forty_pairs():
    rng = np.random.default_rng(40)
    pairs = []
    for j in range(40):
        m, kind = int(rng.integers(0, 301)), ("plane", "rotation")[j % 2]
        pairs.append((hrefitref.planted_model(kind),) + hrefitref.seam_pair(200 + j, m, kind))
    pairs[6] = (hrefitref.planted_model(),) + hrefitref.seam_pair(206, 0)
    none = hrefitref.planted_model()
    none["best"] = -1
    pairs[9] = (none,) + hrefitref.seam_pair(209, 130)
    pairs[12] = hrefitref.one_point_pair()
    pairs[15] = hrefitref.one_line_pair()
    mt, qp, tp = hrefitref.seam_pair(213, 5000)                                 # one pair with two blocks among the short ones
    pairs[13] = (hrefitref.planted_model(), mt, qp[:300], tp[:300])             # ... most of its records past the capacities
    return pairs


def test_forty_unequal_pairs_of_mixed_kinds_in_one_call_equal_forty_calls(env):
    ctx, torch = env
    pairs = forty_pairs()
    epi = np.zeros(40, capi.EPIPOLAR_DTYPE)
    epi["n_inliers"], epi["best"] = np.arange(40) * 11, np.where(np.arange(40) % 5 == 4, -1, 2)   # verdicts of both kinds
    epi["F"] = np.arange(9) + 1.0
    call = Call(torch, pairs, 5000, 310, epi=epi)
    whole = call.run(ctx, torch)
    again = Call(torch, pairs, 5000, 310, epi=epi).run(ctx, torch)  # two runs of one call: byte-identical
    assert all(whole[k].tobytes() == again[k].tobytes() for k in whole)
    call.check_rows_past_the_call(whole)
    for j in range(40):
        got = Call(torch, pairs[j:j + 1], 5000, 310, epi=epi[j:j + 1]).run(ctx, torch)
        for k in whole:
            assert whole[k][j].tobytes() == got[k][0].tobytes(), (k, j)
    res = [call.check(whole, j) for j in range(40)]
    stops = [int(r[1]["stop"]) for r in res]
    assert stops[9] == 5 and stops[6] == 1 and stops[12] == 2 and stops[15] == 3 and stops[0] in (0, 4)
    assert {int(r[0]["degenerate"][0]) for r in res} == {0, 1}


@pytest.mark.parametrize("rounds", [1, 2, 8])
def test_rounds(env, rounds):
    ctx, torch = env
    m4, q4, t4, seed4 = hrefitref.scene(*hrefitref.FEWER_INLIERS)[:4]
    pairs = [(hrefitref.planted_model(),) + hrefitref.seam_pair(31, 300), (seed4, m4, q4, t4), hrefitref.scene("rotation", 7, 300)[3:4] + hrefitref.scene("rotation", 7, 300)[:3]]
    call = Call(torch, pairs, 303, 303)
    got = call.run(ctx, torch, rounds=rounds)
    info = [call.check(got, j, rounds=rounds)[1] for j in range(3)]
    assert int(info[0]["accepted"]) <= rounds and int(info[1]["stop"]) == 4 and int(info[1]["accepted"]) == 0
    assert (int(info[2]["accepted"]), int(info[2]["stop"])) == (rounds, 0) if rounds <= 4 else int(info[2]["accepted"]) >= 4


def test_with_and_without_epipolar_models_and_the_verdicts_boundaries(env):
    ctx, torch = env
    m, qp, tp, model = hrefitref.scene("plane", 0, 300)[:4]
    stale = model.copy()
    stale["n_epipolar"], stale["degenerate"] = 12345, 1
    call = Call(torch, [(stale, m, qp, tp)], 300, 300)
    got = call.run(ctx, torch)
    out = call.check(got, 0)[0]
    assert (int(out["n_epipolar"][0]), int(out["degenerate"][0])) == (12345, 1)     # without epipolar_models: copied through
    nh = int(out["n_inliers"][0])
    epi = np.zeros(1, capi.EPIPOLAR_DTYPE)
    epi["best"], epi["F"] = 0, np.arange(9) + 1.0
    for ne, num, den, min_inliers, want in ((2 * nh, 1, 2, 16, 1), (2 * nh + 1, 1, 2, 16, 0), (nh, 1, 1, nh, 1), (nh, 1, 1, nh + 1, 0),
                                            (2 ** 32 - 1, 2 ** 32 - 1, nh, 16, 0), (0, 1, 2, 16, 1)):
        epi["n_inliers"] = ne
        c = Call(torch, [(stale, m, qp, tp)], 300, 300, epi=epi)
        v = dict(degenerate_num=num, degenerate_den=den, min_inliers=min_inliers)
        r = c.check(c.run(ctx, torch, **v), 0, num=num, den=den, min_inliers=min_inliers)[0]
        assert (int(r["n_epipolar"][0]), int(r["degenerate"][0])) == (ne, want), (ne, num, den, min_inliers)
    with pytest.raises(capi.VslamError):
        ctx.hrefit(*call.d_in, n_pairs=1, models=call.out["models"], gated_models=torch.zeros(22, dtype=torch.int32, device=DEV))  # gate without F
    with pytest.raises(capi.VslamError):
        ctx.hrefit(*call.d_in, n_pairs=1, models=call.out["models"], epipolar_models=c.d_epi, degenerate_den=0)
    ctx.hrefit(*call.d_in, n_pairs=1, models=call.out["models"], degenerate_den=0)          # without a verdict the denominator is not read
    torch.cuda.synchronize()


def test_each_optional_output_alone_in_place_and_bad_arguments(env):
    ctx, torch = env
    pair = (hrefitref.planted_model(),) + hrefitref.seam_pair(31, 300)
    epi = np.zeros(1, capi.EPIPOLAR_DTYPE)
    epi["best"], epi["n_inliers"], epi["F"] = 1, 400, np.arange(9) + 1.0   # 181 inliers of H against 400 of F: not degenerate
    call = Call(torch, [pair], 303, 303, epi=epi)
    want = call.run(ctx, torch)
    assert int(call.check(want, 0)[0]["degenerate"][0]) == 0 and want["gated_models"][0].tobytes() == epi.tobytes()
    for only in (("models",), ("models", "info"), ("models", "inlier_bits"), ("models", "inlier_counts"), ("models", "inliers", "inlier_counts"),
                 ("models", "gated_models")):
        got = Call(torch, [pair], 303, 303, epi=epi).run(ctx, torch, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == want[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    # models aliased onto the input, the gate aliased onto the epipolar models - of a degenerate pair, so that the gate writes
    epi["n_inliers"] = 100
    deg = Call(torch, [pair], 303, 303, epi=epi)
    want = deg.run(ctx, torch)
    assert int(deg.check(want, 0)[0]["degenerate"][0]) == 1 and int(want["gated_models"][0].view(capi.EPIPOLAR_DTYPE)["best"][0]) == -1
    alias = Call(torch, [pair], 303, 303, epi=epi)
    got = alias.run(ctx, torch, in_place=True, gate_in_place=True)
    assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    with pytest.raises(capi.VslamError):
        ctx.hrefit(*call.d_in, n_pairs=1, models=torch.zeros(41, dtype=torch.int32, device=DEV))  # undersized
    for rounds, d2 in ((0, 4.0), (9, 4.0), (4, 0.0), (4, float("nan"))):
        with pytest.raises(capi.VslamError):
            ctx.hrefit(*call.d_in, n_pairs=1, rounds=rounds, max_dist2=d2, models=deg.out["models"])
    torch.cuda.synchronize()
    assert deg.out["models"].cpu().numpy().tobytes() == want["models"].tobytes()   # a refused call writes nothing


def test_host_entry_point_and_the_cxx_wrapper(env, tmp_path):
    ctx, torch = env
    model = hrefitref.planted_model()
    mt, qp, tp = hrefitref.seam_pair(31, 300)
    epi = np.zeros(1, capi.EPIPOLAR_DTYPE)
    epi["best"], epi["n_inliers"], epi["F"] = 1, 100, np.arange(9) + 1.0
    want, info, flags, _ = hrefitref.hrefit(model, mt, qp, tp, 4, 4.0, epipolar=epi)
    gm, gi, gb, gl, total, gg = ctx.hrefit_host(model, mt, qp, tp, 4, 4.0, epipolar_model=epi)
    assert gm.tobytes() == want[0].tobytes() and gi.tobytes() == info[0].tobytes() and gb.tobytes() == epiref.bits(flags, 5).tobytes()
    assert total == int(flags.sum()) and gl.tobytes() == mt[flags].tobytes() and gg.tobytes() == homref.gate(epi, want).tobytes()
    assert int(gm["degenerate"]) == 1 and int(gg["best"]) == -1
    plain = hrefitref.hrefit(model, mt, qp, tp, 4, 4.0)[0]
    gm, gi, gb, gl, total, gg = ctx.hrefit_host(model, mt, qp, tp, 4, 4.0, want_bits=False, want_inliers=False)
    assert gm.tobytes() == plain[0].tobytes() and gb is None and gl is None and total is None and gg is None
    gm, gi, gb, gl, total, gg = ctx.hrefit_host(model, mt[:0], qp, tp, 4, 4.0)           # no records: fewer than 4 members
    assert int(gi["stop"]) == 1 and int(gi["n_before"]) == 0 and total == 0 and gm["H"].tobytes() == model["H"][0].tobytes()
    # the C++ wrapper (vslam::refitHomography) through a small driver: the same bytes
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    archive = os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a")
    assert os.path.exists(archive), "visualslam_amd/bin/libvslam_cxx.a is missing: __graft_entry__.build() builds it"
    exe = str(tmp_path / "hrefit_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "hrefit_cxx_driver.cpp"), archive,
                        "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blob = tmp_path / "pair.bin"
    with open(blob, "wb") as f:
        f.write(np.array([len(mt), len(qp), len(tp), 1], np.uint64).tobytes() + np.asarray(model).tobytes() + epi.tobytes() + mt.tobytes() + qp.tobytes()
                + tp.tobytes())
    r = subprocess.run([exe, str(blob), "4", "4.0", "1", "2", "16", str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = open(tmp_path / "out.bin", "rb").read()
    assert out[:168] == want[0].tobytes() and out[168:184] == info[0].tobytes() and out[184:272] == homref.gate(epi, want).tobytes()
    assert out[272:] == np.array([int(flags.sum())], np.uint64).tobytes() + mt[flags].tobytes()


@pytest.fixture(scope="module")
def cpu_chain():
    """A planted plane scene with repeated structure (guidedhfref.repeated_scene) through the restatements, once: match -> RANSAC F
    and H with the verdict -> refit of H (4 rounds, the verdict again, the gate) -> guided matching under (gate, H) -> pose of the
    gated model and pose from H over the refit's inliers."""
    s = guidedhfref.repeated_scene(5, "plane")
    _, m0 = matchref.match(s["q"], s["t"], 0.64)
    emodel = epiref.ransac(m0, s["qp"], s["tp"], 512, 1, 4.0)[0]
    hmodel = homref.verdict(homref.ransac(m0, s["qp"], s["tp"], 512, 1, 4.0)[0], emodel)
    href, info, flags, _ = hrefitref.hrefit(hmodel, m0, s["qp"], s["tp"], 4, 4.0, epipolar=emodel)
    gated = homref.gate(emodel, href)
    nn1, m1 = guidedhfref.guided_hf(s["q"], s["t"], s["qp"], s["tp"], gated, href, 0.64, np.inf, 4.0, 4.0)
    inl = m0[flags]
    k, n = len(inl), len(s["q"])
    pose, _, front, X = poseref.pose(gated[0], inl, s["qp"], s["tp"], K)
    poses, pts, bits = pose.copy(), np.zeros((1, n, 3)), np.zeros((1, (n + 63) // 64), np.uint64)
    bits[0] = epiref.bits(front, (n + 63) // 64)
    if X is not None:
        pts[0, :k] = X
    mt = np.zeros((1, n), capi.MATCH_DTYPE)
    mt[0, :k] = inl
    hinfo, _ = hposeref.fill(href, mt, np.array([k]), s["qp"][None], s["tp"][None], K, poses, pts, bits)
    print("repeated plane scene, CPU chain: H inliers", int(hmodel["n_inliers"][0]), "->", int(href["n_inliers"][0]), "info", info[0], "guided", len(m1),
          "hpose kind", int(hinfo["kind"][0]), "best", int(poses["best"][0]))
    return dict(s=s, m0=m0, emodel=emodel, hmodel=hmodel, href=href, info=info, flags=flags, gated=gated, nn1=nn1, m1=m1, poses=poses, pts=pts, bits=bits,
                hinfo=hinfo)


def test_planted_plane_scene_end_to_end_like_the_cpu_chain(env, cpu_chain):
    """match -> epipolar -> homography -> hrefit (in place, gate in place) -> match_guided_hf -> pose -> hpose on the device,
    nothing downloaded in between, against the chain of the restatements."""
    ctx, torch = env
    w = cpu_chain
    s = w["s"]
    n = len(s["q"])
    d = torch.from_numpy(np.stack([s["q"], s["t"]])).to(DEV)
    c = torch.full((2,), n, dtype=torch.int32, device=DEV)
    df = torch.ones((2, n), dtype=torch.uint8, device=DEV)
    pts = torch.from_numpy(np.stack([s["qp"], s["tp"]]).view(np.int32).reshape(2, n, 6)).to(DEV)
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    Q, T = capi.desc_sets(d[:1], c[:1], df[:1], pts[:1]), capi.desc_sets(d[1:], c[1:], df[1:], pts[1:])
    m0, c0, emod, hmod, rinfo = z(1, n, 3), z(1), z(1, 22), z(1, 42), z(1, 4)
    ctx.match(Q, T, 1, 0.64, False, matches=m0, match_counts=c0)
    ctx.epipolar(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, models=emod)
    ctx.homography(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, epipolar_models=emod, models=hmod)
    torch.cuda.synchronize()
    assert hmod.cpu().numpy().tobytes() == w["hmodel"].tobytes() and emod.cpu().numpy().tobytes() == w["emodel"].tobytes()
    inl = torch.full((1, n, 3), SENT, dtype=torch.int32, device=DEV)
    icnt = z(1)
    ctx.hrefit(hmod, m0, c0, pts[:1], pts[1:], 1, 4, 4.0, epipolar_models=emod, models=hmod, info=rinfo, inliers=inl, inlier_counts=icnt, gated_models=emod)
    nn1, m1, c1 = z(1, n, 3), z(1, n, 3), z(1)
    ctx.match_guided_hf(Q, T, emod, hmod, 1, 0.64, np.inf, 4.0, 4.0, False, nn=nn1, matches=m1, match_counts=c1)
    poses, hinfo = z(1, 28), z(1, 36)
    X, fb = torch.zeros((1, n, 3), dtype=torch.float64, device=DEV), torch.zeros((1, (n + 63) // 64), dtype=torch.int64, device=DEV)
    ctx.pose(emod, inl, icnt, pts[:1], pts[1:], K, poses=poses, points=X, front_bits=fb)
    ctx.hpose(hmod, inl, icnt, pts[:1], pts[1:], K, poses=poses, info=hinfo, points=X, front_bits=fb)
    torch.cuda.synchronize()
    k = int(icnt[0])
    assert hmod.cpu().numpy().tobytes() == w["href"].tobytes() and rinfo.cpu().numpy().tobytes() == w["info"].tobytes()
    assert emod.cpu().numpy().tobytes() == w["gated"].tobytes() and int(w["gated"]["best"][0]) == -1 and int(w["href"]["degenerate"][0]) == 1
    assert k == int(w["flags"].sum()) >= int(w["hmodel"]["n_inliers"][0])
    gi = inl.cpu().numpy()[0]
    assert gi[:k].tobytes() == w["m0"][w["flags"]].tobytes() and (gi[k:] == SENT).all()
    assert int(c1[0]) == len(w["m1"]) and m1.cpu().numpy()[0, :len(w["m1"])].tobytes() == w["m1"].tobytes()
    assert nn1.cpu().numpy().tobytes() == w["nn1"].tobytes()
    assert poses.cpu().numpy().tobytes() == w["poses"].tobytes() and hinfo.cpu().numpy().tobytes() == w["hinfo"].tobytes()
    assert int(w["poses"]["best"][0]) >= 0 and int(w["hinfo"]["kind"][0]) == capi.HPOSE_PLANE
    assert fb.cpu().numpy().tobytes() == w["bits"].tobytes() and X.cpu().numpy()[0, :k].tobytes() == w["pts"][0, :k].tobytes()


def test_match_executable_reports_the_hrefit_of_the_python_path(env, tmp_path):
    from tests.test_gpu_match import building_crops, detect

    ctx, torch = env
    exe = os.path.join(ROOT, "visualslam_amd", "bin", "Match")
    assert os.path.exists(exe), "visualslam_amd/bin/Match is missing: __graft_entry__.build() builds it"
    paths = []
    for k, img in enumerate(building_crops()):
        paths.append(str(tmp_path / f"crop{k}.pgm"))
        with open(paths[-1], "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes())
    r = subprocess.run([exe, "--epipolar", "--homography", "--hrefit", "4", paths[0], paths[1], "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    # the Python path over the same crops: detect -> match -> epipolar -> homography -> hrefit
    p, o = detect(ctx, torch, np.stack(building_crops()))
    cap = p.oriented_cap
    dd, cc, df, pts = o["descriptors"], o["oriented_counts"], o["descriptor_defined"], o["oriented_points"]
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=DEV)
    m0, c0, emod, hmod, rinfo = z(1, cap, 3), z(1), z(1, 22), z(1, 42), z(1, 4)
    ctx.match(capi.desc_sets(dd[:1], cc[:1], df[:1]), capi.desc_sets(dd[1:], cc[1:], df[1:]), 1, 0.64, False, matches=m0, match_counts=c0)
    ctx.epipolar(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, models=emod)
    ctx.homography(m0, c0, pts[:1], pts[1:], 1, 512, 1, 4.0, epipolar_models=emod, models=hmod)
    before = hmod.cpu().numpy().view(capi.HOMOGRAPHY_DTYPE).reshape(-1).copy()
    ctx.hrefit(hmod, m0, c0, pts[:1], pts[1:], 1, 4, 4.0, epipolar_models=emod, models=hmod, info=rinfo)
    torch.cuda.synchronize()
    after, i = hmod.cpu().numpy().view(capi.HOMOGRAPHY_DTYPE).reshape(-1), rinfo.cpu().numpy().view(capi.HREFIT_DTYPE).reshape(-1)[0]
    e = rep["hrefit"]
    assert (e["rounds"], e["n_before"], e["n_after"], e["accepted"], e["stop"]) == (4, int(i["n_before"]), int(i["n_after"]), int(i["accepted"]), int(i["stop"]))
    assert (e["n_epipolar"], e["degenerate"]) == (int(after["n_epipolar"][0]), int(after["degenerate"][0]))
    assert np.array(e["H"], np.float64).tobytes() == after["H"][0].tobytes()                     # 17 significant digits: the same doubles
    assert rep["homography"]["n_inliers"] == int(before["n_inliers"][0]) == e["n_before"] <= e["n_after"]
    assert np.array(rep["homography"]["H"], np.float64).tobytes() == before["H"][0].tobytes()
    bad = subprocess.run([exe, "--epipolar", "--homography", "--hrefit", "9", "64x48"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "1 .. 8" in bad.stderr

"""The bundle adjustment on the GPU (vslam_bundle_dev / vslam_bundle_host / vslam::bundleAdjust, include/vslam.h): every
comparison is bytes-equal against the CPU restatement in tests/bundleref.py - every track row, every camera record, every
point_info row and every word of member_bits - with sentinels intact past every count.  The inputs are built directly as
buffers, as tests/test_gpu_tracks.py builds them, with the restatements' outputs for chain, tracks_in and refs."""
import subprocess

import numpy as np
import pytest

from tests import bundleref, epiref, tracksref
from tests.test_bundle_cpu import build_cxx_driver, cxx_driver_buffers, perturbed_cams
from tests.test_gpu_tracks import Inputs, Scene, forty_pairs
from tests.test_tracks_cpu import K, five_frames_with_points, planted_tracks
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
WIDE = 1e7          # the random lists of Inputs reproject anywhere: a wide test, so that views are members and steps are taken


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


class Call:
    """One vslam_bundle_dev call over Inputs: tracks_in and refs from the tracks restatement (rows past m_j: sentinel bytes), the
    device copies, and the outputs pre-filled with a sentinel, one row more than the call writes."""

    def __init__(self, torch, inp, max_dist2=WIDE, min_views=2, cams_in=None, edit=None):
        self.inp, self.max_dist2, self.min_views, self.cams_in = inp, max_dist2, min_views, cams_in
        n, cap = inp.n, inp.cap
        ms, rows, refs, _, _, _ = tracksref.tracks(inp.poses, inp.matches, inp.counts, inp.bits, inp.pcap, inp.chain, inp.frames, K, max_dist2, 2)
        self.tracks_in, self.refs = bundleref.dense_tracks(ms, rows, refs, cap, fill=0xB3)
        if edit:
            edit(self)
        dev = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape).copy()).to(DEV)
        self.d_in = dict(poses=dev(inp.poses, (n, 28), np.int32), matches=dev(inp.matches, (n, cap, 3), np.int32), match_counts=dev(inp.counts, (n,), np.int32),
                         front_bits=dev(inp.bits, (n, inp.words), np.int64), chain=dev(inp.chain, (n, 44), np.int32),
                         frame_points=dev(inp.frames, (n + 1, inp.pcap, 6), np.int32), tracks_in=dev(self.tracks_in, (n, cap, 6), np.int64),
                         refs=dev(self.refs, (n, cap, 2), np.int32))
        self.d_cams_in = None if cams_in is None else dev(cams_in, (n, 20), np.int64)
        full = lambda shape: torch.full(shape, SENT, dtype=torch.int64, device=DEV)
        self.out = dict(tracks=full((n + 1, cap, 6)), cams=full((n + 1, 20)), point_info=full((n + 1, cap, 5)), member_bits=full((n + 1, 2, inp.words)))

    def want(self, sweeps, cams_in="same"):
        i = self.inp
        return bundleref.bundle(i.poses, i.matches, i.counts, i.bits, i.pcap, i.chain, i.frames, self.tracks_in, self.refs, K, self.max_dist2, self.min_views,
                                sweeps, self.cams_in if isinstance(cams_in, str) else cams_in)

    def run(self, ctx, torch, sweeps, only=None, n_pairs=None, **over):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        d = dict(self.d_in, **over)
        ctx.bundle(d["poses"], d["matches"], d["match_counts"], d["front_bits"], self.inp.pcap, d["chain"], d["frame_points"], d["tracks_in"], d["refs"], K,
                   self.max_dist2, self.min_views, sweeps, n_pairs=self.inp.n if n_pairs is None else n_pairs, cams_in=over.get("cams_in", self.d_cams_in), **outs)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def check(self, got, want, aliased=False):
        n, cap, words = self.inp.n, self.inp.cap, self.inp.words
        assert got["cams"][:n].tobytes() == want["cams"].tobytes(), ("cams", got["cams"][:n].view(capi.BUNDLE_CAM_DTYPE), want["cams"])
        for j in range(n):
            m = int(want["ms"][j])
            g = got["tracks"][j, :m].view(capi.TRACK_DTYPE).reshape(-1)
            bad = [i for i in range(m) if g[i].tobytes() != want["tracks"][j, i].tobytes()]
            assert not bad, ("tracks", j, len(bad), bad[:4], g[bad[0]], want["tracks"][j, bad[0]])
            past = got["tracks"][j, m:]
            assert (past == SENT).all() if not aliased else past.tobytes() == self.tracks_in[j, m:].tobytes(), "track rows past the count were written"
            wr = want["written"][j]
            pi = got["point_info"][j].view(capi.BUNDLE_POINT_DTYPE).reshape(-1)
            bad = [i for i in np.flatnonzero(wr) if pi[i].tobytes() != want["point_info"][j, i].tobytes()]
            assert not bad, ("point_info", j, len(bad), bad[:4], pi[bad[0]], want["point_info"][j, bad[0]])
            assert (got["point_info"][j][~wr] == SENT).all(), "point_info rows that are not heads of active tracks were written"
            w = (m + 63) // 64
            for half in (0, 1):
                assert got["member_bits"][j, half, :w].tobytes() == epiref.bits(want["member"][j, half, :m], w).tobytes(), ("member_bits", j, half)
                assert (got["member_bits"][j, half, w:] == SENT).all(), "member_bits words past the count were written"
        for name in self.out:
            assert (got[name][n] == SENT).all(), name + ": the row past n_pairs was written"


# ---- seams

@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("n", [2, 3, 6])
def test_chains_with_the_seam_in_each_position(env, n, m):
    ctx, torch = env
    lengths, moved = set(), 0
    for pos in range(n):
        ms = [300] * n
        ms[pos] = m
        call = Call(torch, Inputs(ms, seed=pos))
        want = call.want(2)
        call.check(call.run(ctx, torch, 2), want)
        lengths |= {len(p) for h, p in tracksref.paths(call.inp.poses, call.inp.matches, call.inp.counts, call.inp.bits, 512, call.inp.chain)[2].items()}
        moved += int(want["cams"]["accepted"].sum()) + int(want["point_info"]["accepted"].sum())
    assert moved > 0
    if m >= 63:
        assert lengths >= set(range(1, n + 1)), lengths                              # tracks of 1 .. n_pairs records


@pytest.mark.parametrize("m0,m1", [(4095, 3), (4096, 1), (4090, 10), (2049, 2049), (8193, 0)])
def test_the_block_seam_of_the_ordered_sum(env, m0, m1):
    """Camera T_1 of three pairs has m0 train rows and then m1 head rows: the seam between blocks of 4096 rows falls in the train
    rows, exactly between the halves, and inside the head rows."""
    ctx, torch = env
    inp = Inputs([300, m0, m1], pcap=16384, seed=m0 % 7)
    k = min(m1, 3)                      # the first records of pair 2 start tracks for certain: in front, on trusted points no record of pair 1 ends at
    inp.matches["query"][2, :k] = 16383 - np.arange(k)
    inp.bits[2, 0] |= np.uint64(7)
    inp.frames["octave"][2, 16383 - np.arange(k)] = 1
    assert not np.isin(16383 - np.arange(k), inp.matches["train"][1, :m0]).any()
    inp.chain["linked"][2] = int(m1 > 0)   # (three records seldom give the trajectory a ratio: the link is set by hand)
    call = Call(torch, inp)
    assert call.inp.chain["linked"].tolist() == [0, 1, int(m1 > 0)]
    want = call.want(1)
    rows = bundleref.Problem(call.inp.poses, call.inp.matches, call.inp.counts, call.inp.bits, 16384, call.inp.chain, call.inp.frames, call.tracks_in,
                             call.refs, K, WIDE, 2).rows_of(1)
    counting = ~np.isnan(rows["u"])
    assert len(rows) == m0 + m1 and counting[:m0].sum() > m0 // 4 and (m1 == 0 or counting[m0:].any()) and (m1 < 10 or not counting[m0:].all())
    assert want["cams"]["n_before"][1] >= 6
    call.check(call.run(ctx, torch, 1), want)


# ---- hostile inputs

def hostile_edit(call):
    t = call.tracks_in
    heads = np.argwhere(t["n_views"] > 0)
    for k, (j, i) in enumerate(heads):
        if k % 3 == 1:
            t["status"][j, i] &= ~np.uint32(1)                                     # inactive tracks interleaved
        elif k % 11 == 0:
            t["X"][j, i, k % 3] = [np.nan, np.inf, -np.inf, 2.0 ** 300, 2.0 ** -300][(k // 11) % 5]
        elif k % 13 == 0:
            t["X"][j, i] *= 2.0 ** (300 if k % 2 else -300)
    t["n_views"][heads[5][0], heads[5][1]] = 0xFFFFFFFF                             # a count no path has


def test_hostile_values_indices_counts_and_a_break(env):
    ctx, torch = env
    inp = Inputs([300, 200, 300, 280, 300, 260], match_cap=290, counts=[300, 200, 100000, 280, 300, 260], seed=9)   # m = 290, 200, 290, ...
    inp.chain["linked"][2] = 0                                                      # a break in the middle
    inp.poses["best"][4] = -1                                                       # an invalid pair in the middle ...
    inp.chain["linked"][4] = 1                                                      # ... whose chain record claims a link anyway
    q, t = inp.matches["query"].astype(np.int64) & 0xFFFFFFFF, inp.matches["train"].astype(np.int64) & 0xFFFFFFFF
    octs = inp.frames["octave"]
    assert (q[:, :200] >= 512).sum() >= 3 and (t > 2 ** 31).any() and ((octs < 0) | (octs > 31)).sum() > 20
    cams_in = perturbed_cams(inp.poses, inp.chain, seed=3)
    cams_in["W"][1, 4] = np.array([0x7FF4000000ABCDEF], np.uint64).view(np.float64)[0]     # a NaN with a payload
    cams_in["w"][3, 0] = np.inf
    call = Call(torch, inp, min_views=3, cams_in=cams_in, edit=hostile_edit)
    want = call.want(3)
    c = want["cams"]
    assert c["skipped"][4] == 3 and c["W"][4].tolist() == np.eye(3).reshape(9).tolist() and c["n_after"][4] == 0
    assert np.isnan(c["W"][1]).any() and (c["W"][1].view(np.uint64)[np.isnan(c["W"][1])] == 0x7FF8000000000000).all() and c["skipped"][1] == 3
    assert c["accepted"][[0, 2, 5]].sum() > 0
    call.check(call.run(ctx, torch, 3), want)


@pytest.mark.parametrize("m,skipped", [(5, True), (6, False)])
def test_a_camera_with_exactly_five_and_exactly_six_members(env, m, skipped):
    ctx, torch = env
    inp = Scene(3, m)
    call = Call(torch, inp, max_dist2=4.0, cams_in=perturbed_cams(inp.poses, inp.chain, seed=1, angle=1e-4, scale=1e-4))
    want = call.want(2)
    assert (want["cams"]["n_before"] == m).all() and (want["cams"]["skipped"] == (2 if skipped else 0)).all()
    assert skipped or want["cams"]["accepted"].sum() > 0
    call.check(call.run(ctx, torch, 2), want)


def test_every_view_behind_its_camera(env):
    ctx, torch = env
    inp = Scene(4, 70)
    F = np.diag([-1.0, 1.0, -1.0])                                                  # tests/test_gpu_tracks.py's "behind": every camera turned half round where it stands
    for j in range(4):
        inp.chain["W"][j], inp.chain["w"][j] = (F @ inp.chain["W"][j].reshape(3, 3)).reshape(9), F @ inp.chain["w"][j]
        inp.poses["R"][j], inp.poses["t"][j] = (F @ inp.poses["R"][j].reshape(3, 3) @ F).reshape(9), F @ inp.poses["t"][j]
    inp.frames["row"] = 1080 - inp.frames["row"]
    call = Call(torch, inp, max_dist2=4.0)
    assert (call.tracks_in["status"][0, :70] == 1).all()                              # solved, nothing ok
    want = call.want(2)
    # the held camera of pair 0 is not turned: its view may be a member, one member is fewer than two; every train camera sees nothing
    assert (want["cams"]["n_before"] == 0).all() and (want["cams"]["skipped"] == 2).all() and (want["point_info"]["skipped"][0, :70] == 2).all()
    assert want["tracks"]["X"][0, :70].tobytes() == call.tracks_in["X"][0, :70].tobytes()
    call.check(call.run(ctx, torch, 2), want)


# ---- sweeps, re-entry, whole calls

def small_problem(torch):
    inp = Scene(4, 70)
    return Call(torch, inp, max_dist2=400.0, min_views=3, cams_in=perturbed_cams(inp.poses, inp.chain, seed=2))


@pytest.mark.parametrize("sweeps", [1, 2, 8, 64])
def test_sweep_counts_on_a_small_scene(env, sweeps):
    ctx, torch = env
    call = small_problem(torch)
    want = call.want(sweeps)
    c = want["cams"]
    assert ((c["accepted"] + c["rejected"] + c["invalid"] + c["skipped"]) == sweeps).all() and c["accepted"].min() >= 1
    assert c["cost_after"].sum() < c["cost_before"].sum()
    call.check(call.run(ctx, torch, sweeps), want)


def test_eight_calls_of_one_sweep_equal_one_call_of_eight(env):
    ctx, torch = env
    call = small_problem(torch)
    once = call.run(ctx, torch, 8)
    step = small_problem(torch)
    tracks_in, cams_in = step.d_in["tracks_in"], step.d_cams_in
    for _ in range(8):
        got = step.run(ctx, torch, 1, tracks_in=tracks_in, cams_in=cams_in)
        tracks_in, cams_in = step.out["tracks"][:4].clone(), step.out["cams"][:4].clone()
    a, b = once["tracks"][:4].view(capi.TRACK_DTYPE), got["tracks"][:4].view(capi.TRACK_DTYPE)
    for f in ("X", "n_ok", "status"):
        assert a[f][:, :70].tobytes() == b[f][:, :70].tobytes(), f
    ca, cb = once["cams"][:4].view(capi.BUNDLE_CAM_DTYPE), got["cams"][:4].view(capi.BUNDLE_CAM_DTYPE)
    assert ca["W"].tobytes() == cb["W"].tobytes() and ca["w"].tobytes() == cb["w"].tobytes()
    assert (a["status"][0, :70] & 1).all()


def test_forty_unequal_pairs_and_a_repeat(env):
    ctx, torch = env
    inp = forty_pairs()
    call = Call(torch, inp, min_views=3)
    want = call.want(2)
    assert (want["cams"]["skipped"][[7, 30]] == 2).all() and want["cams"]["accepted"].sum() > 20
    first = call.run(ctx, torch, 2)
    call.check(first, want)
    again = Call(torch, inp, min_views=3).run(ctx, torch, 2)                          # a second run of the same call: identical bytes
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)


def test_aliasing_each_optional_output_alone_cams_in_and_the_rejections(env):
    ctx, torch = env
    inp = Inputs([257, 300, 64, 129], seed=6)
    cams_in = perturbed_cams(inp.poses, inp.chain, seed=4)
    call = Call(torch, inp, min_views=3, cams_in=cams_in)
    want = call.want(2)
    full = call.run(ctx, torch, 2)
    call.check(full, want)
    without = Call(torch, inp, min_views=3)                                            # cams_in absent: the cameras start from the chain
    w0 = without.want(2)
    assert w0["cams"].tobytes() != want["cams"].tobytes()
    without.check(without.run(ctx, torch, 2), w0)
    for only in (("tracks", "cams"), ("tracks", "cams", "point_info"), ("tracks", "cams", "member_bits")):
        got = Call(torch, inp, min_views=3, cams_in=cams_in).run(ctx, torch, 2, only=only)
        for k in got:
            assert got[k].tobytes() == full[k].tobytes() if k in only else (got[k] == SENT).all(), (only, k)
    alias = Call(torch, inp, min_views=3, cams_in=cams_in)                             # tracks is the very pointer tracks_in
    alias.out["tracks"] = torch.cat([alias.d_in["tracks_in"], torch.full((1, inp.cap, 6), SENT, dtype=torch.int64, device=DEV)])
    alias.check(alias.run(ctx, torch, 2, tracks_in=alias.out["tracks"]), want, aliased=True)
    none = Call(torch, inp)
    none.run(ctx, torch, 2, n_pairs=0)                                                 # no pairs: nothing is written
    assert all((v.cpu().numpy() == SENT).all() for v in none.out.values())
    d = call.d_in
    args = (d["poses"], d["matches"], d["match_counts"], d["front_bits"], 512, d["chain"], d["frame_points"])
    for bad in (dict(sweeps=0), dict(sweeps=65), dict(min_views=1), dict(max_dist2=0.0)):
        kw = dict(dict(max_dist2=4.0, min_views=2, sweeps=1), **bad)
        with pytest.raises(capi.VslamError):
            ctx.bundle(*args, d["tracks_in"], d["refs"], K, tracks=call.out["tracks"], cams=call.out["cams"], **kw)
    with pytest.raises(capi.VslamError):                                               # tracks_in one row into tracks: overlapping, not equal
        ctx.bundle(*args, call.out["tracks"].view(-1)[6:], d["refs"], K, n_pairs=3, tracks=call.out["tracks"], cams=call.out["cams"])
    with pytest.raises(capi.VslamError):
        ctx.bundle(*args, d["tracks_in"], d["refs"], K, tracks=call.out["tracks"], cams=torch.zeros(4 * 20 - 1, dtype=torch.int64, device=DEV))


def test_host_entry_point_and_cxx_wrapper(env, tmp_path):
    ctx, torch = env
    inp = Inputs([257, 300, 64, 129], seed=6)
    call = Call(torch, inp, min_views=3)
    want = call.want(2)
    n, cap, words = inp.n, inp.cap, inp.words
    tr = call.tracks_in.copy()
    pi, mb = np.full((n, cap, 5), SENT, np.int64), np.full((n, 2, words), SENT, np.int64)
    tracks, cams = ctx.bundle_host(inp.poses, inp.matches, inp.counts, inp.bits, 512, inp.chain, inp.frames, call.tracks_in, call.refs, K, WIDE, 3, 2,
                                   tracks=tr, point_info=pi.view(capi.BUNDLE_POINT_DTYPE).reshape(n, cap), member_bits=mb.view(np.uint64))
    got = dict(tracks=np.concatenate([tr.view(np.int64).reshape(n, cap, 6), np.full((1, cap, 6), SENT)]),
               cams=np.concatenate([cams.view(np.int64).reshape(n, 20), np.full((1, 20), SENT)]),
               point_info=np.concatenate([pi, np.full((1, cap, 5), SENT)]), member_bits=np.concatenate([mb, np.full((1, 2, words), SENT)]))
    call.check(got, want, aliased=True)
    # the C++ wrapper on the buffers tests/bundle_cxx_driver.cpp builds
    r = subprocess.run([build_cxx_driver(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {l.split()[0]: bytes.fromhex(l.split()[1]) for l in r.stdout.splitlines()}
    poses, mt, counts, bits, frames, chain, tracks_in, refs = cxx_driver_buffers()
    assert out["chain"] == chain.tobytes() and out["tracks_in"] == tracks_in.tobytes() and out["refs"] == refs.tobytes()
    w = bundleref.bundle(poses, mt, counts, bits, 8, chain, frames, tracks_in, refs, K, 4.0, 2, 3)
    assert w["cams"]["accepted"].sum() > 0 and w["point_info"]["accepted"].sum() > 0 and chain["linked"].tolist() == [0, 1, 1]
    assert out["tracks"] == w["tracks"].tobytes() and out["cams"] == w["cams"].tobytes()
    assert out["point_info"] == w["point_info"].tobytes()                              # zero where nothing is written, as the wrapper presets it
    assert out["member_bits"] == np.stack([[epiref.bits(w["member"][j, h], 1) for h in (0, 1)] for j in range(3)]).tobytes()


def test_planted_five_frames_end_to_end_like_the_cpu_chain(env):
    """One planted five-frame scene through epipolar -> pose -> chain -> tracks -> bundle on the device, nothing downloaded in
    between, against the CPU chain of the restatements."""
    ctx, torch = env
    seed, n = 1, 300
    (poses, mt, counts, pts, bits, chain, frames), maps, (ms, rows, refs, goods, summary, paths), world, perms = planted_tracks(seed, n)
    matches = np.stack(five_frames_with_points(seed, n)[0])
    words = (n + 63) // 64
    dev = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape).copy()).to(DEV)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    dm, dc, dp = dev(matches, (4, n, 3), np.int32), torch.full((4,), n, dtype=torch.int32, device=DEV), dev(frames, (5, n, 6), np.int32)
    models, inliers, icounts = z((4, 22), torch.int32), z((4, n, 3), torch.int32), z((4,), torch.int32)
    ctx.epipolar(dm, dc, dp[:4], dp[1:], 4, 512, seed, 4.0, models=models, inliers=inliers, inlier_counts=icounts)
    dposes, X, fb = z((4, 28), torch.int32), z((4, n, 3), torch.float64), z((4, words), torch.int64)
    ctx.pose(models, inliers, icounts, dp[:4], dp[1:], K, poses=dposes, points=X, front_bits=fb)
    dchain = z((4, 44), torch.int32)
    ctx.chain(dposes, inliers, icounts, X, fb, n, 16, n_pairs=4, chain=dchain)
    full = lambda shape: torch.full(shape, SENT, dtype=torch.int64, device=DEV)
    dtracks, drefs = full((4, n, 6)), torch.full((4, n, 2), SENT, dtype=torch.int32, device=DEV)
    ctx.tracks(dposes, inliers, icounts, fb, n, dchain, dp, K, 4.0, 2, n_pairs=4, tracks=dtracks, refs=drefs)
    out = dict(tracks=full((5, n, 6)), cams=full((5, 20)), point_info=full((5, n, 5)), member_bits=full((5, 2, words)))
    ctx.bundle(dposes, inliers, icounts, fb, n, dchain, dp, dtracks, drefs, K, 4.0, 3, 8, n_pairs=4, **out)
    torch.cuda.synchronize()
    assert dchain.cpu().numpy().tobytes() == chain.tobytes()
    tracks_in, refs_in = bundleref.dense_tracks(ms, rows, refs, n, fill=0xB3)        # (SENT as bytes: the rows the tracks call left untouched)
    assert dtracks.cpu().numpy()[0, :ms[0]].tobytes() == rows[0].tobytes()
    want = bundleref.bundle(poses, mt, counts, bits, n, chain, frames, tracks_in, refs_in, K, 4.0, 3, 8)
    assert want["cams"]["accepted"].min() >= 1 and want["cams"]["cost_after"].sum() < want["cams"]["cost_before"].sum()

    class Shape:
        pass

    call = Call.__new__(Call)
    call.inp, call.out, call.tracks_in = Shape(), out, tracks_in
    call.inp.n, call.inp.cap, call.inp.words = 4, n, words
    got = {k: v.cpu().numpy() for k, v in out.items()}
    call.check(got, want)
    # every (track, frame) observation is one row of one camera or a held view: the device's totals, with the restatement's held views
    held = int(want["point_info"]["n_after"][want["written"]].sum()) - int(want["cams"]["n_after"].sum())
    over_tracks = int(got["point_info"][:4].view(capi.BUNDLE_POINT_DTYPE).reshape(4, n)["n_after"][want["written"]].sum())
    assert held > 0 and over_tracks == int(got["cams"][:4].view(capi.BUNDLE_CAM_DTYPE)["n_after"].sum()) + held

"""The tracks step on the GPU (vslam_tracks_dev / vslam_tracks_host, include/vslam.h): every comparison is bytes-equal against
the CPU restatement of the arithmetic in tests/tracksref.py - every track row, every ref, every word of good_bits and the
summary - with sentinels intact past every count.  The inputs are built directly as buffers (synthetic poses, chain records,
point lists and front bits): the entry point takes them as they are, so every seam can be placed exactly."""
import numpy as np
import pytest

from tests import chainref, epiref, tracksref
from tests.test_tracks_cpu import K, build_cxx_driver, planted_tracks, small_scene
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
QNAN_BITS = 0x7FF8000000000000


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def random_rotation(rng):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-0.6, 0.6)
    A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A


class Inputs:
    """The input buffers of one call, as numpy arrays to be edited before run(): n pairs of ms[j] records over point lists of
    capacity pcap.  Random poses with a winner, about 85 % of the front bits set - over the whole capacity, so also on records
    past m_j -; every even record i matches point i to point i, so that tracks run through many pairs, every odd record has
    indices uniform in 0 .. pcap - 1 - shared queries and shared trains, so the one-to-one rule is decided on the device -
    except about 3 % that point past the capacity (some of them negative: huge as unsigned).  The chain records are the
    trajectory restatement's over random points; the point lists have octaves 0 .. 2 and, one in 25, an octave that is not
    trusted (-1, 32) or 31."""

    def __init__(self, ms, pcap=512, match_cap=None, seed=0, counts=None, hostile=True):
        rng = np.random.default_rng(seed * 7919 + sum(ms) + len(ms))
        n = len(ms)
        self.n, self.pcap = n, pcap
        self.cap = cap = (max(list(ms) + [1]) + 3) if match_cap is None else match_cap
        self.words = (cap + 63) // 64
        self.poses = np.zeros(n, capi.POSE_DTYPE)
        for j in range(n):
            t = rng.normal(size=3)
            self.poses["R"][j], self.poses["t"][j] = random_rotation(rng).reshape(9), t / np.linalg.norm(t)
            self.poses["n_matches"][j], self.poses["valid"][j] = min(ms[j], cap), 1
        self.matches = np.zeros((n, cap), capi.MATCH_DTYPE)
        self.matches["query"], self.matches["train"] = rng.integers(0, pcap, (n, cap)), rng.integers(0, pcap, (n, cap))
        even = np.arange(0, min(cap, pcap), 2)
        self.matches["query"][:, even] = self.matches["train"][:, even] = even
        if hostile:
            for name in ("query", "train"):
                past = rng.random((n, cap)) < 0.015
                self.matches[name][past] = rng.choice([pcap, pcap + 1, 2 ** 31 - 1, -1, -2 ** 31], int(past.sum()))
        self.counts = np.array(ms if counts is None else counts, np.int64).astype(np.uint32)
        self.bits = np.packbits(rng.random((n, self.words * 64)) < 0.85, axis=1, bitorder="little").view(np.uint64).reshape(n, self.words)
        points = rng.uniform(-5, 5, (n, cap, 3)) + np.array([0, 0, 9.0])
        self.chain = chainref.chain(self.poses, self.matches, self.counts, points, self.bits, pcap, 1)[0] if n else np.zeros(0, capi.CHAIN_DTYPE)
        self.frames = np.zeros((n + 1, pcap), capi.POINT_DTYPE)
        self.frames["row"], self.frames["col"] = rng.integers(0, 1100, (n + 1, pcap)), rng.integers(0, 2000, (n + 1, pcap))
        self.frames["padding"], self.frames["octave"] = rng.integers(0, 2, (n + 1, pcap)), rng.integers(0, 3, (n + 1, pcap))
        self.frames["value"], self.frames["level"] = rng.integers(-300, 300, (n + 1, pcap)), rng.integers(0, 6, (n + 1, pcap))
        if hostile:
            odd = rng.random((n + 1, pcap)) < 0.04
            self.frames["octave"][odd] = rng.choice([-1, 32, 31, -2 ** 31], int(odd.sum()))

    def want(self, max_dist2=4.0, min_views=2):
        return tracksref.tracks(self.poses, self.matches, self.counts, self.bits, self.pcap, self.chain, self.frames, K, max_dist2, min_views)


class Call:
    """One vslam_tracks_dev call over Inputs: the device copies, and the outputs pre-filled with a sentinel, one row more than the
    call writes."""

    def __init__(self, torch, inp):
        self.inp, n, cap = inp, inp.n, inp.cap
        dev = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape).copy()).to(DEV)
        self.d_in = dict(poses=dev(inp.poses, (n, 28), np.int32), matches=dev(inp.matches, (n, cap, 3), np.int32), match_counts=dev(inp.counts, (n,), np.int32),
                         front_bits=dev(inp.bits, (n, inp.words), np.int64), chain=dev(inp.chain, (n, 44), np.int32),
                         frame_points=dev(inp.frames, (n + 1, inp.pcap, 6), np.int32))
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.out = dict(tracks=full((n + 1, cap, 6), torch.int64), refs=full((n + 1, cap, 2), torch.int32), good_bits=full((n + 1, inp.words), torch.int64),
                        summary=full((n + 1, 4), torch.int32))

    def run(self, ctx, torch, max_dist2=4.0, min_views=2, only=None, n_pairs=None):
        outs = {k: v for k, v in self.out.items() if only is None or k in only}
        d = self.d_in
        ctx.tracks(d["poses"], d["matches"], d["match_counts"], d["front_bits"], self.inp.pcap, d["chain"], d["frame_points"], K, max_dist2, min_views,
                   n_pairs=self.inp.n if n_pairs is None else n_pairs, **outs)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def check(self, got, want):
        ms, rows, refs, goods, summary, paths = want
        n = self.inp.n
        for j in range(n):
            m = ms[j]
            g = got["tracks"][j, :m].view(capi.TRACK_DTYPE).reshape(-1)
            bad = [i for i in range(m) if g[i].tobytes() != rows[j][i].tobytes()]
            assert not bad, ("tracks", j, len(bad), bad[:4], g[bad[0]], rows[j][bad[0]])
            assert (got["tracks"][j, m:] == SENT).all(), "track rows past the count were written"
            r = got["refs"][j, :m].view(capi.TRACK_REF_DTYPE).reshape(-1)
            bad = [i for i in range(m) if r[i].tobytes() != refs[j][i].tobytes()]
            assert not bad, ("refs", j, len(bad), bad[:4], r[bad[0]], refs[j][bad[0]])
            assert (got["refs"][j, m:] == SENT).all(), "refs past the count were written"
            w = (m + 63) // 64
            assert got["good_bits"][j, :w].tobytes() == epiref.bits(goods[j], w).tobytes(), ("good_bits", j)
            assert (got["good_bits"][j, w:] == SENT).all(), "good_bits words past the count were written"
        assert got["summary"][:n].tobytes() == summary.tobytes(), (got["summary"][:n], summary)
        for name in self.out:
            assert (got[name][n] == SENT).all(), name + ": the row past n_pairs was written"


# ---- seams

@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 255, 256, 257])
@pytest.mark.parametrize("n", [2, 3, 6])
def test_chains_with_the_seam_in_each_position(env, n, m):
    ctx, torch = env
    lengths = set()
    for pos in range(n):
        ms = [300] * n
        ms[pos] = m
        inp = Inputs(ms, seed=pos)
        want = inp.want()
        call = Call(torch, inp)
        call.check(call.run(ctx, torch), want)
        lengths |= {len(p) for p in want[5].values()}
        if m >= 255 and pos == 1:
            # point_cap = 512: records share queries and trains, so some record has two candidates and keeps the lowest
            live = chainref.live_records(inp.poses[1], inp.matches[1], inp.counts[1], inp.bits[1], 512)[1]
            q = inp.matches[1]["query"][: len(live)][live]
            assert len(np.unique(q)) < len(q)
    if m >= 63:
        assert lengths >= set(range(1, n + 1)), lengths                              # tracks of 1 .. n_pairs records


def test_indices_past_the_capacity_counts_above_it_bits_past_the_count_and_untrusted_points(env):
    ctx, torch = env
    inp = Inputs([300, 200, 300], match_cap=260, counts=[300, 200, 100000])      # m = 260, 200, 260
    q, t = inp.matches["query"].astype(np.int64) & 0xFFFFFFFF, inp.matches["train"].astype(np.int64) & 0xFFFFFFFF
    assert (q[:, :200] >= 512).sum() >= 3 and (t[:, :200] >= 512).sum() >= 3 and (t > 2 ** 31).any()
    front = np.unpackbits(inp.bits[1].view(np.uint8), bitorder="little")
    assert front[200:260].sum() > 30                                              # front bits on records past m_1
    want = inp.want()
    ms, rows, refs, goods, summary, paths = want
    assert ms == [260, 200, 260]
    heads = np.concatenate([r[r["n_views"] > 0] for r in rows])
    octs = inp.frames["octave"]
    assert ((octs < 0) | (octs > 31)).sum() > 20 and (octs == 31).sum() > 5
    # an untrusted point record inside a track: NaN carried through to X and det, the canonical one, and nothing is ok
    nan = np.isnan(heads["det"])
    assert nan.sum() > 10 and (heads["X"][nan].view(np.uint64) == QNAN_BITS).all() and (heads["n_ok"][nan] == 0).all() and (heads["status"][nan] == 0).all()
    call = Call(torch, inp)
    call.check(call.run(ctx, torch), want)


def test_a_break_in_the_middle(env):
    ctx, torch = env
    inp = Inputs([300] * 6, seed=12)
    inp.chain["linked"][2] = 0                                                      # not linked, though both poses are there
    inp.poses["best"][4] = -1                                                       # no pose: no live record
    inp.chain["linked"][4] = 1                                                      # (a chain record that claims a link anyway)
    want = inp.want()
    ms, rows, refs, goods, summary, paths = want
    assert summary["n_heads"][4] == 0 and (refs[4]["pos"] == 0xFFFFFFFF).all() and max(len(p) for p in paths.values()) == 2
    assert not any(p[0][0] < 2 <= p[-1][0] for p in paths.values())
    live2 = chainref.live_records(inp.poses[2], inp.matches[2], inp.counts[2], inp.bits[2], 512)[1]
    assert summary["n_heads"][2] == live2.sum()                                     # every live record of the pair after the break is a head
    call = Call(torch, inp)
    call.check(call.run(ctx, torch), want)


# ---- numeric edge cases, on a clean scene under the true cameras

class Scene(Inputs):
    def __init__(self, n_pairs, m, seed=3):
        args, _ = small_scene(n_pairs, m, seed)
        self.poses, self.matches, self.counts, self.bits, self.pcap, self.chain, self.frames = args
        self.poses["best"] = 0
        self.n, self.cap, self.words = n_pairs, m, (m + 63) // 64


@pytest.mark.parametrize("kind", ["clean", "parallel rays", "one centre", "nan and inf", "scaled up", "scaled down", "behind"])
def test_numeric_edge_cases_equal_the_restatement(env, kind):
    ctx, torch = env
    inp = Scene(4, 70)
    ch = inp.chain
    if kind == "parallel rays":
        ch["W"][:] = np.eye(3).reshape(9)
        inp.poses["R"][:] = np.eye(3).reshape(9)
        inp.frames["col"], inp.frames["row"] = 960, 540                              # the principal point in every view: d = (0, 0, 1), P = diag(1, 1, 0) exactly
    elif kind == "one centre":
        ch["w"][:], ch["C"][:], ch["Ct"][:], ch["scale"][:] = 0.0, 0.0, 0.0, 0.0
    elif kind == "nan and inf":
        ch["W"][1][4], ch["w"][2][0], ch["Ct"][3][1] = np.nan, np.inf, -np.inf
    elif kind in ("scaled up", "scaled down"):
        s = 2.0 ** (300 if kind == "scaled up" else -300)
        for f in ("w", "C", "Ct", "scale"):
            ch[f] *= s
    elif kind == "behind":
        # every camera turned half round about its own y axis, F = diag(-1, 1, -1), where it stands: (Z0, Z1, Z2) becomes (-Z0, Z1, -Z2),
        # which projects to (u, -v) - the rows mirrored about cy keep every ray, and every point is behind every camera
        F = np.diag([-1.0, 1.0, -1.0])
        for j in range(4):
            ch["W"][j], ch["w"][j] = (F @ ch["W"][j].reshape(3, 3)).reshape(9), F @ ch["w"][j]
            inp.poses["R"][j], inp.poses["t"][j] = (F @ inp.poses["R"][j].reshape(3, 3) @ F).reshape(9), F @ inp.poses["t"][j]
        inp.frames["row"] = 1080 - inp.frames["row"]
    want = inp.want(max_dist2=4.0)
    rows = want[1][0]
    if kind == "clean":
        assert (rows["status"] == 3).all() and (rows["n_views"] == 5).all()
    elif kind == "parallel rays":
        assert (rows["det"] == 0.0).all() and (rows["status"] == 0).all() and not np.isfinite(rows["X"]).any()
    elif kind == "one centre":
        assert (rows["status"] == 1).all() and (rows["n_ok"] == 0).all() and (rows["X"] == 0.0).all()
    elif kind == "nan and inf":
        assert (rows["status"] == 0).all() and (rows["det"].view(np.uint64) == QNAN_BITS).all()
    elif kind == "scaled up":
        assert (rows["status"] == 3).all() and rows["X"][:, 2].min() > 2.0 ** 300       # the depths are 5 .. 10
    elif kind == "scaled down":
        assert (rows["status"] == 3).all() and 0 < rows["X"][:, 2].max() < 2.0 ** -296
    else:
        assert (rows["status"] == 1).all() and (rows["n_ok"] == 0).all() and (rows["n_views"] == 5).all()   # solved, every view behind its camera
    call = Call(torch, inp)
    call.check(call.run(ctx, torch), want)


# ---- whole calls

def forty_pairs():
    rng = np.random.default_rng(40)
    ms = [int(v) for v in rng.integers(100, 301, 40)]
    ms[20] = 5
    inp = Inputs(ms, seed=40)
    inp.poses["best"][[7, 30]] = -1                                                 # two pairs without a pose
    inp.chain = chainref.chain(inp.poses, inp.matches, inp.counts, np.random.default_rng(41).uniform(3, 9, (40, inp.cap, 3)), inp.bits, 512, 16)[0]
    return inp


def test_forty_unequal_pairs_and_a_repeat(env):
    ctx, torch = env
    inp = forty_pairs()
    want = inp.want()
    assert sorted(set(inp.chain["segment"].tolist())) == [0, 7, 8, 20, 21, 30, 31]
    assert max(len(p) for p in want[5].values()) >= 9
    call = Call(torch, inp)
    first = call.run(ctx, torch)
    call.check(first, want)
    again = Call(torch, inp).run(ctx, torch)                                         # a second run of the same call: identical bytes
    assert all(first[k].tobytes() == again[k].tobytes() for k in first)


def test_each_optional_output_alone_the_parameters_and_the_host_entry_point(env):
    ctx, torch = env
    inp = Inputs([257, 300, 64, 129], seed=6)
    want = inp.want(1e7, 3)                                                          # a wide test, so that good tracks exist; three views at least
    assert 0 < want[4]["n_good"].sum() < want[4]["n_heads"].sum()
    call = Call(torch, inp)
    full = call.run(ctx, torch, 1e7, 3)
    call.check(full, want)
    for only in (("tracks",), ("tracks", "refs"), ("tracks", "good_bits"), ("tracks", "summary")):
        got = Call(torch, inp).run(ctx, torch, 1e7, 3, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == full[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    one = Inputs([130], seed=8)                                                       # one pair: tracks of two views
    c1 = Call(torch, one)
    w1 = one.want(1e7)
    assert all(len(p) == 1 for p in w1[5].values())
    c1.check(c1.run(ctx, torch, 1e7), w1)
    none = Call(torch, one)
    none.run(ctx, torch, n_pairs=0)                                                   # no pairs: nothing is written
    assert all((v.cpu().numpy() == SENT).all() for v in none.out.values())
    d = call.d_in
    with pytest.raises(capi.VslamError):
        ctx.tracks(d["poses"], d["matches"], d["match_counts"], d["front_bits"], 512, d["chain"], d["frame_points"], K, 4.0, 1, tracks=call.out["tracks"])
    with pytest.raises(capi.VslamError):
        ctx.tracks(d["poses"], d["matches"], d["match_counts"], d["front_bits"], 512, d["chain"], d["frame_points"], K, 4.0, 2,
                   tracks=torch.zeros(4 * inp.cap * 6 - 1, dtype=torch.int64, device=DEV))
    # the host entry point: the same bytes, and the rows the call leaves untouched keep the caller's
    n, cap = inp.n, inp.cap
    tr, refs, good, summ = (np.full(shape, SENT, dt) for shape, dt in (((n, cap, 6), np.int64), ((n, cap, 2), np.int32), ((n, inp.words), np.int64),
                                                                        ((n, 4), np.int32)))
    ctx.tracks_host(inp.poses, inp.matches, inp.counts, inp.bits, 512, inp.chain, inp.frames, K, 1e7, 3, tracks=tr.view(capi.TRACK_DTYPE).reshape(n, cap),
                    refs=refs.view(capi.TRACK_REF_DTYPE).reshape(n, cap), good_bits=good.view(np.uint64), summary=summ.view(capi.TRACK_SUMMARY_DTYPE).reshape(n))
    assert tr.tobytes() == full["tracks"][:n].tobytes() and refs.tobytes() == full["refs"][:n].tobytes()
    assert good.tobytes() == full["good_bits"][:n].tobytes() and summ.tobytes() == full["summary"][:n].tobytes()
    alone = ctx.tracks_host(inp.poses, inp.matches, inp.counts, inp.bits, 512, inp.chain, inp.frames, K, 1e7, 3)
    for j in range(n):
        assert alone[j, : want[0][j]].tobytes() == want[1][j].tobytes()


def test_cxx_wrapper_gives_the_bytes_of_the_restatement(env, tmp_path):
    import subprocess

    r = subprocess.run([build_cxx_driver(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {l.split()[0]: bytes.fromhex(l.split()[1]) for l in r.stdout.splitlines()}
    # the buffers tests/tracks_cxx_driver.cpp builds
    n, cap = 3, 8
    poses, mt = np.zeros(n, capi.POSE_DTYPE), np.zeros((n, cap), capi.MATCH_DTYPE)
    i = np.arange(cap)
    poses["R"], poses["t"], poses["valid"], poses["n_matches"] = [0.6, 0.0, 0.8, 0.0, 1.0, 0.0, -0.8, 0.0, 0.6], [1.0, 0.0, 0.0], 1, [8, 5, 8]
    mt["query"], mt["train"] = i, (i * 3) % 8
    pts = np.stack([np.stack([i - 3.0 + 0.25 * j, 0.5 * i - 1.0, 4.0 + i + j], axis=1) for j in range(n)])
    counts, bits = np.array([8, 5, 8], np.uint32), np.array([[0xFF], [0xF7], [0xFF]], np.uint64)
    frames = np.zeros((n + 1, cap), capi.POINT_DTYPE)
    for f in range(n + 1):
        frames["row"][f], frames["col"][f], frames["padding"][f], frames["octave"][f] = 100 + 37 * i + 5 * f, 200 + 53 * i - 7 * f, 1, i % 3
    chain = chainref.chain(poses, mt, counts, pts, bits, 8, 2)[0]
    assert got["chain"] == chain.tobytes() and chain["linked"].tolist() == [0, 1, 1]
    ms, rows, refs, goods, summary, paths = tracksref.tracks(poses, mt, counts, bits, 8, chain, frames, K, 1e12, 2)
    assert max(len(p) for p in paths.values()) == 3
    wt, wr, wg = np.zeros((n, cap), capi.TRACK_DTYPE), np.full((n, cap, 2), 0xFFFFFFFF, np.uint32), np.zeros((n, 1), np.uint64)
    for j in range(n):
        wt[j, :ms[j]], wr[j, :ms[j]], wg[j] = rows[j], refs[j].view(np.uint32).reshape(-1, 2), epiref.bits(goods[j], 1)
    assert got["tracks"] == wt.tobytes() and got["refs"] == wr.tobytes() and got["good_bits"] == wg.tobytes() and got["summary"] == summary.tobytes()


def test_planted_five_frames_end_to_end_like_the_cpu_chain(env):
    """One planted five-frame scene through epipolar -> pose -> chain -> tracks on the device, nothing downloaded in between,
    against the CPU chain of the restatements."""
    ctx, torch = env
    seed, n = 1, 300
    (poses, mt, counts, pts, bits, chain, frames), maps, want, world, perms = planted_tracks(seed, n)
    from tests.test_tracks_cpu import five_frames_with_points

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
    full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
    out = dict(tracks=full((5, n, 6), torch.int64), refs=full((5, n, 2), torch.int32), good_bits=full((5, words), torch.int64), summary=full((5, 4), torch.int32))
    ctx.tracks(dposes, inliers, icounts, fb, n, dchain, dp, K, 4.0, 2, n_pairs=4, **out)
    torch.cuda.synchronize()
    assert icounts.cpu().numpy().tolist() == counts.tolist()
    assert dposes.cpu().numpy().tobytes() == poses.tobytes() and dchain.cpu().numpy().tobytes() == chain.tobytes()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    ms, rows, refs, goods, summary, paths = want
    assert summary["n_good"].sum() > 300 and max(len(p) for p in paths.values()) == 4
    for j in range(4):
        m = ms[j]
        assert got["tracks"][j, :m].tobytes() == rows[j].tobytes() and (got["tracks"][j, m:] == SENT).all(), j
        assert got["refs"][j, :m].tobytes() == refs[j].tobytes() and (got["refs"][j, m:] == SENT).all(), j
        w = (m + 63) // 64
        assert got["good_bits"][j, :w].tobytes() == epiref.bits(goods[j], w).tobytes() and (got["good_bits"][j, w:] == SENT).all(), j
    assert got["summary"][:4].tobytes() == summary.tobytes() and all((got[k][4] == SENT).all() for k in got)

"""The resection step on the GPU (vslam_resect_dev / vslam_resect_host, include/vslam.h): every comparison is bytes-equal against
the CPU restatement of the arithmetic in tests/resectref.py - the models, every hypothesis, every correspondence, every link and
every inlier word - with sentinels intact past every count.  The inputs are built directly as buffers (resectref.synthetic: a
planted rigid scene, then edited), so every seam can be placed exactly."""
import subprocess

import numpy as np
import pytest

from tests import epiref, resectref
from visualslam_amd import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -77
D2 = 4.0
OUTS = ("models", "inlier_bits", "hypotheses", "correspondences", "links")


@pytest.fixture(scope="module")
def env():
    import torch

    capi.build()
    c = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    yield c, torch
    c.close()


def with_obs_cap(d, cap):
    """The same inputs with the observation list at capacity `cap`: the rows past the old capacity repeat plausible records."""
    out = dict(d)
    old = d["obs_matches"]
    reps = -(-cap // old.shape[1])
    out["obs_matches"] = np.ascontiguousarray(np.tile(old, (1, reps))[:, :cap])
    return out


def scene(n_corr, seed, extra=None):
    """Two pairs; pair 1 has exactly n_corr usable correspondences among n_corr + extra observation records: the others, at
    random places, fail one of step 2's needs each (no link, a query or a train index past its capacity, an octave out of range)."""
    extra = n_corr // 8 + 3 if extra is None else extra
    n = n_corr + extra
    d = resectref.synthetic(2, n, seed)
    rng = np.random.default_rng(seed + 1000 * n_corr)
    bad = rng.choice(n, extra, replace=False)
    obs, tp = d["obs_matches"], d["train_points"]
    front = np.ones(n, bool)
    for k, b in enumerate(bad):
        kind = k % 5
        if kind == 0:
            obs["query"][1, b] = n + int(rng.integers(0, 5))        # past point_cap
        elif kind == 1:
            obs["query"][1, b] = -1 - int(rng.integers(0, 5))       # negative: huge as unsigned
        elif kind == 2:
            obs["train"][1, b] = n + int(rng.integers(0, 5))        # past train_cap
        elif kind == 3:
            tp["octave"][1, obs["train"][1, b]] = int(rng.choice([32, -1, 1 << 20]))   # an untrusted train point
        else:
            front[obs["query"][1, b]] = False                       # the structure record is not in front: no link
    d["front_bits"][0] = epiref.bits(front, d["front_bits"].shape[1])
    return d


class Call:
    """One vslam_resect_dev call over a dict of inputs: the device copies, and the outputs pre-filled with a sentinel, one row
    more than the call writes."""

    def __init__(self, torch, d, nh, alias=False):
        self.d, self.nh = d, nh
        self.n = n = len(d["poses"])
        self.cap, self.ocap, self.tcap = d["matches"].shape[1], d["obs_matches"].shape[1], d["train_points"].shape[1]
        self.words, self.owords = (self.cap + 63) // 64, (self.ocap + 63) // 64
        dev = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape).copy()).to(DEV)
        self.struct = (dev(d["poses"], (n, 28), np.int32), dev(d["matches"], (n, self.cap, 3), np.int32), dev(d["match_counts"].astype(np.uint32), (n,), np.int32),
                       dev(d["points"], (n, self.cap, 3), np.float64), dev(d["front_bits"], (n, self.words), np.int64))
        if alias:
            self.obs = (self.struct[1], self.struct[2])
        else:
            self.obs = (dev(d["obs_matches"], (n, self.ocap, 3), np.int32), dev(d["obs_counts"].astype(np.uint32), (n,), np.int32))
        self.train = dev(d["train_points"], (n, self.tcap, 6), np.int32)
        full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
        self.out = dict(models=full((n + 1, 30), torch.int32), inlier_bits=full((n + 1, self.owords), torch.int64),
                        hypotheses=full((n + 1, nh * 26), torch.int32), correspondences=full((n + 1, self.ocap, 6), torch.int64),
                        links=full((n + 1, self.ocap), torch.int32))

    def run(self, ctx, torch, seed=3, only=None, first=0, max_dist2=D2):
        """first: the call starts at pair `first`, every pointer advanced."""
        outs = {k: v[first:] for k, v in self.out.items() if only is None or k in only}
        ctx.resect(*(t[first:] for t in self.struct), self.d["point_cap"], self.obs[0][first:], self.obs[1][first:], self.train[first:], self.d["K"],
                   self.nh, seed, max_dist2, n_pairs=self.n - first, **outs)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.out.items()}

    def want(self, seed=3, max_dist2=D2):
        return resectref.run(self.d, self.nh, seed, max_dist2)

    def check(self, got, want):
        models, links, corrs, flags, hyps = want
        n = self.n
        rec = got["models"][:n].view(capi.RESECT_DTYPE).reshape(-1)
        for j in range(n):
            assert rec[j].tobytes() == models[j].tobytes(), ("models", j, rec[j], models[j])
            n_obs, n_corr = int(models["n_obs"][j]), int(models["n_corr"][j])
            hy = got["hypotheses"][j].view(capi.RESECT_HYP_DTYPE).reshape(-1)
            bad = [h for h in range(self.nh) if hy[h].tobytes() != hyps[j][h].tobytes()]
            assert not bad, ("hypotheses", j, len(bad), bad[:4], hy[bad[0]], hyps[j][bad[0]])
            assert got["links"][j, :n_obs].tobytes() == links[j].tobytes(), ("links", j)
            assert (got["links"][j, n_obs:] == SENT).all(), "links past the count were written"
            co = got["correspondences"][j].view(capi.RESECT_CORR_DTYPE).reshape(-1)
            assert co[:n_corr].tobytes() == corrs[j].tobytes(), ("correspondences", j)
            assert (got["correspondences"][j, n_corr:] == SENT).all(), "correspondences past n_corr were written"
            used = (n_obs + 63) // 64
            assert got["inlier_bits"][j, :used].tobytes() == epiref.bits(flags[j], used).tobytes(), ("inlier_bits", j)
            assert (got["inlier_bits"][j, used:] == SENT).all(), "inlier words past the count were written"
        for name in self.out:
            assert (got[name][n] == SENT).all(), name + ": the row past n_pairs was written"


# ---- seams

@pytest.mark.parametrize("n_corr", [0, 5, 6, 7, 63, 64, 65, 255, 256, 257, 513])
def test_two_pairs_at_the_workgroup_tile_and_compaction_seams(env, n_corr):
    ctx, torch = env
    base = scene(n_corr, 17)
    tight = base["obs_matches"].shape[1]
    for nh in (1, 64, 65, 256, 257):
        want = None
        for cap in (tight, 1100):
            d = base if cap == tight else with_obs_cap(base, cap)
            call = Call(torch, d, nh)
            want = call.want() if want is None else want            # the capacity plays no part in the result
            call.check(call.run(ctx, torch), want)
        models = want[0]
        assert int(models["n_corr"][1]) == n_corr and int(models["n_obs"][1]) == tight and int(models["best"][0]) == -1
        assert (int(models["best"][1]) >= 0) == (int(models["n_valid"][1]) > 0)
        if n_corr < 6:
            assert int(models["n_valid"][1]) == 0
        elif nh >= 64:
            assert int(models["n_valid"][1]) > 0


# ---- caps and counts

def test_counts_above_the_capacities_and_indices_past_them(env):
    ctx, torch = env
    d = scene(300, 5)
    n = d["obs_matches"].shape[1]
    d["match_counts"] = np.array([100000, n], np.uint32)                     # m_0 = the capacity
    d["obs_counts"] = np.array([n, 0xFFFFFFFF], np.uint32)                   # n_obs = the capacity
    d["point_cap"] = n - 40                                                  # the last 40 points of every frame are past point_cap
    call = Call(torch, d, 64)
    want = call.want()
    assert int(want[0]["n_obs"][1]) == n and 200 < int(want[0]["n_corr"][1]) < 300 and (want[1][1][-40:] == -1).all()
    call.check(call.run(ctx, torch), want)
    short = dict(d)
    short["train_points"] = np.ascontiguousarray(d["train_points"][:, : n - 50])     # train_cap below some train indices
    call = Call(torch, short, 64)
    want2 = call.want()
    assert int(want2[0]["n_corr"][1]) < int(want[0]["n_corr"][1])
    call.check(call.run(ctx, torch), want2)


def test_octave_31_train_points_and_an_untrusted_record_between_usable_ones(env):
    ctx, torch = env
    d = resectref.synthetic(2, 100, 9)
    d["train_points"]["octave"][1, [10, 50]] = 31                            # x' = (col - padding) * 2^30: usable, never an inlier of a sane model
    d["train_points"]["octave"][1, 30] = 32                                  # not trusted, between usable records
    d["train_points"]["octave"][1, 31] = -1
    call = Call(torch, d, 64)
    want = call.want()
    assert int(want[0]["n_corr"][1]) == 98 and 30 not in want[2][1]["b"] and 31 not in want[2][1]["b"] and 10 in want[2][1]["b"]
    assert np.abs(want[2][1]["u"]).max() > 2.0 ** 20
    call.check(call.run(ctx, torch), want)


# ---- hostile structure

def hostile(kind):
    d = resectref.synthetic(2, 130, 23)
    P, X = d["poses"], d["points"]
    if kind == "nan and inf points":
        X[0, 5:40:7, 1] = np.nan
        X[0, 6:40:7, 2] = np.inf
        X[0, 7:40:7, 0] = -np.inf
    elif kind == "one point":
        X[0, :] = X[0, 0]
    elif kind == "coplanar":
        X[0, :, 2] = 8 + 0.3 * X[0, :, 0] - 0.2 * X[0, :, 1]
    elif kind == "exactly 6":
        d["obs_counts"] = np.array([130, 6], np.uint32)
    elif kind == "behind the camera":
        X[0, ::2] = -X[0, ::2]
    elif kind == "nan in the pose":
        P["t"][0, 1] = np.nan
    elif kind == "nan in the rotation":
        P["R"][0, 4] = np.nan
    elif kind == "scaled up":
        X[0] *= 2.0 ** 300
        P["t"][0] *= 2.0 ** 300
    elif kind == "scaled down":
        X[0] *= 2.0 ** -300
        P["t"][0] *= 2.0 ** -300
    return d


@pytest.mark.parametrize("kind", ["nan and inf points", "one point", "coplanar", "exactly 6", "behind the camera", "nan in the pose", "nan in the rotation",
                                  "scaled up", "scaled down"])
def test_hostile_structure(env, kind):
    ctx, torch = env
    d = hostile(kind)
    call = Call(torch, d, 128)
    want = call.want()
    m = want[0][1]
    if kind == "nan and inf points":
        assert int(m["n_corr"]) == 130 - 15 and int(m["best"]) >= 0
    elif kind == "one point":
        assert int(m["n_corr"]) == 130 and int(m["n_valid"]) == 0 and int(m["best"]) == -1          # d == 0 in every sample
    elif kind == "exactly 6":
        assert int(m["n_corr"]) == 6 and int(m["n_valid"]) > 0
    elif kind in ("nan in the pose", "nan in the rotation"):
        assert int(m["n_corr"]) == 0 and int(m["best"]) == -1 and int(m["n_obs"]) == 130
    elif kind in ("scaled up", "scaled down"):
        assert int(m["n_corr"]) == 130 and int(m["n_valid"]) > 0 and np.isfinite(m["R"]).all() and np.isfinite(m["t"]).all()
    assert np.isfinite(want[0]["R"]).all() and np.isfinite(want[0]["t"]).all()
    call.check(call.run(ctx, torch), want)


# ---- many pairs

def test_forty_unequal_pairs_a_call_that_starts_later_and_a_repeat(env):
    ctx, torch = env
    d = resectref.synthetic(40, 300, 41, no_pose=(7, 20))
    rng = np.random.default_rng(4)
    d["match_counts"] = rng.integers(20, 301, 40).astype(np.uint32)
    d["obs_counts"] = rng.integers(0, 301, 40).astype(np.uint32)
    d["obs_counts"][[3, 12]] = [0, 5]
    call = Call(torch, d, 64)
    want = call.want(seed=9)
    models = want[0]
    assert models["n_corr"][[0, 8, 21, 3]].tolist() == [0, 0, 0, 0] and int(models["best"][12]) == -1 and (models["best"] >= 0).sum() >= 30
    full = call.run(ctx, torch, seed=9)
    call.check(full, want)
    again = Call(torch, d, 64).run(ctx, torch, seed=9)                          # a repeat: identical bytes
    assert all(full[k].tobytes() == again[k].tobytes() for k in full)
    # a second call that starts at pair s, its seed advanced by s: pairs s + 1 .. give the same records (pair s is its pair 0)
    s = 15
    part = Call(torch, d, 64).run(ctx, torch, seed=9 + s, first=s)
    for k in OUTS:
        assert part[k][s + 1:].tobytes() == full[k][s + 1:].tobytes(), k
        assert (part[k][:s] == SENT).all(), k
    first = part["models"][s].view(capi.RESECT_DTYPE)[0]
    assert int(first["best"]) == -1 and int(first["n_corr"]) == 0 and int(first["n_obs"]) == int(models["n_obs"][s])


# ---- outputs, aliasing, the host form, the C++ wrapper

def test_each_optional_output_alone_the_aliased_list_and_the_host_entry_point(env):
    ctx, torch = env
    d = resectref.synthetic(3, 290, 6)
    d["obs_counts"] = np.array([290, 257, 129], np.uint32)
    call = Call(torch, d, 65)
    want = call.want()
    full = call.run(ctx, torch)
    call.check(full, want)
    for only in (("models",), ("models", "inlier_bits"), ("models", "hypotheses"), ("models", "correspondences"), ("models", "links")):
        got = Call(torch, d, 65).run(ctx, torch, only=only)
        for k in got:
            if k in only:
                assert got[k].tobytes() == full[k].tobytes(), (only, k)
            else:
                assert (got[k] == SENT).all(), (only, k)
    none = Call(torch, d, 65)
    ctx.resect(*none.struct, d["point_cap"], *none.obs, none.train, d["K"], 65, 3, D2, n_pairs=0, **none.out)     # no pairs: nothing is written
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == SENT).all() for v in none.out.values())
    one = Call(torch, resectref.synthetic(1, 70, 2), 16)                          # one pair: no links, no model
    w1 = one.want()
    assert int(w1[0]["best"][0]) == -1
    one.check(one.run(ctx, torch), w1)
    with pytest.raises(capi.VslamError):
        ctx.resect(*call.struct, d["point_cap"], *call.obs, call.train, d["K"], 0, 3, D2, models=call.out["models"])          # no hypotheses
    with pytest.raises(capi.VslamError):
        ctx.resect(*call.struct, d["point_cap"], *call.obs, call.train, d["K"], 65, 3, D2, models=torch.zeros(3 * 30 - 1, dtype=torch.int32, device=DEV))
    # the observation list aliased onto the structure list: the very same device buffers
    al = dict(d)
    al["obs_matches"], al["obs_counts"] = d["matches"], d["match_counts"]
    ac = Call(torch, al, 65, alias=True)
    assert ac.obs[0].data_ptr() == ac.struct[1].data_ptr()
    ac.check(ac.run(ctx, torch), ac.want())
    # the host entry point: the same bytes, and the rows the call leaves untouched keep the caller's
    n, ocap = 3, 290
    ib, hy = np.full((n, (ocap + 63) // 64), SENT, np.int64), np.zeros((n, 65), capi.RESECT_HYP_DTYPE)
    co, links = np.full((n, ocap, 6), SENT, np.int64), np.full((n, ocap), SENT, np.int32)
    hm = ctx.resect_host(*(d[k] for k in resectref.ARGS), 65, 3, D2, inlier_bits=ib.view(np.uint64), hypotheses=hy,
                         correspondences=co.view(capi.RESECT_CORR_DTYPE).reshape(n, ocap), links=links)
    assert hm.tobytes() == want[0].tobytes()
    assert ib.tobytes() == full["inlier_bits"][:n].tobytes() and hy.tobytes() == full["hypotheses"][:n].tobytes()
    assert co.tobytes() == full["correspondences"][:n].tobytes() and links.tobytes() == full["links"][:n].tobytes()
    assert ctx.resect_host(*(d[k] for k in resectref.ARGS), 65, 3, D2).tobytes() == want[0].tobytes()


def test_cxx_wrapper_gives_the_bytes_of_the_restatement(env, tmp_path):
    from tests.test_resect_cpu import build_cxx_driver

    r = subprocess.run([build_cxx_driver(tmp_path), "run"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {l.split()[0]: bytes.fromhex(l.split()[1]) for l in r.stdout.splitlines()}
    # the buffers tests/resect_cxx_driver.cpp builds
    n, cap = 2, 8
    i = np.arange(cap)
    poses, mt, tp = np.zeros(n, capi.POSE_DTYPE), np.zeros((n, cap), capi.MATCH_DTYPE), np.zeros((n, cap), capi.POINT_DTYPE)
    poses["R"], poses["t"], poses["valid"], poses["n_matches"] = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0], [1.0, 0.0, 0.0], 1, 8
    mt["query"] = mt["train"] = i
    pts = np.stack([np.stack([(i - 3.5) * 0.7, ((i * 3) % 8 - 3.5) * 0.5, np.array([6.0, 9.5, 7.0, 8.0, 10.5, 6.5, 9.0, 7.5])], axis=1)] * n)
    tp["col"], tp["row"], tp["octave"] = [1740, 1943, 2096, 2223, 2270, 2638, 2577, 2858], [622, 1046, 1382, 836, 1126, 1535, 953, 1256], 0
    counts, bits = np.array([8, 8], np.uint32), np.array([[0xFF], [0xFF]], np.uint64)
    models, links, corrs, flags, _ = resectref.resect(poses, mt, counts, pts, bits, 8, mt, counts, tp, (800.0, 800.0, 960.0, 540.0), 64, 3, 4.0)
    assert int(models["n_corr"][1]) == 8 and int(models["best"][1]) >= 0 and int(models["n_inliers"][1]) == 8
    assert got["models"] == models.tobytes()
    wb, wc, wl = np.zeros((n, 1), np.uint64), np.zeros((n, cap), capi.RESECT_CORR_DTYPE), np.full((n, cap), -1, np.int32)
    for j in range(n):
        wb[j] = epiref.bits(flags[j], 1)
        wc[j, : len(corrs[j])], wl[j, : len(links[j])] = corrs[j], links[j]
    assert got["bits"] == wb.tobytes() and got["correspondences"] == wc.tobytes() and got["links"] == wl.tobytes()


# ---- end to end on planted data

@pytest.mark.parametrize("rotation", [False, True])
def test_planted_frames_end_to_end_like_the_cpu_chain(env, rotation):
    """A planted five-frame scene (and the same with a pure rotation at pair 1) through epipolar -> homography gate -> pose ->
    resect on the device, nothing downloaded in between, against the CPU chain of the restatements."""
    from tests import test_chain_cpu as T
    from tests.test_resect_cpu import K, NH, ROT_ONLY, planted

    ctx, torch = env
    seed, n = 1, 300
    inputs, _, judged = planted(seed, n, ROT_ONLY if rotation else T.BASELINES, True)
    want = resectref.run(inputs, NH, seed, D2)
    assert [int(x["degenerate"]) for x in judged] == ([0, 1, 0, 0] if rotation else [0, 0, 0, 0])
    assert (want[0]["best"][1:] >= 0).tolist() == ([True, False, True] if rotation else [True, True, True])
    words = (n + 63) // 64
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV)
    dev = lambda a, shape, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt).reshape(shape).copy()).to(DEV)
    raw, rcounts = dev(inputs["obs_matches"], (4, n, 3), np.int32), dev(inputs["obs_counts"], (4,), np.int32)
    # the five point lists: frame 0's is not among the inputs of the resection, so it is rebuilt as planted() built it
    saved = T.BASELINES
    T.BASELINES = ROT_ONLY if rotation else saved
    try:
        lists = T.five_frames(seed, n)[1]
    finally:
        T.BASELINES = saved
    pts = dev(np.stack(lists), (5, n, 6), np.int32)
    models, inliers, icounts = z((4, 22), torch.int32), z((4, n, 3), torch.int32), z((4,), torch.int32)
    ctx.epipolar(raw, rcounts, pts[:4], pts[1:], 4, NH, seed, D2, models=models, inliers=inliers, inlier_counts=icounts)
    hm, gated = z((4, 42), torch.int32), z((4, 22), torch.int32)
    ctx.homography(raw, rcounts, pts[:4], pts[1:], 4, NH, seed, D2, epipolar_models=models, models=hm, gated_models=gated)
    dposes, X, fb = z((4, 28), torch.int32), z((4, n, 3), torch.float64), z((4, words), torch.int64)
    ctx.pose(gated, inliers, icounts, pts[:4], pts[1:], K, poses=dposes, points=X, front_bits=fb)
    full = lambda shape, dt: torch.full(shape, SENT, dtype=dt, device=DEV)
    out = dict(models=full((5, 30), torch.int32), inlier_bits=full((5, words), torch.int64), links=full((5, n), torch.int32))
    ctx.resect(dposes, inliers, icounts, X, fb, n, raw, rcounts, pts[1:], K, NH, seed, D2, n_pairs=4, **out)
    torch.cuda.synchronize()
    assert icounts.cpu().numpy().tolist() == inputs["match_counts"].tolist()
    assert dposes.cpu().numpy().tobytes() == inputs["poses"].tobytes()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["models"][:4].tobytes() == want[0].tobytes(), (got["models"][:4].view(capi.RESECT_DTYPE), want[0])
    for j in range(4):
        assert got["links"][j].tobytes() == want[1][j].tobytes()
        assert got["inlier_bits"][j].tobytes() == epiref.bits(want[3][j], words).tobytes()
    assert all((got[k][4] == SENT).all() for k in got)

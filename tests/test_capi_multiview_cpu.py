"""What the bindings of the five multi-view stages (capi.Context.chain, resect, resect_refine, tracks, bundle and their *_host
twins) do before the library is called, held without a GPU, a context or the library.

The checks are module-level helpers of capi.py (_check_tensors, _check_records, _check_sets, _host_structure, _check_host_outs,
_fill_out); the wrappers state what each stage passes them.  Here every wrapper runs over CPU tensors and numpy arrays on a bare
Context whose `where` is the CPU, with capi.lib replaced by a recorder: one call per ValueError a wrapper can raise before it
reaches the library, with the whole message asserted, and one valid call whose n, capacities and out struct (pointers, _bytes,
struct_size) are compared with the values worked out by hand."""
import ctypes as C

import numpy as np
import pytest
import torch

from visualslam_amd import capi

N, CAP, PCAP, OCAP, TCAP, H = 3, 70, 50, 40, 60, 8
WORDS, OWORDS = 2, 1
K = (800.0, 800.0, 960.0, 540.0)


class Recorder:
    """Stands in for the loaded library: every entry point returns 0 and keeps its arguments."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def ctx(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    c = object.__new__(capi.Context)
    c._h, c.device, c.where, c.rec = None, 0, torch.device("cpu"), rec
    return c


def raw(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8)


def structure():
    return dict(poses=raw(N * 112), matches=torch.zeros(N, CAP, 3, dtype=torch.int32), match_counts=torch.zeros(N, dtype=torch.int32),
                front_bits=torch.zeros(N, WORDS, dtype=torch.int64), point_cap=PCAP)


def dev_call(stage):
    """A valid device call of the stage: keyword arguments, the names of its output tensors, and its scalars in the ABI's call by position."""
    s = structure()
    pts = dict(points=torch.zeros(N, CAP, 3, dtype=torch.float64))
    trk = dict(chain=raw(N * 176), frame_points=torch.zeros(N + 1, PCAP, 6, dtype=torch.int32), intrinsics=K)
    if stage == "chain":
        return dict(**s, **pts, chain=raw(N * 176), map=torch.zeros(N, CAP, 3, dtype=torch.float64), links=torch.zeros(N, CAP, dtype=torch.int32),
                    ratios=torch.zeros(N, CAP, dtype=torch.float64)), ("chain", "map", "links", "ratios"), {4: CAP, 7: PCAP, 8: N}
    if stage == "tracks":
        return dict(**s, **trk, tracks=raw(N * CAP * 48), refs=raw(N * CAP * 8), good_bits=torch.zeros(N, WORDS, dtype=torch.int64),
                    summary=raw(N * 16)), ("tracks", "refs", "good_bits", "summary"), {4: CAP, 6: PCAP, 7: N}
    if stage == "bundle":
        return dict(**s, **trk, tracks_in=raw(N * CAP * 48), refs=raw(N * CAP * 8), cams_in=raw(N * 160), tracks=raw(N * CAP * 48), cams=raw(N * 160),
                    point_info=raw(N * CAP * 40), member_bits=torch.zeros(N, 2, WORDS, dtype=torch.int64)), ("tracks", "cams", "point_info", "member_bits"), \
            {4: CAP, 6: PCAP, 7: N}
    if stage == "resect":
        return dict(**s, **pts, obs_matches=torch.zeros(N, OCAP, 3, dtype=torch.int32), obs_counts=torch.zeros(N, dtype=torch.int32),
                    train_points=torch.zeros(N, TCAP, 6, dtype=torch.int32), intrinsics=K, n_hypotheses=H, models=raw(N * 120),
                    inlier_bits=torch.zeros(N, OWORDS, dtype=torch.int64), hypotheses=raw(N * H * 104), correspondences=raw(N * OCAP * 48),
                    links=torch.zeros(N, OCAP, dtype=torch.int32)), ("models", "inlier_bits", "hypotheses", "correspondences", "links"), \
            {4: CAP, 7: PCAP, 10: OCAP, 12: TCAP, 13: N}
    assert stage == "resect_refine"
    return dict(models_in=raw(N * 120), correspondences=raw(N * OCAP * 48), obs_cap=OCAP, intrinsics=K, models=raw(N * 120), info=raw(N * 32),
                inlier_bits=torch.zeros(N, OWORDS, dtype=torch.int64)), ("models", "info", "inlier_bits"), {3: OCAP, 4: N}


FIRST = {"chain": "poses", "tracks": "poses", "bundle": "poses", "resect": "poses", "resect_refine": "models_in"}
LAST_REQUIRED = {"chain": "chain", "tracks": "tracks", "bundle": "cams", "resect": "models", "resect_refine": "models"}
FEWER = {s: f"{s}: fewer sets than pairs" for s in ("chain", "tracks", "bundle", "resect")}
FEWER["resect_refine"] = "resect_refine: models_in must hold n_pairs * 120 bytes, correspondences n_pairs * obs_cap * 48"
STAGES = ("chain", "resect", "resect_refine", "tracks", "bundle")


def out_fields(out):
    return {name: getattr(out, name) for name, _ in out._fields_}


def by_hand(kw, outs, struct):
    want = {"struct_size": C.sizeof(struct)}
    for name in outs:
        want[name], want[name + "_bytes"] = kw[name].data_ptr(), kw[name].numel() * kw[name].element_size()
    return want


@pytest.mark.parametrize("stage", STAGES)
def test_device_wrapper_passes_a_valid_call_on_as_worked_out_by_hand(ctx, stage):
    kw, outs, scalars = dev_call(stage)
    getattr(ctx, stage)(**kw)
    (name, args), = ctx.rec.calls
    assert name == f"vslam_{stage}_dev"
    for at, v in scalars.items():
        assert args[at] == v, (at, args[at], v)
    out = args[-1]._obj
    assert out_fields(out) == by_hand(kw, outs, type(out))
    # the optional outputs left out: null pointers, no bytes
    ctx.rec.calls.clear()
    getattr(ctx, stage)(**{k: v for k, v in kw.items() if k not in outs[1:] or k == LAST_REQUIRED[stage]})
    left = out_fields(ctx.rec.calls[0][1][-1]._obj)
    for name in outs[1:]:
        if name != LAST_REQUIRED[stage]:
            assert left[name] is None and left[name + "_bytes"] == 0


@pytest.mark.parametrize("stage", STAGES)
def test_device_wrapper_errors_before_the_library(ctx, stage):
    def says(message, **change):
        kw = dev_call(stage)[0]
        kw.update(change)
        with pytest.raises(ValueError) as e:
            getattr(ctx, stage)(**kw)
        assert str(e.value) == message
        assert not ctx.rec.calls

    first, kw = FIRST[stage], dev_call(stage)[0]
    ctx.where = torch.device("cuda", 0)
    says(f"{stage}: {first} must be a contiguous tensor on cuda:0")                   # wrong device: the first tensor in argument order
    ctx.where = torch.device("cpu")
    last_out = dev_call(stage)[1][-1]
    says(f"{stage}: {last_out} must be a contiguous tensor on cpu", **{last_out: torch.zeros(N * 64, 4, dtype=torch.int64)[:, :2]})   # not contiguous
    says(f"{stage}: {first} is required", **{first: None})
    says(f"{stage}: {LAST_REQUIRED[stage]} is required", **{LAST_REQUIRED[stage]: None})
    says(FEWER[stage], n_pairs=N + 1)                                                 # too few sets, through every list in turn
    for name in {"chain": ("poses", "points", "front_bits", "match_counts"), "tracks": ("poses", "chain", "front_bits", "frame_points"),
                 "bundle": ("chain", "frame_points", "tracks_in", "refs", "cams_in"), "resect": ("poses", "points", "front_bits", "obs_counts", "obs_matches", "train_points"),
                 "resect_refine": ("models_in", "correspondences")}[stage]:
        t = kw[name]
        says(FEWER[stage], n_pairs=N, **{name: t[:-1].contiguous()})
    if stage != "resect_refine":
        says(FEWER[stage], match_counts=torch.zeros(N, dtype=torch.int64))            # counts that are not 4-byte
        shape = "[n, cap, 3]" if stage == "resect" else "[n, match_cap, 3]"
        says(f"{stage}: matches must be {shape} 4-byte elements", matches=torch.zeros(N, CAP, 2, dtype=torch.int32))   # wrong record width
        says(f"{stage}: matches must be {shape} 4-byte elements", matches=torch.zeros(N * CAP, 3, dtype=torch.int32))
    if stage == "resect":
        says("resect: obs_matches must be [n, cap, 3] 4-byte elements", obs_matches=torch.zeros(N, OCAP, 3, dtype=torch.int64))
        says("resect: train_points must be [n, train_cap, 6] 4-byte elements", train_points=torch.zeros(N, TCAP, 3, dtype=torch.int32))
    if stage == "bundle":
        ctx.bundle(**{**kw, "cams_in": None})                                         # (optional)
        assert ctx.rec.calls.pop()[1][12] is None


def host_call(stage):
    """A valid host call of the stage: keyword arguments, the optional outputs with (dtype, elements), the broken-input message."""
    s = dict(poses=np.zeros(N, capi.POSE_DTYPE), matches=np.zeros((N, CAP), capi.MATCH_DTYPE), match_counts=np.zeros(N, np.uint32),
             front_bits=np.zeros((N, WORDS), np.uint64), point_cap=PCAP)
    pts = dict(points=np.zeros((N, CAP, 3)))
    trk = dict(chain=np.zeros(N, capi.CHAIN_DTYPE), frame_points=np.zeros((N + 1, PCAP), capi.POINT_DTYPE), intrinsics=K)
    if stage == "chain":
        return dict(**s, **pts), dict(map=(np.float64, N * CAP * 3), links=(np.int32, N * CAP), ratios=(np.float64, N * CAP)), \
            "chain_host: one count, match_cap points and (match_cap + 63) // 64 words per pair"
    if stage == "tracks":
        return dict(**s, **trk), dict(tracks=(capi.TRACK_DTYPE, N * CAP), refs=(capi.TRACK_REF_DTYPE, N * CAP), good_bits=(np.uint64, N * WORDS),
                                      summary=(capi.TRACK_SUMMARY_DTYPE, N)), \
            "tracks_host: one count, one chain record and (match_cap + 63) // 64 words per pair, point_cap points per frame"
    if stage == "bundle":
        return dict(**s, **trk, tracks_in=np.zeros((N, CAP), capi.TRACK_DTYPE), refs=np.zeros((N, CAP), capi.TRACK_REF_DTYPE),
                    cams_in=np.zeros(N, capi.BUNDLE_CAM_DTYPE)), \
            dict(tracks=(capi.TRACK_DTYPE, N * CAP), point_info=(capi.BUNDLE_POINT_DTYPE, N * CAP), member_bits=(np.uint64, N * 2 * WORDS)), \
            ("bundle_host: one count, one chain record, one camera and (match_cap + 63) // 64 words per pair, match_cap tracks and refs, "
             "point_cap points per frame")
    if stage == "resect":
        return dict(**s, **pts, obs_matches=np.zeros((N, OCAP), capi.MATCH_DTYPE), obs_counts=np.zeros(N, np.uint32),
                    train_points=np.zeros((N, TCAP), capi.POINT_DTYPE), intrinsics=K, n_hypotheses=H), \
            dict(inlier_bits=(np.uint64, N * OWORDS), hypotheses=(capi.RESECT_HYP_DTYPE, N * H), correspondences=(capi.RESECT_CORR_DTYPE, N * OCAP),
                 links=(np.int32, N * OCAP)), "resect_host: one count, match_cap points and (match_cap + 63) // 64 words per pair"
    assert stage == "resect_refine"
    return dict(models_in=np.zeros(N, capi.RESECT_DTYPE), correspondences=np.zeros((N, OCAP), capi.RESECT_CORR_DTYPE), intrinsics=K), \
        dict(inlier_bits=(np.uint64, N * OWORDS)), None


@pytest.mark.parametrize("stage", STAGES)
def test_host_wrapper_passes_a_valid_call_on_and_names_every_bad_output(ctx, stage):
    kw, outs, _ = host_call(stage)
    given = {name: np.zeros(size, dt) for name, (dt, size) in outs.items()}
    ret = getattr(ctx, stage + "_host")(**kw, **given)
    (name, args), = ctx.rec.calls
    assert name == f"vslam_{stage}_host"
    out = args[-1]._obj
    got = out_fields(out)
    assert got["struct_size"] == C.sizeof(type(out))
    for name, a in given.items():
        assert got[name] == a.ctypes.data and got[name + "_bytes"] == a.nbytes == a.size * np.dtype(outs[name][0]).itemsize
    # the outputs the wrapper makes itself: n records each, returned to the caller
    made = {"chain": ("chain",), "resect": ("models",), "resect_refine": ("models", "info"), "tracks": (), "bundle": ("cams",)}[stage]
    sizes = dict(chain=176, models=120, info=32, cams=160)
    rets = ret if isinstance(ret, tuple) else (ret,)
    for name in made:
        assert got[name + "_bytes"] == N * sizes[name] and any(r.ctypes.data == got[name] and len(r) == N for r in rets)
    scalars = {"chain": {4: CAP, 7: PCAP, 8: N}, "tracks": {4: CAP, 6: PCAP, 7: N}, "bundle": {4: CAP, 6: PCAP, 7: N},
               "resect": {4: CAP, 7: PCAP, 10: OCAP, 12: TCAP, 13: N}, "resect_refine": {3: OCAP, 4: N}}[stage]
    for at, v in scalars.items():
        assert args[at] == v, (at, args[at], v)
    ctx.rec.calls.clear()
    for name, (dt, size) in outs.items():
        message = f"{stage}_host: {name} must be a C-contiguous {np.dtype(dt).name} array of {size} elements"
        other = np.float32 if np.dtype(dt) != np.float32 else np.int32
        for bad in (np.zeros(size, other), np.zeros(size + 1, dt), np.zeros(2 * size, dt)[::2], [0] * size):   # dtype, size, contiguity, no array
            with pytest.raises(ValueError) as e:
                getattr(ctx, stage + "_host")(**kw, **{name: bad})
            assert str(e.value) == message
    assert not ctx.rec.calls


@pytest.mark.parametrize("stage", STAGES)
def test_host_wrapper_errors_over_its_inputs(ctx, stage):
    kw, _, message = host_call(stage)

    def says(message, **change):
        with pytest.raises(ValueError) as e:
            getattr(ctx, stage + "_host")(**{**kw, **change})
        assert str(e.value) == message
        assert not ctx.rec.calls

    if stage == "resect_refine":
        says("resect_refine_host: correspondences must be [n, obs_cap]", correspondences=kw["correspondences"][:-1])
        says("resect_refine_host: correspondences must be [n, obs_cap]", correspondences=kw["correspondences"].reshape(-1))
        return
    shape = "resect_host: matches, obs_matches and train_points must be [n, capacity]" if stage == "resect" else f"{stage}_host: matches must be [n, match_cap]"
    says(shape, matches=kw["matches"][:-1])
    says(shape, matches=kw["matches"].reshape(-1))
    if stage == "resect":
        says(shape, obs_matches=kw["obs_matches"][:-1])
        says(shape, train_points=kw["train_points"].reshape(-1))
    lists = {"chain": ("match_counts", "points", "front_bits"), "resect": ("match_counts", "obs_counts", "points", "front_bits"),
             "tracks": ("match_counts", "front_bits", "chain", "frame_points"),
             "bundle": ("match_counts", "front_bits", "chain", "frame_points", "tracks_in", "refs", "cams_in")}[stage]
    for name in lists:
        says(message, **{name: kw[name][:-1]})

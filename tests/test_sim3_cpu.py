"""Frame structure and loop alignment without a GPU: the C ABI's new symbols, struct layouts and argument checks, the bindings
over CPU tensors, the C++ wrapper failing loudly, and the CPU restatement of the arithmetic itself (tests/sim3ref.py), which the
GPU tests compare against byte for byte: the frame rule on hand-made chains, Horn's closed form against an SVD solution, the
composition against numpy products, and the planted two-visit scenes that are the measurement behind the documented default of
max_dist2."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import chainref, epiref, poseref, sim3ref
from tests.test_chain_cpu import random_rotation, synthetic_chain
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
K = (800.0, 800.0, 960.0, 540.0)
KERNELS = (b"k_frame_index", b"k_frame_cams", b"k_sim3_corr", b"k_sim3_gather", b"k_sim3_models", b"k_sim3_score", b"k_sim3_select", b"k_sim3_flags")
ENTRIES = ("vslam_frame_world_dev", "vslam_frame_world_host", "vslam_sim3_dev", "vslam_sim3_host")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- the ABI

def test_sim3_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ENTRIES:
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in KERNELS:
        assert k in names


def test_sim3_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_frame_cam": capi.FrameCam, "vslam_frame_world_out": capi.FrameWorldOut, "vslam_sim3_side": capi.Sim3Side,
               "vslam_sim3_params": capi.Sim3Params, "vslam_sim3_hyp": capi.Sim3Hyp, "vslam_sim3_corr": capi.Sim3Corr, "vslam_sim3": capi.Sim3,
               "vslam_sim3_out": capi.Sim3Out}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()}
    for cname, ct in structs.items():
        assert rows[cname] == [C.sizeof(ct)] + [getattr(ct, f[0]).offset for f in ct._fields_], cname
    for cname, ct, dt, size in (("vslam_frame_cam", capi.FrameCam, capi.FRAME_CAM_DTYPE, 112), ("vslam_sim3_hyp", capi.Sim3Hyp, capi.SIM3_HYP_DTYPE, 112),
                                ("vslam_sim3_corr", capi.Sim3Corr, capi.SIM3_CORR_DTYPE, 88), ("vslam_sim3", capi.Sim3, capi.SIM3_DTYPE, 136)):
        assert rows[cname][0] == size == dt.itemsize, cname
        assert [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_], cname
    assert rows["vslam_sim3_side"][0] == 56 and C.sizeof(sim3ref.Side) == 56


class FrameArgs:
    """A valid vslam_frame_world_dev / _host call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, match_cap=100, point_cap=50):
        words = (match_cap + 63) // 64
        self.keep = [np.zeros(n_pairs, capi.POSE_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32),
                     np.zeros((n_pairs, words), np.uint64), np.zeros(n_pairs, capi.CHAIN_DTYPE), np.zeros(n_pairs + 1, capi.FRAME_CAM_DTYPE),
                     np.zeros((n_pairs + 1, point_cap), np.int32)]
        self.poses, self.matches, self.counts, self.bits, self.chain = (a.ctypes.data for a in self.keep[:5])
        self.match_cap, self.point_cap, self.n_pairs = match_cap, point_cap, n_pairs
        cams, index = self.keep[5:]
        self.out = capi.FrameWorldOut(C.sizeof(capi.FrameWorldOut), cams.ctypes.data, cams.nbytes, index.ctypes.data, index.nbytes)

    def call(self, fn, out="out"):
        return fn(None, self.poses, self.matches, self.counts, self.match_cap, self.bits, self.point_cap, self.chain, self.n_pairs,
                  None if out is None else C.byref(self.out))


class Sim3Args:
    """A valid vslam_sim3_dev / _host call over host arrays: 3 slots of capacity 70 between two sides."""

    def __init__(self):
        self.keep = [np.zeros(8, capi.FRAME_CAM_DTYPE), np.zeros((8, 50), np.int32), np.zeros((7, 100, 3)), np.zeros((8, 60), capi.POINT_DTYPE),
                     np.zeros(3, capi.SET_PAIR_DTYPE), np.zeros((3, 70), capi.MATCH_DTYPE), np.zeros(3, np.uint32), np.zeros((3, 2), np.uint64),
                     np.zeros(3, capi.SIM3_DTYPE), np.zeros((3, 2), np.uint64), np.zeros((3, 16), capi.SIM3_HYP_DTYPE), np.zeros((3, 70), capi.SIM3_CORR_DTYPE),
                     np.zeros((3, 70, 2), np.int32)]
        cams, index, mp, pts, pairs, mt, cnt, sel, models, bits, hyps, corr, links = self.keep
        self.q = capi.Sim3Side(cams.ctypes.data, index.ctypes.data, mp.ctypes.data, pts.ctypes.data, 100, 50, 60, 7, 8, 0)
        self.t = capi.Sim3Side(cams.ctypes.data, index.ctypes.data, mp.ctypes.data, pts.ctypes.data, 100, 50, 60, 7, 8, 0)
        self.pairs, self.matches, self.counts, self.select = (a.ctypes.data for a in (pairs, mt, cnt, sel))
        self.match_cap, self.n_pairs = 70, 3
        self.prm = capi.Sim3Params(16, 1, 16.0, capi.PoseParams(*K))
        self.out = capi.Sim3Out(C.sizeof(capi.Sim3Out), models.ctypes.data, models.nbytes, bits.ctypes.data, bits.nbytes, hyps.ctypes.data, hyps.nbytes,
                                corr.ctypes.data, corr.nbytes, links.ctypes.data, links.nbytes)

    def call(self, fn, q="q", t="t", prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return fn(None, ref(q), ref(t), self.pairs, self.matches, self.counts, self.match_cap, self.select, self.n_pairs, ref(prm), ref(out))


def _bad(cls, fn, **change):
    a = cls()
    for k, v in change.items():
        obj, field = k.split("__")
        setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
    return a.call(fn)


@pytest.mark.parametrize("entry", ["vslam_frame_world_dev", "vslam_frame_world_host"])
def test_frame_world_rejects_bad_arguments_before_it_needs_a_gpu(lib, entry):
    fn, gpu = getattr(lib, entry), torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert FrameArgs().call(fn) == (INVALID if gpu else HIP)
    assert FrameArgs().call(fn, out=None) == INVALID
    bad = lambda **c: _bad(FrameArgs, fn, **c)
    for name in ("poses", "matches", "counts", "bits", "chain"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.FrameWorldOut) - 8) == INVALID
    assert bad(out__cams=None) == INVALID and bad(out__cams_bytes=3 * 112 - 1) == INVALID
    assert bad(out__index=None) == INVALID and bad(out__index_bytes=3 * 50 * 4 - 1) == INVALID
    assert bad(a__match_cap=0) == INVALID and bad(a__point_cap=0) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    if not gpu:  # no pairs and one pair are valid calls
        assert bad(a__n_pairs=0) == HIP and bad(a__n_pairs=1) == HIP and bad(a__n_pairs=0, out__cams_bytes=0, out__index_bytes=0) == HIP


@pytest.mark.parametrize("entry", ["vslam_sim3_dev", "vslam_sim3_host"])
def test_sim3_rejects_bad_arguments_before_it_needs_a_gpu(lib, entry):
    fn, gpu = getattr(lib, entry), torch.cuda.is_available()
    assert Sim3Args().call(fn) == (INVALID if gpu else HIP)
    for name in ("q", "t", "prm", "out"):
        assert Sim3Args().call(fn, **{name: None}) == INVALID, name
    bad = lambda **c: _bad(Sim3Args, fn, **c)
    for name in ("pairs", "matches", "counts"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.Sim3Out) - 8) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID and bad(a__match_cap=0) == INVALID
    assert bad(prm__n_hypotheses=0) == INVALID and bad(prm__n_hypotheses=65536) == INVALID
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert bad(prm__max_dist2=v) == INVALID, v
    for k in (capi.PoseParams(0.0, 800.0, 1.0, 1.0), capi.PoseParams(800.0, -1.0, 1.0, 1.0), capi.PoseParams(800.0, 800.0, float("nan"), 1.0),
              capi.PoseParams(800.0, 800.0, 1.0, float("inf"))):
        assert bad(prm__K=k) == INVALID
    for side in ("q", "t"):
        for field in ("cams", "index", "map", "points"):
            assert bad(**{f"{side}__{field}": None}) == INVALID, (side, field)
        for field in ("map_cap", "point_cap", "points_cap", "n_map_pairs"):
            assert bad(**{f"{side}__{field}": 0}) == INVALID, (side, field)
        assert bad(**{f"{side}__n_frames": -1}) == INVALID and bad(**{f"{side}__n_frames": 65537}) == INVALID
        assert bad(**{f"{side}__n_map_pairs": 65536}) == INVALID and bad(**{f"{side}__reserved": 1}) == INVALID
    assert bad(out__models=None) == INVALID and bad(out__models_bytes=3 * 136 - 1) == INVALID
    assert bad(out__inlier_bits_bytes=3 * 2 * 8 - 1) == INVALID and bad(out__hypotheses_bytes=3 * 16 * 112 - 1) == INVALID
    assert bad(out__correspondences_bytes=3 * 70 * 88 - 1) == INVALID and bad(out__links_bytes=3 * 70 * 8 - 1) == INVALID
    if not gpu:  # the optional input and outputs may be absent; no slots, no frames and the extremes are valid calls
        assert bad(a__select=None, out__inlier_bits=None, out__hypotheses=None, out__correspondences=None, out__links=None) == HIP
        assert bad(a__n_pairs=0) == HIP and bad(q__n_frames=0) == HIP and bad(t__n_frames=65536, t__n_map_pairs=65535) == HIP
        assert bad(prm__n_hypotheses=1) == HIP and bad(prm__seed=0xFFFFFFFF) == HIP


def _sanitized(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "sim3_plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "sim3_plan_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    return str(exe)


def test_plan_and_argument_checks_under_the_sanitizers(tmp_path):
    out = subprocess.run([_sanitized(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    assert rows["frames"]["bad"] == "0" and int(rows["frames"]["checked"]) == 21 * 21 * 15 * 5, rows["frames"]
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 15 * 10 * 10, rows["plan"]
    assert rows["fargs"]["bad"] == "0" and int(rows["fargs"]["checked"]) >= 28, rows["fargs"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 78, rows["args"]   # (every message and the order of the checks)
    src = open(os.path.join(CSRC, "vslam_sim3_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


def hostile_matrices():
    rng = np.random.default_rng(31)
    ms = [np.eye(3), np.diag([2.0, 0, 0]), np.zeros((3, 3)), np.outer([1.0, 2.0, 3.0], [4.0, -5.0, 6.0]), np.diag([1.0, 1.0, -1.0]),     # rank 1, 0; a reflection
          np.array([[2.0, 0, 1], [0, 3, 1], [0, 0, 1]])]
    ms += [rng.standard_normal((3, 3)) * 10.0 ** rng.uniform(-150, 150) for _ in range(200)]
    ms += [np.outer(rng.standard_normal(3), rng.standard_normal(3)) + np.outer(rng.standard_normal(3), rng.standard_normal(3)) for _ in range(100)]  # rank 2
    inf, nan = float("inf"), float("nan")
    ms += [np.full((3, 3), 1e200), np.full((3, 3), 1e-200), np.array([[nan, 0, 0], [0, 1, 0], [0, 0, 1.0]]), np.array([[inf, 0, 0], [0, 1, 0], [0, 0, 1.0]])]
    return np.ascontiguousarray(ms, dtype=np.float64)


def test_the_shared_rotation_helper_equals_the_restatement_bit_for_bit(tmp_path):
    """g3_nearest_rotation (kernels_geom3.hip.h: the text k_sim3_models compiles), run on the host under the sanitizers."""
    ms = hostile_matrices()
    (tmp_path / "in.bin").write_bytes(ms.tobytes())
    r = subprocess.run([_sanitized(tmp_path), "rot", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(ms), 13)
    valid = 0
    for M, row in zip(ms, got):
        want = sim3ref.rotation(M)
        assert (row[0] == 1.0) == (want is not None)
        if want is not None:
            valid += 1
            assert row[1:10].tobytes() == want[0].tobytes() and row[10:].tobytes() == want[1].tobytes()
    assert 250 <= valid < len(ms)


# ---- the bindings over CPU tensors (a bare Context whose `where` is the CPU, the library replaced by a recorder)

class Recorder:
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


def fields(out):
    return {name: getattr(out, name) for name, _ in out._fields_}


def test_frame_world_wrapper_over_cpu_tensors(ctx):
    kw = dict(poses=raw(3 * 112), matches=torch.zeros(3, 70, 3, dtype=torch.int32), match_counts=torch.zeros(3, dtype=torch.int32),
              front_bits=torch.zeros(3, 2, dtype=torch.int64), point_cap=50, chain=raw(3 * 176), cams=raw(4 * 112), index=torch.zeros(4, 50, dtype=torch.int32))
    ctx.frame_world(**kw)
    (name, args), = ctx.rec.calls
    assert name == "vslam_frame_world_dev" and args[4] == 70 and args[6] == 50 and args[8] == 3
    assert fields(args[-1]._obj) == dict(struct_size=C.sizeof(capi.FrameWorldOut), cams=kw["cams"].data_ptr(), cams_bytes=448, index=kw["index"].data_ptr(),
                                         index_bytes=800)
    ctx.rec.calls.clear()
    for change, message in ((dict(cams=None), "frame_world: cams is required"), (dict(chain=raw(3 * 176 - 1)), "frame_world: fewer sets than pairs"),
                            (dict(cams=raw(4 * 112 - 1)), "frame_world: fewer sets than pairs"), (dict(n_pairs=4), "frame_world: fewer sets than pairs"),
                            (dict(index=torch.zeros(4, 49, dtype=torch.int32)), "frame_world: fewer sets than pairs"),
                            (dict(matches=torch.zeros(3, 70, 2, dtype=torch.int32)), "frame_world: matches must be [n, match_cap, 3] 4-byte elements"),
                            (dict(index=torch.zeros(4, 100, dtype=torch.int32)[:, :50]), "frame_world: index must be a contiguous tensor on cpu")):
        with pytest.raises(ValueError) as e:
            ctx.frame_world(**{**kw, **change})
        assert str(e.value) == message and not ctx.rec.calls


def test_sim3_wrapper_over_cpu_tensors(ctx):
    side = capi.sim3_side(raw(8 * 112), torch.zeros(8, 50, dtype=torch.int32), torch.zeros(7, 100, 3, dtype=torch.float64), torch.zeros(8, 60, 6, dtype=torch.int32))
    assert (side.map_cap, side.point_cap, side.points_cap, side.n_map_pairs, side.n_frames, side.reserved) == (100, 50, 60, 7, 8, 0)
    assert side.cams == side.keep[0].data_ptr() and side.points == side.keep[3].data_ptr()
    with pytest.raises(ValueError):
        capi.sim3_side(raw(8 * 112 - 1), torch.zeros(8, 50, dtype=torch.int32), torch.zeros(7, 100, 3, dtype=torch.float64), torch.zeros(8, 60, 6, dtype=torch.int32))
    with pytest.raises(ValueError):
        capi.sim3_side(raw(8 * 112), torch.zeros(8, 50, dtype=torch.int32), torch.zeros(7, 100, 3, dtype=torch.float32), torch.zeros(8, 60, 6, dtype=torch.int32))
    kw = dict(query=side, train=side, pairs=torch.zeros(3, 2, dtype=torch.int32), matches=torch.zeros(3, 70, 3, dtype=torch.int32),
              match_counts=torch.zeros(3, dtype=torch.int32), intrinsics=K, select_bits=torch.zeros(3, 2, dtype=torch.int64), n_hypotheses=16, seed=-1,
              models=raw(3 * 136), inlier_bits=torch.zeros(3, 2, dtype=torch.int64), hypotheses=raw(3 * 16 * 112), correspondences=raw(3 * 70 * 88),
              links=torch.zeros(3, 70, 2, dtype=torch.int32))
    ctx.sim3(**kw)
    (name, args), = ctx.rec.calls
    assert name == "vslam_sim3_dev" and args[6] == 70 and args[7] == kw["select_bits"].data_ptr() and args[8] == 3
    prm = args[9]._obj
    assert (prm.n_hypotheses, prm.seed, prm.max_dist2, prm.K.fx, prm.K.cy) == (16, 0xFFFFFFFF, capi.SIM3_MAX_DIST2, 800.0, 540.0)
    want = {"struct_size": C.sizeof(capi.Sim3Out)}
    for nm in ("models", "inlier_bits", "hypotheses", "correspondences", "links"):
        want[nm], want[nm + "_bytes"] = kw[nm].data_ptr(), kw[nm].numel() * kw[nm].element_size()
    assert fields(args[-1]._obj) == want
    ctx.rec.calls.clear()
    ctx.sim3(**{k: v for k, v in kw.items() if k not in ("select_bits", "inlier_bits", "hypotheses", "correspondences", "links")})
    (name, args), = ctx.rec.calls
    left = fields(args[-1]._obj)
    assert args[7] is None and all(left[nm] is None and left[nm + "_bytes"] == 0 for nm in ("inlier_bits", "hypotheses", "correspondences", "links"))
    ctx.rec.calls.clear()
    for change, message in ((dict(models=None), "sim3: models is required"), (dict(pairs=None), "sim3: pairs is required"),
                            (dict(n_pairs=4), "sim3: fewer sets than pairs"), (dict(select_bits=torch.zeros(3, 1, dtype=torch.int64)), "sim3: fewer sets than pairs"),
                            (dict(links=torch.zeros(3, 70, 4, dtype=torch.int32)[:, :, :2]), "sim3: links must be a contiguous tensor on cpu")):
        with pytest.raises(ValueError) as e:
            ctx.sim3(**{**kw, **change})
        assert str(e.value) == message and not ctx.rec.calls


def test_host_wrappers_over_numpy_arrays(ctx):
    poses, mt, counts, pts, bits = synthetic_chain(3, m=40)
    chain = chainref.chain(poses, mt, counts, pts, bits, 40, 16)[0]
    cams, index = ctx.frame_world_host(poses, mt, counts, bits, 40, chain)
    (name, args), = ctx.rec.calls
    assert name == "vslam_frame_world_host" and args[4] == 40 and args[6] == 40 and args[8] == 3 and cams.shape == (4,) and index.shape == (4, 40)
    assert fields(args[-1]._obj)["cams_bytes"] == 4 * 112 and fields(args[-1]._obj)["index_bytes"] == 4 * 40 * 4
    with pytest.raises(ValueError):
        ctx.frame_world_host(poses, mt, counts, bits, 40, chain[:2])
    ctx.rec.calls.clear()
    side = sim3ref.make_side(np.zeros(4, capi.FRAME_CAM_DTYPE), index, np.zeros((3, 40, 3)), np.zeros((4, 45), capi.POINT_DTYPE))
    pairs, matches = np.zeros(2, capi.SET_PAIR_DTYPE), np.zeros((2, 30), capi.MATCH_DTYPE)
    links = np.full((2, 30, 2), 7, np.int32)
    models = ctx.sim3_host(side, side, pairs, matches, [30, 30], K, n_hypotheses=8, links=links)
    (name, args), = ctx.rec.calls
    q, t = args[1]._obj, args[2]._obj
    assert name == "vslam_sim3_host" and q is t and (q.map_cap, q.point_cap, q.points_cap, q.n_map_pairs, q.n_frames) == (40, 40, 45, 3, 4)
    assert args[6] == 30 and args[7] is None and args[8] == 2 and models.shape == (2,) and models.dtype == capi.SIM3_DTYPE
    out = fields(args[-1]._obj)
    assert out["links"] == links.ctypes.data and out["links_bytes"] == 2 * 30 * 8 and out["models_bytes"] == 2 * 136 and out["hypotheses"] is None
    for change in (dict(links=np.zeros((2, 30), np.int32)), dict(inlier_bits=np.zeros((2, 1), np.int64)), dict(select_bits=np.zeros((2, 2), np.uint64)),
                   dict(hypotheses=np.zeros((2, 9), capi.SIM3_HYP_DTYPE))):
        with pytest.raises(ValueError):
            ctx.sim3_host(side, side, pairs, matches, [30, 30], K, n_hypotheses=8, **change)
    with pytest.raises(ValueError):
        ctx.sim3_host(dict(side, index=index[:3]), side, pairs, matches, [30, 30], K)


def build_cxx_driver(tmp_path):
    """tests/sim3_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_sim3.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "sim3_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "sim3_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrappers_refuse_bad_sizes_and_fail_loudly_without_a_gpu(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = build_cxx_driver(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = subprocess.run([exe, "--valid"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"status {0 if torch.cuda.is_available() else HIP}", r.stdout + r.stderr


# ---- the frame rule on hand-made chains

def frames_of(args, point_cap=40, min_links=16):
    poses, mt, counts, pts, bits = args
    chain = chainref.chain(poses, mt, counts, pts, bits, point_cap, min_links)[0]
    return chain, sim3ref.frame_world(poses, mt, counts, bits, point_cap, chain)


def test_frame_sources_query_train_and_none_around_an_invalid_pair():
    args = synthetic_chain(6, invalid=(3,))
    chain, (cams, index) = frames_of(args)
    assert chain["valid"].tolist() == [1, 1, 1, 0, 1, 1]
    assert cams["pair"].tolist() == [0, 1, 2, 2, 4, 5, 5] and cams["side"].tolist() == [0, 0, 0, 1, 0, 0, 1] and cams["valid"].all()
    assert cams["segment"].tolist() == [0, 0, 0, 0, 4, 4, 4]
    for f in (0, 1, 2, 4, 5):                                               # query side: copies
        assert cams["W"][f].tobytes() == chain["W"][f].tobytes() and cams["w"][f].tobytes() == chain["w"][f].tobytes()
    for f, j in ((3, 2), (6, 5)):                                           # train side: (R W, R w + scale t), whose centre is the chain's Ct
        R, t = args[0]["R"][j].reshape(3, 3), args[0]["t"][j]
        W, w = chain["W"][j].reshape(3, 3), chain["w"][j]
        assert np.abs(cams["W"][f].reshape(3, 3) - R @ W).max() <= 1e-14 and np.abs(cams["w"][f] - (R @ w + chain["scale"][j] * t)).max() <= 1e-13
        assert np.abs(-cams["W"][f].reshape(3, 3).T @ cams["w"][f] - chain["Ct"][j]).max() <= 1e-13
    assert (index == np.arange(40)).all()                                   # record i: query i, train i, all live
    # two invalid pairs in a row: the frame between them has no source
    args = synthetic_chain(5, invalid=(1, 2))
    chain, (cams, index) = frames_of(args)
    assert cams["valid"].tolist() == [1, 1, 0, 1, 1, 1] and cams["pair"].tolist() == [0, 0, -1, 3, 4, 4] and cams["side"].tolist() == [0, 1, 0, 0, 0, 1]
    assert cams["segment"].tolist() == [0, 0, -1, 3, 3, 3] and cams[2].tobytes() == np.array([(np.zeros(9), np.zeros(3), -1, -1, 0, 0)], capi.FRAME_CAM_DTYPE).tobytes()
    assert (index[2] == -1).all() and (index[[0, 1, 3, 4, 5]] == np.arange(40)).all()
    # every pair invalid; and one pair
    _, (cams, index) = frames_of(synthetic_chain(2, invalid=(0, 1)))
    assert not cams["valid"].any() and (index == -1).all() and (cams["pair"] == -1).all()
    _, (cams, index) = frames_of(synthetic_chain(1))
    assert cams["pair"].tolist() == [0, 0] and cams["side"].tolist() == [0, 1] and index.shape == (2, 40)
    assert sim3ref.frame_world(*[a[:0] for a in synthetic_chain(1)[:3]], synthetic_chain(1)[4][:0], 40, np.zeros(0, capi.CHAIN_DTYPE))[0].shape == (0,)


def test_shared_indices_lowest_record_wins_and_dead_records_do_not_count():
    poses, mt, counts, pts, bits = synthetic_chain(2, m=40)
    mt["query"][0, [5, 9, 30]] = 7                                          # records 5, 7, 9, 30 of pair 0 share query 7
    mt["train"][1, [4, 6]] = 2                                              # records 2, 4, 6 of pair 1 share train 2
    mt["train"][0, 20] = 40                                                 # not live: an index at point_cap
    mt["query"][1, 21] = -1
    flags = np.ones(40, bool)
    flags[[5, 2]] = False                                                   # not in front: dead, in both pairs
    bits[0] = bits[1] = epiref.bits(flags, 1)
    counts[1] = 35                                                          # records 35 .. 39 of pair 1 are past the count
    chain, (cams, index) = frames_of((poses, mt, counts, pts, bits))
    assert cams["pair"].tolist() == [0, 1, 1] and cams["side"].tolist() == [0, 0, 1]
    assert index[0, 7] == 7 and index[0, 5] == -1 and index[0, 9] == -1 and index[0, 30] == -1 and index[0, 20] == -1 and index[0, 2] == -1
    mt["query"][0, 7] = 8                                                   # without record 7 the next live one of the four is 9 (5 is dead)
    _, (_, index2) = frames_of((poses, mt, counts, pts, bits))
    assert index2[0, 7] == 9 and index2[0, 8] == 7
    assert index[1, 2] == -1 and index[1, 21] == -1 and index[1, 36] == -1 and index[1, 34] == 34          # frame 1 reads pair 1's query side
    assert index[2, 2] == 4 and index[2, 4] == -1 and index[2, 6] == -1 and index[2, 21] == -1 and index[2, 35] == -1 and index[2, 34] == 34


# ---- the closed form and the composition against numpy

def umeyama(X, Y):
    """Y ~ s R X + t by SVD with the reflection fix, and the symmetric scale sqrt(sum |B|^2 / sum |A|^2)."""
    A, B = X - X.mean(0), Y - Y.mean(0)
    U, _, Vt = np.linalg.svd(B.T @ A)
    R = U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt
    s = np.sqrt((B * B).sum() / (A * A).sum())
    return s, R, Y.mean(0) - s * R @ X.mean(0)


CLOSED_FORM_BOUND, SVD_BOUND = 1.2e-6, 6.0e-8  # 100 x the worst measured below (1.2e-8 and 6.0e-10), tighter than the 1e-5 they may not exceed


def test_closed_form_equals_an_svd_solution_and_returns_planted_similarities():
    """Measured over 1000 exact and 1000 noisy 3-point samples: the planted (s, R, t) comes back to 1.2e-8 at worst (six Jacobi
    sweeps on samples as thin as they come), and on noisy samples, whose M has rank 2 and either sign of the third singular
    direction, the restatement differs from the SVD solution with the reflection fix by 6.0e-10 at worst.  A transposed R or an
    inverted scale is off by order 1."""
    rng = np.random.default_rng(3)
    exact, noisy = 0.0, 0.0
    for trial in range(2000):
        X = rng.uniform(-5, 5, (3, 3))
        s, R, t = rng.uniform(0.2, 5.0), random_rotation(rng), rng.uniform(-5, 5, 3)
        Y = s * X @ R.T + t
        if trial % 2:
            Y += rng.normal(0, 0.05, (3, 3))
        got = sim3ref.model_from_3(X, Y)
        assert got is not None
        gs, gR, gt = got
        assert abs(np.linalg.det(gR) - 1.0) <= 1e-9 and np.abs(gR @ gR.T - np.eye(3)).max() <= 1e-9
        if trial % 2:
            ws, wR, wt = umeyama(X, Y)
            noisy = max(noisy, abs(gs - ws) / ws, np.abs(gR - wR).max(), np.abs(gt - wt).max())
        else:
            exact = max(exact, abs(gs - s) / s, np.abs(gR - R).max(), np.abs(gt - t).max())
    print("closed form: worst error on exact samples", exact, "worst difference from the SVD solution on noisy samples", noisy)
    assert exact <= CLOSED_FORM_BOUND and noisy <= SVD_BOUND


def test_collinear_and_coincident_samples_are_invalid():
    line = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0]])
    assert sim3ref.model_from_3(line, line) is None                          # M = diag(2, 0, 0): n2 is exactly 0
    assert sim3ref.model_from_3(line @ np.array([[0.0, 1, 0], [0, 0, 1], [1, 0, 0]]), line * 4.0) is None
    same = np.tile([1.0, 2.0, 3.0], (3, 1))
    spread = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert sim3ref.model_from_3(same, spread) is None and sim3ref.model_from_3(spread, same) is None     # a2 == 0; b2 == 0
    assert sim3ref.model_from_3(np.where(spread > 0, np.inf, 0.0), spread) is None and sim3ref.model_from_3(spread * 1e200, spread) is None   # a2 not finite
    assert sim3ref.model_from_3(spread, spread * 1e-200) is None              # b2 underflows to 0
    s, R, t = sim3ref.model_from_3(spread, 2.0 * spread + 1.0)
    assert s == 2.0 and np.abs(R - np.eye(3)).max() <= 1e-15 and np.abs(t - 1.0).max() <= 1e-15
    assert sim3ref.sample3(1, 0, 0, 2) is None and len(set(sim3ref.sample3(1, 0, 0, 3))) == 3


def test_composition_equals_numpy_products_and_the_two_tests_are_reprojections():
    rng = np.random.default_rng(8)
    worst = 0.0
    for trial in range(50):
        s, R, t = rng.uniform(0.3, 3.0), random_rotation(rng), rng.uniform(-3, 3, 3)
        Wq, wq, Wt, wt = random_rotation(rng), rng.uniform(-2, 2, 3), random_rotation(rng), rng.uniform(-2, 2, 3)
        cq, ct = sim3ref.as_cam(Wq, wq), sim3ref.as_cam(Wt, wt)
        Af, af, Ab, ab = sim3ref.compose(s, R, t, cq, ct)
        worst = max(worst, np.abs(Af - s * Wt @ R).max(), np.abs(af - (Wt @ t + wt)).max(), np.abs(Ab - Wq @ R.T / s).max(),
                    np.abs(ab - (wq - Wq @ R.T @ t / s)).max())
        # points in front of both cameras, observed exactly: inliers both ways; a point moved by 3 px fails at 2 px and passes at 4
        Xq = (rng.uniform(-1, 1, (20, 3)) + [0, 0, 6.0] - wq) @ Wq            # x_cam = Wq X + wq
        Y = s * Xq @ R.T + t
        xq, xt = Xq @ Wq.T + wq, Y @ Wt.T + wt
        corr = np.zeros(20, capi.SIM3_CORR_DTYPE)
        corr["X"], corr["Y"], corr["uq"], corr["vq"], corr["ut"], corr["vt"] = Xq, Y, xq[:, 0] / xq[:, 2], xq[:, 1] / xq[:, 2], xt[:, 0] / xt[:, 2], xt[:, 1] / xt[:, 2]
        front = xt[:, 2] > 0
        n, flags = sim3ref.score(s, R, t, cq, ct, K, corr, 1e-12)
        assert (flags == front).all() and n == front.sum()
        moved = corr.copy()
        moved["ut"] += 3.0 / K[0]
        assert not sim3ref.score(s, R, t, cq, ct, K, moved, 4.0)[1].any() and (sim3ref.score(s, R, t, cq, ct, K, moved, 16.0)[1] == front).all()
        assert sim3ref.score(s, R, t, cq, ct, K, moved, 4.0, which=2)[1].all()                         # the backward test alone does not see it (every point is in front of the query camera)
        moved = corr.copy()
        moved["vq"] -= 3.0 / K[1]
        assert not sim3ref.score(s, R, t, cq, ct, K, moved, 4.0)[1].any() and (sim3ref.score(s, R, t, cq, ct, K, moved, 4.0, which=1)[1] == front).all()
    print("composition against numpy products over 50 similarities: worst |difference|", worst)
    assert worst <= 1e-13


# ---- the planted two-visit scenes: the measurement

BASE_A, BASE_B = (0.5, 0.9, 0.4, 0.7), (0.6, 0.45, 0.8, 0.5)
YAW_A, YAW_B = 0.04, -0.03
LOOPS = ((0, 0), (2, 1), (4, 3), (1, 4))                                   # (frame of B, frame of A): query- and train-side sources on either end


def _yaw(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def two_visits(seed, n, wrong=0.2, width=1920, height=1080, f=800.0):
    """Two five-camera passes over one set of n scene points, in the scheme of test_chain_cpu.five_frames: pass A starts at the
    identity with a yaw of 0.04 per step and baselines BASE_A, pass B from another pose (yawed 0.06, pitched 0.02, moved by (0.8,
    0.1, 0.3)) with a yaw of -0.03 per step and baselines BASE_B; every frame lists the points in an order of its own, at mixed
    octaves and paddings, rounded to the octave pitch; every pair of a pass and every loop list has a fraction `wrong` of its train
    indices drawn at random.  -> (visits [2]: (matches [4][n], point lists [5][n], cameras), loops [len(LOOPS)]: (matches [n]
    query-ascending, true bool [n]))."""
    rng = np.random.default_rng(seed)
    Km = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1.0]])
    pitch = np.array([[1, 0, 0], [0, np.cos(0.02), -np.sin(0.02)], [0, np.sin(0.02), np.cos(0.02)]])
    cams = [[(np.eye(3), np.zeros(3))], [(_yaw(0.06) @ pitch, np.array([0.8, 0.1, 0.3]))]]
    for v, (bases, a) in enumerate(((BASE_A, YAW_A), (BASE_B, YAW_B))):
        for b in bases:
            R, t = cams[v][-1]
            cams[v].append((_yaw(a) @ R, _yaw(a) @ t + np.array([-b, 0, 0])))
    allc = cams[0] + cams[1]
    pix = [[] for _ in allc]
    while len(pix[0]) < n:
        X = np.array([rng.uniform(-6, 6), rng.uniform(-3.5, 3.5), rng.uniform(4, 12)])
        uv = []
        for R, t in allc:
            a = Km @ (R @ X + t)
            uv.append(a[:2] / a[2])
        if all(0 <= a[0] < width - 1 and 0 <= a[1] < height - 1 for a in uv):
            for k in range(10):
                pix[k].append(uv[k])
    octave, padding = rng.integers(0, 3, n).astype(np.int32), rng.integers(0, 2, n).astype(np.int32)
    perms = [rng.permutation(n) for _ in allc]
    lists = []
    for k in range(10):
        p = np.zeros(n, capi.POINT_DTYPE)
        p[perms[k]] = epiref.to_points(np.array(pix[k]), octave, padding)
        lists.append(p)

    def match_list(pq, pt):
        m = np.zeros(n, capi.MATCH_DTYPE)
        bad = rng.random(n) < wrong
        m["query"], m["train"] = pq, np.where(bad, rng.integers(0, n, n), pt)
        m["dist2"] = rng.random(n).astype(np.float32)
        order = np.argsort(m["query"], kind="stable")                       # ascending query order, as the matchers write them
        return m[order], (m["train"] == pt)[order]

    visits = [([match_list(perms[5 * v + j], perms[5 * v + j + 1])[0] for j in range(4)], lists[5 * v:5 * v + 5], cams[v]) for v in range(2)]
    return visits, [match_list(perms[5 + fb], perms[fa]) for fb, fa in LOOPS]


def chain_visit(visit, seed, n):
    """RANSAC (512 hypotheses, 2 px), pose and chain of one pass by the restatements, then its frames -> (the pass as a side of
    sim3(), its chain records, and the arrays frame_world() took)."""
    matches, lists, _ = visit
    words = (n + 63) // 64
    poses, mt, counts = np.zeros(4, capi.POSE_DTYPE), np.zeros((4, n), capi.MATCH_DTYPE), np.zeros(4, np.uint32)
    pts, bits = np.zeros((4, n, 3), np.float64), np.zeros((4, words), np.uint64)
    for j in range(4):
        model, flags, _ = epiref.ransac(matches[j], lists[j], lists[j + 1], 512, seed, 4.0, pair=j)
        inl = matches[j][flags]
        pose, _, front, X = poseref.pose(model, inl, lists[j], lists[j + 1], K)
        k = len(inl)
        poses[j], mt[j, :k], counts[j] = pose[0], inl, k
        bits[j] = epiref.bits(front, words)
        if X is not None:
            pts[j, :k] = X
    chain, ms, maps, _, _, _ = chainref.chain(poses, mt, counts, pts, bits, n, 16)
    mp = np.zeros((4, n, 3))                                                # (rows past a pair's count: never addressed by index)
    for j in range(4):
        if maps[j] is not None:
            mp[j, :ms[j]] = maps[j]
    cams, index = sim3ref.frame_world(poses, mt, counts, bits, n, chain)
    return sim3ref.make_side(cams, index, mp, np.stack(lists)), chain, (poses, mt, counts, pts, bits)


def truth(visits):
    """The similarity from B's world (camera B0, unit BASE_B[0]) to A's (camera A0 = the scene's frame, unit BASE_A[0])."""
    R0, t0 = visits[1][2][0]
    return BASE_B[0] / BASE_A[0], R0.T, -R0.T @ t0 / BASE_A[0]


def loop_table(loops):
    pairs = np.zeros(len(LOOPS), capi.SET_PAIR_DTYPE)
    pairs["query_set"], pairs["train_set"] = [l[0] for l in LOOPS], [l[1] for l in LOOPS]
    return pairs, np.stack([l[0] for l in loops]), np.full(len(loops), len(loops[0][0]), np.uint32)


ROT_BOUND, SCALE_BOUND, T_BOUND = 3.33, 0.4126, 1.3758  # twice the worst measured at max_dist2 = 16, see the docstring below
N_SCENE = 300


@pytest.mark.parametrize("seed", range(1, 17))
def test_restatement_aligns_the_planted_two_visit_scenes(seed):
    """Measured with this restatement over seeds 1 .. 16, 300 points, 4 loop slots each, 512 hypotheses.  Every pass chains into one
    segment; every slot has at least 137 usable true correspondences and at most 51 usable wrong ones.  Worst over the 64 slots, per
    max_dist2 in pixels^2 - rotation error in degrees / relative scale error / translation error in first baselines of A / fewest
    inliers on true correspondences / most inliers on wrong ones:
        1: 5.39 / 0.183 / 2.17 / 0 / 0      4: 4.27 / 0.183 / 1.62 / 7 / 0       9: 1.98 / 0.204 / 0.79 / 15 / 0
       16: 1.67 / 0.206 / 0.69 / 25 / 0    25: 1.80 / 0.206 / 0.71 / 31 / 0     36: 1.46 / 0.184 / 0.55 / 38 / 0
       64: 1.43 / 0.206 / 0.54 / 62 / 0   100: 1.79 / 0.183 / 0.65 / 84 / 0
    3-point samples of two-view triangulations do separate true from wrong correspondences: no wrong one is an inlier of a winner
    at any of these thresholds.  The rotation and translation errors stop improving between 9 and 16 (1.4 .. 2.0 degrees and 0.54 ..
    0.79 from there on, without a trend); 16 (4 px, twice the two-view threshold: a correspondence carries two triangulations' noise)
    is the documented default, capi.SIM3_MAX_DIST2.  The scale error is the chains' own (test_chain_cpu measures 0.146 per pass), not
    the alignment's: it does not move with the threshold.  Each bound is twice the worst at 16, the inlier floor half the fewest.
    They are sanity bounds on the convention (an inverted similarity errs by 0.31 in scale and by the full rotation), not accuracy
    claims."""
    visits, loops = two_visits(seed, N_SCENE)
    A, chA, _ = chain_visit(visits[0], seed, N_SCENE)
    B, chB, _ = chain_visit(visits[1], seed + 100, N_SCENE)
    assert chA["linked"].tolist() == chB["linked"].tolist() == [0, 1, 1, 1]
    s0, R0, t0 = truth(visits)
    pairs, mt, cnt = loop_table(loops)
    models, links, corrs, flags, _ = sim3ref.sim3(B, A, pairs, mt, cnt, K, 512, seed, capi.SIM3_MAX_DIST2)
    assert capi.SIM3_MAX_DIST2 == 16.0
    for p in range(len(LOOPS)):
        md, good = models[p], loops[p][1]
        assert md["best"] >= 0 and md["query_segment"] == 0 and md["train_segment"] == 0 and md["n_matches"] == N_SCENE
        R = md["R"].reshape(3, 3)
        rot = np.degrees(np.arccos(np.clip((np.trace(R @ R0.T) - 1) / 2, -1, 1)))
        scale, t_err = abs(md["s"] - s0) / s0, np.linalg.norm(md["t"] - t0)
        true_in, wrong_in = int((flags[p] & good).sum()), int((flags[p] & ~good).sum())
        print(f"two visits seed {seed} slot {p}: n_corr {md['n_corr']} rotation {rot:.3f} deg scale {scale:.4f} translation {t_err:.4f} "
              f"inliers true {true_in} wrong {wrong_in}")
        assert rot <= ROT_BOUND and scale <= SCALE_BOUND and t_err <= T_BOUND
        assert true_in >= 12 and wrong_in == 0 and md["n_inliers"] == true_in

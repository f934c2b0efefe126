"""The bundle adjustment without a GPU: the C ABI's new symbols, struct layouts and argument checks, the plan header under the
sanitizers, the C++ wrapper, and the CPU restatement of the arithmetic itself (tests/bundleref.py), which the GPU tests compare
against byte for byte: its rules on small hand-made lists, bit for bit against the existing restatements, its re-entry, against
finite differences and scipy's least squares, and on the planted five-frame scenes through the whole chain of restatements."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bundleref, chainref, epiref, resectrefineref, tracksref
from tests.test_tracks_cpu import K, five_frames_with_points, planted_of, planted_tracks, small_scene, true_records
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
KM = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- the ABI

def test_bundle_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_bundle_dev", "vslam_bundle_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_ba_init", b"k_ba_points", b"k_ba_cam_pass", b"k_ba_cam_step", b"k_ba_member_bits", b"k_ba_points_final"):
        assert k in names


def test_bundle_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_bundle_params": capi.BundleParams, "vslam_bundle_out": capi.BundleOut, "vslam_bundle_cam": capi.BundleCam,
               "vslam_bundle_point": capi.BundlePoint}
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
    for cname, ct, dt, size in (("vslam_bundle_cam", capi.BundleCam, capi.BUNDLE_CAM_DTYPE, 160), ("vslam_bundle_point", capi.BundlePoint, capi.BUNDLE_POINT_DTYPE, 40)):
        assert rows[cname][0] == size == dt.itemsize and size % 8 == 0
        assert [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]
    assert rows["vslam_bundle_params"][0] == 48


class Args:
    """A valid vslam_bundle_dev / vslam_bundle_host call over host arrays (nothing is launched without a GPU: the pointers are
    never followed)."""

    def __init__(self, n_pairs=2, match_cap=100, point_cap=50):
        words = (match_cap + 63) // 64
        self.keep = [np.zeros(n_pairs, capi.POSE_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32),
                     np.zeros((n_pairs, words), np.uint64), np.zeros(n_pairs, capi.CHAIN_DTYPE), np.zeros((n_pairs + 1, point_cap), capi.POINT_DTYPE),
                     np.zeros((n_pairs, match_cap), capi.TRACK_DTYPE), np.zeros((n_pairs, match_cap), capi.TRACK_REF_DTYPE),
                     np.zeros(n_pairs, capi.BUNDLE_CAM_DTYPE), np.zeros((n_pairs + 1, match_cap), capi.TRACK_DTYPE), np.zeros(n_pairs, capi.BUNDLE_CAM_DTYPE),
                     np.zeros((n_pairs, match_cap), capi.BUNDLE_POINT_DTYPE), np.zeros((n_pairs, 2, words), np.uint64)]
        poses, m, mc, bits, chain, frames, tracks_in, refs, cams_in, tracks, cams, info, mb = self.keep
        self.poses, self.matches, self.counts, self.bits, self.chain, self.frames, self.tracks_in, self.refs, self.cams_in = (
            a.ctypes.data for a in (poses, m, mc, bits, chain, frames, tracks_in, refs, cams_in))
        self.match_cap, self.point_cap, self.n_pairs = match_cap, point_cap, n_pairs
        self.prm = capi.BundleParams(capi.PoseParams(*K), 4.0, 2, 4)
        self.out = capi.BundleOut(C.sizeof(capi.BundleOut), tracks.ctypes.data, n_pairs * match_cap * 48, cams.ctypes.data, cams.nbytes, info.ctypes.data,
                                  info.nbytes, mb.ctypes.data, mb.nbytes)

    def call(self, fn, prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return fn(None, self.poses, self.matches, self.counts, self.match_cap, self.bits, self.point_cap, self.n_pairs, self.chain, self.frames,
                  self.tracks_in, self.refs, self.cams_in, ref(prm), ref(out))


@pytest.mark.parametrize("entry", ["vslam_bundle_dev", "vslam_bundle_host"])
def test_bundle_rejects_bad_arguments_before_it_needs_a_gpu(lib, entry):
    import torch

    fn = getattr(lib, entry)
    gpu = torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(fn) == (INVALID if gpu else HIP)
    assert Args().call(fn, prm=None) == INVALID and Args().call(fn, out=None) == INVALID

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            if obj == "K":
                setattr(a.prm.K, field, v)
            elif obj == "a":
                setattr(a, field, v)
            else:
                setattr(getattr(a, obj), field, v)
        return a.call(fn)

    for name in ("poses", "matches", "counts", "bits", "chain", "frames", "tracks_in", "refs"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.BundleOut) - 8) == INVALID
    assert bad(out__tracks=None) == INVALID and bad(out__tracks_bytes=2 * 100 * 48 - 1) == INVALID
    assert bad(out__cams=None) == INVALID and bad(out__cams_bytes=2 * 160 - 1) == INVALID
    assert bad(out__point_info_bytes=2 * 100 * 40 - 1) == INVALID
    assert bad(out__member_bits_bytes=2 * 2 * 2 * 8 - 1) == INVALID
    assert bad(a__match_cap=0) == INVALID and bad(a__point_cap=0) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    assert bad(prm__sweeps=0) == INVALID and bad(prm__sweeps=65) == INVALID
    assert bad(prm__min_views=0) == INVALID and bad(prm__min_views=1) == INVALID
    for field in ("fx", "fy", "cx", "cy"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert bad(**{"K__" + field: v}) == INVALID, (field, v)
    assert bad(K__fx=0.0) == INVALID and bad(K__fy=0.0) == INVALID and bad(K__fx=-1.0) == INVALID and bad(K__fy=-1.0) == INVALID
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert bad(prm__max_dist2=v) == INVALID, v
    a = Args()                                                                        # tracks overlapping tracks_in without being equal to it
    a.tracks_in = a.out.tracks + 48
    assert a.call(fn) == INVALID
    if not gpu:  # the optional input and outputs may be absent, tracks may be tracks_in, and no pairs and one pair are valid calls
        assert bad(out__point_info=None, out__member_bits=None, a__cams_in=None) == HIP
        assert bad(a__n_pairs=0) == HIP and bad(a__n_pairs=1) == HIP and bad(prm__sweeps=1) == HIP and bad(prm__sweeps=64) == HIP
        a = Args()
        a.tracks_in = a.out.tracks
        assert a.call(fn) == HIP


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/bundle_plan_driver.cpp is a stand-alone program with its own main: nothing is loaded into Python under a sanitizer."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "bundle_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    # match_cap 1 .. 2^32 - 1 (22 values) x point_cap 1 .. 2^32 - 1 (5) x n_pairs 1 .. 65535 (15), 7 checks each
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 22 * 5 * 15 * 7, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 70, rows["args"]
    src = open(os.path.join(CSRC, "vslam_bundle_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


def build_cxx_driver(tmp_path):
    """tests/bundle_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_bundle.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "bundle_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "bundle_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def cxx_driver_buffers():
    """The buffers tests/bundle_cxx_driver.cpp builds with "run", and the chain, tracks and refs the restatements give for them."""
    n, cap = 3, 8
    poses, mt = np.zeros(n, capi.POSE_DTYPE), np.zeros((n, cap), capi.MATCH_DTYPE)
    i = np.arange(cap)
    poses["R"], poses["t"], poses["valid"], poses["n_matches"] = np.eye(3).reshape(9), [-1.0, 0.0, 0.0], 1, [8, 5, 8]
    mt["query"] = mt["train"] = i
    X = np.stack([i - 3.5, 0.5 * i - 1.5, 6.0 + i % 3], axis=1)
    pts = np.stack([X - [float(j), 0.0, 0.0] for j in range(n)])
    counts, bits = np.array([8, 5, 8], np.uint32), np.array([[0xFF], [0xF7], [0xFF]], np.uint64)
    frames = np.zeros((n + 1, cap), capi.POINT_DTYPE)
    for f in range(n + 1):
        x, y = 800.0 * (X[:, 0] - float(f)) / X[:, 2] + 960.0, 800.0 * X[:, 1] / X[:, 2] + 540.0
        frames["row"][f], frames["col"][f], frames["octave"][f] = np.floor(y + 0.5), np.floor(x + 0.5), 1
    chain = chainref.chain(poses, mt, counts, pts, bits, 8, 2)[0]
    ms, rows, refs, _, _, _ = tracksref.tracks(poses, mt, counts, bits, 8, chain, frames, K, 4.0, 2)
    tracks_in, refs_in = np.zeros((n, cap), capi.TRACK_DTYPE), np.full((n, cap, 2), 0xFFFFFFFF, np.uint32).view(capi.TRACK_REF_DTYPE).reshape(n, cap)
    for j in range(n):
        tracks_in[j, :ms[j]], refs_in[j, :ms[j]] = rows[j], refs[j]
    return poses, mt, counts, bits, frames, chain, tracks_in, refs_in


def test_cxx_wrapper_takes_no_pairs_and_refuses_sizes_that_do_not_fit(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run([build_cxx_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- scenes

def rodrigues(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * A + (1 - np.cos(angle)) * A @ A


def start_cams(poses, chain):
    """cams_in [n] holding the cameras a call without cams_in starts from."""
    n = len(poses)
    cams = np.zeros(n, capi.BUNDLE_CAM_DTYPE)
    for j in range(n):
        bundleref.lib().ba_init_cam(C.c_void_p(poses[j:j + 1].ctypes.data), C.c_void_p(chain[j:j + 1].ctypes.data), None, C.c_int(int(poses["best"][j] >= 0)),
                                    C.c_void_p(cams[j:j + 1].ctypes.data), C.c_void_p(cams[j:j + 1].ctypes.data + 72))
    return cams


def perturbed_cams(poses, chain, seed, angle=np.deg2rad(0.5), scale=0.02):
    """start_cams turned by `angle` about a random axis where they stand, and their w stretched by 1 + scale."""
    rng = np.random.default_rng(seed)
    cams = start_cams(poses, chain)
    for j in range(len(cams)):
        D = rodrigues(rng.normal(size=3), angle)
        cams["W"][j], cams["w"][j] = (D @ cams["W"][j].reshape(3, 3)).reshape(9), (D @ cams["w"][j]) * (1 + scale)
    return cams


class Small:
    """small_scene through the tracks restatement: the arguments of bundleref.Problem."""

    def __init__(self, n_pairs=4, m=40, seed=3, max_dist2=4.0, min_views=2, edit=None):
        self.args, self.X = small_scene(n_pairs, m, seed)
        self.args[0]["best"] = 0
        if edit:
            edit(self.args)
        self.n, self.m, self.max_dist2, self.min_views = n_pairs, m, max_dist2, min_views
        self.ms, rows, refs, self.goods, _, self.paths = tracksref.tracks(*self.args, K, max_dist2, 2)
        self.tracks_in, self.refs = bundleref.dense_tracks(self.ms, rows, refs, m)

    def problem(self, cams_in=None, tracks_in=None):
        return bundleref.Problem(*self.args, self.tracks_in if tracks_in is None else tracks_in, self.refs, K, self.max_dist2, self.min_views, cams_in)


def member_totals(P, out):
    """(members over the active tracks, over the cameras, in held views) under the output of P.run()."""
    over_tracks = int(out["point_info"]["n_after"][out["written"]].sum())
    held = sum(int(P.point_eval(h)[4][0]) for h in P.active_heads() if P.views(h)[0][0] < 0)
    return over_tracks, int(out["cams"]["n_after"].sum()), held


# ---- the rules on hand-made lists

def test_clean_scene_every_view_a_member_and_the_totals_agree():
    s = Small()
    P = s.problem()
    out = P.run(3)
    c, pi = out["cams"], out["point_info"]
    assert out["written"][0].all() and not out["written"][1:].any()                  # every track starts in pair 0
    assert (pi["n_before"][0] == 5).all() and (pi["n_after"][0] == 5).all() and (c["n_before"] == 40).all() and (c["n_after"] == 40).all()
    assert ((c["accepted"] + c["rejected"] + c["invalid"] + c["skipped"]) == 3).all()
    assert ((pi["accepted"] + pi["rejected"] + pi["invalid"] + pi["skipped"])[0] == 3).all()
    assert out["member"][:, :, :40].all()
    assert member_totals(P, out) == (200, 160, 40)
    t = out["tracks"]
    assert (t["status"][0] == 3).all() and (t["n_ok"][0] == 5).all() and t["det"][0].tobytes() == s.tracks_in["det"][0].tobytes()
    assert t[1:].tobytes() == s.tracks_in[1:].tobytes()                              # records that are not heads: byte for byte
    for j in range(4):                                                                # the centre by the trajectory's expression
        W, w = c["W"][j].reshape(3, 3), c["w"][j]
        assert c["C"][j].tolist() == [-((W[0, i] * w[0] + W[1, i] * w[1]) + W[2, i] * w[2]) for i in range(3)]


def test_an_inactive_track_is_copied_through_and_a_held_camera_never_moves():
    s = Small(min_views=3)
    s.tracks_in["status"][0, 5] = 2                                                   # bit 0 cleared: not solved, so not active
    s.tracks_in["n_views"][0, 6] = 2                                                  # fewer views than min_views
    s.tracks_in["X"][0, 5] = [1.0, np.nan, -np.inf]
    s.tracks_in["X"].view(np.uint64)[0, 5, 1] = 0x7FF4000000000123                    # a NaN with a payload survives a copy
    P = s.problem(perturbed_cams(s.args[0], s.args[5], 1))
    out = P.run(4)
    assert out["tracks"][0, 5].tobytes() == s.tracks_in[0, 5].tobytes() and out["tracks"][0, 6].tobytes() == s.tracks_in[0, 6].tobytes()
    assert not out["written"][0, [5, 6]].any() and out["written"][0].sum() == 38
    assert not out["member"][:, :, [5, 6]].any() and (out["cams"]["n_before"] <= 38).all()
    # the held camera is no unknown: view 0 of every track is evaluated under (I, 0) whatever cams_in says, and nothing in the output holds it
    assert all(P.views(h)[0][0] == -1 for h in P.heads)
    H, g, cost, n, fl = P.point_eval((0, 0))
    X = out["tracks"]["X"][0, 0]
    p = s.args[6][0, 0]
    u, v = (float(p["col"]) - K[2]) / K[0], (float(p["row"]) - K[3]) / K[1]
    assert fl[0] == (X[2] > 0 and ((u * X[2] - X[0]) * K[0]) ** 2 + ((v * X[2] - X[1]) * K[1]) ** 2 < 4.0 * X[2] * X[2])


def test_fewer_than_six_members_is_skipped():
    s = Small(m=5)
    out = s.problem().run(3)
    assert (out["cams"]["skipped"] == 3).all() and (out["cams"]["n_before"] == 5).all() and out["cams"]["accepted"].sum() == 0
    start = start_cams(s.args[0], s.args[5])
    assert out["cams"]["W"].tobytes() == start["W"].tobytes() and out["cams"]["w"].tobytes() == start["w"].tobytes()
    assert (out["cams"]["n_after"] == 5).all() and (out["point_info"]["accepted"][0] >= 1).all()        # the points still move


def one_place(m=64):
    """The refinement's one-point fixture as a call: one pair, fx = fy = 1024, every record sees pixel (64, 64) in both frames,
    every point at (0, 0, 8), T_0 = (I, 0) like the held camera.  Every Jacobian entry and every sum is a power of two or zero: the
    two views of a point share a centre, so its H is diag(2 * 128^2, 2 * 128^2, 0) and det = 0 exactly - invalid, the points stay -,
    and the camera's H has rank 2 exactly, the elimination finds no third pivot - invalid.  -> (args, tracks_in, refs, cams_in, K)"""
    poses, chain = np.zeros(1, capi.POSE_DTYPE), np.zeros(1, capi.CHAIN_DTYPE)
    poses["R"], poses["t"], poses["valid"] = np.eye(3).reshape(9), [1.0, 0.0, 0.0], 1
    chain["W"], chain["scale"], chain["valid"] = np.eye(3).reshape(9), 1.0, 1
    mt = np.zeros((1, m), capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(m)
    frames = np.zeros((2, m), capi.POINT_DTYPE)
    frames["row"], frames["col"], frames["octave"] = 64, 64, 1
    tracks_in, refs = np.zeros((1, m), capi.TRACK_DTYPE), np.zeros((1, m), capi.TRACK_REF_DTYPE)
    tracks_in["X"], tracks_in["det"], tracks_in["n_views"], tracks_in["status"] = [0.0, 0.0, 8.0], 1.0, 2, 1
    refs["head_record"] = np.arange(m)
    cams_in = np.zeros(1, capi.BUNDLE_CAM_DTYPE)
    cams_in["W"] = np.eye(3).reshape(9)
    args = [poses, mt, np.full(1, m, np.uint32), epiref.bits(np.ones(m, bool), (m + 63) // 64).reshape(1, -1), m, chain, frames]
    return args, tracks_in, refs, cams_in, (1024.0, 1024.0, 0.0, 0.0)


def test_all_points_of_a_camera_at_one_place_make_the_step_invalid_and_the_camera_comes_back_bit_identical():
    args, tracks_in, refs, cams_in, K1 = one_place()
    out = bundleref.bundle(*args, tracks_in, refs, K1, 1e12, 2, 4, cams_in)
    c, pi = out["cams"][0], out["point_info"][0]
    assert (int(c["invalid"]), int(c["accepted"]), int(c["rejected"]), int(c["skipped"])) == (4, 0, 0, 0) and int(c["n_before"]) == int(c["n_after"]) == 64
    assert c["W"].tobytes() == cams_in["W"].tobytes() and c["w"].tobytes() == cams_in["w"].tobytes() and float(c["cost_after"]) == 64 * 2 * 64.0 ** 2
    assert (pi["invalid"] == 4).all() and (pi["n_after"] == 2).all() and out["tracks"]["X"].tobytes() == tracks_in["X"].tobytes()
    P = bundleref.Problem(*args, tracks_in, refs, K1, 1e12, 2, cams_in)
    H, g, _, n = resectrefineref.evaluate(P.W[0], P.w[0], K1, P.rows_of(0), 1e12)
    assert n == 64 and np.linalg.matrix_rank(H) == 2 and resectrefineref.step(P.W[0], P.w[0], H, g) is None
    Hp, gp, _, _, _ = P.point_eval((0, 0))
    assert Hp.tolist() == [[2 * 128.0 ** 2, 0, 0], [0, 2 * 128.0 ** 2, 0], [0, 0, 0]] and P.point_delta(Hp, gp) is None


def test_exact_data_at_the_optimum_comes_out_bit_identical():
    """Cameras (I, 0), (I, (-1, 0, 0)), ... and points whose pixels are whole: every residual is exactly 0, so g = 0, every step is
    delta = 0 exactly, and a candidate with the same members and the same cost is not better: rejected, never accepted."""
    n_pairs, m = 3, 8
    cams = [(np.eye(3), np.array([-float(k), 0.0, 0.0])) for k in range(n_pairs + 1)]
    X = np.array([[2.0 * (i % 4) - 3.0, 1.0 * (i // 4) - 0.5, 4.0] for i in range(m)])       # depth 4: 800 / 4 = 200 px per unit
    frames = np.zeros((n_pairs + 1, m), capi.POINT_DTYPE)
    for k, (R, t) in enumerate(cams):
        a = (KM @ (X @ R.T + t).T).T
        pix = a[:, :2] / a[:, 2:]
        assert (pix == np.round(pix)).all()
        frames[k] = epiref.to_points(pix, np.ones(m, np.int32), np.zeros(m, np.int32))
    poses, chain = true_records(cams)
    poses["best"] = 0
    mt = np.zeros((n_pairs, m), capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(m)
    bits = np.stack([epiref.bits(np.ones(m, bool), 1)] * n_pairs)
    args = [poses, mt, np.full(n_pairs, m, np.uint32), bits, m, chain, frames]
    ms, rows, refs, goods, _, _ = tracksref.tracks(*args, K, 4.0, 2)
    assert np.abs(rows[0]["X"] - X).max() < 1e-12 and (rows[0]["status"] == 3).all()   # the linear solve is exact up to rounding:
    tracks_in, refs_in = bundleref.dense_tracks(ms, rows, refs, m)
    tracks_in["X"][0] = X                                                               # the planted points themselves
    cams_in = start_cams(poses, chain)
    out = bundleref.bundle(*args, tracks_in, refs_in, K, 4.0, 2, 5, cams_in)
    c, pi = out["cams"], out["point_info"][0]
    assert c["accepted"].sum() == 0 and pi["accepted"].sum() == 0 and ((c["rejected"] + c["invalid"]) == 5).all() and ((pi["rejected"] + pi["invalid"]) == 5).all()
    assert c["W"].tobytes() == cams_in["W"].tobytes() and c["w"].tobytes() == cams_in["w"].tobytes()
    assert out["tracks"]["X"].tobytes() == tracks_in["X"].tobytes() and (c["cost_after"] == 0).all() and (pi["cost_after"] == 0).all()
    assert out["tracks"][0].tobytes() == tracks_in[0].tobytes()                       # n_ok and status recomputed to what they were


def test_no_pairs_and_one_pair():
    e = lambda dt, *shape: np.zeros(shape, dt)
    out = bundleref.bundle(e(capi.POSE_DTYPE, 0), e(capi.MATCH_DTYPE, 0, 4), e(np.uint32, 0), e(np.uint64, 0, 1), 4, e(capi.CHAIN_DTYPE, 0),
                           e(capi.POINT_DTYPE, 1, 4), e(capi.TRACK_DTYPE, 0, 4), e(capi.TRACK_REF_DTYPE, 0, 4), K, 4.0, 2, 3)
    assert len(out["cams"]) == 0 and out["tracks"].size == 0
    s = Small(n_pairs=1, m=30, max_dist2=1e6)
    P = s.problem(perturbed_cams(s.args[0], s.args[5], 2, scale=0.0))
    out = P.run(6)
    assert (out["point_info"]["n_before"][0] == 2).all() and out["cams"]["n_before"][0] == 30 and out["cams"]["accepted"][0] >= 1
    assert member_totals(P, out) == (60, 30, 30)


def test_a_break_and_an_invalid_pair_in_the_middle():
    def edit(args):
        args[5]["linked"][2] = 0                                                      # a break: pair 2 starts a segment, its query camera is held
        args[0]["best"][4] = -1                                                       # an invalid pair: the chain links neither it nor the pair after it
        args[5]["linked"][[4, 5]] = 0

    s = Small(n_pairs=6, m=30, edit=edit, max_dist2=1e9)
    P = s.problem()
    out = P.run(3)
    c = out["cams"]
    assert c["skipped"][4] == 3 and c["W"][4].tolist() == np.eye(3).reshape(9).tolist() and not c["w"][4].any() and not c["C"][4].any()
    assert c["n_before"][4] == c["n_after"][4] == c["accepted"][4] == 0 and c["cost_after"][4] == 0
    assert np.signbit(c["C"][4]).sum() == 0                                           # centre +0.0
    heads = {h[0] for h in P.heads}
    assert heads == {0, 2, 5}                                                         # pair 3 continues pair 2; nothing is live in pair 4; pair 5 starts anew
    assert P.views((2, 0))[0][0] == -1 and P.views((0, 0))[-1][0] == 1 and P.views((5, 0))[0][0] == -1 and P.views((2, 0))[-1][0] == 3
    assert len(P.rows_of(1)) == 30 and len(P.rows_of(2)) == 60 and len(P.rows_of(3)) == 30 and not out["member"][4].any()
    tr, cam, held = member_totals(P, out)
    assert tr == cam + held


def test_a_view_behind_its_camera_is_never_a_member():
    s = Small(max_dist2=1e12)
    F = np.diag([-1.0, 1.0, -1.0])
    cams_in = start_cams(s.args[0], s.args[5])
    cams_in["W"][2], cams_in["w"][2] = (F @ cams_in["W"][2].reshape(3, 3)).reshape(9), F @ cams_in["w"][2]   # camera T_2 turned half round where it stands
    P = s.problem(cams_in)
    assert all(not P.point_eval(h)[4][3] and P.point_eval(h)[3] == 4 for h in P.heads)
    rows = P.rows_of(2)
    assert resectrefineref.evaluate(P.W[2], P.w[2], K, rows, 1e12)[3] == 0
    out = P.run(2)
    assert out["cams"]["skipped"][2] == 2 and out["cams"]["n_after"][2] == 0 and not out["member"][2, 1].any() and not out["member"][3, 0].any()


# ---- bit for bit against the existing restatements

def test_evaluate_and_step_equal_the_refinement_restatement_on_rows_of_and_the_start_is_the_chain():
    (poses, mt, counts, pts, bits, chain, frames), maps, (ms, rows, refs, goods, summary, paths), world, perms = planted_tracks(2, 300)
    tracks_in, refs_in = bundleref.dense_tracks(ms, rows, refs, 300)
    P = bundleref.Problem(poses, mt, counts, bits, 300, chain, frames, tracks_in, refs_in, K, 4.0, 3)
    assert chain["linked"].tolist() == [0, 1, 1, 1]
    for j in range(3):                                                                # cams_in absent: T_j is chain[j + 1]'s camera, bit for bit
        assert P.W[j].tobytes() == chain["W"][j + 1].tobytes() and P.w[j].tobytes() == chain["w"][j + 1].tobytes()
    before = [(P.W[j].copy(), P.w[j].copy(), P.rows_of(j)) for j in range(4)]
    # one sweep with the points frozen (every point step rejected is not something to arrange): run the sweep, then redo its camera half by hand
    X0 = P.tracks["X"].copy()
    out = P.run(1)
    Q = bundleref.Problem(poses, mt, counts, bits, 300, chain, frames, tracks_in, refs_in, K, 4.0, 3)
    Q.tracks["X"][...] = out["tracks"]["X"]                                            # the points as step A left them (canonical: they are finite)
    for j in range(4):
        W, w, _ = before[j]
        rows_j = Q.rows_of(j)
        assert len(rows_j) == ms[j] + (ms[j + 1] if j < 3 else 0)
        H, g, cost, n = resectrefineref.evaluate(W, w, K, rows_j, 4.0)
        c = out["cams"][j]
        assert (n, cost) == (int(c["n_before"]), float(c["cost_before"])) and n >= 6
        st = resectrefineref.step(W, w, H, g)
        assert st is not None
        Hn, gn, cost_n, nn = resectrefineref.evaluate(st[0], st[1], K, rows_j, 4.0)
        kept = nn > n or (nn == n and cost_n < cost)
        assert (int(c["accepted"]), int(c["rejected"])) == ((1, 0) if kept else (0, 1))
        Wf, wf = (st[0].reshape(9), st[1]) if kept else (W, w)
        assert c["W"].tobytes() == Wf.tobytes() and c["w"].tobytes() == wf.tobytes()
        assert (int(c["n_after"]), float(c["cost_after"])) == ((nn, cost_n) if kept else (n, cost))
    assert any(out["cams"]["accepted"])


@pytest.mark.parametrize("k", [2, 3, 8])
def test_one_call_of_k_sweeps_equals_k_calls_of_one(k):
    (poses, mt, counts, pts, bits, chain, frames), maps, (ms, rows, refs, goods, summary, paths), world, perms = planted_tracks(3, 300)
    tracks_in, refs_in = bundleref.dense_tracks(ms, rows, refs, 300)
    args = (poses, mt, counts, bits, 300, chain, frames)
    once = bundleref.bundle(*args, tracks_in, refs_in, K, 4.0, 3, k)
    t, cams = tracks_in, None
    for _ in range(k):
        out = bundleref.bundle(*args, t, refs_in, K, 4.0, 3, 1, cams)
        # status bit 0 survives, so the active set of the next call is this one's
        assert ((out["tracks"]["status"] & 1) == (tracks_in["status"] & 1)).all() and (out["tracks"]["n_views"] == tracks_in["n_views"]).all()
        t, cams = out["tracks"], out["cams"]
    for f in ("X", "n_ok", "status"):
        assert out["tracks"][f].tobytes() == once["tracks"][f].tobytes(), f
    assert out["cams"]["W"].tobytes() == once["cams"]["W"].tobytes() and out["cams"]["w"].tobytes() == once["cams"]["w"].tobytes()


# ---- against independent answers

def numpy_residuals(P, head, X, cams=None):
    """(rx, ry) of every view of a track at X, in numpy, from the problem's cameras (or cams: {index: (W, w)})."""
    r = []
    for cam, frame, idx in P.views(head):
        W, w = (np.eye(3), np.zeros(3)) if cam < 0 else (P.W[cam].reshape(3, 3), P.w[cam]) if cams is None else cams[cam]
        x, y = tracksref.pixel(P.frames[frame, idx])
        Z = W @ X + w
        r += [(Z[0] / Z[2] - (x - K[2]) / K[0]) * K[0], (Z[1] / Z[2] - (y - K[3]) / K[1]) * K[1]]
    return np.array(r)


FD_POINT_BOUND, FD_CAM_BOUND = 100 * 6.1e-10, 100 * 3.7e-10      # 100 x the worst relative difference measured (below)


def test_point_and_camera_sums_equal_a_finite_difference_jacobian():
    """H = J^T J and g = J^T r with J the central finite-difference Jacobian of numpy residuals (step 1e-6 on X, 1e-7 on the camera's
    six parameters), relative to the largest entry.  Measured over the 40 tracks and 4 cameras: 6.04e-10 for the point step, 3.67e-10
    for the camera rows; the bounds are 100 x those, as for the resection's refinement."""
    s = Small(max_dist2=1e6)
    P = s.problem(perturbed_cams(s.args[0], s.args[5], 7))
    worst = 0.0
    for head in P.heads:
        X = P.tracks["X"][head].copy()
        H, g, cost, n, fl = P.point_eval(head)
        assert fl.all()
        r = numpy_residuals(P, head, X)
        J = np.stack([(numpy_residuals(P, head, X + 1e-6 * e) - numpy_residuals(P, head, X - 1e-6 * e)) / 2e-6 for e in np.eye(3)], axis=1)
        worst = max(worst, np.abs(H - J.T @ J).max() / np.abs(H).max(), np.abs(g - J.T @ r).max() / max(np.abs(g).max(), np.abs(J).max() * np.abs(r).max()))
        assert abs(cost - r @ r) <= 1e-9 * cost
    print(f"point step against finite differences: worst relative difference {worst:.2e}")
    assert worst < FD_POINT_BOUND
    worst = 0.0
    for j in range(4):
        rows = P.rows_of(j)
        W, w = P.W[j].reshape(3, 3), P.w[j]
        H, g, cost, n = resectrefineref.evaluate(W, w, K, rows, 1e6)
        rows = rows[~np.isnan(rows["u"])]                                             # (the rows that count: the train sides)
        assert n == len(rows) == 40

        def res(d):
            D = rodrigues(d[:3], np.linalg.norm(d[:3])) if np.linalg.norm(d[:3]) else np.eye(3)
            Z = rows["Y"] @ (D @ W).T + (D @ w + d[3:])
            return np.stack([(Z[:, 0] / Z[:, 2] - rows["u"]) * K[0], (Z[:, 1] / Z[:, 2] - rows["v"]) * K[1]], axis=1).reshape(-1)

        r = res(np.zeros(6))
        J = np.stack([(res(1e-7 * e) - res(-1e-7 * e)) / 2e-7 for e in np.eye(6)], axis=1)
        worst = max(worst, np.abs(H - J.T @ J).max() / np.abs(H).max(), np.abs(g - J.T @ r).max() / max(np.abs(g).max(), 1e-300))
    print(f"camera rows against finite differences: worst relative difference {worst:.2e}")
    assert worst < FD_CAM_BOUND


STRUCTURE_SWEEPS = 3      # measured: the sweeps after which every point is within 1e-9 (relative) of scipy's


def test_structure_only_reaches_scipys_least_squares():
    """Structure only: cameras exact and held, points off by 1 %, every view a member.  The cameras are held by chaining calls of
    one sweep and handing the exact cameras in again each time as cams_in: within a sweep the point step comes first, so every
    point step sees the exact cameras.  Each point after k sweeps against scipy.optimize.least_squares on the same residuals (numpy)
    from the same start, tolerances 1e-15.  Measured: every point within 1e-9 (relative) after 3 sweeps; 3 + 1 <= 64."""
    from scipy.optimize import least_squares

    s = Small(n_pairs=4, m=24, max_dist2=1e8)
    s.tracks_in["X"][0] *= 1.01
    cams_in = start_cams(s.args[0], s.args[5])
    t = s.tracks_in
    want = {}
    P0 = s.problem(cams_in)
    for head in P0.heads:
        sol = least_squares(lambda X: numpy_residuals(P0, head, X), t["X"][head], x_scale=1.0, xtol=1e-15, ftol=1e-15, gtol=1e-15)
        want[head] = sol.x
    reached = None
    for sweep in range(1, 64):
        out = bundleref.bundle(*s.args, t, s.refs, K, 1e8, 2, 1, cams_in)
        t = out["tracks"]
        err = max(np.linalg.norm(t["X"][h] - want[h]) / np.linalg.norm(want[h]) for h in want)
        if err < 1e-9:
            reached = sweep
            break
    print(f"structure only: within 1e-9 of scipy after {reached} sweeps")
    assert reached is not None and reached + 1 <= 64 and reached <= STRUCTURE_SWEEPS


def full_problem():
    s = Small(n_pairs=3, m=16, seed=5, max_dist2=1e8)
    # (the lists hold whole pixels, so the optimum's cost is the rounding's, not zero)
    s.tracks_in["X"][0] = s.X * 1.01
    return s, perturbed_cams(s.args[0], s.args[5], 11)


def scipy_optimum(s, cams_in):
    """The full problem from the same start: the first camera fixed, x_scale and tolerances of 1e-15 -> the optimal total cost."""
    from scipy.optimize import least_squares

    P = s.problem(cams_in)
    heads, n = P.heads, s.n

    def unpack(x):
        cams = {}
        for j in range(n):
            d = x[6 * j: 6 * j + 6]
            a = np.linalg.norm(d[:3])
            D = rodrigues(d[:3], a) if a else np.eye(3)
            cams[j] = (D @ P.W[j].reshape(3, 3), D @ P.w[j] + d[3:])
        return cams, x[6 * n:].reshape(-1, 3)

    def res(x):
        cams, X = unpack(x)
        return np.concatenate([numpy_residuals(P, h, X[k], cams) for k, h in enumerate(heads)])

    x0 = np.concatenate([np.zeros(6 * n), np.concatenate([P.tracks["X"][h] for h in heads])])
    sol = least_squares(res, x0, x_scale=1.0, xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return float(res(x0) @ res(x0)), float(2 * sol.cost)


def test_full_problem_cost_never_rises_and_closes_on_scipys_optimum():
    """Cameras off by 0.5 degrees and 2 %, points off by 1 %, every view a member.  The total cost (numpy's sum of the cameras'
    cost_after plus the held views') over sweeps = 1, 2, 4, .., 64 is non-increasing and never below scipy's optimum; the share of
    the gap closed is positive after 8 sweeps and larger after 64 (measured: see DESIGN 5.19)."""
    s, cams_in = full_problem()
    start, opt = scipy_optimum(s, cams_in)
    costs = {}
    for sweeps in (1, 2, 4, 8, 16, 32, 64):
        out = bundleref.bundle(*s.args, s.tracks_in, s.refs, K, 1e8, 2, sweeps, cams_in)
        assert (out["point_info"]["n_after"][0] == s.n + 1).all()                     # every view stays a member
        costs[sweeps] = float(np.sum(out["point_info"]["cost_after"][0]))
    seq = [costs[k] for k in (1, 2, 4, 8, 16, 32, 64)]
    share = {k: (start - costs[k]) / (start - opt) for k in (8, 64)}
    print(f"full problem: start {start:.6g}, scipy optimum {opt:.6g}, after 1 .. 64 sweeps {['%.6g' % c for c in seq]}, gap closed after 8: {share[8]:.4f}, after 64: {share[64]:.4f}")
    assert all(b <= a for a, b in zip(seq, seq[1:])) and seq[0] <= start
    assert all(c >= opt * (1 - 1e-9) - 1e-12 for c in seq)
    assert 0 < share[8] < share[64] <= 1 + 1e-9


# ---- the planted scenes through the restatements

def align(src, dst):
    """The similarity (s, R, t) with dst ~ s R src + t that maps the first two points of src onto those of dst (rotation: the
    smallest one that turns one baseline onto the other)."""
    a, b = src[1] - src[0], dst[1] - dst[0]
    sc = np.linalg.norm(b) / np.linalg.norm(a)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    v, c = np.cross(a, b), float(a @ b)
    A = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    R = np.eye(3) + A + A @ A / (1 + c)
    return sc, R, dst[0] - sc * R @ src[0]


@functools.lru_cache(maxsize=None)
def planted_bundle(seed, n):
    (poses, mt, counts, pts, bits, chain, frames), maps, (ms, rows, refs, goods, summary, paths), world, perms = planted_tracks(seed, n)
    tracks_in, refs_in = bundleref.dense_tracks(ms, rows, refs, n)
    P = bundleref.Problem(poses, mt, counts, bits, n, chain, frames, tracks_in, refs_in, K, 4.0, 3)
    first = bundleref.Problem(poses, mt, counts, bits, n, chain, frames, tracks_in, refs_in, K, 4.0, 3).run(1)
    out = P.run(8)
    cams = five_frames_with_points(seed, n)[2]
    truth_c = np.array([-R.T @ t for R, t in cams])                                   # the true centres of frames 0 .. 4, camera 0's frame

    def errors(X, centres):
        """(median point error of the good active tracks, mean centre error of frames 2 .. 4), after aligning frames 0 and 1."""
        est_c = np.vstack([np.zeros(3), centres])
        sc, R, t = align(est_c[:2], truth_c[:2])
        e = []
        for (j0, i0) in P.heads:
            if j0 == 0 and goods[0][i0] and tracks_in["n_views"][0, i0] >= 3:
                e.append(np.linalg.norm(sc * R @ X[0, i0] + t - world[planted_of(perms, 0, int(mt["query"][0, i0]))]))
        ce = np.linalg.norm((sc * (R @ est_c.T).T + t) - truth_c, axis=1)[2:]
        return float(np.median(e)), float(ce.mean()), len(e)

    c0 = start_cams(poses, chain)
    centre = lambda W, w: -(W.reshape(3, 3).T @ w)
    before = errors(tracks_in["X"], np.array([centre(c0["W"][j], c0["w"][j]) for j in range(4)]))
    after = errors(out["tracks"]["X"], out["cams"]["C"])
    return first, out, before, after


SCENES = [(seed, n) for n in (300, 1000) for seed in range(1, 9)]
POINT_AFTER_WORST_BOUND, CENTRE_AFTER_WORST_BOUND = 2 * 0.9128, 2 * 0.0879     # twice the worst measured, below (both seed 7, n 300)


@pytest.mark.parametrize("seed,n", SCENES)
def test_planted_scenes_members_do_not_fall_and_the_cost_does_not_rise(seed, n):
    first, out, before, after = planted_bundle(seed, n)
    c = out["cams"]
    wr = out["written"]
    pi = out["point_info"]
    # by construction: a step is kept only with more members, or as many at a lower cost - but the other block moves in between,
    # so the claim is on the totals the run reports, first evaluation to last
    nb, na = int(pi["n_before"][wr].sum()), int(pi["n_after"][wr].sum())
    print(f"planted bundle seed {seed} n {n}: members {nb} -> {na}, cost {pi['cost_before'][wr].sum():.2f} -> {pi['cost_after'][wr].sum():.2f}; "
          f"median point error {before[0]:.4f} -> {after[0]:.4f} over {before[2]} tracks, centre error {before[1]:.4f} -> {after[1]:.4f}")
    assert na >= nb
    if na == nb:
        assert pi["cost_after"][wr].sum() <= pi["cost_before"][wr].sum()
    assert ((c["accepted"] + c["rejected"] + c["invalid"] + c["skipped"]) == 8).all()


def test_planted_scenes_gain_against_the_planted_truth():
    """The 16 planted five-frame scenes through epiref.ransac -> poseref.pose -> chainref.chain -> tracksref.tracks -> 8 sweeps at
    max_dist2 = 4, min_views = 3.  Each segment is aligned to the truth by the similarity that maps the estimated centres of
    frames 0 and 1 onto the true ones; then the median distance to the planted point over the good tracks of at least three views
    that start in pair 0, and the mean distance of the centres of frames 2 .. 4, in scene units (the first baseline is 0.5), before
    (the tracks stage's X, the chain's cameras) -> after.  Measured, seeds 1 .. 8 at n = 300 then at n = 1000:
      points   0.2785 -> 0.1575, 0.4613 -> 0.0311, 0.2558 -> 0.1959, 0.5140 -> 0.4243, 0.2133 -> 0.2113, 0.9365 -> 0.4814, 1.3277 -> 0.9128,
               0.4943 -> 0.3874; 0.4806 -> 0.3473, 0.3062 -> 0.2432, 0.4125 -> 0.2027, 0.3923 -> 0.0489, 0.2107 -> 0.0967, 0.2118 -> 0.1625,
               0.5800 -> 0.3208, 0.5738 -> 0.4602
      centres  0.0539 -> 0.0102, 0.1058 -> 0.0043, 0.0641 -> 0.0619, 0.0512 -> 0.0426, 0.0593 -> 0.0759, 0.1545 -> 0.0452, 0.1672 -> 0.0879,
               0.0668 -> 0.0486; 0.0849 -> 0.0369, 0.0329 -> 0.0195, 0.1116 -> 0.0200, 0.0948 -> 0.0105, 0.0290 -> 0.0101, 0.0345 -> 0.0230,
               0.1348 -> 0.0221, 0.0670 -> 0.0545
    The points gain in 16 of 16 scenes, the centres in 15 (seed 5, n = 300, 30 tracks: worse); the median over the scenes of after /
    before is 0.705 for the points and 0.480 for the centres.  Required: both medians below 1, and each worst figure after within
    twice its measured value - sanity bounds on the convention, as for the tracks, not accuracy claims."""
    res = [planted_bundle(seed, n) for seed, n in SCENES]
    pr = np.array([after[0] / before[0] for _, _, before, after in res])
    cr = np.array([after[1] / before[1] for _, _, before, after in res])
    print(f"planted bundle over 16 scenes: median after / before, points {np.median(pr):.3f} (gain in {(pr < 1).sum()}), centres {np.median(cr):.3f} (gain in {(cr < 1).sum()})")
    assert np.median(pr) < 1 and np.median(cr) < 1
    assert max(after[0] for _, _, _, after in res) <= POINT_AFTER_WORST_BOUND and max(after[1] for _, _, _, after in res) <= CENTRE_AFTER_WORST_BOUND

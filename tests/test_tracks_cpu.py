"""The tracks step without a GPU: the C ABI's new symbols, struct layouts and argument checks, the plan header under the
sanitizers, and the CPU restatement of the arithmetic itself (tests/tracksref.py), which the GPU tests compare against byte for
byte: its rules on small hand-made lists, against numpy's least squares, on exact data, on planted five-frame scenes under the
true cameras, and on the same scenes through the whole chain of restatements."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import chainref, epiref, poseref, tracksref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
K = (800.0, 800.0, 960.0, 540.0)


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- the ABI

def test_tracks_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_tracks_dev", "vslam_tracks_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_trk_next", b"k_trk_walk", b"k_trk_rows"):
        assert k in names


class TrackRec(C.Structure):
    _fields_ = [("X", C.c_double * 3), ("det", C.c_double), ("n_views", C.c_uint32), ("n_ok", C.c_uint32), ("status", C.c_uint32), ("reserved", C.c_uint32)]


class TrackRef(C.Structure):
    _fields_ = [("head_record", C.c_uint32), ("pos", C.c_uint32)]


class TrackSummary(C.Structure):
    _fields_ = [("n_heads", C.c_uint32), ("n_good", C.c_uint32), ("max_views", C.c_uint32), ("reserved", C.c_uint32)]


def test_tracks_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_tracks_params": capi.TracksParams, "vslam_tracks_out": capi.TracksOut, "vslam_track": TrackRec, "vslam_track_ref": TrackRef,
               "vslam_track_summary": TrackSummary}
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
    for cname, ct, dt, size in (("vslam_track", TrackRec, capi.TRACK_DTYPE, 48), ("vslam_track_ref", TrackRef, capi.TRACK_REF_DTYPE, 8),
                                ("vslam_track_summary", TrackSummary, capi.TRACK_SUMMARY_DTYPE, 16)):
        assert rows[cname][0] == size == dt.itemsize
        assert [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]
    assert rows["vslam_tracks_params"][0] == 48


class Args:
    """A valid vslam_tracks_dev / vslam_tracks_host call over host arrays (nothing is launched without a GPU: the pointers are
    never followed)."""

    def __init__(self, n_pairs=2, match_cap=100, point_cap=50):
        words = (match_cap + 63) // 64
        self.keep = [np.zeros(n_pairs, capi.POSE_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32),
                     np.zeros((n_pairs, words), np.uint64), np.zeros(n_pairs, capi.CHAIN_DTYPE), np.zeros((n_pairs + 1, point_cap), capi.POINT_DTYPE),
                     np.zeros((n_pairs, match_cap), capi.TRACK_DTYPE), np.zeros((n_pairs, match_cap), capi.TRACK_REF_DTYPE),
                     np.zeros((n_pairs, words), np.uint64), np.zeros(n_pairs, capi.TRACK_SUMMARY_DTYPE)]
        poses, m, mc, bits, chain, frames, tracks, refs, good, summary = self.keep
        self.poses, self.matches, self.counts, self.bits, self.chain, self.frames = (a.ctypes.data for a in (poses, m, mc, bits, chain, frames))
        self.match_cap, self.point_cap, self.n_pairs = match_cap, point_cap, n_pairs
        self.prm = capi.TracksParams(capi.PoseParams(*K), 4.0, 2, 0)
        self.out = capi.TracksOut(C.sizeof(capi.TracksOut), tracks.ctypes.data, tracks.nbytes, refs.ctypes.data, refs.nbytes, good.ctypes.data, good.nbytes,
                                  summary.ctypes.data, summary.nbytes)

    def call(self, fn, prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return fn(None, self.poses, self.matches, self.counts, self.match_cap, self.bits, self.point_cap, self.n_pairs, self.chain, self.frames, ref(prm),
                  ref(out))


@pytest.mark.parametrize("entry", ["vslam_tracks_dev", "vslam_tracks_host"])
def test_tracks_rejects_bad_arguments_before_it_needs_a_gpu(lib, entry):
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

    for name in ("poses", "matches", "counts", "bits", "chain", "frames"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.TracksOut) - 8) == INVALID
    assert bad(out__tracks=None) == INVALID and bad(out__tracks_bytes=2 * 100 * 48 - 1) == INVALID
    assert bad(out__refs_bytes=2 * 100 * 8 - 1) == INVALID
    assert bad(out__good_bits_bytes=2 * 2 * 8 - 1) == INVALID
    assert bad(out__summary_bytes=2 * 16 - 1) == INVALID
    assert bad(a__match_cap=0) == INVALID and bad(a__point_cap=0) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for field in ("fx", "fy", "cx", "cy"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert bad(**{"K__" + field: v}) == INVALID, (field, v)
    assert bad(K__fx=0.0) == INVALID and bad(K__fy=0.0) == INVALID and bad(K__fx=-1.0) == INVALID and bad(K__fy=-1.0) == INVALID
    for v in (0.0, -1.0, float("nan"), float("inf")):
        assert bad(prm__max_dist2=v) == INVALID, v
    assert bad(prm__min_views=0) == INVALID and bad(prm__min_views=1) == INVALID
    if not gpu:  # the optional outputs may be absent, and no pairs and one pair are valid calls
        assert bad(out__refs=None, out__good_bits=None, out__summary=None) == HIP
        assert bad(a__n_pairs=0) == HIP and bad(a__n_pairs=1) == HIP and bad(prm__min_views=2) == HIP and bad(prm__min_views=0xFFFFFFFF) == HIP
        assert bad(K__cx=-5.0, K__cy=0.0) == HIP


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    """tests/tracks_plan_driver.cpp is a stand-alone program with its own main: nothing is loaded into Python under a sanitizer."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tracks_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    # match_cap 1 .. 2^32 - 1 (18 values) x point_cap 1 .. 2^32 - 1 (5) x n_pairs 1 .. 65535 (15), 8 checks each
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 18 * 5 * 15 * 8, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 55, rows["args"]
    src = open(os.path.join(CSRC, "vslam_tracks_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


def build_cxx_driver(tmp_path):
    """tests/tracks_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_tracks.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "tracks_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "tracks_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrapper_takes_no_pairs_and_refuses_sizes_that_do_not_fit(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run([build_cxx_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- scenes under the true cameras

def random_rotation(rng, most=0.3):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(-most, most)
    A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A


def true_records(cams):
    """The pose and chain records of the pairs between consecutive cameras (R_k, t_k), x_k = R_k x_world + t_k, as the pose and
    trajectory stages would give them for exact data: |pose.t| = 1 and the length in chain.scale, one segment."""
    n = len(cams) - 1
    poses, chain = np.zeros(n, capi.POSE_DTYPE), np.zeros(n, capi.CHAIN_DTYPE)
    for j in range(n):
        (R0, t0), (R1, t1) = cams[j], cams[j + 1]
        Rr = R1 @ R0.T
        tr = t1 - Rr @ t0
        s = np.linalg.norm(tr)
        poses["R"][j], poses["t"][j], poses["valid"][j] = Rr.reshape(9), tr / s, 1
        chain["W"][j], chain["w"][j], chain["C"][j], chain["Ct"][j] = R0.reshape(9), t0, -R0.T @ t0, -R1.T @ t1
        chain["scale"][j], chain["linked"][j], chain["valid"][j] = s, int(j >= 1), 1
    return poses, chain


def small_scene(n_pairs, m, seed=3):
    """m points seen by n_pairs + 1 cameras on a gentle random path; every frame lists the points in index order at octave 1,
    padding 0 (whole pixels), record i of every pair matches point i to point i, every record in front.
    -> (the arguments of tracksref.tracks up to frame_points, the planted points)."""
    rng = np.random.default_rng(seed)
    Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    cams = [(np.eye(3), np.zeros(3))]
    for _ in range(n_pairs):
        R, t = cams[-1]
        Rs = random_rotation(rng, 0.05)
        cams.append((Rs @ R, Rs @ t + np.array([-rng.uniform(0.4, 0.9), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])))
    X = np.stack([rng.uniform(-3, 3, m), rng.uniform(-2, 2, m), rng.uniform(5, 10, m)], axis=1)
    frames = np.zeros((n_pairs + 1, m), capi.POINT_DTYPE)
    for k, (R, t) in enumerate(cams):
        a = (Km @ (X @ R.T + t).T).T
        frames[k] = epiref.to_points(a[:, :2] / a[:, 2:], np.ones(m, np.int32), np.zeros(m, np.int32))
    poses, chain = true_records(cams)
    mt = np.zeros((n_pairs, m), capi.MATCH_DTYPE)
    mt["query"] = mt["train"] = np.arange(m)
    bits = np.stack([epiref.bits(np.ones(m, bool), (m + 63) // 64) for _ in range(n_pairs)])
    return [poses, mt, np.full(n_pairs, m, np.uint32), bits, m, chain, frames], X


def run(args, max_dist2=4.0, min_views=2, **kw):
    return tracksref.tracks(*args, K, max_dist2, min_views, **kw)


# ---- the rules

def test_every_point_of_a_clean_scene_is_one_track_through_all_pairs():
    args, X = small_scene(4, 20)
    ms, rows, refs, goods, summary, paths = run(args)
    assert ms == [20] * 4 and sorted(paths) == [(0, i) for i in range(20)]
    assert (rows[0]["n_views"] == 5).all() and (rows[0]["n_ok"] == 5).all() and (rows[0]["status"] == 3).all() and goods[0].all()
    assert np.abs(rows[0]["X"] - X).max() < 0.05                                  # whole-pixel rounding at depth 5 .. 10
    for j in range(1, 4):                                                          # not heads: NaN, NaN, 0, 0, 0
        assert rows[j].tobytes() == np.full(20, tracksref.empty_track()).tobytes() and not goods[j].any()
        assert (refs[j]["head_record"] == np.arange(20)).all() and (refs[j]["pos"] == j).all()
    assert summary["n_heads"].tolist() == [20, 0, 0, 0] and summary["n_good"].tolist() == [20, 0, 0, 0] and summary["max_views"].tolist() == [5, 0, 0, 0]
    assert np.isnan(rows[1]["X"]).all() and rows[1]["X"].view(np.uint64).max() == 0x7FF8000000000000 == rows[1]["det"].view(np.uint64).min()


def test_a_record_with_two_candidates_keeps_the_lowest():
    args, _ = small_scene(3, 12)
    args[1]["query"][1, 7] = args[1]["query"][1, 3]                               # records 3 and 7 of pair 1 both continue record 3 of pair 0
    ms, rows, refs, goods, summary, paths = run(args)
    assert paths[(0, 3)] == [(0, 3), (1, 3), (2, 3)] and paths[(1, 7)] == [(1, 7), (2, 7)] and (0, 7) in paths and paths[(0, 7)] == [(0, 7)]
    assert rows[1]["n_views"][7] == 3 and rows[0]["n_views"][7] == 2 and rows[0]["n_views"][3] == 4
    assert tuple(refs[1][7]) == (7, 0) and tuple(refs[2][7]) == (7, 1) and tuple(refs[1][3]) == (3, 1)
    assert summary["n_heads"].tolist() == [12, 1, 0]
    lengths = sorted(len(p) for p in paths.values())
    assert sum(lengths) == 36                                                     # every live record lies on exactly one track


def test_two_records_on_one_train_point_the_lowest_is_continued():
    args, _ = small_scene(3, 12)
    args[1]["train"][0, 5] = args[1]["train"][0, 2]                               # records 2 and 5 of pair 0 both end on point 2 of frame 1
    ms, rows, refs, goods, summary, paths = run(args)
    assert paths[(0, 2)] == [(0, 2), (1, 2), (2, 2)] and paths[(0, 5)] == [(0, 5)]
    assert paths[(1, 5)] == [(1, 5), (2, 5)]                                      # point 5 of frame 1 has no record before it: a head
    assert rows[0]["n_views"][5] == 2 and not goods[0][5]                         # two rays that do not meet within 2 px
    assert sum(len(p) for p in paths.values()) == 36


def test_a_pair_that_is_not_linked_ends_every_track_and_starts_new_ones():
    args, X = small_scene(5, 10)
    args[5]["linked"][2] = 0
    ms, rows, refs, goods, summary, paths = run(args)
    assert sorted(paths) == [(0, i) for i in range(10)] + [(2, i) for i in range(10)]
    assert (rows[0]["n_views"] == 3).all() and (rows[2]["n_views"] == 4).all() and summary["n_heads"].tolist() == [10, 0, 10, 0, 0]
    assert summary["max_views"].tolist() == [3, 0, 4, 0, 0] and (refs[2]["pos"] == 0).all() and (refs[4]["pos"] == 2).all()
    # a pair without a pose has no live record: nothing continues into it or out of it
    args[0]["best"][2] = -1
    ms, rows, refs, goods, summary, paths = run(args)
    assert sorted(paths) == [(0, i) for i in range(10)] + [(3, i) for i in range(10)]
    assert (refs[2]["head_record"] == 0xFFFFFFFF).all() and (refs[2]["pos"] == 0xFFFFFFFF).all() and summary["n_heads"].tolist() == [10, 0, 0, 10, 0]


def test_no_pairs_and_one_pair():
    args, X = small_scene(1, 10)
    ms, rows, refs, goods, summary, paths = run(args)
    assert ms == [10] and (rows[0]["n_views"] == 2).all() and goods[0].all() and summary[0].tolist() == (10, 10, 2, 0)
    assert np.abs(rows[0]["X"] - X).max() < 0.2
    empty = tracksref.tracks(args[0][:0], args[1][:0], args[2][:0], args[3][:0], 10, args[5][:0], args[6][:1], K, 4.0, 2)
    assert empty[0] == [] and len(empty[4]) == 0 and empty[5] == {}


def test_min_views_at_and_one_above_the_track_length():
    args, _ = small_scene(3, 10)
    at, above = run(args, min_views=4), run(args, min_views=5)
    assert (at[1][0]["n_views"] == 4).all() and (at[1][0]["status"] == 3).all() and at[3][0].all()
    assert (above[1][0]["status"] == 1).all() and not above[3][0].any() and above[4]["n_good"].tolist() == [0, 0, 0]
    assert at[1][0]["X"].tobytes() == above[1][0]["X"].tobytes() and (above[1][0]["n_ok"] == 4).all()


def exact_views(rng, n, X):
    """n cameras that all see X in front, with the exact (unrounded) pixel of X in each."""
    v = np.zeros(n, tracksref.VIEW_DTYPE)
    for p in range(n):
        while True:
            R = random_rotation(rng, 0.4)
            Cw = rng.uniform(-3, 3, 3)
            t = -R @ Cw
            Z = R @ X + t
            if Z[2] > 1.0:
                break
        v["W"][p], v["w"][p], v["C"][p] = R.reshape(9), t, Cw
        v["x"][p], v["y"][p] = K[0] * Z[0] / Z[2] + K[2], K[1] * Z[1] / Z[2] + K[3]
    return v


def test_a_view_behind_its_camera_is_not_ok():
    rng = np.random.default_rng(11)
    X = np.array([0.5, -0.25, 8.0])
    v = exact_views(rng, 4, X)
    t = tracksref.solve(v, K, 1e-6, 2)
    assert t["n_ok"] == 4 and t["status"] == 3
    # the third camera turned half round about its own y axis, the pixel mirrored: the same ray, but X is behind it
    flip = np.diag([-1.0, 1.0, -1.0])
    v["W"][2], v["w"][2] = (flip @ v["W"][2].reshape(3, 3)).reshape(9), flip @ v["w"][2]
    v["y"][2] = 2 * K[3] - v["y"][2]                                               # (-Z0, Z1, -Z2) projects to (Z0 / Z2, -Z1 / Z2)
    b = tracksref.solve(v, K, 1e-6, 2)
    assert b["n_views"] == 4 and b["n_ok"] == 3 and b["status"] == 1 and np.abs(b["X"] - X).max() < 1e-9


# ---- (a) steps 3 and 4 against numpy's least squares

LSTSQ_WORST = 2.3e-12   # measured, see the docstring below
LSTSQ_BOUND = 100 * LSTSQ_WORST


def test_point_equals_numpy_least_squares_on_the_stacked_projector_rows():
    """600 random tracks of 2 .. 9 views, the pixels perturbed by up to 3 px so that the rays do not meet: X against
    numpy.linalg.lstsq on the stacked rows (I - d d^T / dd)(X - C) = 0.  Only systems whose smallest singular value is at least
    1e-3 of the largest are kept (the filter may drop at most 5 % of the draws; it dropped none of these).  Measured: worst
    |difference| 2.3e-12 over the 600 draws (coordinates reach ~12; the cofactor solve works on the normal equations, whose
    condition is the square of the stacked system's); the bound is 100 x that."""
    rng = np.random.default_rng(23)
    worst, kept, draws = 0.0, 0, 600
    for trial in range(draws):
        n = int(rng.integers(2, 10))
        X = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(5, 12)])
        v = exact_views(rng, n, X)
        v["x"] += rng.uniform(-3, 3, n)
        v["y"] += rng.uniform(-3, 3, n)
        rows, rhs = [], []
        for p in range(n):
            W = v["W"][p].reshape(3, 3)
            d = W.T @ np.array([(v["x"][p] - K[2]) / K[0], (v["y"][p] - K[3]) / K[1], 1.0])
            P = np.eye(3) - np.outer(d, d) / (d @ d)
            rows.append(P), rhs.append(P @ v["C"][p])
        A, b = np.concatenate(rows), np.concatenate(rhs)
        sv = np.linalg.svd(A, compute_uv=False)
        if sv[-1] < 1e-3 * sv[0]:
            continue
        kept += 1
        want = np.linalg.lstsq(A, b, rcond=None)[0]
        got = tracksref.solve(v, K, 1e6, 2)
        assert got["status"] & 1 and got["det"] > 0
        worst = max(worst, np.abs(got["X"] - want).max())
    print(f"steps 3 - 4 against numpy.linalg.lstsq: kept {kept} of {draws} draws, worst |difference| {worst:.3e}")
    assert kept >= 0.95 * draws
    assert worst <= LSTSQ_BOUND


# ---- (b) exact data

def test_exact_cameras_and_exact_pixels_give_the_planted_point():
    rng = np.random.default_rng(29)
    worst = 0.0
    for trial in range(200):
        n = int(rng.integers(2, 10))
        X = np.array([rng.uniform(-4, 4), rng.uniform(-3, 3), rng.uniform(5, 12)])
        t = tracksref.solve(exact_views(rng, n, X), K, 1e-6, 2)
        assert t["n_views"] == n and t["n_ok"] == n and t["status"] == 3, trial
        worst = max(worst, np.abs(t["X"] - X).max())
    print(f"exact cameras and pixels, 200 tracks of 2 .. 9 views: worst |X - planted| {worst:.3e}")
    assert worst <= 1e-9


# ---- (c) the gain from more views, under the true cameras

BASELINES = (0.5, 0.9, 0.4, 0.7)
YAW = 0.04


def five_frames_with_points(seed, n, wrong=0.2, width=1920, height=1080, f=800.0):
    """The draws of tests/test_chain_cpu.py's five_frames, in its order, also returning the planted points and each frame's
    permutation: n points seen by five cameras, x_{k+1} = R x_k + t_k with a yaw of 0.04 per step and t_k = (-baseline_k, 0, 0);
    every frame lists the points in an order of its own (point i is record perms[k][i] of frame k), at mixed octaves and paddings,
    rounded to the octave pitch; pair j matches frame j to frame j + 1, a fraction `wrong` of its records with a random train
    index.  -> (matches [4][n], point lists [5][n], the cameras, the points [n, 3] in camera 0's frame, perms)."""
    rng = np.random.default_rng(seed)
    Km = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1.0]])
    Ry = np.array([[np.cos(YAW), 0, np.sin(YAW)], [0, 1, 0], [-np.sin(YAW), 0, np.cos(YAW)]])
    cams = [(np.eye(3), np.zeros(3))]
    for b in BASELINES:
        R, t = cams[-1]
        cams.append((Ry @ R, Ry @ t + np.array([-b, 0, 0])))
    pix, world = [[] for _ in cams], []
    while len(pix[0]) < n:
        X = np.array([rng.uniform(-6, 6), rng.uniform(-3.5, 3.5), rng.uniform(4, 12)])
        uv = []
        for R, t in cams:
            a = Km @ (R @ X + t)
            uv.append(a[:2] / a[2])
        if all(0 <= a[0] < width - 1 and 0 <= a[1] < height - 1 for a in uv):
            world.append(X)
            for k in range(5):
                pix[k].append(uv[k])
    octave = rng.integers(0, 3, n).astype(np.int32)
    padding = rng.integers(0, 2, n).astype(np.int32)
    perms = [rng.permutation(n) for _ in cams]
    lists = []
    for k in range(5):
        p = np.zeros(n, capi.POINT_DTYPE)
        p[perms[k]] = epiref.to_points(np.array(pix[k]), octave, padding)
        lists.append(p)
    matches = []
    for j in range(4):
        m = np.zeros(n, capi.MATCH_DTYPE)
        bad = rng.random(n) < wrong
        m["query"], m["train"] = perms[j], np.where(bad, rng.integers(0, n, n), perms[j + 1])
        m["dist2"] = rng.random(n).astype(np.float32)
        matches.append(m[np.argsort(m["query"], kind="stable")])
    return matches, lists, cams, np.array(world), perms


def planted_of(perms, j, q):
    """The planted point's index of record q of frame j's list."""
    inv = np.empty(len(perms[j]), np.int64)
    inv[perms[j]] = np.arange(len(perms[j]))
    return inv[q]


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("seed", range(1, 9))
def test_five_views_beat_two_under_the_true_cameras(seed, n):
    """Chain records from the TRUE cameras, pixels rounded to the octave pitch, a fifth of every pair's records mismatched.  Over
    the full-length tracks (five views) that are good at 2 px, the median distance to the planted point of the head's query
    record from all five views must be below 0.5 x the median of the same tracks cut to their first two views.  Measured over
    seeds 1 .. 8, n = 300 and 1000: 81 .. 101 and 285 .. 310 such tracks, median error 0.0063 .. 0.0095 scene units from five
    views and 0.0350 .. 0.0569 from two, ratio 0.134 .. 0.229."""
    matches, lists, cams, world, perms = five_frames_with_points(seed, n)
    poses, chain = true_records(cams)
    args = [poses, np.stack(matches), np.full(4, n, np.uint32), np.stack([epiref.bits(np.ones(n, bool), (n + 63) // 64)] * 4), n, chain, np.stack(lists)]
    ms, rows, refs, goods, summary, paths = run(args)
    cut = run(args, cut=2)[1]
    full = np.flatnonzero(goods[0] & (rows[0]["n_views"] == 5))
    assert len(full) >= n // 4
    truth = world[planted_of(perms, 0, args[1]["query"][0, full])]
    e5 = np.linalg.norm(rows[0]["X"][full] - truth, axis=1)
    e2 = np.linalg.norm(cut[0]["X"][full] - truth, axis=1)
    assert (cut[0]["n_views"][full] == 2).all()
    print(f"true cameras seed {seed} n {n}: {len(full)} full-length good tracks, median error five views {np.median(e5):.4f} two views {np.median(e2):.4f} "
          f"ratio {np.median(e5) / np.median(e2):.3f}")
    assert np.median(e5) < 0.5 * np.median(e2)


# ---- (d) planted frames through the whole chain of restatements

@functools.lru_cache(maxsize=None)
def planted_tracks(seed, n, min_links=16):
    """RANSAC (512 hypotheses, 2 px) and pose of every pair by the restatements, the chain, then the tracks at 2 px."""
    matches, lists, cams, world, perms = five_frames_with_points(seed, n)
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
    chain, _, maps, _, _, _ = chainref.chain(poses, mt, counts, pts, bits, n, min_links)
    out = tracksref.tracks(poses, mt, counts, bits, n, chain, np.stack(lists), K, 4.0, 2)
    return (poses, mt, counts, pts, bits, chain, np.stack(lists)), maps, out, world, perms


TRACK_MEDIAN_BOUND, TRACK_WORST_BOUND, MAP_MEDIAN_BOUND, MAP_WORST_BOUND = 2 * 1.6126, 2 * 19.5541, 2 * 1.6084, 2 * 19.5541  # twice the worst measured, below


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("seed", range(1, 9))
def test_restatements_track_the_planted_frames(seed, n):
    """epiref.ransac -> poseref.pose -> chainref.chain -> tracksref.tracks on the planted five-frame scenes.  For the heads of
    good tracks: the distance of the track's X to the planted point of the head's query record, and of the chain's map row of the
    same record, both in units of the first baseline (the chain's world unit).  Measured over seeds 1 .. 8 and n = 300, 1000:
    241 .. 1235 good tracks per scene, 113 .. 135 and 383 .. 417 of all tracks with five views; track points, median 0.1766 ..
    1.6126 (seed 6, n 300) and worst 1.1789 .. 19.5541 (seed 8, n 300); map rows, median 0.2399 .. 1.6084 and worst 1.6542 ..
    19.5541.  The worst figures are two-view tracks over a mismatch that lies along the epipolar line: two rays always nearly
    meet, so the reprojection test cannot refuse them, and the track's point is the map's.  The bounds are twice the worst of
    each: sanity bounds on the convention (the medians: a point in the wrong frame or unit is off by the scene's depth, 8 .. 24
    units), not accuracy claims.  The estimated poses' error is in both figures; whether the track points beat the map rows is
    printed, not required: by the median they did in 11 of the 16 scenes."""
    (poses, mt, counts, pts, bits, chain, frames), maps, (ms, rows, refs, goods, summary, paths), world, perms = planted_tracks(seed, n)
    assert chain["linked"].tolist() == [0, 1, 1, 1]
    et, em, by_length = [], [], {}
    for (j0, i0), path in paths.items():
        by_length[len(path) + 1] = by_length.get(len(path) + 1, 0) + 1
        if not goods[j0][i0]:
            continue
        truth = world[planted_of(perms, j0, int(mt["query"][j0, i0]))] / BASELINES[0]
        et.append(np.linalg.norm(rows[j0]["X"][i0] - truth))
        em.append(np.linalg.norm(maps[j0][i0] - truth))
    et, em = np.array(et), np.array(em)
    print(f"planted tracks seed {seed} n {n}: tracks by views {dict(sorted(by_length.items()))}, good {len(et)}; track points median {np.median(et):.4f} "
          f"worst {et.max():.4f}; map rows median {np.median(em):.4f} worst {em.max():.4f}; tracks better: {bool(np.median(et) < np.median(em))}")
    assert len(et) >= n // 4 and summary["n_good"].sum() == len(et) and summary["n_heads"].sum() == len(paths)
    assert np.median(et) <= TRACK_MEDIAN_BOUND and et.max() <= TRACK_WORST_BOUND
    assert np.median(em) <= MAP_MEDIAN_BOUND and em.max() <= MAP_WORST_BOUND

"""Pose from homography without a GPU: the C ABI's new symbols, struct layouts and argument checks with their messages, the host
sizing under the sanitizers, the capi wrappers on CPU tensors, and the CPU restatement of the arithmetic itself
(tests/hposeref.py), which the GPU tests compare against byte for byte: against the planted motion and a numpy SVD
decomposition, on the planted planes and rotations of tests/homref.py, the ambiguity rule at its boundaries, the merge rule, and
the five-frame plane scene through the chain."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import chainref, epiref, homref, hposeref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
K = hposeref.K_PLANTED


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_hpose_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_hpose_dev", "vslam_hpose_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_hpose_candidates", b"k_hpose_vote", b"k_hpose_select", b"k_hpose_points"):
        assert k in names


def test_hpose_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_hpose_params": capi.HposeParams, "vslam_hpose_cand": capi.HposeCand, "vslam_hpose": capi.Hpose, "vslam_hpose_out": capi.HposeOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
    lines += ['  printf("kinds %d %d %d\\n", VSLAM_HPOSE_NONE, VSLAM_HPOSE_PLANE, VSLAM_HPOSE_ROTATION);', "  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()}
    for cname, ct in structs.items():
        assert rows[cname] == [C.sizeof(ct)] + [getattr(ct, f[0]).offset for f in ct._fields_], cname
    assert rows["vslam_hpose_params"][0] == 64 and rows["vslam_hpose_cand"][0] == 128 and rows["vslam_hpose"][0] == 144
    assert rows["kinds"] == [capi.HPOSE_NONE, capi.HPOSE_PLANE, capi.HPOSE_ROTATION]
    assert capi.HPOSE_CAND_DTYPE.itemsize == 128 and capi.HPOSE_DTYPE.itemsize == 144
    for dt, ct in ((capi.HPOSE_CAND_DTYPE, capi.HposeCand), (capi.HPOSE_DTYPE, capi.Hpose)):
        assert [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]


class Args:
    """A valid vslam_hpose_dev / vslam_hpose_host call over host arrays (nothing is launched without a GPU: the pointers are never
    followed)."""

    def __init__(self, n_pairs=2, match_cap=100, cap=50):
        self.keep = [np.zeros(n_pairs, capi.HOMOGRAPHY_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32),
                     np.zeros((n_pairs, cap), capi.POINT_DTYPE), np.zeros(n_pairs, capi.POSE_DTYPE), np.zeros(n_pairs, capi.HPOSE_DTYPE),
                     np.zeros((n_pairs, 4), capi.HPOSE_CAND_DTYPE), np.zeros((n_pairs, match_cap, 3), np.float64),
                     np.zeros((n_pairs, (match_cap + 63) // 64), np.uint64)]
        mod, m, mc, p, poses, info, cand, pts, bits = self.keep
        self.models, self.matches, self.counts, self.qp, self.tp = mod.ctypes.data, m.ctypes.data, mc.ctypes.data, p.ctypes.data, p.ctypes.data
        self.match_cap, self.query_cap, self.train_cap, self.n_pairs = match_cap, cap, cap, n_pairs
        self.prm = capi.HposeParams(capi.PoseParams(*K), 4.0, capi.HPOSE_MIN_SPREAD, capi.HPOSE_AMBIGUOUS_NUM, capi.HPOSE_AMBIGUOUS_DEN, 1, 0)
        self.K = self.prm.K
        self.out = capi.HposeOut(C.sizeof(capi.HposeOut), poses.ctypes.data, poses.nbytes, info.ctypes.data, info.nbytes, cand.ctypes.data, cand.nbytes,
                                 pts.ctypes.data, pts.nbytes, bits.ctypes.data, bits.nbytes)

    def call(self, fn, prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return fn(None, self.models, self.matches, self.counts, self.match_cap, self.qp, self.query_cap, self.tp, self.train_cap, self.n_pairs, None,
                  ref(prm), ref(out))


@pytest.mark.parametrize("entry", ["vslam_hpose_dev", "vslam_hpose_host"])
def test_hpose_rejects_bad_arguments_before_it_needs_a_gpu(lib, entry):
    import torch

    fn, gpu = getattr(lib, entry), torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(fn) == (INVALID if gpu else HIP)
    assert Args().call(fn, prm=None) == INVALID and Args().call(fn, out=None) == INVALID

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
        return a.call(fn)

    for name in ("models", "matches", "counts", "qp", "tp"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.HposeOut) - 8) == INVALID
    assert bad(out__poses=None) == INVALID and bad(out__poses_bytes=2 * 112 - 1) == INVALID
    assert bad(out__info=None) == INVALID and bad(out__info_bytes=2 * 144 - 1) == INVALID
    assert bad(out__candidates_bytes=2 * 4 * 128 - 1) == INVALID
    assert bad(out__points_bytes=2 * 100 * 24 - 1) == INVALID
    assert bad(out__front_bits_bytes=2 * 2 * 8 - 1) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for field in ("fx", "fy", "cx", "cy"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert bad(**{"K__" + field: v}) == INVALID, (field, v)
    for field in ("fx", "fy"):
        for v in (0.0, -0.0, -800.0):
            assert bad(**{"K__" + field: v}) == INVALID, (field, v)
    for field in ("max_dist2", "min_spread"):
        for v in (0.0, -1.0, float("nan"), float("inf")):
            assert bad(**{"prm__" + field: v}) == INVALID, (field, v)
    assert bad(prm__ambiguous_den=0) == INVALID and bad(prm__only_degenerate=2) == INVALID and bad(prm__only_degenerate=-1) == INVALID
    assert bad(prm__reserved=1) == INVALID
    assert bad(a__match_cap=0) == INVALID and bad(a__query_cap=0) == INVALID and bad(a__train_cap=0) == INVALID
    if not gpu:  # the optional outputs may be absent, every pair may be asked for, and no pairs is a valid call
        assert bad(out__candidates=None, out__points=None, out__front_bits=None) == HIP
        assert bad(prm__only_degenerate=0, prm__ambiguous_num=0) == HIP and bad(a__n_pairs=0) == HIP


# the message of every check, byte for byte: the entry points put "hpose: " / "hpose_host: " in front and callers match on them
MESSAGES = [
    ("valid", "-"),
    ("null params", "null argument"),
    ("null out", "null argument"),
    ("struct_size", "out->struct_size is not sizeof(vslam_hpose_out)"),
    ("pairs < 0", "0 .. 65535 pairs per call"),
    ("pairs > 65535", "0 .. 65535 pairs per call"),
    ("fx nan", "the intrinsics must be finite"),
    ("cy inf", "the intrinsics must be finite"),
    ("fx zero", "fx and fy must be positive"),
    ("fy negative", "fx and fy must be positive"),
    ("max_dist2 nan", "max_dist2 must be finite and positive"),
    ("max_dist2 zero", "max_dist2 must be finite and positive"),
    ("min_spread nan", "min_spread must be finite and positive"),
    ("min_spread zero", "min_spread must be finite and positive"),
    ("den zero", "ambiguous_den must be positive"),
    ("only_degenerate 2", "only_degenerate must be 0 or 1"),
    ("reserved", "reserved must be 0"),
    ("null models", "null input"),
    ("null train", "null input"),
    ("query_cap 0", "a capacity is zero"),
    ("null poses", "poses is required"),
    ("poses short", "poses buffer too small"),
    ("null info", "info is required"),
    ("info short", "info buffer too small"),
    ("candidates short", "candidates buffer too small"),
    ("points short", "points buffer too small"),
    ("front_bits short", "front_bits buffer too small"),
    ("poses and info alone", "-"),
]


def test_host_sizing_checks_and_messages_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hpose_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines() if not l.startswith("msg ")}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 18 * 15 * 7, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 50, rows["args"]
    assert rows["order"]["bad"] == "0" and int(rows["order"]["checked"]) == 16, rows["order"]
    got = [tuple(l[4:].split("|", 1)) for l in out.stdout.splitlines() if l.startswith("msg ")]
    assert got == MESSAGES
    src = open(os.path.join(CSRC, "vslam_hpose_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src
    for stage in ("hpose: ", "hpose_host: "):
        assert f'std::string("{stage}") + why' in open(os.path.join(CSRC, "vslam_hpose.hip")).read()


def test_capi_wrappers_check_their_tensors_without_a_gpu():
    import torch

    n, cap = 2, 64
    t = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8)
    good = dict(models=t(n * 168), matches=torch.zeros((n, cap, 3), dtype=torch.int32), match_counts=torch.zeros(n, dtype=torch.int32),
                query_points=torch.zeros((n, 10, 6), dtype=torch.int32), train_points=torch.zeros((n, 10, 6), dtype=torch.int32), intrinsics=K,
                poses=t(n * 112), info=t(n * 144))
    ctx = capi.Context.__new__(capi.Context)  # no library call is reached: every case below fails a check first
    ctx.where = torch.device("cpu")
    with pytest.raises(ValueError, match="hpose: poses is required"):
        ctx.hpose(**dict(good, poses=None))
    with pytest.raises(ValueError, match="hpose: info is required"):
        ctx.hpose(**dict(good, info=None))
    with pytest.raises(ValueError, match="hpose: models must hold n_pairs \\* 168 bytes"):
        ctx.hpose(**dict(good, models=t(n * 168 - 1)))
    with pytest.raises(ValueError, match="hpose: priors must hold n_pairs \\* 112 bytes"):
        ctx.hpose(**dict(good, priors=t(n * 112 - 1)))
    with pytest.raises(ValueError, match="hpose: matches must be"):
        ctx.hpose(**dict(good, matches=torch.zeros((n, cap), dtype=torch.int32)))
    with pytest.raises(ValueError, match="hpose: points must be a contiguous tensor"):
        ctx.hpose(**dict(good, points=torch.zeros((n, cap, 6), dtype=torch.float64)[:, :, ::2]))
    with pytest.raises(ValueError, match="hpose: fewer sets than pairs"):
        ctx.hpose(**dict(good, n_pairs=3))
    models, mt = np.zeros(n, capi.HOMOGRAPHY_DTYPE), np.zeros((n, cap), capi.MATCH_DTYPE)
    pts = np.zeros((n, 10), capi.POINT_DTYPE)
    with pytest.raises(ValueError, match="hpose_host: poses is required"):
        ctx.hpose_host(models, mt, np.zeros(n), pts, pts, K, None)
    with pytest.raises(ValueError, match="hpose_host: poses must be a C-contiguous"):
        ctx.hpose_host(models, mt, np.zeros(n), pts, pts, K, np.zeros(n + 1, capi.POSE_DTYPE))
    with pytest.raises(ValueError, match="hpose_host: points must be a C-contiguous float64 array of 384 elements"):
        ctx.hpose_host(models, mt, np.zeros(n), pts, pts, K, np.zeros(n, capi.POSE_DTYPE), points=np.zeros((n, cap, 3), np.float32))
    with pytest.raises(ValueError, match="hpose_host: one count and one prior per pair"):
        ctx.hpose_host(models, mt, np.zeros(n + 1), pts, pts, K, np.zeros(n, capi.POSE_DTYPE))
    with pytest.raises(ValueError, match="hpose_host: matches, query_points and train_points"):
        ctx.hpose_host(models, mt, np.zeros(n), pts[:1], pts, K, np.zeros(n, capi.POSE_DTYPE))


def build_cxx_driver(tmp_path):
    """tests/hpose_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_hpose.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "hpose_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "hpose_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrapper_refuses_matches_without_points_and_a_pose_of_other_matches(tmp_path):
    """vslam::poseFromHomography without a GPU: what the wrapper refuses itself, before it asks for a context - and the pose it was
    given is left as it was."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run([build_cxx_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the restatement itself

def random_plane_motion(rng):
    """A random rotation (up to ~0.5 rad), a random translation over distance T = t / d with |T| in 0.05 .. 0.6, and a random unit
    normal with a positive third component (the plane faces the query camera)."""
    R = hposeref.rotation(rng.normal(size=3), rng.uniform(-0.5, 0.5))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    n = np.array([rng.uniform(-0.7, 0.7), rng.uniform(-0.7, 0.7), 1.0])
    return R, t, n / np.linalg.norm(n), rng.uniform(0.05, 0.6)


def svd_decomposition(A):
    """The four (R, t, n) of A ~ R + T n^T from numpy's SVD (Ma, Soatto, Kosecka, Sastry, An Invitation to 3-D Vision, 5.3.3)."""
    s = np.linalg.svd(A, compute_uv=False)
    A = A / s[1]
    _, s, Vt = np.linalg.svd(A)
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    v1, v2, v3 = Vt
    l1, l3 = s[0] ** 2, s[2] ** 2
    out = []
    for sg in (1.0, -1.0):
        u = (np.sqrt(1 - l3) * v1 + sg * np.sqrt(l1 - 1) * v3) / np.sqrt(l1 - l3)
        U = np.stack([v2, u, np.cross(v2, u)], axis=1)
        W = np.stack([A @ v2, A @ u, np.cross(A @ v2, A @ u)], axis=1)
        R, n = W @ U.T, np.cross(v2, u)
        T = (A - R) @ n
        out += [(R, T / np.linalg.norm(T), n), (R, -T / np.linalg.norm(T), -n)]
    return out


SVD_BOUND, PLANTED_BOUND, DET_BOUND, ORTH_BOUND = 100 * 3.81e-14, 100 * 6.49e-15, 100 * 4.22e-15, 100 * 3.77e-15  # 100 x the worst measured, see the docstring below


def test_candidates_contain_the_planted_motion_and_equal_the_svd_decomposition():
    """Measured with this restatement over 48 random motions (seed 7), each at a random scale in 0.1 .. 10, through K = identity
    and through the planted K in turn: the worst difference of a candidate's R, t or n from the numpy SVD decomposition's is
    3.81e-14 (numpy's own error included), from the planted (R, t / |t|, n) 6.49e-15; |det R - 1| <= 4.22e-15 and |R^T R - I| <=
    3.77e-15 - twice the relative pose's 2e-15: R is a sum of three outer products of the scaled A's images, not of vectors
    normalised one by one.  Each bound is 100 x the worst measured; a transposed or twin-swapped result errs by order 1."""
    rng = np.random.default_rng(7)
    worst_svd, worst_planted, worst_det, worst_orth = 0.0, 0.0, 0.0, 0.0
    for trial in range(48):
        R, t, n, inv_d = random_plane_motion(rng)
        A = (R + inv_d * np.outer(t, n)) * rng.uniform(0.1, 10)
        if trial % 2:
            model = hposeref.model_record(A)      # either sign rule satisfied: H and G come with the homography section's signs
            A_in = hposeref.euclidean(model["H"][0], K)
        else:
            A_in = A
        kind, c, info, invd = hposeref.decompose(A_in, 1e-6)
        assert kind == capi.HPOSE_PLANE and c["valid"].all() and (c["front"] == 0).all()
        diff = lambda k, Rw, tw, nw: max(np.abs(c["R"][k].reshape(3, 3) - Rw).max(), np.abs(c["t"][k] - tw).max(), np.abs(c["n"][k] - nw).max())
        used = set()
        for Rw, tw, nw in svd_decomposition(A_in):
            d = [diff(k, Rw, tw, nw) for k in range(4)]
            k = int(np.argmin(d))
            worst_svd = max(worst_svd, d[k])
            used.add(k)
        assert used == {0, 1, 2, 3}
        worst_planted = max(worst_planted, min(diff(k, R, t, n) for k in range(4)))
        best = int(np.argmin([diff(k, R, t, n) for k in range(4)]))
        assert abs(invd[best >> 1] - inv_d) <= SVD_BOUND
        # the layout: c and c ^ 1 share R and differ in the signs of t and n, bit for bit
        assert c["R"][0].tobytes() == c["R"][1].tobytes() and c["R"][2].tobytes() == c["R"][3].tobytes()
        for k in (0, 2):
            assert (c["t"][k] == -c["t"][k + 1]).all() and (c["n"][k] == -c["n"][k + 1]).all()
        for k in range(4):
            Rk = c["R"][k].reshape(3, 3)
            worst_det = max(worst_det, abs(np.linalg.det(Rk) - 1.0))
            worst_orth = max(worst_orth, np.abs(Rk.T @ Rk - np.eye(3)).max())
    print(f"decomposition: worst against the SVD {worst_svd:.3g}, against the planted motion {worst_planted:.3g}, |det - 1| {worst_det:.3g}, "
          f"|R^T R - I| {worst_orth:.3g}")
    assert worst_svd <= SVD_BOUND and worst_planted <= PLANTED_BOUND
    assert worst_det <= DET_BOUND and worst_orth <= ORTH_BOUND


def test_invalid_inputs_give_no_candidates():
    for A in (np.zeros((3, 3)), np.full((3, 3), np.nan), np.full((3, 3), np.inf)):
        kind, c, info, invd = hposeref.decompose(A, capi.HPOSE_MIN_SPREAD)
        assert kind == capi.HPOSE_NONE and c.tobytes() == bytes(c.nbytes) and info.tobytes() == bytes(info.nbytes) and (invd == 0).all()
    # the identity: spread 0 exactly, a rotation, R = I
    kind, c, info, _ = hposeref.decompose(np.eye(3) * 3.0, capi.HPOSE_MIN_SPREAD)
    assert kind == capi.HPOSE_ROTATION and info["spread"][0] == 0.0 and (info["R"][0] == np.eye(3).ravel()).all() and c.tobytes() == bytes(c.nbytes)
    # min_spread is compared with >=: the spread itself is a plane, one ulp above it a rotation
    R, t, n, inv_d = random_plane_motion(np.random.default_rng(3))
    A = R + inv_d * np.outer(t, n)
    spread = float(hposeref.decompose(A, 1e-6)[2]["spread"][0])
    assert hposeref.decompose(A, spread)[0] == capi.HPOSE_PLANE and hposeref.decompose(A, np.nextafter(spread, 1.0))[0] == capi.HPOSE_ROTATION
    # |T| = 0 exactly: a spread of a few ulps passes a min_spread of 1e-300, T = A n - R n cancels, and that sign's candidates are invalid
    for name, (Au, valid) in hposeref.UNDERFLOW_A.items():
        kind, c, info, invd = hposeref.decompose(np.array(Au), hposeref.UNDERFLOW_MIN_SPREAD)
        assert kind == capi.HPOSE_PLANE and c["valid"].tolist() == valid and 0 < info["spread"][0] < 1e-14, name
        assert [bool(v) for v in invd] == [bool(valid[0]), bool(valid[2])] and all(c[k].tobytes() == bytes(128) for k in range(4) if not valid[k])
        assert hposeref.decompose(np.array(Au), capi.HPOSE_MIN_SPREAD)[0] == capi.HPOSE_ROTATION      # under the default it is a rotation


def angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


PLANTED_R = hposeref.rotation((0.0, 1.0, 0.0), 0.05)
PLANTED_T = np.array([-1.0, 0.0, 0.0])
SCENES = [(seed, n) for n in (300, 1000) for seed in range(1, 9)]
_planted = {}


def planted(kind, seed, n):
    """One planted scene of homref (kinds "plane" and "rotation") through homref.ransac (512 hypotheses, seed 7, 4 px^2) and the
    restatement, computed once."""
    key = (kind, seed, n)
    if key not in _planted:
        m, qp, tp, _ = homref.planted_scene(seed, n, kind)
        model = homref.ransac(m, qp, tp, 512, 7, 4.0)[0]
        _planted[key] = (model, hposeref.pair(model[0], m, qp, tp, K))
    return _planted[key]


@pytest.mark.parametrize("seed,n", SCENES)
def test_planted_planes_get_the_planted_motion(seed, n):
    """Measured over seeds 1 .. 8 and n = 300, 1000: the winner has every supported record in front (184 .. 701), its twin 0.50 ..
    0.54 of them and the other two candidates none and the rest; the rotation is within 0.140 degrees of the planted yaw (0.156 on the planted rotations), the
    direction of t within 2.061 degrees of the planted one (seed 3, n 300).  The bounds are tests/test_pose_cpu.py's sanity bounds on
    the convention, 1 and 10 degrees."""
    model, (info, cands, pose, flags, X) = planted("plane", seed, n)
    i = info[0]
    assert i["kind"] == capi.HPOSE_PLANE and i["ambiguous"] == 0 and i["resolved"] == 0 and pose["best"][0] == i["best"] >= 0
    assert i["front"] == i["n_support"] == model["n_inliers"][0] == pose["n_front"][0] == flags.sum()
    R, t = pose["R"][0].reshape(3, 3), pose["t"][0]
    rot_err, dir_err = angle(R, PLANTED_R), float(np.degrees(np.arccos(np.clip(t @ PLANTED_T, -1, 1))))
    print(f"planted plane seed {seed} n {n}: spread {i['spread']:.4f} fronts {cands['front'].tolist()} twin share {i['front_runner'] / i['front']:.3f} "
          f"rotation error {rot_err:.3f} deg direction error {dir_err:.3f} deg")
    assert rot_err <= 1.0 and dir_err <= 10.0
    assert i["front_runner"] * capi.HPOSE_AMBIGUOUS_DEN < capi.HPOSE_AMBIGUOUS_NUM * i["front"]
    # the plane: Z = 8 + 0.3 X - 0.2 Y has the normal (-0.3, 0.2, 1) normalised, at a distance of 8 / |(-0.3, 0.2, 1)| = 7.53 baselines of 0.5
    nrm = np.array([-0.3, 0.2, 1.0]) / np.linalg.norm([-0.3, 0.2, 1.0])
    assert np.degrees(np.arccos(np.clip(i["n"] @ nrm, -1, 1))) <= 10.0 and abs(i["inv_d"] - 0.5 * np.linalg.norm([-0.3, 0.2, 1.0]) / 8) <= 0.02
    # points: supported records in front lie on the plane, in units of the baseline
    Xf = X[flags] * 0.5
    assert np.abs(Xf[:, 2] - (8 + 0.3 * Xf[:, 0] - 0.2 * Xf[:, 1])).max() <= 1.5
    assert np.isnan(X[~flags]).all()


@pytest.mark.parametrize("seed,n", SCENES)
def test_planted_rotations_get_a_rotation_and_no_pose(seed, n):
    model, (info, cands, pose, flags, X) = planted("rotation", seed, n)
    i = info[0]
    assert i["kind"] == capi.HPOSE_ROTATION and i["best"] == -1 and i["n_support"] == model["n_inliers"][0] and i["front"] == 0
    assert pose["best"][0] == -1 and pose["valid"][0] == 0 and (pose["R"][0] == 0).all() and pose["n_matches"][0] == n
    assert X is None and not flags.any() and cands.tobytes() == bytes(cands.nbytes)
    err = angle(i["R"].reshape(3, 3), PLANTED_R)
    print(f"planted rotation seed {seed} n {n}: spread {i['spread']:.3e} rotation error {err:.3f} deg")
    assert err <= 1.0


def test_the_default_min_spread_separates_the_planted_kinds():
    """Measured: the spread of the 16 planted rotations is 1.509e-3 .. 6.527e-3, of the 16 planted planes 0.1273 .. 0.1384.  The
    default is their geometric mean sqrt(6.527e-3 * 0.1273) = 0.0288, and both ranges lie strictly on their own side of it."""
    rot = [float(planted("rotation", s, n)[1][0]["spread"][0]) for s, n in SCENES]
    pln = [float(planted("plane", s, n)[1][0]["spread"][0]) for s, n in SCENES]
    print(f"spread: rotations {min(rot):.4g} .. {max(rot):.4g}, planes {min(pln):.4g} .. {max(pln):.4g}, geometric mean {np.sqrt(max(rot) * min(pln)):.4g}")
    assert max(rot) < capi.HPOSE_MIN_SPREAD < min(pln)
    assert abs(capi.HPOSE_MIN_SPREAD / np.sqrt(max(rot) * min(pln)) - 1) < 0.005


# ---- the ambiguity rule

def test_a_narrow_view_of_a_plane_is_ambiguous_and_a_prior_resolves_it():
    model, m, qp, tp, R, t, nrm = hposeref.narrow_plane()
    info, cands, pose, flags, X = hposeref.pair(model[0], m, qp, tp, K)
    i = info[0]
    assert i["kind"] == capi.HPOSE_PLANE and i["n_support"] == 60 and cands["front"].tolist() == [0, 60, 60, 0]
    assert i["ambiguous"] == 1 and i["resolved"] == 0 and i["best"] == 1 and i["front"] == i["front_runner"] == 60
    assert pose["best"][0] == -1 and pose["valid"][0] == 1 and (pose["R"][0] == 0).all() and X is None and not flags.any()
    near = lambda k: max(np.abs(cands["R"][k].reshape(3, 3) - R).max(), np.abs(cands["t"][k] - t).max(), np.abs(cands["n"][k] - nrm).max())
    assert near(1) <= 1e-12 and near(2) >= 0.1        # the planted motion and its twin
    prior = np.zeros(1, capi.POSE_DTYPE)
    for want, Rp in ((1, R), (2, cands["R"][2].reshape(3, 3))):
        prior["R"][0], prior["best"] = Rp.ravel(), 0
        info, c2, pose, flags, X = hposeref.pair(model[0], m, qp, tp, K, prior=prior)
        assert info["ambiguous"][0] == 1 and info["resolved"][0] == 1 and info["best"][0] == want == pose["best"][0]
        assert pose["R"][0].tobytes() == cands["R"][want].tobytes() and pose["t"][0].tobytes() == cands["t"][want].tobytes()
        assert info["n"][0].tobytes() == cands["n"][want].tobytes() and flags.all() and np.isfinite(X).all() and pose["n_front"][0] == 60
    # a prior without a pose resolves nothing; an exact tie of the two scores (P = 0) and a NaN score keep the lowest c
    prior["best"] = -1
    assert hposeref.pair(model[0], m, qp, tp, K, prior=prior)[2]["best"][0] == -1
    for P in (0.0, np.nan):
        prior["R"][0], prior["best"] = P, 0
        info, _, pose, _, _ = hposeref.pair(model[0], m, qp, tp, K, prior=prior)
        assert info["resolved"][0] == 1 and pose["best"][0] == 1


def ratio_boundaries(most, runner):
    """(num, den, ambiguous) rows around runner * den == num * most: the products equal, one short, and den near 2^32, where a
    32-bit product would wrap."""
    den = next(d for d in range(1, most + 1) if (runner * d + 1) % most == 0)       # runner * den + 1 == num * most (most, runner coprime)
    rows = [(runner, most, 1), (runner + 1, most, 0), ((runner * den + 1) // most, den, 0), ((runner * den + 1) // most - 1, den, 1)]
    big = 2 ** 32 - 1
    rows += [(runner * big // most, big, 1), (runner * big // most + 1, big, 0), (big, big, int(runner == most)), (0, big, 1), (1, 1, int(runner == most))]
    return rows


def test_the_ambiguity_rule_at_its_boundaries():
    m, qp, tp, _ = homref.planted_scene(1, 300, "plane")
    model = homref.ransac(m, qp, tp, 512, 7, 4.0)[0]
    base = hposeref.pair(model[0], m, qp, tp, K)
    most, runner = int(base[0]["front"][0]), int(base[0]["front_runner"][0])
    assert (most, runner) == (223, 115)
    for num, den, want in ratio_boundaries(most, runner):
        info, cands, pose, flags, X = hposeref.pair(model[0], m, qp, tp, K, num=num, den=den)
        assert info["ambiguous"][0] == want == int(runner * den >= num * most), (num, den)
        assert (pose["best"][0] == -1) == bool(want) and info["best"][0] == base[0]["best"][0]
        assert cands.tobytes() == base[1].tobytes()


# ---- the merge rule and the chain

def test_only_the_selected_pairs_are_written():
    d = hposeref.plane_chain_inputs(1, 300)
    models = d["models"].copy()
    models["degenerate"][1], models["best"][2] = 0, -1             # pair 1: not degenerate; pair 2: no homography at all
    rng = np.random.default_rng(5)
    poses = np.frombuffer(rng.bytes(4 * 112), capi.POSE_DTYPE).copy()
    pts, bits = rng.random((4, 300, 3)), rng.integers(0, 2 ** 63, (4, 5)).astype(np.uint64)
    for only, untouched in ((True, (1, 2)), (False, (2,))):
        p, x, b = poses.copy(), pts.copy(), bits.copy()
        info, cands = hposeref.fill(models, d["matches"], d["counts"], d["query"], d["train"], K, p, x, b, only_degenerate=only)
        for j in range(4):
            if j in untouched:
                assert p[j].tobytes() == poses[j].tobytes() and x[j].tobytes() == pts[j].tobytes() and b[j].tobytes() == bits[j].tobytes()
                assert info[j].tobytes() == bytes(144) and cands[j].tobytes() == bytes(4 * 128)
            else:
                k = int(d["counts"][j])
                assert info["kind"][j] == capi.HPOSE_PLANE and p["best"][j] >= 0 and p["n_matches"][j] == k
                assert x[j, k:].tobytes() == pts[j, k:].tobytes() and b[j, (k + 63) // 64:].tobytes() == bits[j, (k + 63) // 64:].tobytes()
                assert x[j, :k].tobytes() != pts[j, :k].tobytes()


SCALE_BOUND, CENTRE_BOUND = 2 * 0.0530, 2 * 0.1541  # twice the worst measured, see the docstring below


@pytest.mark.parametrize("n", [300, 1000])
@pytest.mark.parametrize("seed", range(1, 9))
def test_the_plane_scene_chains_into_one_segment(seed, n):
    """The feature's claim, in integers.  Five frames of the plane Z = 8 + 0.3 X - 0.2 Y (hposeref.five_plane_frames: the lists as
    vslam_match_dev writes them, built like tests/test_chain_cpu.py's) through epiref.ransac, homref's verdict and gate, poseref on
    the gated models, and chainref: the gate judges all four pairs degenerate, none gets a pose, and every pair is its own invalid
    segment.  With hposeref.fill into the same buffers there is one segment of four linked pairs.  Measured over seeds 1 .. 8 and
    n = 300, 1000: no pair is ambiguous (the prior was never needed), every pair has 167 .. 650 usable links, the worst relative
    error of a scale against the true baseline ratio is 0.0530 (seed 8, n 300), the worst error of a camera centre in units of the
    first baseline 0.1541 (seed 1, n 300) - against 0.1456 and 0.3736 on the general scenes of tests/test_chain_cpu.py.  Each bound
    is twice the worst seed."""
    d = hposeref.plane_chain_inputs(seed, n)
    assert d["models"]["degenerate"].tolist() == [1, 1, 1, 1] and (d["gated"]["best"] == -1).all() and (d["poses"]["best"] == -1).all()
    before = chainref.chain(d["poses"], d["matches"], d["counts"], d["points"], d["bits"], n, 16)[0]
    assert before["valid"].tolist() == [0, 0, 0, 0] and before["segment"].tolist() == [0, 1, 2, 3] and before["linked"].tolist() == [0, 0, 0, 0]
    poses, pts, bits = d["poses"].copy(), d["points"].copy(), d["bits"].copy()
    info, _ = hposeref.fill(d["models"], d["matches"], d["counts"], d["query"], d["train"], K, poses, pts, bits)
    assert (info["kind"] == capi.HPOSE_PLANE).all() and (info["ambiguous"] == 0).all() and (poses["best"] >= 0).all()
    chain = chainref.chain(poses, d["matches"], d["counts"], pts, bits, n, 16)[0]
    assert chain["valid"].tolist() == [1, 1, 1, 1] and chain["segment"].tolist() == [0, 0, 0, 0] and chain["linked"].tolist() == [0, 1, 1, 1]
    assert int(chain["n_links"][0]) == 0 and (chain["n_links"][1:] >= 16).all()
    B, scale_err, centre_err = hposeref.BASELINES, 0.0, 0.0
    for j in range(4):
        true_scale = B[j] / B[0]
        scale_err = max(scale_err, abs(chain["scale"][j] - true_scale) / true_scale)
        for (R, t), C_ in ((d["cams"][j], chain["C"][j]), (d["cams"][j + 1], chain["Ct"][j])):
            centre_err = max(centre_err, np.abs(C_ - (-R.T @ t) / B[0]).max())
    print(f"plane chain seed {seed} n {n}: links {chain['n_links'].tolist()} worst relative scale error {scale_err:.4f} worst centre error {centre_err:.4f}")
    assert scale_err <= SCALE_BOUND and centre_err <= CENTRE_BOUND

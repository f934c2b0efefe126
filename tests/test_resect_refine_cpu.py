"""The refinement of the resected pose without a GPU: the C ABI's new symbols, struct layouts and argument checks, the plan
header under the sanitizers, and the CPU restatement of the arithmetic itself (tests/resectrefineref.py), which the GPU tests
compare against byte for byte: against a finite-difference Jacobian, against the planted pose of exact correspondences, against
scipy's Levenberg-Marquardt, against the planted five-frame scenes, and the rules of the header."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import resectref, resectrefineref as rr
from tests import test_chain_cpu as T
from tests import test_resect_cpu as TR
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
K = T.K
NH, D2 = 512, 4.0
ALL = 1e30  # a max_dist2 under which every row in front of the camera is a member: membership is fixed
ENTRIES = ("vslam_resect_refine_dev", "vslam_resect_refine_host")
KERNELS = (b"k_rr_init", b"k_rr_pass", b"k_rr_step", b"k_rr_flags_zero", b"k_rr_flags")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- the ABI

def test_resect_refine_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ENTRIES:
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in KERNELS:
        assert k in names


def test_resect_refine_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_resect_refine_params": capi.ResectRefineParams, "vslam_resect_refine": capi.ResectRefine,
               "vslam_resect_refine_out": capi.ResectRefineOut, "vslam_resect": capi.Resect}
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
    assert rows["vslam_resect_refine"][0] == 32 == capi.RESECT_REFINE_DTYPE.itemsize and rows["vslam_resect"][0] == 120
    dt = capi.RESECT_REFINE_DTYPE
    assert [dt.fields[f[0]][1] for f in capi.ResectRefine._fields_] == [getattr(capi.ResectRefine, f[0]).offset for f in capi.ResectRefine._fields_]


class Args:
    """A valid vslam_resect_refine_dev / _host call over host arrays (nothing is launched without a GPU: the pointers are never
    followed)."""

    def __init__(self, n_pairs=2, obs_cap=70):
        words = (obs_cap + 63) // 64
        self.keep = [np.zeros(n_pairs + 2, capi.RESECT_DTYPE), np.zeros((n_pairs, obs_cap), capi.RESECT_CORR_DTYPE), np.zeros(n_pairs + 2, capi.RESECT_DTYPE),
                     np.zeros(n_pairs, capi.RESECT_REFINE_DTYPE), np.zeros((n_pairs, words), np.uint64)]
        mi, cs, mo, info, bits = self.keep
        assert cs.ctypes.data % 16 == 0
        self.models_in, self.corr, self.obs_cap, self.n_pairs = mi.ctypes.data, cs.ctypes.data, obs_cap, n_pairs
        self.prm = capi.ResectRefineParams(4, 4.0, capi.PoseParams(*K))
        self.out = capi.ResectRefineOut(C.sizeof(capi.ResectRefineOut), mo.ctypes.data, n_pairs * 120, info.ctypes.data, info.nbytes, bits.ctypes.data,
                                        bits.nbytes)

    def call(self, fn, prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return fn(None, self.models_in, self.corr, self.obs_cap, self.n_pairs, ref(prm), ref(out))


@pytest.mark.parametrize("entry", ENTRIES)
def test_resect_refine_rejects_bad_arguments_before_it_needs_a_gpu(lib, entry):
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
            if obj == "a":
                setattr(a, field, v(a) if callable(v) else v)
            elif obj == "K":
                setattr(a.prm.K, field, v)
            else:
                setattr(getattr(a, obj), field, v(a) if callable(v) else v)
        return a.call(fn)

    for name in ("models_in", "corr"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.ResectRefineOut) - 8) == INVALID
    assert bad(out__models=None) == INVALID and bad(out__models_bytes=2 * 120 - 1) == INVALID
    assert bad(out__info_bytes=2 * 32 - 1) == INVALID
    assert bad(out__inlier_bits_bytes=2 * 2 * 8 - 1) == INVALID
    assert bad(a__obs_cap=0) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for r in (0, 9, 2 ** 32 - 1):
        assert bad(prm__rounds=r) == INVALID, r
    for v in (0.0, -0.0, -4.0, float("nan"), float("inf"), -float("inf")):
        assert bad(prm__max_dist2=v) == INVALID, v
    for f in ("fx", "fy"):
        for v in (0.0, -800.0, float("nan"), float("inf")):
            assert bad(**{"K__" + f: v}) == INVALID, (f, v)
    for f in ("cx", "cy"):
        for v in (float("nan"), float("inf"), -float("inf")):
            assert bad(**{"K__" + f: v}) == INVALID, (f, v)
    # models overlapping models_in without being equal to it, from either side
    assert bad(out__models=lambda a: a.models_in + 120) == INVALID
    assert bad(a__models_in=lambda a: a.out.models + 120) == INVALID
    if entry.endswith("_dev"):
        assert bad(a__corr=lambda a: a.corr + 8) == INVALID       # the device path loads 16 bytes at a time
    if not gpu:  # the optional outputs may be absent, models may be models_in itself, and no pairs and one pair are valid calls
        assert bad(out__info=None, out__inlier_bits=None) == HIP
        assert bad(out__models=lambda a: a.models_in) == HIP
        assert bad(out__models=lambda a: a.models_in + 240) == HIP  # right behind it
        assert bad(a__n_pairs=0) == HIP and bad(a__n_pairs=1) == HIP and bad(K__cx=-5.0, K__cy=0.0) == HIP
        for r in range(1, 9):
            assert bad(prm__rounds=r) == HIP
        if entry.endswith("_host"):
            assert bad(a__corr=lambda a: a.corr + 8) == HIP


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "resect_refine_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 15 * 9, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 60, rows["args"]   # (the order of the checks is among them)
    src = open(os.path.join(CSRC, "vslam_resect_refine_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


def build_cxx_driver(tmp_path):
    """tests/resect_refine_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_resect_refine.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "resect_refine_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "resect_refine_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrapper_takes_no_pairs_and_refuses_sizes_that_do_not_fit(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run([build_cxx_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the restatement against independent answers

def rodrigues(w):
    th = np.linalg.norm(w)
    A = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + A
    return np.eye(3) + np.sin(th) / th * A + (1 - np.cos(th)) / th ** 2 * A @ A


def residuals(xi, R, t, Y, u, v, fx, fy):
    """(rx, ry) stacked per row, in numpy, of the pose (exp(w) R, exp(w) t + tau): the left perturbation Z' = exp(w) Z + tau."""
    Z = (Y @ R.T + t) @ rodrigues(xi[:3]).T + xi[3:]
    return np.stack([(Z[:, 0] / Z[:, 2] - u) * fx, (Z[:, 1] / Z[:, 2] - v) * fy], 1).reshape(-1)


def exact_scene(seed, n=200, noise_px=0.0):
    """resectref.synthetic's pair 1 with the observations replaced by the exact projections under the planted pose (its own are
    rounded to the pixel lattice), plus Gaussian noise of noise_px pixels -> (corr [n], R, t)."""
    d = resectref.synthetic(2, n, seed)
    corr = resectref.run(d, 1, seed, D2)[2][1]
    R, t = d["truth"][1]
    Z = corr["Y"] @ R.T + t
    rng = np.random.default_rng(1000 + seed)
    corr = corr.copy()
    corr["u"] = Z[:, 0] / Z[:, 2] + rng.normal(size=len(Z)) * noise_px / K[0]
    corr["v"] = Z[:, 1] / Z[:, 2] + rng.normal(size=len(Z)) * noise_px / K[1]
    return corr, R, t


def perturbed(R, t, rng, degrees, rel_t):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    d = rng.normal(size=3)
    d /= np.linalg.norm(d)
    return rodrigues(np.radians(degrees) * axis) @ R, t + rel_t * np.linalg.norm(t) * d


def as_model(R, t, corr, best=0):
    m = np.zeros(1, capi.RESECT_DTYPE)
    m["R"][0], m["t"][0], m["n_obs"], m["n_corr"], m["best"], m["n_valid"] = np.asarray(R).reshape(9), t, len(corr), len(corr), best, 1
    return m


FD_WORST_H, FD_WORST_G = 1.13e-11, 1.05e-11  # measured, see the docstring below


def test_h_and_g_of_one_round_agree_with_a_finite_difference_jacobian():
    """H = J^T J and g = J^T r of EVALUATE against a central finite-difference Jacobian (step 1e-6) of numpy residuals under the
    exponential-map perturbation, over the members of 12 scenes (noise 1 px, pose off by 0.3 degrees and 1 %, max_dist2 = 25:
    some rows are not members).  Measured worst |H - H_fd| / max|H| 1.13e-11 and worst |g - g_fd| / max|g| 1.05e-11 - the finite
    difference's own error; each bound is 100 x that.  A wrong sign or a swapped column errs by order 1."""
    worst_h = worst_g = 0.0
    for seed in range(1, 13):
        corr, R, t = exact_scene(seed, 150, 1.0)
        rng = np.random.default_rng(seed)
        R0, t0 = perturbed(R, t, rng, 0.3, 0.01)
        H, g, cost, n = rr.evaluate(R0, t0, K, corr, 25.0)
        _, fl = resectref.score(R0, t0, K, corr, 25.0)
        assert n == int(fl.sum()) and 6 <= n
        Y, u, v = corr["Y"][fl], corr["u"][fl], corr["v"][fl]
        r0 = residuals(np.zeros(6), R0, t0, Y, u, v, K[0], K[1])
        J = np.zeros((len(r0), 6))
        for k in range(6):
            e = np.zeros(6)
            e[k] = 1e-6
            J[:, k] = (residuals(e, R0, t0, Y, u, v, K[0], K[1]) - residuals(-e, R0, t0, Y, u, v, K[0], K[1])) / 2e-6
        Hf, gf = J.T @ J, J.T @ r0
        worst_h, worst_g = max(worst_h, np.abs(H - Hf).max() / np.abs(Hf).max()), max(worst_g, np.abs(g - gf).max() / np.abs(gf).max())
        assert abs(cost - r0 @ r0) <= 1e-12 * cost
    print("H, g against the finite difference: worst rel |H - H_fd|", worst_h, "worst rel |g - g_fd|", worst_g)
    assert worst_h <= 100 * FD_WORST_H and worst_g <= 100 * FD_WORST_G


def test_exact_correspondences_come_back_to_the_planted_pose_within_the_rounds():
    """Exact correspondences, the pose off by 2 degrees and 5 % of |t|, every row a member: the number of rounds until R and t are
    within 1e-9 of the planted pose, per scene (measured: 3 on each of the 12 scenes); that count + 1 must fit the 8 rounds of the ABI."""
    counts = []
    for seed in range(1, 13):
        corr, R, t = exact_scene(seed, 200)
        R0, t0 = perturbed(R, t, np.random.default_rng(seed), 2.0, 0.05)
        out, info, _, trace = rr.refine_pair(as_model(R0, t0, corr), corr, 8, ALL, K)
        err = [max(np.abs(tr[:9].reshape(3, 3) - R).max(), np.abs(tr[9:] - t).max()) for tr in trace[: int(info["accepted"][0]) + 1]]
        first = next((i for i, e in enumerate(err) if e <= 1e-9), None)
        print(f"exact scene {seed}: errors per kept round {['%.1e' % e for e in err]} stop {int(info['stop'][0])}")
        assert first is not None
        counts.append(first)
        assert int(info["n_after"][0]) == int(info["n_before"][0]) == len(corr)
    print("rounds to 1e-9:", counts)
    assert max(counts) + 1 <= 8


LM_WORST_R, LM_WORST_T = 1.69e-8, 2.75e-7  # measured, see the docstring below


def test_eight_rounds_agree_with_scipy_levenberg_marquardt():
    """Noisy correspondences (0.5 px), the pose off by 0.5 degrees and 2 %, every row a member, 8 rounds against
    scipy.optimize.least_squares(method="lm", xtol = ftol = gtol = 1e-15) on the same residuals from the same pose.  A scene whose scipy run does not report convergence is left out (at most 5 %).  Measured over 24 scenes, none left out:
    worst |R - R_lm| entry 1.69e-8, worst |t - t_lm| entry 2.75e-7 (|t| about 1); each bound is 100 x that.  Every scene ends with
    stop 4 after 3 .. 6 kept rounds and a cost equal to scipy's in all nine digits printed (scipy's lm differentiates by forward
    differences, which bounds its own answer near 1e-8)."""
    from scipy.optimize import least_squares

    worst_r = worst_t = 0.0
    left_out = total = 0
    for seed in range(1, 25):
        corr, R, t = exact_scene(seed, 200, 0.5)
        R0, t0 = perturbed(R, t, np.random.default_rng(seed), 0.5, 0.02)
        out, info, _, _ = rr.refine_pair(as_model(R0, t0, corr), corr, 8, ALL, K)
        total += 1
        sol = least_squares(residuals, np.zeros(6), args=(R0, t0, corr["Y"], corr["u"], corr["v"], K[0], K[1]), method="lm", xtol=1e-15, ftol=1e-15,
                            gtol=1e-15)
        if not sol.success or sol.status <= 0:
            left_out += 1
            continue
        Rl, tl = rodrigues(sol.x[:3]) @ R0, rodrigues(sol.x[:3]) @ t0 + sol.x[3:]
        dr, dt = np.abs(out["R"][0].reshape(3, 3) - Rl).max(), np.abs(out["t"][0] - tl).max()
        print(f"lm scene {seed}: |R - R_lm| {dr:.2e} |t - t_lm| {dt:.2e} accepted {int(info['accepted'][0])} stop {int(info['stop'][0])} "
              f"cost {float(info['cost_before'][0]):.3f} -> {float(info['cost_after'][0]):.6f} lm {2 * sol.cost:.6f}")
        worst_r, worst_t = max(worst_r, dr), max(worst_t, dt)
    print("against scipy lm: worst |R - R_lm|", worst_r, "worst |t - t_lm|", worst_t, "left out", left_out, "of", total)
    assert left_out <= 0.05 * total
    assert worst_r <= 100 * LM_WORST_R and worst_t <= 100 * LM_WORST_T


# ---- accuracy on the planted five-frame scenes

@functools.lru_cache(maxsize=None)
def planted_refined(seed, n, rounds=8):
    """The resection of TR.planted(seed, n) by the restatement and its refinement -> (models before, corrs, models after, info)."""
    inputs, cams, _ = TR.planted(seed, n)
    models, _, corrs, _, _ = resectref.run(inputs, NH, seed, D2)
    after, info, _ = rr.refine(models, corrs, rounds, D2, K, n)
    return models, corrs, after, info, cams


# twice the worst measured (the docstring below)
ROT_BOUND, DIR_BOUND, SCALE_BOUND = 2 * 0.4963, 2 * 5.2337, 2 * 0.0333
ORTHO_BOUND = 100 * 1.78e-15  # 100 x the worst |R R^T - I| measured


def test_refinement_improves_the_planted_resections():
    """The 48 planted pairs (seeds 1 .. 8, n = 300, 1000, pairs 1 .. 3; 512 hypotheses, max_dist2 = 4, 8 rounds).  Measured
    before -> after: rotation error median 0.1429 -> 0.1101 degrees, worst 0.7310 -> 0.4963 (better on 36 pairs); direction error of t
    median 1.2411 -> 0.5649 degrees, worst 4.8805 -> 5.2337 (better on 37; the worst is seed 7, n = 300, pair 1 with 69 -> 82
    inliers, and is recorded, not required to fall); | |t| - true | / true median 0.0177 -> 0.0126, worst 0.0736 -> 0.0333 (better on
    34); inliers 13474 -> 16226 in all, no pair loses any; worst |R R^T - I| entry after 8 rounds 1.78e-15.  Each worst error is
    bounded by twice its measured value, the orthogonality by 100 x."""
    before, after = {"rot": [], "dir": [], "scale": []}, {"rot": [], "dir": [], "scale": []}
    ortho = 0.0
    nb = na = 0
    for seed in range(1, 9):
        for n in (300, 1000):
            models, _, ref, info, cams = planted_refined(seed, n)
            assert int(info["stop"][0]) == 5 and ref[0].tobytes() == models[0].tobytes()
            for j in (1, 2, 3):
                assert int(info["n_after"][j]) >= int(info["n_before"][j]) == int(models["n_inliers"][j])
                assert int(ref["n_inliers"][j]) == int(info["n_after"][j])
                nb, na = nb + int(info["n_before"][j]), na + int(info["n_after"][j])
                for store, m in ((before, models[j]), (after, ref[j])):
                    rot, direction, nt, true = TR.errors(m, cams, j, T.BASELINES[j - 1])
                    store["rot"].append(rot), store["dir"].append(direction), store["scale"].append(abs(nt - true) / true)
                Rm = ref["R"][j].reshape(3, 3)
                ortho = max(ortho, np.abs(Rm @ Rm.T - np.eye(3)).max())
                print(f"planted refine seed {seed} n {n} pair {j}: inliers {int(info['n_before'][j])} -> {int(info['n_after'][j])} accepted {int(info['accepted'][j])} "
                      f"stop {int(info['stop'][j])} rot {before['rot'][-1]:.4f} -> {after['rot'][-1]:.4f} dir {before['dir'][-1]:.3f} -> {after['dir'][-1]:.3f} "
                      f"scale {before['scale'][-1]:.4f} -> {after['scale'][-1]:.4f}")
    for k in ("rot", "dir", "scale"):
        print(f"{k}: median {np.median(before[k]):.4f} -> {np.median(after[k]):.4f}  worst {max(before[k]):.4f} -> {max(after[k]):.4f}  "
              f"improved on {sum(a < b for a, b in zip(after[k], before[k]))} of {len(after[k])}")
    print("total inliers", nb, "->", na, " worst |R R^T - I|", ortho)
    for k in ("rot", "dir", "scale"):
        assert np.median(after[k]) < np.median(before[k]), k
    assert max(after["scale"]) < max(before["scale"])
    assert max(after["rot"]) <= ROT_BOUND and max(after["dir"]) <= DIR_BOUND and max(after["scale"]) <= SCALE_BOUND
    assert ortho <= ORTHO_BOUND


# ---- the rules

def test_a_pair_without_a_model_is_copied_through():
    corr, R, t = exact_scene(3, 40, 0.5)
    m = as_model(R, t, corr, best=-1)
    m["n_inliers"], m["reserved"], m["R"][0, 4] = 17, 99, np.nan
    out, info, flags, _ = rr.refine_pair(m, corr, 8, D2, K)
    assert out.tobytes() == m.tobytes() and not flags.any()
    assert info[0].tolist() == (0, 0, 0, 5, 0.0, 0.0)


def test_five_members_stop_at_once_and_six_do_not():
    corr, R, t = exact_scene(4, 40, 0.3)
    R0, t0 = perturbed(R, t, np.random.default_rng(4), 0.05, 0.002)
    _, fl = resectref.score(R0, t0, K, corr, D2)
    inl, outl = np.flatnonzero(fl), corr[:30].copy()
    outl["u"] += 0.5                                                   # 400 px off: never members
    for k, stop in ((5, 1), (6, None), (0, 1)):
        rows = np.concatenate([outl[:7], corr[inl[:k]], outl[7:]])
        rows["b"] = np.arange(len(rows))
        out, info, flags, _ = rr.refine_pair(as_model(R0, t0, rows), rows, 8, D2, K)
        assert int(info["n_before"][0]) == k
        if stop is not None:
            assert int(info["stop"][0]) == stop and int(info["accepted"][0]) == 0 and out["R"].tobytes() == R0.tobytes()
        else:
            assert int(info["stop"][0]) in (0, 4) and int(info["n_after"][0]) >= 6
        assert int(flags.sum()) == int(info["n_after"][0]) == int(out["n_inliers"][0])


def one_point_pair(n=64):
    """n rows whose Y all lie at one point on the optical axis, observed 64 px off, with the identity pose and fx = fy = 1024:
    every Jacobian entry and every sum is a power of two or zero, H has rank 2 exactly, the elimination reaches rows of exact
    zeros and finds no third pivot: stop 3.  (With rounding in the way a rank-deficient H gives tiny pivots instead, and the
    step they make is refused by the acceptance rule: stop 4.)  -> (model [1], corr [n], K)"""
    corr = resectref.as_corr(np.tile([0.0, 0.0, 8.0], (n, 1)), np.full(n, 0.0625), np.full(n, 0.0625))
    return as_model(np.eye(3), np.zeros(3), corr), corr, (1024.0, 1024.0, 0.0, 0.0)


def test_all_points_at_one_place_make_the_step_invalid():
    m, corr, K1 = one_point_pair()
    out, info, flags, _ = rr.refine_pair(m, corr, 8, ALL, K1)
    assert int(info["stop"][0]) == 3 and int(info["n_before"][0]) == int(info["n_after"][0]) == 64 and int(info["accepted"][0]) == 0
    assert out["R"].tobytes() == np.eye(3).tobytes() and flags.all() and float(info["cost_after"][0]) == 64 * 2 * 64.0 ** 2
    H, g, _, _ = rr.evaluate(np.eye(3), np.zeros(3), K1, corr, ALL)
    assert np.linalg.matrix_rank(H) == 2 and rr.step(np.eye(3), np.zeros(3), H, g) is None


def test_a_pose_at_the_optimum_stops_with_4_and_comes_out_bit_identical():
    corr, R, t = exact_scene(5, 120, 0.5)
    R0, t0 = perturbed(R, t, np.random.default_rng(5), 0.3, 0.01)
    first, info1, _, _ = rr.refine_pair(as_model(R0, t0, corr), corr, 8, ALL, K)
    assert int(info1["stop"][0]) == 4 and int(info1["accepted"][0]) >= 2          # it ran until the cost stopped falling
    again, info2, _, _ = rr.refine_pair(first, corr, 8, ALL, K)
    assert int(info2["stop"][0]) == 4 and int(info2["accepted"][0]) == 0
    assert again.tobytes() == first.tobytes()
    assert float(info2["cost_before"][0]) == float(info2["cost_after"][0]) == float(info1["cost_after"][0])


def test_the_ordered_sum_follows_the_header_and_ignores_what_lies_behind_n_corr():
    from tests import refitref

    rng = np.random.default_rng(9)
    for m in (0, 1, 255, 256, 257, 4095, 4096, 4097, 8193):
        t, f = rng.normal(size=m) * 10.0 ** rng.integers(-8, 8, m), rng.random(m) < 0.7
        assert rr.ordered_sum(t, f) == refitref.ordered_sum_py(t, f), m        # the definition as a direct Python loop
    corr, R, t = exact_scene(6, 300, 0.5)
    R0, t0 = perturbed(R, t, np.random.default_rng(6), 0.2, 0.01)
    m = as_model(R0, t0, corr)
    m["n_corr"] = 257
    a = rr.refine_pair(m, corr, 4, D2, K, obs_cap=300)
    junk = corr.copy()
    junk[257:] = resectref.as_corr(rng.normal(size=(43, 3)) * 1e6, rng.normal(size=43), rng.normal(size=43))
    junk["Y"][260] = np.nan
    b = rr.refine_pair(m, junk, 4, D2, K, obs_cap=300)
    c = rr.refine_pair(m, corr[:257], 4, D2, K, obs_cap=257)
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1].tobytes() == b[1].tobytes() == c[1].tobytes()
    assert (a[2] == b[2]).all() and (a[2][:257] == c[2]).all() and not a[2][257:].any()
    H1, g1, c1, n1 = rr.evaluate(R0, t0, K, corr[:257], D2)
    assert n1 == int(a[1]["n_before"][0]) and c1 == float(a[1]["cost_before"][0])

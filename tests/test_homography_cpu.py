"""Homography and the degeneracy verdict without a GPU: the C ABI's new symbols, struct layouts and argument checks, the host
sizing under the sanitizers, and the CPU restatement of the arithmetic itself (tests/homref.py), which the GPU tests compare
against byte for byte: the model against a numpy SVD DLT, the inlier predicate against exact rational arithmetic, the
separation of general from planar and rotation-only scenes, the `building` crops, and the verdict's integer boundaries."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import epiref, homref, matchref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
KINDS = ("general", "plane", "rotation")
SCENES = [(kind, seed, n) for kind in KINDS for n in (300, 1000) for seed in range(1, 9)]
NH, SEED, D2, NUM, DEN, MIN_INLIERS = 512, 1, 4.0, 1, 2, 16  # the issue's settings


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


@pytest.fixture(scope="module")
def scenes():
    """The 48 planted scenes with both RANSAC models and the verdict, computed once."""
    out = {}
    for kind, seed, n in SCENES:
        m, qp, tp, planted = homref.planted_scene(seed, n, kind)
        em, _, _ = epiref.ransac(m, qp, tp, NH, SEED, D2)
        hm, hflags, _ = homref.ransac(m, qp, tp, NH, SEED, D2)
        out[kind, seed, n] = (m, qp, tp, planted, em, homref.verdict(hm, em, NUM, DEN, MIN_INLIERS), hflags)
    return out


def test_homography_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_homography_dev", "vslam_homography_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_hom_models", b"k_hom_score", b"k_hom_select", b"k_hom_flags", b"k_hom_verdict"):
        assert k in names
    assert lib.vslam_version() == 200


def test_homography_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_homography_params": capi.HomographyParams, "vslam_homography_hyp": capi.HomographyHyp, "vslam_homography": capi.Homography,
               "vslam_homography_out": capi.HomographyOut}
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
    assert rows["vslam_homography_hyp"][0] == 152 == capi.HOMOGRAPHY_HYP_DTYPE.itemsize
    assert rows["vslam_homography"][0] == 168 == capi.HOMOGRAPHY_DTYPE.itemsize
    for ct, dt in ((capi.HomographyHyp, capi.HOMOGRAPHY_HYP_DTYPE), (capi.Homography, capi.HOMOGRAPHY_DTYPE)):
        assert [dt.fields[f[0]][1] for f in ct._fields_] == [getattr(ct, f[0]).offset for f in ct._fields_]


class Args:
    """A valid vslam_homography_dev call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, match_cap=100, cap=50, inlier_cap=40, nh=8):
        self.keep = [np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32), np.zeros((n_pairs, cap), capi.POINT_DTYPE),
                     np.zeros(n_pairs, capi.EPIPOLAR_DTYPE), np.zeros(n_pairs, capi.HOMOGRAPHY_DTYPE), np.zeros((n_pairs, (match_cap + 63) // 64), np.uint64),
                     np.zeros((n_pairs, inlier_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32), np.zeros((n_pairs, nh), capi.HOMOGRAPHY_HYP_DTYPE),
                     np.zeros(n_pairs, capi.EPIPOLAR_DTYPE)]
        m, mc, p, epi, models, bits, inl, icnt, hyp, gated = self.keep
        self.matches, self.counts, self.qp, self.tp, self.epi = m.ctypes.data, mc.ctypes.data, p.ctypes.data, p.ctypes.data, epi.ctypes.data
        self.match_cap, self.query_cap, self.train_cap, self.n_pairs = match_cap, cap, cap, n_pairs
        self.prm = capi.HomographyParams(nh, 1, 4.0, 1, 2, 16)
        self.out = capi.HomographyOut(C.sizeof(capi.HomographyOut), models.ctypes.data, models.nbytes, bits.ctypes.data, bits.nbytes, inl.ctypes.data,
                                      inl.nbytes, icnt.ctypes.data, icnt.nbytes, inlier_cap, hyp.ctypes.data, hyp.nbytes, gated.ctypes.data, gated.nbytes)

    def call(self, lib, prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return lib.vslam_homography_dev(None, self.matches, self.counts, self.match_cap, self.qp, self.query_cap, self.tp, self.train_cap, self.n_pairs,
                                        self.epi, ref(prm), ref(out))


def test_homography_dev_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    gpu = torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(lib) == (INVALID if gpu else HIP)
    assert Args().call(lib, prm=None) == INVALID and Args().call(lib, out=None) == INVALID

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
        return a.call(lib)

    for name in ("matches", "counts", "qp", "tp"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.HomographyOut) - 8) == INVALID
    assert bad(out__models=None) == INVALID and bad(out__models_bytes=2 * 168 - 1) == INVALID
    assert bad(out__inlier_bits_bytes=2 * 2 * 8 - 1) == INVALID
    assert bad(out__inliers_bytes=2 * 40 * 12 - 1) == INVALID
    assert bad(out__inlier_counts_bytes=2 * 4 - 1) == INVALID
    assert bad(out__hypotheses_bytes=2 * 8 * 152 - 1) == INVALID
    assert bad(out__gated_models_bytes=2 * 88 - 1) == INVALID
    assert bad(a__epi=None) == INVALID                                                       # the gate without epipolar models
    assert bad(out__inlier_counts=None) == INVALID and bad(out__inlier_cap=0) == INVALID      # inliers without its totals / its capacity
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for nh in (0, 65536, 2 ** 32 - 1):
        assert bad(prm__n_hypotheses=nh) == INVALID, nh
    for v in (0.0, -0.0, -4.0, float("nan"), float("inf"), -float("inf")):
        assert bad(prm__max_dist2=v) == INVALID, v
    assert bad(prm__degenerate_den=0) == INVALID
    assert bad(a__match_cap=0) == INVALID and bad(a__query_cap=0) == INVALID and bad(a__train_cap=0) == INVALID
    if not gpu:  # the optional outputs may be absent, the gate may be written in place, and no pairs is a valid call
        assert bad(out__inlier_bits=None, out__inliers=None, out__inlier_counts=None, out__inlier_cap=0, out__hypotheses=None, out__gated_models=None) == HIP
        assert bad(out__gated_models=None, a__epi=None) == HIP and bad(a__n_pairs=0) == HIP
        assert bad(prm__degenerate_num=0, prm__degenerate_den=2 ** 32 - 1, prm__min_inliers=2 ** 32 - 1) == HIP
        a = Args()
        a.out.gated_models = a.epi
        assert a.call(lib) == HIP


def test_homography_host_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    m, qp, tp, _ = epiref.planted_scene(1, n=20)
    model, epi, gated = np.zeros(1, capi.HOMOGRAPHY_DTYPE), np.zeros(1, capi.EPIPOLAR_DTYPE), np.zeros(1, capi.EPIPOLAR_DTYPE)
    good = capi.HomographyParams(8, 1, 4.0, 1, 2, 16)
    inl = np.zeros(20, capi.MATCH_DTYPE)
    total = C.c_size_t()

    def call(prm=good, mp=m.ctypes.data, q=qp.ctypes.data, nq=20, ep=None, outp=model.ctypes.data, inliers=None, cap=0, tot=None, gp=None):
        return lib.vslam_homography_host(None, mp, 20, q, nq, tp.ctypes.data, 20, ep, None if prm is None else C.byref(prm), outp, None, inliers, cap, tot,
                                         None, gp)

    assert call() == (INVALID if torch.cuda.is_available() else HIP)
    assert call(prm=None) == INVALID and call(outp=None) == INVALID and call(mp=None) == INVALID and call(q=None) == INVALID
    for bad in ((0, 1, 4.0, 1, 2, 16), (65536, 1, 4.0, 1, 2, 16), (8, 1, 0.0, 1, 2, 16), (8, 1, -1.0, 1, 2, 16), (8, 1, float("nan"), 1, 2, 16),
                (8, 1, float("inf"), 1, 2, 16), (8, 1, 4.0, 1, 0, 16)):
        assert call(prm=capi.HomographyParams(*bad)) == INVALID, bad
    assert call(q=None, nq=0) == INVALID                                      # match records without points
    assert call(inliers=inl.ctypes.data, cap=20) == INVALID                    # inliers without n_inliers
    assert call(inliers=inl.ctypes.data, cap=0, tot=C.byref(total)) == INVALID  # ... without a capacity
    assert call(gp=gated.ctypes.data) == INVALID                               # the gate without an epipolar model
    if not torch.cuda.is_available():
        assert call(ep=epi.ctypes.data, gp=gated.ctypes.data, inliers=inl.ctypes.data, cap=20, tot=C.byref(total)) == HIP


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "homography_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 15 * 10 * 11, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 62, rows["args"]   # (the order of the checks is among them)
    src = open(os.path.join(CSRC, "vslam_homography_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


# ---- the restatement itself

def svd_dlt(p):
    """numpy's answer for the same four records: Hartley normalisation, the 8 x 9 system's null vector by SVD, denormalised,
    Frobenius norm 1 (the sign is free)."""
    def T(pts):
        c = pts.mean(0)
        s = np.sqrt(2) / np.sqrt(((pts - c) ** 2).sum(1)).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1]])

    Tq, Tt = T(p[:, :2]), T(p[:, 2:])
    q, t = (Tq @ np.c_[p[:, :2], np.ones(4)].T).T, (Tt @ np.c_[p[:, 2:], np.ones(4)].T).T
    A = []
    for (x, y, _), (u, v, _) in zip(q, t):
        A += [[x, y, 1, 0, 0, 0, -u * x, -u * y, -u], [0, 0, 0, x, y, 1, -v * x, -v * y, -v]]
    H = np.linalg.inv(Tt) @ np.linalg.svd(np.array(A))[2][-1].reshape(3, 3) @ Tq
    return H / np.linalg.norm(H)


def test_sample4_follows_the_counter_hash():
    for seed, j, h, m in ((1, 0, 0, 4), (7, 3, 511, 300), (0xFFFFFFFF, 65534, 65534, 5), (9, 1, 2, 1000)):
        base = epiref.mix(epiref.mix((seed + j) & 0xFFFFFFFF) + h)
        want = []
        for t in range(64):
            i = (epiref.mix(base + t) * m) >> 32
            if i not in want:
                want.append(i)
        assert homref.sample4(seed, j, h, m) == (want[:4] if len(want) >= 4 else None)
        assert len(set(homref.sample4(seed, j, h, m))) == 4
    assert all(homref.sample4(1, 0, h, 3) is None for h in range(16))                 # m < 4
    assert all(sorted(homref.sample4(1, 0, h, 4)) == [0, 1, 2, 3] for h in range(64) if homref.sample4(1, 0, h, 4))


def test_model_from_4_agrees_with_a_numpy_svd_dlt():
    """Worst |H - H_svd| entry over 3072 samples (64 per scene): 1.22e-10 with this restatement (ill-conditioned 4-point
    samples included); the bound is 100 x that.  A transposed product errs by order 1."""
    worst, n_models, worst_g = 0.0, 0, 0.0
    for kind, seed, n in SCENES:
        m, qp, tp, _ = homref.planted_scene(seed, n, kind)
        xy = epiref.coords(m, qp, tp)
        for h in range(64):
            r = homref.model_from_4(xy[homref.sample4(SEED, 0, h, n)])
            if r is None:
                continue
            H, G = r
            S = svd_dlt(xy[homref.sample4(SEED, 0, h, n)])
            worst = max(worst, min(np.abs(H - S).max(), np.abs(H + S).max()))
            assert abs(np.linalg.norm(H) - 1) < 1e-15 * 8
            # G is the way back, up to scale, with the sign that keeps the sample's first record in front
            Gi = np.linalg.inv(H)
            Gi, Gn = Gi / np.linalg.norm(Gi), G / np.linalg.norm(G)
            worst_g = max(worst_g, min(np.abs(Gn - Gi).max(), np.abs(Gn + Gi).max()))
            x0 = xy[homref.sample4(SEED, 0, h, n)[0]]
            assert H[2] @ [x0[0], x0[1], 1] > 0 and G[2] @ [x0[2], x0[3], 1] > 0
            n_models += 1
    print("model_from_4 against the SVD DLT: worst entry difference", worst, "over", n_models, "models; G against inv(H):", worst_g)
    assert n_models > 3000
    assert worst <= 100 * 1.22e-10
    assert worst_g <= 100 * 8.3e-13     # measured 8.27e-13, the same 100 x


def test_model_from_4_refuses_what_the_header_calls_invalid():
    sq = np.array([[0, 0, 10, 10], [100, 0, 110, 10], [100, 100, 110, 110], [0, 100, 10, 110]], np.float64)
    H, G = homref.model_from_4(sq)
    assert np.abs(H / H[2, 2] - [[1, 0, 10], [0, 1, 10], [0, 0, 1]]).max() < 1e-12
    assert homref.model_from_4(np.tile(sq[0], (4, 1))) is None                       # d == 0 on both sides
    one = sq.copy()
    one[:, 2:] = 5.0
    assert homref.model_from_4(one) is None                                          # d == 0 on the train side
    nan = sq.copy()
    nan[2, 1] = np.nan
    assert homref.model_from_4(nan) is None                                          # a record that is not trusted
    col = sq.copy()
    col[:, 0], col[:, 1] = [0, 50, 100, 150], [0, 50, 100, 150]                      # four collinear query points: rank < 8
    assert homref.model_from_4(col) is None


def test_the_rounded_inlier_test_equals_the_exact_predicate_outside_a_near_band(scenes):
    checked = near_seen = 0
    for key in (("general", 1, 300), ("plane", 2, 300), ("rotation", 3, 300)):
        m, qp, tp, _, _, hm, _ = scenes[key]
        xy = epiref.coords(m, qp, tp)
        _, _, hyps = homref.ransac(m, qp, tp, 24, SEED, D2)
        models = [(hm["H"][0], hm["G"][0])] + [(h["H"], h["G"]) for h in hyps if h["valid"]][:5]
        for H, G in models:
            for d2 in (D2, 0.25):
                _, flags = homref.score(H, G, xy, d2)
                inl, near, trusted = homref.exact_inlier(H, G, xy, d2)
                assert trusted.all()
                assert (flags == inl)[~near].all()
                checked += int((~near).sum())
                near_seen += int(near.sum())
    print("exact predicate: records checked", checked, "inside the near band", near_seen)
    assert checked > 3000 and near_seen < 0.01 * checked
    # records that are not trusted are never inliers; the horizon (p2 <= 0) is never an inlier
    H = np.array([[1, 0, 0], [0, 1, 0], [0.01, 0, -1.0]])       # p2 = 0.01 x - 1: the horizon is x = 100
    G = H.copy()                                                # this H is its own inverse: adj(H) = -H, negated by the sign rule

    def rec(x, y):
        p2 = 0.01 * x - 1
        return [x, y, x / p2, y / p2] if p2 else [x, y, 0.0, 0.0]
    xy = np.array([rec(200, 50), rec(50, 50), rec(100, 50), [np.nan] * 4])
    n, flags = homref.score(H, G, xy, D2)
    assert flags.tolist() == [True, False, False, False] and n == 1


def test_general_scenes_are_kept_and_planar_and_rotation_scenes_are_degenerate(scenes):
    """n_H / n_F with this restatement: general 0.0776 .. 0.159, plane 0.945 .. 0.976, rotation 0.937 .. 0.981 - 1/2 lies
    strictly between.  Planted matches that are H-inliers on the degenerate scenes: at least 95.0 %."""
    ratio = {k: [] for k in KINDS}
    planted_found = []
    for (kind, seed, n), (m, qp, tp, planted, em, hm, hflags) in scenes.items():
        nf, nh = int(em["n_inliers"][0]), int(hm["n_inliers"][0])
        assert int(em["best"][0]) >= 0 and int(hm["best"][0]) >= 0 and int(hm["n_epipolar"][0]) == nf
        ratio[kind].append(nh / nf)
        assert int(hm["degenerate"][0]) == (0 if kind == "general" else 1), (kind, seed, n, nh, nf)
        if kind != "general":
            planted_found.append(hflags[planted].sum() / planted.sum())
            assert planted_found[-1] >= 0.90, (kind, seed, n, planted_found[-1])
    for kind in KINDS:
        print(kind, "n_H / n_F: min", min(ratio[kind]), "max", max(ratio[kind]))
    print("planted matches found by H on the degenerate scenes: min", min(planted_found))
    assert max(ratio["general"]) < NUM / DEN < min(min(ratio["plane"]), min(ratio["rotation"]))


def test_building_crops_are_a_translation_and_degenerate():
    """Measured with this restatement: H has 715 inliers (the 710 exact translations and 5 near ones) against F's 719; the
    worst entry of H / H[2][2] against the translation by (-24, -24) is off by 6.04e-14; the bound is 100 x that."""
    from tests.test_gpu_match import building_crops, oracle_chain

    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    _, wm = matchref.match(qd, td, 0.64, False, qk, tk)
    q, t = qp[wm["query"]], tp[wm["train"]]
    s = 48 >> q["octave"]
    exact = ((q["octave"] == t["octave"]) & (q["level"] == t["level"]) & (q["value"] == t["value"]) & (q["row"] - t["row"] == s) & (q["col"] - t["col"] == s))
    assert (len(wm), int(exact.sum())) == (730, 710)
    em, _, _ = epiref.ransac(wm, qp, tp, NH, SEED, D2)
    hm, hflags, _ = homref.ransac(wm, qp, tp, NH, SEED, D2)
    v = homref.verdict(hm, em, NUM, DEN, MIN_INLIERS)
    Hn = hm["H"][0].reshape(3, 3) / hm["H"][0][8]
    err = np.abs(Hn - [[1, 0, -24], [0, 1, -24], [0, 0, 1]]).max()
    print("building crops: H inliers", int(hflags.sum()), "F inliers", int(em["n_inliers"][0]), "n_valid", int(hm["n_valid"][0]), "worst entry error", err)
    assert hflags[exact].all()
    assert int(v["degenerate"][0]) == 1 and int(v["n_epipolar"][0]) == int(em["n_inliers"][0])
    assert err <= 100 * 6.04e-14
    g = homref.gate(em, v)
    assert int(g["best"][0]) == -1 and int(g["n_inliers"][0]) == 0 and not g["F"].any()
    assert (int(g["n_matches"][0]), int(g["n_valid"][0])) == (int(em["n_matches"][0]), int(em["n_valid"][0]))


def records(rows):
    """HOMOGRAPHY_DTYPE / EPIPOLAR_DTYPE records from (n_inliers, best) rows."""
    hm, em = np.zeros(len(rows), capi.HOMOGRAPHY_DTYPE), np.zeros(len(rows), capi.EPIPOLAR_DTYPE)
    for j, (nh, hb, ne, eb) in enumerate(rows):
        hm["n_inliers"][j], hm["best"][j], hm["n_matches"][j], hm["n_valid"][j] = nh, hb, 1000 + j, 7
        em["n_inliers"][j], em["best"][j], em["n_matches"][j], em["n_valid"][j], em["F"][j] = ne, eb, 1000 + j, 9 + j, np.arange(9) + 1.0 + j
    return hm, em


VERDICT_CASES = [  # (n_H, H best, n_F, F best), num, den, min_inliers -> degenerate
    ((50, 0, 100, 3), 1, 2, 16, 1),                          # the product equal: 50 * 2 == 1 * 100
    ((49, 0, 100, 3), 1, 2, 16, 0),                          # ... and one short
    ((16, 0, 20, 3), 1, 2, 16, 1),                           # min_inliers equal
    ((16, 0, 20, 3), 1, 2, 17, 0),                           # ... and one above
    ((50, -1, 100, 3), 1, 2, 16, 0),                         # no homography
    ((50, 0, 100, -1), 1, 2, 16, 0),                         # no epipolar model: n_epipolar counts as 0, never degenerate
    ((3, 0, 4294967295, 0), 4294967295, 4294967295, 0, 0),   # den near 2^32: 3 * den < num * n_F only in 64 bits
    ((4294967295, 0, 4294967295, 0), 4294967295, 4294967295, 0, 1),
    ((4294967294, 0, 4294967295, 0), 4294967295, 4294967295, 0, 0),
    ((1, 0, 4294967295, 0), 1, 4294967295, 0, 1),            # 1 * (2^32 - 1) >= 1 * (2^32 - 1): a 32-bit product would wrap elsewhere
    ((2, 0, 3, 0), 2147483648, 2147483649, 0, 0),            # 2 * (2^31 + 1) = 2^32 + 2 < 3 * 2^31; mod 2^32 it would pass
    ((0, 0, 0, 0), 0, 1, 0, 1),                              # 0 >= 0
]


def test_verdict_boundaries_and_the_gates_record_layout():
    for row, num, den, mi, want in VERDICT_CASES:
        hm, em = records([row])
        v = homref.verdict(hm, em, num, den, mi)
        assert int(v["degenerate"][0]) == want, (row, num, den, mi)
        assert int(v["n_epipolar"][0]) == (row[2] if row[3] >= 0 else 0)
        g = homref.gate(em, v)
        if want:
            assert int(g["best"][0]) == -1 and int(g["n_inliers"][0]) == 0 and not g["F"].any()
            assert (int(g["n_matches"][0]), int(g["n_valid"][0])) == (1000, 9)
        else:
            assert g.tobytes() == em.tobytes()
    hm, em = records([(50, 0, 100, 3)])
    v = homref.verdict(hm, None)
    assert int(v["degenerate"][0]) == 0 and int(v["n_epipolar"][0]) == 0      # without epipolar models: no verdict
    # the no-model record is exactly what vslam_epipolar_dev writes for a pair without a winner, with the pair's own counts
    none = epiref.ransac(np.zeros(3, capi.MATCH_DTYPE), np.zeros(1, capi.POINT_DTYPE), np.zeros(1, capi.POINT_DTYPE), 4, 1, 4.0)[0]
    hm, em = records([(50, 0, 100, 3)])
    em["n_matches"], em["n_valid"] = 3, 0
    assert homref.gate(em, homref.verdict(hm, em)).tobytes() == none.tobytes()

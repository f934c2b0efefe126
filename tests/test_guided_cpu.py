"""Guided matching without a GPU: the C ABI's new symbols, struct layout and argument checks, the host sizing under the
sanitizers, the C++ wrapper's own checks, and the CPU restatement of the rule (tests/guidedref.py), which the GPU tests compare
against byte for byte: the rule on hand-made sets whose answer is known by construction, the two identities that tie it to the
matcher's and the two-view restatements, and the planted scenes with repeated structure that show what the pass is for."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import epiref, guidedref, matchref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- ABI

def test_guided_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_match_guided_dev", "vslam_match_guided_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_guided_rows", b"k_match_guided", b"k_match_guided_merge"):
        assert k in names


def test_guided_params_layout_matches_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    ct = capi.GuidedParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {", '  printf("%zu", sizeof(vslam_guided_params));']
    lines += [f'  printf(" %zu", offsetof(vslam_guided_params, {f[0]}));' for f in ct._fields_]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    row = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert row == [C.sizeof(ct)] + [getattr(ct, f[0]).offset for f in ct._fields_]
    assert row[0] == 24 and capi.GUIDED_PARAMS_DTYPE.itemsize == 24
    assert [capi.GUIDED_PARAMS_DTYPE.fields[f[0]][1] for f in ct._fields_] == row[1:]


class Args:
    """A valid vslam_match_guided_dev call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, qcap=50, tcap=60, match_cap=10):
        self.keep = [np.zeros((n_pairs, max(qcap, tcap), 128), np.float32), np.zeros(n_pairs, np.uint32), np.zeros((n_pairs, max(qcap, tcap)), capi.POINT_DTYPE),
                     np.zeros(n_pairs, capi.EPIPOLAR_DTYPE), np.zeros((n_pairs, qcap), capi.NN2_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE),
                     np.zeros(n_pairs, np.uint32)]
        d, cnt, pts, mod, nn, m, mc = self.keep
        assert d.ctypes.data % 16 == 0
        self.Q = capi.DescSets(d.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, qcap)
        self.T = capi.DescSets(d.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, tcap)
        self.models, self.n_pairs = mod.ctypes.data, n_pairs
        self.prm = capi.GuidedParams(0.64, 1.0, 4.0, 0, 0)
        self.out = capi.MatchOut(C.sizeof(capi.MatchOut), nn.ctypes.data, nn.nbytes, m.ctypes.data, m.nbytes, mc.ctypes.data, mc.nbytes, match_cap)

    def call(self, lib, Q="Q", T="T", prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return lib.vslam_match_guided_dev(None, ref(Q), ref(T), self.models, self.n_pairs, ref(prm), ref(out))


def test_guided_dev_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    gpu = torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(lib) == (INVALID if gpu else HIP)
    for name in ("Q", "T", "prm", "out"):
        assert Args().call(lib, **{name: None}) == INVALID, name

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
        return a.call(lib)

    assert bad(a__models=None) == INVALID
    # everything vslam_match_dev rejects
    assert bad(out__struct_size=C.sizeof(capi.MatchOut) - 8) == INVALID
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for s in ("Q", "T"):
        assert bad(**{s + "__desc": None}) == INVALID and bad(**{s + "__counts": None}) == INVALID and bad(**{s + "__cap": 0}) == INVALID
        assert bad(**{s + "__desc": Args().keep[0].ctypes.data + 4}) == INVALID  # misaligned
        assert bad(**{s + "__points": None}) == INVALID                           # points are required on both sides, whatever same_octave
    assert bad(out__nn=None, out__matches=None, out__match_counts=None) == INVALID
    assert bad(out__nn_bytes=2 * 50 * 12 - 1) == INVALID
    assert bad(out__match_counts=None) == INVALID and bad(out__match_cap=0) == INVALID
    assert bad(out__matches_bytes=2 * 10 * 12 - 1) == INVALID and bad(out__match_counts_bytes=7) == INVALID
    # the parameters
    assert bad(prm__reserved=1) == INVALID
    for r in (0.0, -0.64, float("nan"), float("inf")):
        assert bad(prm__ratio2=r) == INVALID
    for d in (0.0, -4.0, float("nan"), float("inf")):
        assert bad(prm__max_dist2=d) == INVALID
    for b in (0.0, -1.0, float("nan"), float("-inf")):
        assert bad(prm__max_desc_dist2=b) == INVALID
    if not gpu:  # +inf is a valid bound, the optional outputs may be absent, no pairs is a valid call
        assert bad(prm__max_desc_dist2=float("inf")) == HIP and bad(prm__same_octave=1) == HIP
        assert bad(out__nn=None) == HIP and bad(out__matches=None, out__match_cap=0) == HIP and bad(a__n_pairs=0) == HIP


def test_guided_host_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    q, t = np.zeros((5, 128), np.float32), np.zeros((6, 128), np.float32)
    qp, tp = np.zeros(5, capi.POINT_DTYPE), np.zeros(6, capi.POINT_DTYPE)
    model, nn, m, total = np.zeros(1, capi.EPIPOLAR_DTYPE), np.zeros(5, capi.NN2_DTYPE), np.zeros(5, capi.MATCH_DTYPE), C.c_size_t()
    good = capi.GuidedParams(0.64, float("inf"), 4.0, 0, 0)

    def call(prm=good, qd=q.ctypes.data, qpp=qp.ctypes.data, tpp=tp.ctypes.data, mod=model.ctypes.data, nnp=nn.ctypes.data, mp=m.ctypes.data, cap=5,
             tot=C.byref(total)):
        return lib.vslam_match_guided_host(None, qd, None, qpp, 5, t.ctypes.data, None, tpp, 6, mod, None if prm is None else C.byref(prm), nnp, mp, cap, tot)

    assert call() == (INVALID if torch.cuda.is_available() else HIP)
    assert call(prm=None) == INVALID and call(mod=None) == INVALID and call(qd=None) == INVALID
    assert call(qpp=None) == INVALID and call(tpp=None) == INVALID
    assert call(prm=capi.GuidedParams(0.64, 1.0, 4.0, 0, 3)) == INVALID
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(prm=capi.GuidedParams(r, 1.0, 4.0, 0, 0)) == INVALID and call(prm=capi.GuidedParams(0.64, 1.0, r, 0, 0)) == INVALID
    for b in (0.0, -1.0, float("nan")):
        assert call(prm=capi.GuidedParams(0.64, b, 4.0, 0, 0)) == INVALID
    assert call(nnp=None, tot=None, mp=None) == INVALID and call(tot=None) == INVALID and call(cap=0) == INVALID
    if not torch.cuda.is_available():
        assert call(mp=None, tot=None) == HIP and call(nnp=None) == HIP


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "guided_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 21 * 13 * 10, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 60, rows["args"]   # (the order of the checks is among them)
    src = open(os.path.join(CSRC, "vslam_guided_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


def build_cxx_driver(tmp_path):
    """tests/guided_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_guided.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "guided_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "guided_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrapper_refuses_lists_that_do_not_fit(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run([build_cxx_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the rule on hand-made sets
#
# The exact-F fixture: F = [[0, 0, 0], [0, 0, -1], [0, 1, 0]] gives a = (0, -1, y), b0 = 0, b1 = 1, e = y - y' and the bound
# max_dist2 * 2, all exact: a train row is in band iff (y - y')^2 < 2 * max_dist2.  With max_dist2 = 2 that is |y - y'| < 2: a row
# offset of exactly 2 pixels is out, 1.5 pixels (an octave-0 point, pitch 1/2) is in.  Descriptors have two non-zero entries of
# small integer value, so that every d2 is an exact small integer: the square of the distance of the two (v, w) pairs.

EXACT_F = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0)
BAND2 = 2.0


def lattice_points(y, octave=1, x=None, padding=0):
    """POINT_DTYPE records at pixel (x, y) (x defaults to 7 * index), each at its octave's pitch 2^(octave - 1); the coordinates
    must lie on that lattice.  An octave outside 0 .. 31 is stored as given (pitch 1 is used for its row and col)."""
    y = np.asarray(y, np.float64)
    n = len(y)
    octave = np.broadcast_to(np.asarray(octave, np.int64), (n,))
    x = 7.0 * np.arange(n) if x is None else np.asarray(x, np.float64)
    pitch = np.where((octave >= 0) & (octave <= 31), 2.0 ** (np.clip(octave, 0, 31) - 1), 1.0)
    row, col = y / pitch, x / pitch
    assert (row == np.rint(row)).all() and (col == np.rint(col)).all()
    p = np.zeros(n, capi.POINT_DTYPE)
    p["row"], p["col"], p["padding"], p["octave"], p["level"] = row.astype(np.int32) + padding, col.astype(np.int32) + padding, padding, octave, 1
    return p


def vw_rows(vw):
    """f32 [n, 128] rows that are zero but for entries 0 and 1 = (v, w)."""
    vw = np.asarray(vw, np.float32).reshape(-1, 2)
    d = np.zeros((len(vw), 128), np.float32)
    d[:, :2] = vw
    return d


def hand_case(q, qy, t, ty, qoct=1, toct=1, qdef=None, tdef=None, F=EXACT_F, best=0, **prm):
    """-> the keyword arguments of guidedref.guided for one hand-made pair (prm: ratio2, max_desc_dist2, max_dist2, same_octave)."""
    prm.setdefault("max_dist2", BAND2)
    return dict(q=vw_rows(q), t=vw_rows(t), q_points=lattice_points(qy, qoct), t_points=lattice_points(ty, toct), model=guidedref.model_record(F, best),
                q_defined=qdef, t_defined=tdef, **prm)


NONE = (-1, INF, INF)
Q10 = [(10, 0)]
NAN_F = EXACT_F[:4] + (np.nan,) + EXACT_F[5:]
INF_F = EXACT_F[:5] + (-np.inf,) + EXACT_F[6:]
# name -> (case, the nn rows that must come out, the accepted query rows)
HAND = {
    # the global nearest (row 0, d2 0) is 10 pixels off the line: the winner is the nearest in the band
    "nearest out of band": (hand_case(Q10, [10], [(10, 0), (12, 0), (20, 0)], [20, 10, 11]), [(1, 4.0, 100.0)], [0]),
    # 4 < 0.64 * 5 is false, 4 < 0.64 * 400 is true: the global second nearest (row 1, d2 5) is out of band
    "second out of band": (hand_case(Q10, [10], [(12, 0), (11, 2), (30, 0)], [10, 40, 11]), [(0, 4.0, 400.0)], [0]),
    "lone candidate": (hand_case(Q10, [10], [(40, 0), (10, 0)], [10, 50]), [(0, 900.0, INF)], [0]),
    "lone candidate, bound": (hand_case(Q10, [10], [(40, 0), (10, 0)], [10, 50], max_desc_dist2=1.0), [(0, 900.0, INF)], []),
    "empty band": (hand_case(Q10, [10], [(10, 0), (11, 0)], [50, 8]), [NONE], []),
    "no train rows": (hand_case(Q10, [10], np.zeros((0, 2)), []), [NONE], []),
    "bound at equality": (hand_case(Q10, [10], [(12, 0), (30, 0)], [10, 10], max_desc_dist2=4.0), [(0, 4.0, 400.0)], []),
    "bound just above": (hand_case(Q10, [10], [(12, 0), (30, 0)], [10, 10], max_desc_dist2=float(np.nextafter(np.float32(4.0), INF))), [(0, 4.0, 400.0)], [0]),
    # three equal rows, the first out of band: the lowest index IN the band, and second == best is rejected by the ratio
    "tie": (hand_case(Q10, [10], [(12, 0), (12, 0), (12, 0), (13, 0)], [30, 11, 9, 10]), [(1, 4.0, 4.0)], []),
    "best < 0": (hand_case(Q10, [10], [(10, 0), (12, 0)], [10, 10], best=-1), [NONE], []),
    "NaN in F": (hand_case(Q10, [10], [(10, 0), (12, 0)], [10, 10], F=NAN_F), [NONE], []),
    "inf in F": (hand_case(Q10, [10], [(10, 0), (12, 0)], [10, 10], F=INF_F), [NONE], []),
    "zero F": (hand_case(Q10, [10], [(10, 0), (12, 0)], [10, 10], F=(0.0,) * 9), [NONE], []),
    # rows that are not trusted: a query gets nothing, a train row is skipped even where it is the exact copy
    "octaves 32 and -1": (hand_case([(10, 0)] * 3, [10, 10, 10], [(10, 0), (10, 0), (12, 0)], [10, 10, 10], qoct=[1, 32, -1], toct=[32, -1, 1]),
                          [(2, 4.0, INF), NONE, NONE], [0]),
    "defined = 0": (hand_case([(10, 0)] * 2, [10, 10], [(10, 0), (12, 0), (30, 0)], [10, 10, 10], qdef=[1, 0], tdef=[0, 1, 1]), [(1, 4.0, 400.0), NONE], [0]),
    "same_octave off": (hand_case(Q10, [10], [(10, 0), (12, 0)], [10, 10], toct=[2, 1]), [(0, 0.0, 4.0)], [0]),
    "same_octave on": (hand_case(Q10, [10], [(10, 0), (12, 0)], [10, 10], toct=[2, 1], same_octave=True), [(1, 4.0, INF)], [0]),
    # exactly 2 pixels off is out ((y - y')^2 = 4 is not below 4), 1.5 pixels - an octave-0 point - is in
    "boundary": (hand_case(Q10, [10], [(10, 0), (10, 0), (12, 0), (13, 0)], [12, 8, 11.5, 8.5], toct=[1, 1, 0, 0]), [(2, 4.0, 9.0)], [0]),
}


def nn_rows(rows):
    a = np.zeros(len(rows), capi.NN2_DTYPE)
    for i, r in enumerate(rows):
        a[i] = r
    return a


@pytest.mark.parametrize("name", list(HAND))
def test_rule_on_hand_made_sets(name):
    case, want_nn, want_acc = HAND[name]
    nn, m = guidedref.guided(**case)
    assert nn.tobytes() == nn_rows(want_nn).tobytes(), (name, nn)
    assert list(m["query"]) == want_acc and (m["train"] == nn["index"][m["query"]]).all() and (m["dist2"] == nn["dist2"][m["query"]]).all()


def test_hand_made_sets_differ_from_the_unguided_matcher_where_they_should():
    """The same sets through the matcher's restatement: its winner is the out-of-band row, its ratio test rejects what the band accepts."""
    c = HAND["nearest out of band"][0]
    assert matchref.match(c["q"], c["t"])[0]["index"][0] == 0
    c = HAND["second out of band"][0]
    nn, m = matchref.match(c["q"], c["t"])
    assert nn["index"][0] == 0 and nn["second_dist2"][0] == 5.0 and len(m) == 0
    band = guidedref.band(HAND["boundary"][0]["model"], HAND["boundary"][0]["q_points"], HAND["boundary"][0]["t_points"], BAND2)
    assert band.tolist() == [[False, False, True, True]]


# ---- two identities

@functools.lru_cache(maxsize=None)
def identity_sets():
    """The crafted 1000 x 777 sets of tests/test_match_epipolar_exact_cpu.py with arbitrary trusted points and a valid F."""
    from tests.test_match_epipolar_exact_cpu import exact_sets

    q, t = exact_sets(False)[:2]
    rng = np.random.default_rng(1777)
    pts = []
    for n in (len(q), len(t)):
        octave = rng.integers(0, 4, n)
        pitch = 2.0 ** (octave - 1)
        pts.append(lattice_points(rng.integers(0, 1080, n) * pitch, octave, rng.integers(0, 1920, n) * pitch, padding=1))
    m, qp, tp, _ = epiref.planted_scene(3)
    model = epiref.ransac(m, qp, tp, 64, 1, 4.0)[0]
    assert model["best"][0] >= 0
    return q, t, pts[0], pts[1], model


def test_identity_a_everything_in_band_is_the_matcher_byte_for_byte():
    q, t, qp, tp, model = identity_sets()
    assert guidedref.band(model, qp, tp, 1e300).all()
    for same_octave in (False, True):
        wnn, wm = matchref.match(q, t, 0.64, same_octave, None, None, qp["octave"], tp["octave"])
        nn, m = guidedref.guided(q, t, qp, tp, model, 0.64, np.inf, 1e300, same_octave)
        assert nn.tobytes() == wnn.tobytes() and m.tobytes() == wm.tobytes() and len(m) > 100


def test_identity_b_every_guided_match_is_an_inlier_of_the_two_view_test():
    for seed in (1, 2):
        s = guidedref.repeated_scene(seed)
        model = scene_model(seed)
        nn, m = guidedref.guided(s["q"], s["t"], s["qp"], s["tp"], model, 0.64, np.inf, 4.0)
        n, flags = epiref.score(model["F"][0], epiref.coords(m, s["qp"], s["tp"]), 4.0)
        assert len(m) > 300 and n == len(m) and flags.all()
        # ... and the nearest of every query row with one is in its band
        has = nn["index"] >= 0
        assert guidedref.band(model, s["qp"], s["tp"], 4.0)[np.flatnonzero(has), nn["index"][has]].all()


# ---- what the pass is for: planted scenes with repeated structure

@functools.lru_cache(maxsize=None)
def scene_model(seed):
    """The first pass over the scene: the matcher's restatement, then the RANSAC restatement (512 hypotheses, seed 1, 4.0)."""
    s = guidedref.repeated_scene(seed)
    _, m = matchref.match(s["q"], s["t"], 0.64)
    return epiref.ransac(m, s["qp"], s["tp"], 512, 1, 4.0)[0]


def scene_figures(seed):
    """-> dict of the figures of DESIGN 5.20's table for one scene, from the restatements."""
    s = guidedref.repeated_scene(seed)
    model = scene_model(seed)
    _, m0 = matchref.match(s["q"], s["t"], 0.64)
    _, m1 = guidedref.guided(s["q"], s["t"], s["qp"], s["tp"], model, 0.64, np.inf, 4.0)
    _, m2 = guidedref.guided(s["q"], s["t"], s["qp"], s["tp"], model, 0.64, 1.0, 4.0)
    return dict(planted=int(s["planted"].sum()), unguided=len(m0), unguided_correct=guidedref.correct(m0, s), guided=len(m1),
                guided_correct=guidedref.correct(m1, s), bounded=len(m2), bounded_correct=guidedref.correct(m2, s),
                band_share=float(guidedref.band(model, s["qp"], s["tp"], 4.0).mean()))


def check_scene_conditions(f):
    """The three conditions of a repeated-structure scene, on the figures of scene_figures() or of a device run."""
    assert f["guided_correct"] >= 0.95 * f["planted"], f
    assert f["guided_correct"] >= 1.5 * f["unguided_correct"], f
    assert f["bounded"] - f["bounded_correct"] <= 8, f


@pytest.mark.parametrize("seed", range(1, 9))
def test_repeated_structure_scenes_guided_finds_what_the_ratio_test_rejects(seed):
    f = scene_figures(seed)
    print("scene", seed, f)
    # the fixture itself: 600 draws at 0.7 (mean 420, sigma 11.2: within 3.5 sigma), and a band of 2 px half-width on a 1080-row
    # image holds well under 2 % of the train points
    assert 380 <= f["planted"] <= 460 and f["band_share"] < 0.02
    check_scene_conditions(f)

"""Guided matching under H or F without a GPU: the C ABI's new symbols, struct layout and argument checks, the host sizing under
the sanitizers, the C++ wrapper's own checks, and the CPU restatement of the rule (tests/guidedhfref.py), which the GPU tests
compare against byte for byte: the rule on hand-made sets whose answer is known by construction, the identities that tie it to
the guided pass's, the matcher's and the homography restatements, and the planted plane and rotation scenes with repeated
structure that show what the pass is for."""
import ctypes as C
import functools
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import epiref, guidedhfref, guidedref, homref, matchref
from tests.test_guided_cpu import BAND2, EXACT_F, INF, NONE, identity_sets, lattice_points, nn_rows, vw_rows
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- ABI

def test_guided_hf_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_match_guided_hf_dev", "vslam_match_guided_hf_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_guided_hf_rows", b"k_guided_hf_kinds", b"k_match_guided_hf", b"k_match_guided_merge"):
        assert k in names


def test_guided_hf_params_layout_matches_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    ct = capi.GuidedHfParams
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {", '  printf("%zu", sizeof(vslam_guided_hf_params));']
    lines += [f'  printf(" %zu", offsetof(vslam_guided_hf_params, {f[0]}));' for f in ct._fields_]
    lines += ['  printf("\\n");', "  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    row = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert row == [C.sizeof(ct)] + [getattr(ct, f[0]).offset for f in ct._fields_]
    assert row[0] == 32 and capi.GUIDED_HF_PARAMS_DTYPE.itemsize == 32
    assert [capi.GUIDED_HF_PARAMS_DTYPE.fields[f[0]][1] for f in ct._fields_] == row[1:]


class Args:
    """A valid vslam_match_guided_hf_dev call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, qcap=50, tcap=60, match_cap=10):
        self.keep = [np.zeros((n_pairs, max(qcap, tcap), 128), np.float32), np.zeros(n_pairs, np.uint32), np.zeros((n_pairs, max(qcap, tcap)), capi.POINT_DTYPE),
                     np.zeros(n_pairs, capi.EPIPOLAR_DTYPE), np.zeros((n_pairs, qcap), capi.NN2_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE),
                     np.zeros(n_pairs, np.uint32), np.zeros(n_pairs, capi.HOMOGRAPHY_DTYPE)]
        d, cnt, pts, mod, nn, m, mc, hmod = self.keep
        assert d.ctypes.data % 16 == 0
        self.Q = capi.DescSets(d.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, qcap)
        self.T = capi.DescSets(d.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, tcap)
        self.emodels, self.hmodels, self.n_pairs = mod.ctypes.data, hmod.ctypes.data, n_pairs
        self.prm = capi.GuidedHfParams(0.64, 1.0, 4.0, 4.0, 0, 0)
        self.out = capi.MatchOut(C.sizeof(capi.MatchOut), nn.ctypes.data, nn.nbytes, m.ctypes.data, m.nbytes, mc.ctypes.data, mc.nbytes, match_cap)

    def call(self, lib, Q="Q", T="T", prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return lib.vslam_match_guided_hf_dev(None, ref(Q), ref(T), self.emodels, self.hmodels, self.n_pairs, ref(prm), ref(out))


def test_guided_hf_dev_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    gpu = torch.cuda.is_available()
    OK = INVALID if gpu else HIP  # a valid call: without a GPU the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(lib) == OK
    for name in ("Q", "T", "prm", "out"):
        assert Args().call(lib, **{name: None}) == INVALID, name

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
        return a.call(lib)

    def rejected(**change):
        return bad(**change) == INVALID

    assert rejected(a__emodels=None, a__hmodels=None)
    # everything vslam_match_guided_dev rejects
    assert rejected(out__struct_size=C.sizeof(capi.MatchOut) - 8)
    assert rejected(a__n_pairs=-1) and rejected(a__n_pairs=65536)
    for s in ("Q", "T"):
        assert rejected(**{s + "__desc": None}) and rejected(**{s + "__counts": None}) and rejected(**{s + "__cap": 0})
        assert rejected(**{s + "__desc": Args().keep[0].ctypes.data + 4})  # misaligned
        assert rejected(**{s + "__points": None})
    assert rejected(out__nn=None, out__matches=None, out__match_counts=None)
    assert rejected(out__nn_bytes=2 * 50 * 12 - 1)
    assert rejected(out__match_counts=None) and rejected(out__match_cap=0)
    assert rejected(out__matches_bytes=2 * 10 * 12 - 1) and rejected(out__match_counts_bytes=7)
    assert rejected(prm__reserved=1)
    for r in (0.0, -0.64, float("nan"), float("inf")):
        assert rejected(prm__ratio2=r)
    for d in (0.0, -4.0, float("nan"), float("inf")):
        assert rejected(prm__max_dist2=d) and rejected(prm__max_transfer2=d)
        # each distance is checked only when its model array is given
        assert bad(prm__max_dist2=d, a__emodels=None) == OK and bad(prm__max_transfer2=d, a__hmodels=None) == OK
        assert rejected(prm__max_dist2=d, a__hmodels=None) and rejected(prm__max_transfer2=d, a__emodels=None)
    for b in (0.0, -1.0, float("nan"), float("-inf")):
        assert rejected(prm__max_desc_dist2=b)
    if not gpu:  # +inf is a valid bound, the optional outputs and either model array may be absent, no pairs is a valid call
        assert bad(prm__max_desc_dist2=float("inf")) == HIP and bad(prm__same_octave=1) == HIP
        assert bad(out__nn=None) == HIP and bad(out__matches=None, out__match_cap=0) == HIP and bad(a__n_pairs=0) == HIP
        assert bad(a__emodels=None) == HIP and bad(a__hmodels=None) == HIP


def test_guided_hf_host_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    q, t = np.zeros((5, 128), np.float32), np.zeros((6, 128), np.float32)
    qp, tp = np.zeros(5, capi.POINT_DTYPE), np.zeros(6, capi.POINT_DTYPE)
    emodel, hmodel = np.zeros(1, capi.EPIPOLAR_DTYPE), np.zeros(1, capi.HOMOGRAPHY_DTYPE)
    nn, m, total = np.zeros(5, capi.NN2_DTYPE), np.zeros(5, capi.MATCH_DTYPE), C.c_size_t()
    P = capi.GuidedHfParams
    good = P(0.64, float("inf"), 4.0, 4.0, 0, 0)

    def call(prm=good, qd=q.ctypes.data, qpp=qp.ctypes.data, tpp=tp.ctypes.data, emod=emodel.ctypes.data, hmod=hmodel.ctypes.data, nnp=nn.ctypes.data,
             mp=m.ctypes.data, cap=5, tot=C.byref(total)):
        return lib.vslam_match_guided_hf_host(None, qd, None, qpp, 5, t.ctypes.data, None, tpp, 6, emod, hmod, None if prm is None else C.byref(prm), nnp, mp,
                                              cap, tot)

    OK = INVALID if torch.cuda.is_available() else HIP
    assert call() == OK and call(emod=None) == OK and call(hmod=None) == OK
    assert call(prm=None) == INVALID and call(emod=None, hmod=None) == INVALID and call(qd=None) == INVALID
    assert call(qpp=None) == INVALID and call(tpp=None) == INVALID
    assert call(prm=P(0.64, 1.0, 4.0, 4.0, 0, 3)) == INVALID
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(prm=P(r, 1.0, 4.0, 4.0, 0, 0)) == INVALID and call(prm=P(0.64, 1.0, r, 4.0, 0, 0)) == INVALID and call(prm=P(0.64, 1.0, 4.0, r, 0, 0)) == INVALID
        assert call(prm=P(0.64, 1.0, r, 4.0, 0, 0), emod=None) == OK and call(prm=P(0.64, 1.0, 4.0, r, 0, 0), hmod=None) == OK
    for b in (0.0, -1.0, float("nan")):
        assert call(prm=P(0.64, b, 4.0, 4.0, 0, 0)) == INVALID
    assert call(nnp=None, tot=None, mp=None) == INVALID and call(tot=None) == INVALID and call(cap=0) == INVALID
    if not torch.cuda.is_available():
        assert call(mp=None, tot=None) == HIP and call(nnp=None) == HIP


def test_python_bindings_refuse_a_call_without_any_model():
    with pytest.raises(ValueError, match="both None"):
        capi.Context.match_guided_hf(None, None, None, n_pairs=1)


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "guided_hf_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines()}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 21 * 13 * 11, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 70, rows["args"]   # (the order of the checks is among them)
    src = open(os.path.join(CSRC, "vslam_guided_hf_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


def build_cxx_driver(tmp_path):
    """tests/guided_hf_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_guided_hf.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "guided_hf_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "guided_hf_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrapper_refuses_lists_that_do_not_fit_and_a_call_without_a_model(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    r = subprocess.run([build_cxx_driver(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ---- the rule on hand-made sets
#
# The exact-H fixture: H = [[1, 0, tx], [0, 1, ty], [0, 0, 1]] with integer tx, ty gives p = (x + tx, y + ty, 1) and L = max_transfer2,
# all exact on half-pixel coordinates: a train row is in window iff (x + tx - x')^2 + (y + ty - y')^2 < max_transfer2.  With
# max_transfer2 = 4 a row 2 pixels from the predicted position is out, one at (1.5, 1) - squared distance 3.25, an octave-0 point - is
# in.  Descriptors as in tests/test_guided_cpu.py: two small integer entries, every d2 an exact integer.

TX, TY = 3.0, -2.0
WINDOW2 = 4.0


def exact_h(tx=TX, ty=TY):
    return (1.0, 0.0, tx, 0.0, 1.0, ty, 0.0, 0.0, 1.0)


EXACT_H = exact_h()
# a horizon through the frame: p2 = 20 - y, so y = 20 has p2 = 0 and every row below it p2 < 0
HORIZON_H = (1.0, 0.0, 3.0, 0.0, 1.0, -2.0, 0.0, -1.0, 20.0)


def xy_points(xy, octave=1):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    return lattice_points(xy[:, 1], octave, xy[:, 0])


def hand_case(q, qxy, t, txy, qoct=1, toct=1, qdef=None, tdef=None, Hm=EXACT_H, hbest=0, F=None, fbest=0, **prm):
    """-> the keyword arguments of guidedhfref.guided_hf for one hand-made pair (prm: ratio2, max_desc_dist2, max_dist2, max_transfer2,
    same_octave).  Hm / F None: that model array is absent."""
    prm.setdefault("max_transfer2", WINDOW2)
    prm.setdefault("max_dist2", BAND2)
    return dict(q=vw_rows(q), t=vw_rows(t), q_points=xy_points(qxy, qoct), t_points=xy_points(txy, toct),
                epipolar_model=None if F is None else guidedref.model_record(F, fbest),
                homography_model=None if Hm is None else guidedhfref.homography_record(Hm, hbest), q_defined=qdef, t_defined=tdef, **prm)


Q10 = [(10, 0)]
AT = [(10, 10)]   # the query's point; H predicts (13, 8)
FAR = (500, 500)
TWO = dict(t=[(10, 0), (12, 0)], txy=[(13, 8), (13, 8)])


def with_entry(Hm, i, v):
    return Hm[:i] + (v,) + Hm[i + 1:]


# name -> (case, the nn rows that must come out, the accepted query rows)
HAND = {
    # the global nearest (row 0, d2 0) is far from the predicted position: the winner is the nearest in the window
    "nearest out of window": (hand_case(Q10, AT, [(10, 0), (12, 0), (20, 0)], [(50, 50), (13, 8), (14, 8)]), [(1, 4.0, 100.0)], [0]),
    # 4 < 0.64 * 5 is false, 4 < 0.64 * 400 is true: the global second nearest (row 1, d2 5) is out of window
    "second out of window": (hand_case(Q10, AT, [(12, 0), (11, 2), (30, 0)], [(13, 8), (40, 40), (13, 9)]), [(0, 4.0, 400.0)], [0]),
    "lone candidate": (hand_case(Q10, AT, [(40, 0), (10, 0)], [(13, 8), FAR]), [(0, 900.0, INF)], [0]),
    "lone candidate, bound": (hand_case(Q10, AT, [(40, 0), (10, 0)], [(13, 8), FAR], max_desc_dist2=1.0), [(0, 900.0, INF)], []),
    "empty window": (hand_case(Q10, AT, [(10, 0), (11, 0)], [(50, 8), (13, 20)]), [NONE], []),
    "no train rows": (hand_case(Q10, AT, np.zeros((0, 2)), np.zeros((0, 2))), [NONE], []),
    # three equal rows, the first out of window: the lowest index IN the window, and second == best is rejected by the ratio
    "tie": (hand_case(Q10, AT, [(12, 0), (12, 0), (12, 0), (13, 0)], [(30, 30), (13, 9), (12, 8), (13, 8)]), [(1, 4.0, 4.0)], []),
    # exactly 2 pixels from (13, 8) is out (4 is not below 4) in either direction; (1.5, 1) off - octave-0 points, 3.25 - is in
    "boundary": (hand_case(Q10, AT, [(10, 0), (10, 0), (12, 0), (13, 0)], [(15, 8), (13, 10), (14.5, 9), (11.5, 7)], toct=[1, 1, 0, 0]), [(2, 4.0, 9.0)], [0]),
    "best < 0 in H": (hand_case(Q10, AT, **TWO, hbest=-1), [NONE], []),
    # rows 1 and 2 are on and below the horizon; row 2's train row 2 would be 13 < 400 "in" if p2 > 0 were not asked
    "horizon": (hand_case([(10, 0)] * 3, [(10, 10), (10, 20), (10, 30)], [(12, 0), (10, 0), (10, 0)], [(1, 1), FAR, (-1, -3)], Hm=HORIZON_H),
                [(0, 4.0, INF), NONE, NONE], [0]),
    "H negated": (hand_case(Q10, AT, **TWO, Hm=tuple(-v for v in EXACT_H)), [NONE], []),
    "zero H": (hand_case(Q10, AT, **TWO, Hm=(0.0,) * 9), [NONE], []),
    "NaN in H": (hand_case(Q10, AT, **TWO, Hm=with_entry(EXACT_H, 4, np.nan)), [NONE], []),
    "NaN in the last row of H": (hand_case(Q10, AT, **TWO, Hm=with_entry(EXACT_H, 6, np.nan)), [NONE], []),
    "inf in H": (hand_case(Q10, AT, **TWO, Hm=with_entry(EXACT_H, 2, np.inf)), [NONE], []),
    "-inf in the last row of H": (hand_case(Q10, AT, **TWO, Hm=with_entry(EXACT_H, 8, -np.inf)), [NONE], []),
    # p2 = +inf: p2*p2 and x'*p2 are inf, dx = 13 - inf = -inf, inf < inf is false
    "+inf in the last row of H": (hand_case(Q10, AT, **TWO, Hm=with_entry(EXACT_H, 8, np.inf)), [NONE], []),
    # rows that are not trusted: a query gets nothing, a train row is skipped even where it is the exact copy
    "octaves 32 and -1": (hand_case([(10, 0)] * 3, AT * 3, [(10, 0), (10, 0), (12, 0)], [(13, 8)] * 3, qoct=[1, 32, -1], toct=[32, -1, 1]),
                          [(2, 4.0, INF), NONE, NONE], [0]),
    "defined = 0": (hand_case([(10, 0)] * 2, AT * 2, [(10, 0), (12, 0), (30, 0)], [(13, 8)] * 3, qdef=[1, 0], tdef=[0, 1, 1]), [(1, 4.0, 400.0), NONE], [0]),
    # (row 0 is an octave-2 point, pitch 2: at (14, 8), one pixel from the predicted position)
    "same_octave off": (hand_case(Q10, AT, [(10, 0), (12, 0)], [(14, 8), (13, 8)], toct=[2, 1]), [(0, 0.0, 4.0)], [0]),
    "same_octave on": (hand_case(Q10, AT, [(10, 0), (12, 0)], [(14, 8), (13, 8)], toct=[2, 1], same_octave=True), [(1, 4.0, INF)], [0]),
}

# kind selection: train row 0 is in the band of F (y' = 10) and far from the window, row 1 at the predicted position (13, 8), which is
# exactly 2 pixels off the query's line and so out of the band
KIND_ROWS = dict(t=[(12, 0), (13, 0)], txy=[(100, 10), (13, 8)])
BY_F, BY_H = [(0, 4.0, INF)], [(1, 9.0, INF)]
for fname, fargs in (("F valid", dict(F=EXACT_F)), ("F best < 0", dict(F=EXACT_F, fbest=-1)), ("F NULL", dict())):
    for hname, hargs in (("H valid", dict()), ("H best < 0", dict(hbest=-1)), ("H NULL", dict(Hm=None))):
        if fname == "F NULL" and hname == "H NULL":
            continue  # rejected: test_kind_selection_the_doubly_null_call_is_rejected
        want = BY_F if fname == "F valid" else BY_H if hname == "H valid" else [NONE]
        HAND[f"kind: {fname}, {hname}"] = (hand_case(Q10, AT, **KIND_ROWS, **fargs, **hargs), want, [] if want == [NONE] else [0])


@pytest.mark.parametrize("name", list(HAND))
def test_rule_on_hand_made_sets(name):
    case, want_nn, want_acc = HAND[name]
    nn, m = guidedhfref.guided_hf(**case)
    assert nn.tobytes() == nn_rows(want_nn).tobytes(), (name, nn)
    assert list(m["query"]) == want_acc and (m["train"] == nn["index"][m["query"]]).all() and (m["dist2"] == nn["dist2"][m["query"]]).all()


def test_kind_selection_the_doubly_null_call_is_rejected():
    case = hand_case(Q10, AT, **KIND_ROWS, Hm=None)
    assert case["epipolar_model"] is None and case["homography_model"] is None
    with pytest.raises(AssertionError):
        guidedhfref.guided_hf(**case)
    K = guidedhfref
    e, h = guidedref.model_record(EXACT_F), K.homography_record(EXACT_H)
    e0, h0 = guidedref.model_record(EXACT_F, -1), K.homography_record(EXACT_H, -1)
    assert [K.kind(a, b) for a in (e, e0, None) for b in (h, h0, None)] == [K.F, K.F, K.F, K.H, K.NONE, K.NONE, K.H, K.NONE, K.NONE]


def test_window_on_the_exact_fixture_is_the_integer_inequality():
    """Every half-pixel offset within 3 pixels of the predicted position: in window iff the squared distance is below 4, exactly."""
    off = np.arange(-6, 7) / 2.0
    txy = np.array([(13 + a, 8 + b) for a in off for b in off])
    w = guidedhfref.window(guidedhfref.homography_record(EXACT_H), xy_points(AT), xy_points(txy, 0), WINDOW2)
    d2 = (txy[:, 0] - 13) ** 2 + (txy[:, 1] - 8) ** 2
    assert (w[0] == (d2 < 4.0)).all() and (d2 == 4.0).sum() == 4 and (d2 == 3.25).sum() == 8 and w[0].sum() == 45
    assert guidedhfref.in_window(EXACT_H, (10, 10), (14.5, 9), WINDOW2) and not guidedhfref.in_window(EXACT_H, (10, 10), (15, 8), WINDOW2)


def test_hand_made_sets_differ_from_the_unguided_matcher_where_they_should():
    c = HAND["nearest out of window"][0]
    assert matchref.match(c["q"], c["t"])[0]["index"][0] == 0
    c = HAND["second out of window"][0]
    nn, m = matchref.match(c["q"], c["t"])
    assert nn["index"][0] == 0 and nn["second_dist2"][0] == 5.0 and len(m) == 0


# ---- identities

def test_identity_a_without_homography_models_the_call_is_the_guided_pass():
    q, t, qp, tp, model = identity_sets()
    none = guidedref.model_record(model["F"][0], best=-1)
    for same_octave in (False, True):
        for md in (1e300, 4.0):
            wnn, wm = guidedref.guided(q, t, qp, tp, model, 0.64, np.inf, md, same_octave)
            nn, m = guidedhfref.guided_hf(q, t, qp, tp, model, None, 0.64, np.inf, md, 4.0, same_octave)
            assert nn.tobytes() == wnn.tobytes() and m.tobytes() == wm.tobytes()
        assert len(m) > 0
    wnn, wm = guidedref.guided(q, t, qp, tp, none)
    nn, m = guidedhfref.guided_hf(q, t, qp, tp, none, None)
    assert nn.tobytes() == wnn.tobytes() and len(m) == len(wm) == 0


def test_identity_b_everything_in_window_is_the_matcher_byte_for_byte():
    q, t, qp, tp, _ = identity_sets()
    h = guidedhfref.homography_record(EXACT_H)
    assert guidedhfref.window(h, qp, tp, 1e300).all()
    for same_octave in (False, True):
        wnn, wm = matchref.match(q, t, 0.64, same_octave, None, None, qp["octave"], tp["octave"])
        nn, m = guidedhfref.guided_hf(q, t, qp, tp, None, h, 0.64, np.inf, 4.0, 1e300, same_octave)
        assert nn.tobytes() == wnn.tobytes() and m.tobytes() == wm.tobytes() and len(m) > 100


def exact_forward(Hm, xy, max_transfer2):
    """The forward clause in exact rational arithmetic - homref.exact_inlier's `one` over H alone, with its `near` -> (in, near)."""
    h = [Fraction(float(v)) for v in np.asarray(Hm, np.float64).reshape(9)]
    md, eps = Fraction(float(max_transfer2)), Fraction(1, 2 ** 40)
    inl, near = np.zeros(len(xy), bool), np.zeros(len(xy), bool)
    for i, rec in enumerate(xy):
        x, y, u, v = (Fraction(float(c)) for c in rec)
        p0, p1, p2 = h[0] * x + h[1] * y + h[2], h[3] * x + h[4] * y + h[5], h[6] * x + h[7] * y + h[8]
        dx, dy = p0 - u * p2, p1 - v * p2
        lhs, rhs = dx * dx + dy * dy, md * p2 * p2
        T = abs(p0) + abs(p1) + (abs(u) + abs(v)) * abs(p2)
        near[i] = abs(lhs - rhs) <= eps * (T * T + rhs) or abs(p2) <= eps * (abs(h[6] * x) + abs(h[7] * y) + abs(h[8]))
        inl[i] = p2 > 0 and lhs < rhs
    return inl, near


@pytest.mark.parametrize("kind", ["plane", "rotation"])
def test_identity_c_every_accepted_match_under_h_satisfies_the_forward_clause_exactly(kind):
    s, f = scene_chain(1, kind)
    m = f["m1"]
    inl, near = exact_forward(f["hmodel"]["H"][0], epiref.coords(m, s["qp"], s["tp"]), 4.0)
    assert len(m) > 300 and (inl | near).all() and inl.sum() >= len(m) - 2
    # ... and the nearest of every query row with one is in its window
    nn = f["nn1"]
    has = nn["index"] >= 0
    assert guidedhfref.window(f["hmodel"], s["qp"], s["tp"], 4.0)[np.flatnonzero(has), nn["index"][has]].all()


# ---- what the pass is for: planted plane and rotation scenes with repeated structure

@functools.lru_cache(maxsize=None)
def scene_chain(seed, kind):
    """One scene through the restatements: matcher (0.64), RANSAC F and H (512 hypotheses, seed 1, 4.0), verdict and gate, then the pass
    under (gated F, H) with the window at 4.0, unbounded and with the bound 1.0 -> (scene, dict of every list and model)."""
    s = guidedhfref.repeated_scene(seed, kind)
    _, m0 = matchref.match(s["q"], s["t"], 0.64)
    emodel = epiref.ransac(m0, s["qp"], s["tp"], 512, 1, 4.0)[0]
    hmodel = homref.verdict(homref.ransac(m0, s["qp"], s["tp"], 512, 1, 4.0)[0], emodel)
    gated = homref.gate(emodel, hmodel)
    nn1, m1 = guidedhfref.guided_hf(s["q"], s["t"], s["qp"], s["tp"], gated, hmodel, 0.64, np.inf, 4.0, 4.0)
    _, m2 = guidedhfref.guided_hf(s["q"], s["t"], s["qp"], s["tp"], gated, hmodel, 0.64, 1.0, 4.0, 4.0)
    return s, dict(m0=m0, emodel=emodel, hmodel=hmodel, gated=gated, nn1=nn1, m1=m1, m2=m2)


def figures_of(s, m0, m1, m2):
    return dict(planted=int(s["planted"].sum()), unguided=len(m0), unguided_correct=guidedref.correct(m0, s), guided=len(m1),
                guided_correct=guidedref.correct(m1, s), bounded=len(m2), bounded_correct=guidedref.correct(m2, s))


def check_scene_conditions(f):
    """The three conditions of a degenerate repeated-structure scene, on figures_of() of the restatements or of a device run."""
    assert f["guided_correct"] >= 0.90 * f["planted"], f
    assert f["guided_correct"] >= 1.5 * f["unguided_correct"], f
    assert f["guided"] - f["guided_correct"] <= 8 and f["bounded"] - f["bounded_correct"] <= 8, f


@pytest.mark.parametrize("seed", range(1, 9))
@pytest.mark.parametrize("kind", ["plane", "rotation"])
def test_degenerate_scenes_the_window_finds_what_the_ratio_test_rejects(kind, seed):
    s, c = scene_chain(seed, kind)
    f = figures_of(s, c["m0"], c["m1"], c["m2"])
    share = float(guidedhfref.window(c["hmodel"], s["qp"], s["tp"], 4.0).mean())
    print("scene", kind, seed, f, "H inliers", int(c["hmodel"]["n_inliers"][0]), "window share", share)
    assert 380 <= f["planted"] <= 460 and share < 0.004  # (the fixture: guidedref's draws; a 2-pixel disc holds the partner, 1 row in 600, and little else)
    assert int(c["hmodel"]["degenerate"][0]) == 1 and int(c["gated"]["best"][0]) == -1 and guidedhfref.kind(c["gated"], c["hmodel"]) == guidedhfref.H
    check_scene_conditions(f)
    # the guided pass under the gated model finds nothing: the pair has no F to guide by
    assert len(guidedref.guided(s["q"], s["t"], s["qp"], s["tp"], c["gated"], 0.64, np.inf, 4.0)[1]) == 0

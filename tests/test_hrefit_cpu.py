"""Least-squares refit of the homography without a GPU: the C ABI's new symbols, struct layouts and argument checks, the host
sizing under the sanitizers, the capi and C++ wrappers, and the CPU restatement of the arithmetic itself (tests/hrefitref.py),
which the GPU tests compare against byte for byte: the 24-sum moment matrix against A^T A of the explicit DLT rows, the
eigenvector against numpy.linalg.eigh, the measurement behind VSLAM_HREFIT_SWEEPS, the acceptance rule on the planted scenes
of tests/homref.py, the verdict run again, and the five-frame plane chain with the refit in it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chainref, epiref, homref, hposeref, hrefitref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
K = hposeref.K_PLANTED
EIGH_TOL = 6.2e-12  # the tolerance tests/test_refit_cpu.py uses for its numpy.linalg.eigh comparison


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_hrefit_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_hrefit_dev", "vslam_hrefit_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_hrefit_init", b"k_hrefit_count", b"k_hrefit_begin", b"k_hrefit_dist", b"k_hrefit_scale", b"k_hrefit_moments", b"k_hrefit_solve"):
        assert k in names


def test_hrefit_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_hrefit_params": capi.HRefitParams, "vslam_hrefit": capi.HRefit, "vslam_hrefit_out": capi.HRefitOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {"]
    for cname, ct in structs.items():
        lines.append(f'  printf("{cname} %zu", sizeof({cname}));')
        lines += [f'  printf(" %zu", offsetof({cname}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
    lines += ['  printf("sweeps %d\\n", VSLAM_HREFIT_SWEEPS);', "  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()}
    for cname, ct in structs.items():
        assert rows[cname] == [C.sizeof(ct)] + [getattr(ct, f[0]).offset for f in ct._fields_], cname
    assert rows["vslam_hrefit"][0] == 16 and capi.HREFIT_DTYPE.itemsize == 16
    assert [capi.HREFIT_DTYPE.fields[f[0]][1] for f in capi.HRefit._fields_] == [getattr(capi.HRefit, f[0]).offset for f in capi.HRefit._fields_]
    assert [f[0] for f in capi.HRefit._fields_] == [f[0] for f in capi.Refit._fields_]          # the fields of vslam_refit
    assert rows["sweeps"] == [hrefitref.SWEEPS]


class Args:
    """A valid vslam_hrefit_dev call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, match_cap=100, cap=50, inlier_cap=40):
        self.keep = [np.zeros(n_pairs, capi.HOMOGRAPHY_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32),
                     np.zeros((n_pairs, cap), capi.POINT_DTYPE), np.zeros(n_pairs, capi.HOMOGRAPHY_DTYPE), np.zeros(n_pairs, capi.HREFIT_DTYPE),
                     np.zeros((n_pairs, (match_cap + 63) // 64), np.uint64), np.zeros((n_pairs, inlier_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32),
                     np.zeros(n_pairs, capi.EPIPOLAR_DTYPE), np.zeros(n_pairs, capi.EPIPOLAR_DTYPE)]
        mod, m, mc, p, models, info, bits, inl, icnt, epi, gated = self.keep
        self.models_in, self.matches, self.counts, self.qp, self.tp = mod.ctypes.data, m.ctypes.data, mc.ctypes.data, p.ctypes.data, p.ctypes.data
        self.epi = epi.ctypes.data
        self.match_cap, self.query_cap, self.train_cap, self.n_pairs = match_cap, cap, cap, n_pairs
        self.prm = capi.HRefitParams(4, 4.0, 1, 2, 16)
        self.out = capi.HRefitOut(C.sizeof(capi.HRefitOut), models.ctypes.data, models.nbytes, info.ctypes.data, info.nbytes, bits.ctypes.data, bits.nbytes,
                                  inl.ctypes.data, inl.nbytes, icnt.ctypes.data, icnt.nbytes, inlier_cap, gated.ctypes.data, gated.nbytes)

    def call(self, lib, prm="prm", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return lib.vslam_hrefit_dev(None, self.models_in, self.matches, self.counts, self.match_cap, self.qp, self.query_cap, self.tp, self.train_cap,
                                    self.n_pairs, self.epi, ref(prm), ref(out))


def test_hrefit_dev_rejects_bad_arguments_before_it_needs_a_gpu(lib):
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

    for name in ("models_in", "matches", "counts", "qp", "tp"):
        assert bad(**{"a__" + name: None}) == INVALID, name
    assert bad(out__struct_size=C.sizeof(capi.HRefitOut) - 8) == INVALID
    assert bad(out__models=None) == INVALID and bad(out__models_bytes=2 * 168 - 1) == INVALID
    assert bad(out__info_bytes=2 * 16 - 1) == INVALID
    assert bad(out__inlier_bits_bytes=2 * 2 * 8 - 1) == INVALID
    assert bad(out__inliers_bytes=2 * 40 * 12 - 1) == INVALID
    assert bad(out__inlier_counts_bytes=2 * 4 - 1) == INVALID
    assert bad(out__gated_models_bytes=2 * 88 - 1) == INVALID
    assert bad(out__inlier_counts=None) == INVALID and bad(out__inlier_cap=0) == INVALID      # inliers without its totals / its capacity
    assert bad(a__epi=None) == INVALID                                                        # gated_models without epipolar_models
    assert bad(prm__degenerate_den=0) == INVALID                                              # ... the verdict needs its denominator
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for rounds in (0, 9, 2 ** 32 - 1):
        assert bad(prm__rounds=rounds) == INVALID, rounds
    for v in (0.0, -0.0, -4.0, float("nan"), float("inf"), -float("inf")):
        assert bad(prm__max_dist2=v) == INVALID, v
    assert bad(a__match_cap=0) == INVALID and bad(a__query_cap=0) == INVALID and bad(a__train_cap=0) == INVALID
    if not gpu:  # the optional outputs may be absent, the models may be written in place, and no pairs is a valid call
        assert bad(out__info=None, out__inlier_bits=None, out__inliers=None, out__inlier_counts=None, out__inlier_cap=0, out__gated_models=None) == HIP
        assert bad(out__inliers=None, out__inlier_cap=0) == HIP and bad(a__n_pairs=0) == HIP
        assert bad(a__epi=None, out__gated_models=None, prm__degenerate_den=0) == HIP         # without a verdict the denominator is not read
        for rounds in (1, 8):
            assert bad(prm__rounds=rounds) == HIP
        a = Args()
        a.out.models, a.out.gated_models = a.models_in, a.epi
        assert a.call(lib) == HIP


def test_hrefit_host_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    m, qp, tp, _ = homref.planted_scene(1, 20, "plane")
    model, out = np.zeros(1, capi.HOMOGRAPHY_DTYPE), np.zeros(1, capi.HOMOGRAPHY_DTYPE)
    epi, gated = np.zeros(1, capi.EPIPOLAR_DTYPE), np.zeros(1, capi.EPIPOLAR_DTYPE)
    good = capi.HRefitParams(4, 4.0, 1, 2, 16)
    inl = np.zeros(20, capi.MATCH_DTYPE)

    def call(prm=good, modp=model.ctypes.data, mp=m.ctypes.data, q=qp.ctypes.data, nq=20, outp=out.ctypes.data, epip=None, inliers=None, cap=0, total=None,
             gatedp=None):
        return lib.vslam_hrefit_host(None, modp, mp, 20, q, nq, tp.ctypes.data, 20, epip, None if prm is None else C.byref(prm), outp, None, None, inliers,
                                     cap, total, gatedp)

    assert call() == (INVALID if torch.cuda.is_available() else HIP)
    assert call(prm=None) == INVALID and call(modp=None) == INVALID and call(outp=None) == INVALID and call(mp=None) == INVALID and call(q=None) == INVALID
    for bad in ((0, 4.0), (9, 4.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf"))):
        assert call(prm=capi.HRefitParams(*bad, 1, 2, 16)) == INVALID, bad
    assert call(prm=capi.HRefitParams(4, 4.0, 1, 0, 16), epip=epi.ctypes.data) == INVALID   # the verdict without its denominator
    assert call(gatedp=gated.ctypes.data) == INVALID                           # gated_model without epipolar_model
    assert call(q=None, nq=0) == INVALID                                      # match records without points
    assert call(inliers=inl.ctypes.data, cap=20) == INVALID                   # inliers without n_inliers
    assert call(inliers=inl.ctypes.data, cap=0, total=C.byref(C.c_size_t())) == INVALID
    if not torch.cuda.is_available():
        assert call(prm=capi.HRefitParams(4, 4.0, 1, 0, 16)) == HIP            # no verdict: the denominator is not read
        assert call(epip=epi.ctypes.data, gatedp=gated.ctypes.data) == HIP


MESSAGES = [
    ("null params", "null argument"), ("null out", "null argument"), ("struct_size", "out->struct_size is not sizeof(vslam_hrefit_out)"),
    ("pairs < 0", "0 .. 65535 pairs per call"), ("pairs > 65535", "0 .. 65535 pairs per call"),
    ("rounds 0", "1 .. 8 rounds"), ("rounds 9", "1 .. 8 rounds"), ("rounds max", "1 .. 8 rounds"),
    ("dist 0", "max_dist2 must be finite and positive"), ("dist < 0", "max_dist2 must be finite and positive"),
    ("dist nan", "max_dist2 must be finite and positive"), ("dist inf", "max_dist2 must be finite and positive"),
    ("den 0 with epipolar_models", "degenerate_den must be positive"),
    ("null models_in", "null input"), ("null matches", "null input"), ("null counts", "null input"), ("null query", "null input"), ("null train", "null input"),
    ("match_cap 0", "a capacity is zero"), ("query_cap 0", "a capacity is zero"), ("train_cap 0", "a capacity is zero"),
    ("no models", "models is required"), ("models short", "models buffer too small"), ("models small", "models buffer too small"),
    ("info short", "info buffer too small"), ("info small", "info buffer too small"),
    ("bits short", "inlier_bits buffer too small"), ("bits small", "inlier_bits buffer too small"),
    ("inliers without counts", "inliers needs inlier_counts and an inlier_cap"), ("inliers without cap", "inliers needs inlier_counts and an inlier_cap"),
    ("inliers short", "inliers buffer too small"), ("inliers small", "inliers buffer too small"),
    ("counts short", "inlier_counts buffer too small"), ("counts small", "inlier_counts buffer too small"),
    ("gated without epipolar_models", "gated_models needs epipolar_models"),
    ("gated short", "gated_models buffer too small"), ("gated small", "gated_models buffer too small"),
]


def test_host_sizing_checks_and_messages_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "hrefit_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines() if not l.startswith("msg ")}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 15 * 9 + 1, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) >= 60, rows["args"]   # (the order of the checks is among them)
    got = [tuple(l[4:].split("|", 1)) for l in out.stdout.splitlines() if l.startswith("msg ")]
    assert got == MESSAGES
    src = open(os.path.join(CSRC, "vslam_hrefit_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src
    unit = open(os.path.join(CSRC, "vslam_hrefit.hip")).read()    # ... and the entry point puts its stage in front of the message
    assert 'std::string("hrefit: ") + why' in unit and unit.index("hrefit_check_args(") < unit.index("usable_ctx(c)")


def test_capi_wrappers_check_their_tensors_without_a_gpu():
    import torch

    n, cap = 2, 64
    t = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8)
    good = dict(models_in=t(n * 168), matches=torch.zeros((n, cap, 3), dtype=torch.int32), match_counts=torch.zeros(n, dtype=torch.int32),
                query_points=torch.zeros((n, 10, 6), dtype=torch.int32), train_points=torch.zeros((n, 10, 6), dtype=torch.int32), models=t(n * 168))
    ctx = capi.Context.__new__(capi.Context)  # no library call is reached: every case below fails a check first
    ctx.where = torch.device("cpu")
    with pytest.raises(ValueError, match="hrefit: models is required"):
        ctx.hrefit(**dict(good, models=None))
    with pytest.raises(ValueError, match="hrefit: models_in must hold n_pairs \\* 168 bytes"):
        ctx.hrefit(**dict(good, models_in=t(n * 168 - 1)))
    with pytest.raises(ValueError, match="hrefit: epipolar_models must hold n_pairs \\* 88 bytes"):
        ctx.hrefit(**dict(good, epipolar_models=t(n * 88 - 1)))
    with pytest.raises(ValueError, match="hrefit: matches must be"):
        ctx.hrefit(**dict(good, matches=torch.zeros((n, cap), dtype=torch.int32)))
    with pytest.raises(ValueError, match="hrefit: points must be"):
        ctx.hrefit(**dict(good, query_points=torch.zeros((n, 10, 5), dtype=torch.int32)))
    with pytest.raises(ValueError, match="hrefit: info must be a contiguous tensor"):
        ctx.hrefit(**dict(good, info=torch.zeros((n, 8), dtype=torch.int32)[:, ::2]))
    with pytest.raises(ValueError, match="hrefit: fewer sets than pairs"):
        ctx.hrefit(**dict(good, n_pairs=3))
    ctx.where = torch.device("cuda", 0)       # ... and CPU tensors are not on the context's device
    with pytest.raises(ValueError, match="hrefit: models_in must be a contiguous tensor on cuda:0"):
        ctx.hrefit(**good)
    assert capi.HREFIT_DTYPE == capi.REFIT_DTYPE


def test_cxx_wrapper_is_refused_without_a_gpu(tmp_path):
    """vslam::refitHomography through tests/hrefit_cxx_driver.cpp: without a usable HIP device the wrapper throws (there is no CPU
    path); with one, the pair without a model comes back with stop 5."""
    import torch

    if not shutil.which("g++"):
        pytest.skip("no g++")
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "hrefit_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "hrefit_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    if torch.cuda.is_available():
        assert r.stdout.strip() == "ran: stop 5"
    else:
        assert r.stdout.startswith("refused: ") and "no usable HIP device" in r.stdout


# ---- the restatement itself

def dlt_rows(xy, norm):
    """The two rows per record of the homography section's step 2 from the normalised coordinates, numpy: [2 m, 9]."""
    cqx, cqy, sq, ctx, cty, st = norm
    x, y, u, v = (xy[:, 0] - cqx) * sq, (xy[:, 1] - cqy) * sq, (xy[:, 2] - ctx) * st, (xy[:, 3] - cty) * st
    o, z = np.ones_like(x), np.zeros_like(x)
    return np.concatenate([np.stack([x, y, o, z, z, z, -u * x, -u * y, -u], axis=1), np.stack([z, z, z, x, y, o, -v * x, -v * y, -v], axis=1)])


def test_the_24_sums_are_ata_of_the_dlt_rows_and_the_eigenvector_is_eighs():
    """M through its block structure against A^T A of the explicit rows, and h against numpy.linalg.eigh's smallest eigenvector up
    to sign, both at the tolerance tests/test_refit_cpu.py uses for its eigh comparison (relative to the largest entry of M)."""
    worst_m = worst_h = 0.0
    for kind, seed, n in hrefitref.PROTOTYPE_SCENES:
        m, qp, tp, model, flags, xy = hrefitref.scene(kind, seed, n)
        stop, cnt, norm, M, sums, members = hrefitref.moments(model["H"][0], model["G"][0], xy, 4.0)
        assert stop == 0 and cnt == int(model["n_inliers"][0]) == int(flags.sum()) and (members == flags).all()
        assert (M == M.T).all() and M[2, 2] == M[5, 5] == cnt == sums[0, 5] and not M[:3, 3:6].any()
        A = dlt_rows(xy[members], norm)
        worst_m = max(worst_m, np.abs(M - A.T @ A).max() / np.abs(M).max())
        h = hrefitref.jacobi9(M)
        e = np.linalg.eigh(M)[1][:, 0]
        worst_h = max(worst_h, min(np.abs(h - e).max(), np.abs(h + e).max()))
        assert abs(np.linalg.norm(h) - 1.0) <= 1e-14
    print("M against A^T A: worst relative difference", worst_m, "; h against numpy.linalg.eigh: worst |difference|", worst_h)
    assert worst_m <= EIGH_TOL and worst_h <= EIGH_TOL


def test_sweep_constant_is_the_measured_fixpoint_plus_two():
    """N = the smallest sweep count such that every count from N to 20 gives a bit-identical h in every round: measured 7 over
    the 32 planted scenes (all 4 rounds; 5 .. 7 each) and the hostile fixtures (1 .. 7); VSLAM_HREFIT_SWEEPS = N + 2 = 9."""
    cases = [(hrefitref.scene(*s)[3], hrefitref.scene(*s)[5], 4.0) for s in hrefitref.PROTOTYPE_SCENES]
    cases += [(model, epiref.coords(mt, qp, tp), d2) for _, model, mt, qp, tp, d2, _ in hrefitref.hostile_fixtures()]
    table = {}
    for model, xy, d2 in cases:
        hs = {s: hrefitref.hrefit_xy(model, xy, 4, d2, sweeps=s)[3].tobytes() for s in range(1, 21)}
        N = 20
        while N > 1 and hs[N - 1] == hs[20]:
            N -= 1
        table[N] = table.get(N, 0) + 1
    print("sweep fixpoint N -> cases:", dict(sorted(table.items())), "of", len(cases))
    assert max(table) + 2 == hrefitref.SWEEPS
    hdr = open(os.path.join(ROOT, "include", "vslam.h")).read()
    assert int(re.search(r"#define VSLAM_HREFIT_SWEEPS (\d+)", hdr).group(1)) == hrefitref.SWEEPS


def test_exact_data_stays_exact():
    """Records that satisfy an exactly representable H with zero error: all are members before, and all stay members."""
    model, mt, qp, tp = hrefitref.exact_pair(200)
    xy = epiref.coords(mt, qp, tp)
    assert homref.score(model["H"][0], model["G"][0], xy, 1e-300)[0] == 200            # zero error: inside any positive bound
    for d2 in (4.0, 1e-12):
        out, info, flags, _ = hrefitref.hrefit_xy(model, xy, 4, d2)
        assert (int(info["n_before"][0]), int(info["n_after"][0]), int(out["n_inliers"][0])) == (200, 200, 200) and flags.all()
        assert int(info["stop"][0]) == 0 and int(info["accepted"][0]) == 4
        H = out["H"][0].reshape(3, 3)
        assert np.abs(H / H[2, 2] - np.array([[1, 0, 16], [0, 1, 32], [0, 0, 1.0]])).max() <= 1e-9


def frobenius_to_planted(H, kind):
    P = hrefitref.planted_H(kind)
    H = np.asarray(H, np.float64).reshape(3, 3)
    H = H / np.linalg.norm(H)
    return min(np.linalg.norm(H - P), np.linalg.norm(H + P))


def test_refit_never_loses_an_inlier_and_moves_h_towards_the_planted_one():
    """The 32 prototype scenes, rounds = 4.  Asserted: n_after >= n_before everywhere, the copied fields, the unit norm and the
    sign rule of the output, and on the eight 300-record plane scenes the median Frobenius distance to the planted H strictly
    below the median before (measured with this restatement: 1.27e-2 -> 1.11e-3; the values are recorded in DESIGN 5.25)."""
    before, after = {}, {}
    for kind, seed, n in hrefitref.PROTOTYPE_SCENES:
        m, qp, tp, model, flags, xy = hrefitref.scene(kind, seed, n)
        out, info, fl, _ = hrefitref.hrefit_xy(model, xy, 4, 4.0)
        i = info[0]
        before[kind, seed, n], after[kind, seed, n] = frobenius_to_planted(model["H"][0], kind), frobenius_to_planted(out["H"][0], kind)
        print(f"{kind} seed {seed} n {n}: inliers {int(i['n_before'])} -> {int(i['n_after'])} accepted {int(i['accepted'])} stop {int(i['stop'])} "
              f"|H - planted| {before[kind, seed, n]:.3e} -> {after[kind, seed, n]:.3e}")
        assert int(i["n_before"]) == int(model["n_inliers"][0]) == int(flags.sum()) and int(i["n_after"]) >= int(i["n_before"])
        assert int(out["n_inliers"][0]) == int(i["n_after"]) == int(fl.sum()) and int(i["stop"]) in (0, 4)
        for f in ("n_matches", "best", "n_valid", "n_epipolar", "degenerate"):
            assert int(out[f][0]) == int(model[f][0]), f
        assert abs(np.linalg.norm(out["H"][0]) - 1.0) <= 1e-14
        if int(i["accepted"]) == 0:
            assert out.tobytes() == model.tobytes()                           # the RANSAC model is kept, bit for bit
        else:
            mean = xy[fl].mean(axis=0)
            assert out["H"][0][6:] @ np.array([mean[0], mean[1], 1.0]) > 0 and out["G"][0][6:] @ np.array([mean[2], mean[3], 1.0]) > 0
    planes = [("plane", seed, 300) for seed in range(8)]
    mb, ma = np.median([before[s] for s in planes]), np.median([after[s] for s in planes])
    better = sum(after[s] < before[s] for s in before)
    print(f"median |H - planted| over the eight 300-record plane scenes: {mb:.3e} -> {ma:.3e}; nearer on {better} of {len(before)} scenes")
    assert ma < mb
    i = hrefitref.hrefit_xy(*[hrefitref.scene(*hrefitref.FEWER_INLIERS)[k] for k in (3, 5)], 4, 4.0)[1][0]
    assert (int(i["stop"]), int(i["accepted"])) == (4, 0)                       # the pinned scene whose first refit loses an inlier


def test_verdict_is_run_again_at_its_integer_boundaries():
    """With an epipolar model the output's n_epipolar and degenerate are homref.verdict's from the NEW inlier count; without
    one both fields are copied through."""
    m, qp, tp, model, flags, xy = hrefitref.scene("plane", 0, 300)
    stale = model.copy()
    stale["n_epipolar"], stale["degenerate"] = 12345, 1
    out = hrefitref.hrefit_xy(stale, xy, 4, 4.0)[0]
    assert (int(out["n_epipolar"][0]), int(out["degenerate"][0])) == (12345, 1)     # copied
    nh = int(out["n_inliers"][0])
    assert nh == 205 and int(model["n_inliers"][0]) == 204                           # the refit gained one inlier: the boundary moves with it
    epi = np.zeros(1, capi.EPIPOLAR_DTYPE)
    epi["best"], epi["n_matches"] = 0, 300
    for ne, num, den, min_inliers, want in ((2 * nh, 1, 2, 16, 1), (2 * nh + 1, 1, 2, 16, 0), (nh, 1, 1, nh, 1), (nh, 1, 1, nh + 1, 0),
                                            (2 ** 32 - 1, 2 ** 32 - 1, nh, 16, 0), (0, 1, 2, 16, 1)):
        epi["n_inliers"] = ne
        got = hrefitref.hrefit_xy(stale, xy, 4, 4.0, epipolar=epi, num=num, den=den, min_inliers=min_inliers)[0]
        assert (int(got["n_epipolar"][0]), int(got["degenerate"][0])) == (ne, want), (ne, num, den, min_inliers)
        assert got["H"].tobytes() == out["H"].tobytes() and int(got["n_inliers"][0]) == nh
        # the unrefitted model sits on the other side of the first boundary
        if (ne, num, den) == (2 * nh, 1, 2):
            assert int(homref.verdict(model, epi, num, den, min_inliers)["degenerate"][0]) == 0
    epi["best"], epi["n_inliers"] = -1, 77
    got = hrefitref.hrefit_xy(stale, xy, 4, 4.0, epipolar=epi)[0]
    assert (int(got["n_epipolar"][0]), int(got["degenerate"][0])) == (0, 0)


def test_hostile_fixtures_stop_where_they_must():
    seen = {}
    for name, model, mt, qp, tp, d2, want in hrefitref.hostile_fixtures():
        out, info, fl, _ = hrefitref.hrefit(model, mt, qp, tp, 4, d2)
        i = info[0]
        seen[name] = int(i["stop"])
        assert want is None or int(i["stop"]) == want, (name, i)
        assert int(i["n_after"]) >= int(i["n_before"]) and int(out["n_inliers"][0] if int(i["stop"]) != 5 else i["n_after"]) == int(i["n_after"])
        if name == "no model":
            assert out.tobytes() == np.asarray(model).tobytes()
    print("stops:", seen)
    assert set(seen.values()) == {0, 1, 2, 3, 4, 5}
    assert seen["one line"] != 0 and seen["nan H"] != 0 and seen["zero H"] != 0      # (measured: 3, 1, 1)
    i = hrefitref.hrefit(*hrefitref.few_members_pair(4), 4, 4.0)[1][0]
    assert int(i["n_before"]) == 4 and int(i["stop"]) != 1                            # exactly the floor of step 1
    i = hrefitref.hrefit(*hrefitref.few_members_pair(3), 4, 4.0)[1][0]
    assert (int(i["n_before"]), int(i["stop"])) == (3, 1)
    # step 5 alone: a normalisation that overflows, h = 0, and a third row that vanishes at the centroid
    one = np.array([0, 0, 1.0, 0, 0, 1.0])
    assert hrefitref.model_from_h(np.eye(3).reshape(9), one) is not None
    assert hrefitref.model_from_h(np.eye(3).reshape(9), np.array([0, 0, 1e200, 0, 0, 1e-200])) is None
    assert hrefitref.model_from_h(np.zeros(9), one) is None
    assert hrefitref.model_from_h(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 0]), one) is None          # w == 0
    assert hrefitref.model_from_h(np.array([1.0, 0, 0, 0, 0, 0, 0, 0, 1]), one) is None          # singular: wg == 0


SCALE_BOUND, CENTRE_BOUND = 2 * 0.0530, 2 * 0.1541  # DESIGN 5.24's bounds for the chain without the refit (tests/test_hpose_cpu.py)


@pytest.mark.parametrize("seed", [1, 8])
def test_the_plane_chain_runs_with_the_refit_in_it(seed):
    """hposeref.five_plane_frames through homref -> hrefitref -> hposeref -> chainref, no GPU: the refitted models still chain
    into one segment of four linked pairs, within the bounds DESIGN 5.24 set for the chain without the refit; the errors before
    and after are printed (tools/bench_hrefit.py records them for all seeds)."""
    n = 300
    d = hposeref.plane_chain_inputs(seed, n)
    full = hposeref.five_plane_frames(seed, n)[0]
    models = d["models"].copy()
    for j in range(4):
        out, info, _, _ = hrefitref.hrefit(models[j:j + 1], full[j], d["query"][j], d["train"][j], 4, 4.0)
        assert int(info["n_after"][0]) >= int(info["n_before"][0]) == int(models["n_inliers"][j]) and int(out["degenerate"][0]) == 1
        models[j] = out[0]
    errs = []
    for mod in (d["models"], models):
        poses, pts, bits = d["poses"].copy(), d["points"].copy(), d["bits"].copy()
        info, _ = hposeref.fill(mod, d["matches"], d["counts"], d["query"], d["train"], K, poses, pts, bits)
        assert (info["kind"] == capi.HPOSE_PLANE).all() and (poses["best"] >= 0).all()
        chain = chainref.chain(poses, d["matches"], d["counts"], pts, bits, n, 16)[0]
        assert chain["valid"].tolist() == [1, 1, 1, 1] and chain["segment"].tolist() == [0, 0, 0, 0] and chain["linked"].tolist() == [0, 1, 1, 1]
        B, scale_err, centre_err = hposeref.BASELINES, 0.0, 0.0
        for j in range(4):
            true_scale = B[j] / B[0]
            scale_err = max(scale_err, abs(chain["scale"][j] - true_scale) / true_scale)
            for (R, t), C_ in ((d["cams"][j], chain["C"][j]), (d["cams"][j + 1], chain["Ct"][j])):
                centre_err = max(centre_err, np.abs(C_ - (-R.T @ t) / B[0]).max())
        errs.append((scale_err, centre_err))
    print(f"plane chain seed {seed} n {n}: worst relative scale error {errs[0][0]:.4f} -> {errs[1][0]:.4f}, worst centre error {errs[0][1]:.4f} -> {errs[1][1]:.4f}")
    assert errs[1][0] <= SCALE_BOUND and errs[1][1] <= CENTRE_BOUND

"""Descriptor matching without a GPU: the C ABI's new symbols, struct layouts and argument checks, and the CPU restatement
of the matcher's arithmetic itself (tests/matchref.py), which the GPU tests compare against byte for byte."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import matchref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, HIP = -1, -2


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


def test_match_symbols_are_exported_by_both_libraries(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_match_dev", "vslam_match_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    assert b"k_desc_norms" in names and b"k_match_nn2" in names
    assert lib.vslam_version() == 200


def test_match_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    structs = {"vslam_nn2": capi.Nn2, "vslam_match": capi.Match, "vslam_desc_sets": capi.DescSets, "vslam_match_out": capi.MatchOut}
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
    assert rows["vslam_nn2"][0] == 12 and rows["vslam_match"][0] == 12
    assert capi.NN2_DTYPE.itemsize == 12 and capi.MATCH_DTYPE.itemsize == 12


class Args:
    """A valid vslam_match_dev call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, cap=8, match_cap=4):
        self.keep = [np.zeros((n_pairs, cap, 128), np.float32), np.zeros(n_pairs, np.uint32), np.zeros((n_pairs, cap), capi.POINT_DTYPE),
                     np.zeros((n_pairs, cap), capi.NN2_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE), np.zeros(n_pairs, np.uint32)]
        d, c, p, nn, m, mc = self.keep
        assert d.ctypes.data % 16 == 0
        self.q = capi.DescSets(d.ctypes.data, None, p.ctypes.data, c.ctypes.data, cap)
        self.t = capi.DescSets(d.ctypes.data, None, p.ctypes.data, c.ctypes.data, cap)
        self.out = capi.MatchOut(C.sizeof(capi.MatchOut), nn.ctypes.data, nn.nbytes, m.ctypes.data, m.nbytes, mc.ctypes.data, mc.nbytes, match_cap)
        self.n_pairs, self.ratio2, self.same_octave = n_pairs, 0.64, 1

    def call(self, lib, q="q", t="t", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return lib.vslam_match_dev(None, ref(q), ref(t), self.n_pairs, self.ratio2, self.same_octave, ref(out))


def test_match_dev_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    gpu = torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(lib) == (INVALID if gpu else HIP)
    assert Args().call(lib, q=None) == INVALID and Args().call(lib, t=None) == INVALID and Args().call(lib, out=None) == INVALID

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
        return a.call(lib)

    assert bad(out__struct_size=C.sizeof(capi.MatchOut) - 8) == INVALID
    assert bad(out__nn_bytes=2 * 8 * 12 - 1) == INVALID
    assert bad(out__matches_bytes=2 * 4 * 12 - 1) == INVALID
    assert bad(out__match_counts_bytes=7) == INVALID
    assert bad(out__match_counts=None) == INVALID                      # matches without match_counts
    assert bad(out__nn=None, out__matches=None, out__match_counts=None) == INVALID   # no output at all
    assert bad(q__points=None) == INVALID and bad(t__points=None) == INVALID       # same_octave without points
    assert bad(q__desc=None) == INVALID and bad(t__counts=None) == INVALID and bad(q__cap=0) == INVALID
    assert bad(a__n_pairs=-1) == INVALID
    for r in (0.0, -0.64, float("nan"), float("inf")):
        assert bad(a__ratio2=r) == INVALID
    if not gpu:
        assert bad(q__points=None, t__points=None, a__same_octave=0) == HIP  # points are optional without same_octave
        assert bad(out__nn=None, out__nn_bytes=0) == HIP and bad(a__n_pairs=0) == HIP


def test_match_host_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    q, t = np.zeros((3, 128), np.float32), np.zeros((4, 128), np.float32)
    nn, m, total = np.zeros(3, capi.NN2_DTYPE), np.zeros(3, capi.MATCH_DTYPE), C.c_size_t()
    pts = np.zeros(4, capi.POINT_DTYPE)

    def call(qp=q.ctypes.data, ratio2=0.64, same=0, points=None, nnp=nn.ctypes.data, mp=m.ctypes.data, tot=C.byref(total)):
        return lib.vslam_match_host(None, qp, None, points, 3, t.ctypes.data, None, points, 4, ratio2, same, nnp, mp, 3, tot)

    assert call() == (INVALID if torch.cuda.is_available() else HIP)
    assert call(qp=None) == INVALID and call(ratio2=0.0) == INVALID and call(ratio2=float("nan")) == INVALID
    assert call(same=1) == INVALID and call(nnp=None, mp=None, tot=None) == INVALID and call(tot=None) == INVALID
    if not torch.cuda.is_available():
        assert call(same=1, points=pts.ctypes.data) == HIP


# ---- the restatement itself

def chain_bound(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return 130 * 2.0 ** -24 * ((a * a).sum() + (b * b).sum() + 2 * np.abs(a * b).sum())


def test_restatement_agrees_with_float64_within_the_chain_bound():
    rng = np.random.default_rng(1)
    rows = [matchref.reference_like_descriptors(rng, 40), rng.normal(0, 1, (40, 128)).astype(np.float32),
            (rng.normal(0, 1, (40, 128)) * 10.0 ** rng.integers(-6, 6, (40, 1))).astype(np.float32)]
    for d in rows:
        for i in range(0, 40, 2):
            a, b = d[i], d[i + 1]
            exact = ((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum()
            assert abs(float(matchref.d2(a, b)) - exact) <= chain_bound(a, b)
            assert matchref.d2(a, a) == 0.0
    near = rows[0][0].copy()
    near[5] = np.nextafter(near[5], np.float32(2))
    assert abs(float(matchref.d2(rows[0][0], near))) <= chain_bound(rows[0][0], near)  # may be slightly negative: no clamp


def test_restatement_selection_rules():
    rng = np.random.default_rng(2)
    d = matchref.reference_like_descriptors(rng, 50)
    nn, m = matchref.match(d, d)  # identical sets
    assert (nn["index"] == np.arange(50)).all() and (nn["dist2"] == 0.0).all() and (nn["second_dist2"] > 0).all()
    assert (m["query"] == np.arange(50)).all() and (m["train"] == np.arange(50)).all()
    t = d.copy()
    t[30] = t[7]
    t[40] = t[7]  # duplicated train rows tie to the lower index, and the ratio test rejects the query (0 < r * 0 is false)
    nn, m = matchref.match(d[7:8], t)
    assert (nn[0]["index"], nn[0]["dist2"], nn[0]["second_dist2"]) == (7, 0.0, 0.0) and len(m) == 0
    t[3] = np.nan
    q = d[:10].copy()
    q[2] = np.nan  # NaN rows never match, on either side
    nn, m = matchref.match(q, t)
    assert nn[2]["index"] == -1 and np.isinf(nn[2]["dist2"]) and (nn["index"] != 3).all() and 2 not in m["query"]
    nn, m = matchref.match(d[:4], np.zeros((0, 128), np.float32))  # empty train set
    assert (nn["index"] == -1).all() and np.isinf(nn["dist2"]).all() and np.isinf(nn["second_dist2"]).all() and len(m) == 0
    nn, m = matchref.match(np.zeros((0, 128), np.float32), d)
    assert len(nn) == 0 and len(m) == 0
    nn, m = matchref.match(d[:4], d[:1])  # one candidate: second stays +inf, accepted
    assert (nn["index"] == 0).all() and np.isinf(nn["second_dist2"]).all() and len(m) == 4
    # skipped rows: undefined on either side, other octaves
    df = np.ones(50, np.uint8)
    df[7] = 0
    nn, _ = matchref.match(d[:10], d, t_defined=df, q_defined=df[:10])
    assert nn[7]["index"] == -1 and (nn["index"][:7] == np.arange(7)).all()
    nn, _ = matchref.match(d[5:9], d, t_defined=df)
    assert nn[2]["index"] != 7 and nn[2]["dist2"] > 0
    oc = np.arange(50, dtype=np.int32) % 3
    nn, _ = matchref.match(d[:9], d + np.float32(0.25), same_octave=True, q_octave=(oc[:9] + 1) % 3, t_octave=oc)
    assert ((nn["index"] % 3) == (oc[:9] + 1) % 3).all()

"""Place recognition without a GPU: the C ABI's new symbols, struct layouts and argument checks, the host sizing under the
sanitizers, the Python and C++ wrappers' own checks, and the CPU restatement of the section (tests/placeref.py), which the GPU
tests compare against byte for byte: every rule of the Place paragraph on hand-made histograms, the restatement against a plain
float bag of words, planted revisits over 16 seeds, and 17 crops of the reference's images through the CPU oracle."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import matchref, placeref, refimg
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
ENTRY_POINTS = ("vslam_vocab_sample_dev", "vslam_words_dev", "vslam_words_host", "vslam_place_dev", "vslam_place_host")
KERNELS = (b"k_vocab_gather", b"k_words_nn", b"k_words_merge", b"k_place_df", b"k_place_self", b"k_place_score", b"k_place_top", b"k_desc_norms")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- ABI

def test_place_symbols_kernel_names_and_version(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in KERNELS:
        assert k in names
    assert lib.vslam_version() == 200


def test_place_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {"]
    want = []
    structs = (("vslam_words_out", capi.WordsOut), ("vslam_place_cand", capi.PlaceCand), ("vslam_place_params", capi.PlaceParams), ("vslam_place_out", capi.PlaceOut))
    for cname, ct in structs:
        lines += [f'  printf("%zu", sizeof({cname}));'] + [f'  printf(" %zu", offsetof({cname}, {f[0]}));' for f in ct._fields_] + ['  printf("\\n");']
        want.append([C.sizeof(ct)] + [getattr(ct, f[0]).offset for f in ct._fields_])
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines) + "\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [[int(v) for v in l.split()] for l in subprocess.run([str(exe)], capture_output=True, text=True).stdout.splitlines()]
    assert rows == want
    assert [r[0] for r in rows] == [56, 12, 24, 104]
    assert capi.PLACE_CAND_DTYPE.itemsize == 12 and [capi.PLACE_CAND_DTYPE.fields[n][1] for n in ("frame", "score", "norm")] == rows[1][1:]


class Mem:
    """Host arrays a valid call points at (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self):
        self.desc = np.zeros((3, 50, 128), np.float32)
        self.vocab = np.zeros((100, 128), np.float32)
        self.u32 = np.zeros(3 * 50 * 100, np.uint32)
        self.u8 = np.zeros(100, np.uint8)
        assert self.desc.ctypes.data % 16 == 0 and self.vocab.ctypes.data % 16 == 0
        self.S = capi.DescSets(self.desc.ctypes.data, None, None, self.u32.ctypes.data, 50)


def test_vocab_sample_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    m = Mem()

    def call(sets=True, n_sets=3, K=100, vocab=m.vocab.ctypes.data, vbytes=100 * 512, vdef=m.u8.ctypes.data, dbytes=100, **s):
        S = capi.DescSets(m.S.desc, None, None, m.S.counts, 50)
        for k, v in s.items():
            setattr(S, k, v)
        return lib.vslam_vocab_sample_dev(None, C.byref(S) if sets else None, n_sets, K, vocab, vbytes, vdef, dbytes)

    assert call() == (INVALID if torch.cuda.is_available() else HIP)
    assert call(sets=False) == INVALID and call(vocab=None) == INVALID and call(vdef=None) == INVALID
    assert call(n_sets=0) == INVALID and call(n_sets=65536) == INVALID and call(K=0) == INVALID and call(K=65537) == INVALID
    assert call(desc=None) == INVALID and call(counts=None) == INVALID and call(cap=0) == INVALID and call(desc=m.desc.ctypes.data + 4) == INVALID
    assert call(vocab=m.vocab.ctypes.data + 8) == INVALID and call(vbytes=100 * 512 - 1) == INVALID and call(dbytes=99) == INVALID
    if not torch.cuda.is_available():
        assert call(n_sets=65535, K=1, vbytes=512, dbytes=1) == HIP


def words_out(m, **change):
    o = capi.WordsOut(C.sizeof(capi.WordsOut), m.u32.ctypes.data, 3 * 50 * 4, m.desc.ctypes.data, 3 * 50 * 4, m.u32.ctypes.data, 3 * 100 * 4)
    for k, v in change.items():
        setattr(o, k, v)
    return o


def test_words_dev_and_host_reject_bad_arguments_before_they_need_a_gpu(lib):
    import torch

    m = Mem()
    gpu = torch.cuda.is_available()

    def dev(sets=True, n_sets=3, vocab=m.vocab.ctypes.data, K=100, out=True, s={}, **o):
        S = capi.DescSets(m.S.desc, None, None, m.S.counts, 50)
        for k, v in s.items():
            setattr(S, k, v)
        return lib.vslam_words_dev(None, C.byref(S) if sets else None, n_sets, vocab, None, K, C.byref(words_out(m, **o)) if out else None)

    def host(desc=m.desc.ctypes.data, counts=m.u32.ctypes.data, cap=50, n_sets=3, vocab=m.vocab.ctypes.data, K=100, out=True, **o):
        return lib.vslam_words_host(None, desc, None, counts, cap, n_sets, vocab, None, K, C.byref(words_out(m, **o)) if out else None)

    assert dev() == (INVALID if gpu else HIP) and host() == (INVALID if gpu else HIP)
    assert dev(sets=False) == INVALID and dev(vocab=None) == INVALID and dev(out=False) == INVALID
    assert dev(struct_size=48) == INVALID and dev(n_sets=-1) == INVALID and dev(n_sets=65536) == INVALID and dev(K=0) == INVALID and dev(K=65537) == INVALID
    assert dev(s=dict(desc=None)) == INVALID and dev(s=dict(counts=None)) == INVALID and dev(s=dict(cap=0)) == INVALID
    assert dev(s=dict(desc=m.desc.ctypes.data + 4)) == INVALID and dev(vocab=m.vocab.ctypes.data + 4) == INVALID
    assert dev(words=None, word_dist2=None, hist=None) == INVALID
    assert dev(words_bytes=3 * 50 * 4 - 1) == INVALID and dev(word_dist2_bytes=3 * 50 * 4 - 1) == INVALID and dev(hist_bytes=3 * 100 * 4 - 1) == INVALID
    assert host(desc=None) == INVALID and host(counts=None) == INVALID and host(cap=0) == INVALID and host(vocab=None) == INVALID and host(out=False) == INVALID
    assert host(struct_size=0) == INVALID and host(n_sets=-1) == INVALID and host(K=0) == INVALID and host(words=None, word_dist2=None, hist=None) == INVALID
    assert host(words_bytes=0) == INVALID and host(word_dist2_bytes=0) == INVALID and host(hist_bytes=0) == INVALID
    if not gpu:  # each optional output may be absent, no sets is a valid call, host arrays need no alignment
        assert dev(words=None) == HIP and dev(word_dist2=None, hist=None) == HIP and dev(n_sets=0) == HIP and dev(K=65536, hist=None) == HIP
        assert host(desc=m.desc.ctypes.data + 4, vocab=m.vocab.ctypes.data + 4) == HIP and host(hist=None) == HIP and host(n_sets=0) == HIP


def test_place_dev_and_host_reject_bad_arguments_before_they_need_a_gpu(lib):
    import torch

    m = Mem()
    gpu = torch.cuda.is_available()
    u = m.u32.ctypes.data

    def make(fn):
        def call(hq=u, nq=20, q_first=7, hd=u, nd=30, db_first=0, K=100, params=True, out=True, p={}, **o):
            P = capi.PlaceParams(4, 3, 1, 5, 0, 0)
            for k, v in p.items():
                setattr(P, k, v)
            O = capi.PlaceOut(C.sizeof(capi.PlaceOut), u, 20 * 3 * 12, u, 20 * 4, u, 100 * 4, u, 20 * 4, u, 30 * 4, u, 20 * 30 * 4)
            for k, v in o.items():
                setattr(O, k, v)
            return fn(None, hq, nq, q_first, hd, nd, db_first, K, C.byref(P) if params else None, C.byref(O) if out else None)
        return call

    for call in (make(lib.vslam_place_dev), make(lib.vslam_place_host)):
        assert call() == (INVALID if gpu else HIP)
        assert call(params=False) == INVALID and call(out=False) == INVALID and call(hq=None) == INVALID and call(hd=None) == INVALID
        assert call(struct_size=96) == INVALID and call(nq=65536) == INVALID and call(nd=65536) == INVALID and call(K=0) == INVALID and call(K=65537) == INVALID
        assert call(q_first=2 ** 31 - 19) == INVALID and call(db_first=2 ** 32 - 1) == INVALID
        assert call(p=dict(max_candidates=0)) == INVALID and call(p=dict(max_candidates=9)) == INVALID and call(p=dict(den=0)) == INVALID
        assert call(p=dict(reserved=1)) == INVALID
        assert call(candidates=None, cand_counts=None, weights=None, self_q=None, self_db=None, scores=None) == INVALID
        assert call(cand_counts=None) == INVALID and call(p=dict(max_candidates=4)) == INVALID
        for name, need in (("candidates", 20 * 3 * 12), ("cand_counts", 80), ("weights", 400), ("self_q", 80), ("self_db", 120), ("scores", 2400)):
            assert call(**{name + "_bytes": need - 1}) == INVALID, name
        if not gpu:
            assert call(nq=0, hq=None) == HIP and call(nd=0, hd=None) == HIP and call(q_first=2 ** 31 - 20) == HIP
            assert call(candidates=None, cand_counts=None, weights=None, self_q=None, self_db=None) == HIP  # scores alone
            assert call(candidates=None, scores=None) == HIP and call(p=dict(min_gap=2 ** 32 - 1, num=2 ** 32 - 1, min_score=2 ** 32 - 1)) == HIP


SIZES_BY_HAND = {  # (cap, K, sets) -> qtiles, ttiles, nsplit, qrow_blocks, part_bytes, hist_elems
    (1, 1, 1): (1, 1, 1, 1, 8, 1),
    (129, 65, 1): (2, 2, 2, 1, 2 * 129 * 8, 65),
    (2000, 4096, 1): (16, 64, 16, 8, 16 * 2000 * 8, 4096),              # one small set against 4096 words: 16 workgroups share its tiles
    (4000, 1024, 256): (32, 16, 1, 16, 256 * 4000 * 8, 256 * 1024),      # 8192 workgroups fill the chip: no split
    (2 ** 32 - 1, 65536, 65535): (2 ** 25, 1024, 1, 2 ** 24, 65535 * (2 ** 32 - 1) * 8, 65535 * 65536),
}


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "place_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines() if not l.startswith("size")}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 19 * 18 * 13 * 7 + 18 * (2 + 12 * 12 * 5), rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) == 103, rows["args"]  # (every message and the order of the checks are among them)
    sizes = {}
    for l in out.stdout.splitlines():
        if l.startswith("size"):
            w = l.split()
            sizes[tuple(int(v) for v in w[1:4])] = tuple(int(x.split("=")[1]) for x in w[4:])
    assert sizes == SIZES_BY_HAND
    src = open(os.path.join(CSRC, "vslam_place_plan.h")).read()  # the header under test is plain host code
    assert "#include <hip" not in src and "__global__" not in src


# ---- the Python wrappers over CPU tensors, the library replaced by a recorder

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
    import torch

    rec = Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    c = object.__new__(capi.Context)
    c._h, c.device, c.where, c.rec = None, 0, torch.device("cpu"), rec
    return c


def test_python_wrappers_pass_valid_calls_on_and_refuse_bad_tensors(ctx):
    import torch

    n, cap, K = 3, 50, 64
    S = capi.DescSets(0, None, None, 0, cap)
    S.n = n
    vocab, vdef = torch.zeros(K, 128), torch.zeros(K, dtype=torch.uint8)
    ctx.vocab_sample(S, vocab, vdef)
    (name, args), = ctx.rec.calls
    assert name == "vslam_vocab_sample_dev" and args[2:] == (n, K, vocab.data_ptr(), K * 512, vdef.data_ptr(), K)
    ctx.rec.calls.clear()
    t = dict(words=torch.zeros(n, cap, dtype=torch.int32), word_dist2=torch.zeros(n, cap), hist=torch.zeros(n, K, dtype=torch.int32))
    ctx.words(S, vocab, vdef, **t)
    (name, args), = ctx.rec.calls
    assert name == "vslam_words_dev" and args[2:6] == (n, vocab.data_ptr(), vdef.data_ptr(), K)
    out = args[-1]._obj
    want = {"struct_size": C.sizeof(capi.WordsOut)}
    for k, v in t.items():
        want[k], want[k + "_bytes"] = v.data_ptr(), v.numel() * 4
    assert {f: getattr(out, f) for f, _ in out._fields_} == want
    ctx.rec.calls.clear()
    ctx.words(S, vocab, None, 2, hist=t["hist"])  # one output alone, no vocab_defined
    args = ctx.rec.calls[0][1]
    assert args[2] == 2 and args[4] is None and (args[-1]._obj.words, args[-1]._obj.word_dist2) == (None, None)
    ctx.rec.calls.clear()
    with pytest.raises(ValueError, match="words: hist must be a contiguous tensor on cpu"):
        ctx.words(S, vocab, hist=t["hist"][:, ::2])
    with pytest.raises(ValueError, match="words: vocab is required"):
        ctx.words(S, None, hist=t["hist"])
    with pytest.raises(ValueError, match=r"words: vocab must be float32 \[K, 128\]"):
        ctx.words(S, torch.zeros(K, 64), hist=t["hist"])
    with pytest.raises(ValueError, match="words: words must have 4-byte elements"):
        ctx.words(S, vocab, words=torch.zeros(n, cap, dtype=torch.int64))
    with pytest.raises(ValueError, match="words: no output requested"):
        ctx.words(S, vocab)
    with pytest.raises(ValueError, match="words: fewer sets than pairs"):
        ctx.words(S, vocab, hist=torch.zeros(n, K - 1, dtype=torch.int32))
    with pytest.raises(ValueError, match="vocab_sample: vocab_defined is required"):
        ctx.vocab_sample(S, vocab, None)
    assert ctx.rec.calls == []
    hq, hd = torch.zeros(5, K, dtype=torch.int32), torch.zeros(9, K, dtype=torch.int32)
    o = dict(candidates=torch.zeros(5, 2, 3, dtype=torch.int32), cand_counts=torch.zeros(5, dtype=torch.int32), scores=torch.zeros(5, 9, dtype=torch.int32))
    ctx.place(hq, hd, q_first=20, db_first=3, min_gap=4, max_candidates=2, num=1, den=5, min_score=7, **o)
    (name, args), = ctx.rec.calls
    assert name == "vslam_place_dev" and args[1:8] == (hq.data_ptr(), 5, 20, hd.data_ptr(), 9, 3, K)
    P, O = args[8]._obj, args[9]._obj
    assert [getattr(P, f) for f, _ in P._fields_] == [4, 2, 1, 5, 7, 0]
    assert (O.candidates, O.candidates_bytes, O.cand_counts_bytes, O.scores_bytes, O.weights, O.self_q, O.self_db) == (o["candidates"].data_ptr(), 120, 20, 180, None, None, None)
    ctx.rec.calls.clear()
    ctx.place(hq, cand_counts=o["cand_counts"])  # one buffer searched in itself
    args = ctx.rec.calls[0][1]
    assert args[1] == args[4] == hq.data_ptr() and args[2] == args[5] == 5
    ctx.rec.calls.clear()
    with pytest.raises(ValueError, match="place: no output requested"):
        ctx.place(hq, hd)
    with pytest.raises(ValueError, match="place: candidates needs cand_counts"):
        ctx.place(hq, hd, candidates=o["candidates"])
    with pytest.raises(ValueError, match="place: hist_q and hist_db must be"):
        ctx.place(hq, torch.zeros(9, K + 1, dtype=torch.int32), cand_counts=o["cand_counts"])
    with pytest.raises(ValueError, match="place: scores must be a contiguous tensor on cpu"):
        ctx.place(hq, hd, scores=torch.zeros(5, 18, dtype=torch.int32)[:, ::2])
    assert ctx.rec.calls == []


def test_python_host_wrappers_shape_their_buffers(ctx):
    desc, vocab = np.zeros((2, 7, 128), np.float32), np.zeros((9, 128), np.float32)
    w, d, h = ctx.words_host(desc, [7, 3], vocab, vocab_defined=np.ones(9, np.uint8), fill=-5)
    (name, args), = ctx.rec.calls
    assert name == "vslam_words_host" and args[4:6] == (7, 2) and args[2] is None and args[7] is not None and args[8] == 9
    assert (w.shape, w.dtype, d.shape, h.shape, h.dtype) == ((2, 7), np.int32, (2, 7), (2, 9), np.uint32) and (w == -5).all() and np.isnan(d).all()
    with pytest.raises(ValueError, match="one count per set"):
        ctx.words_host(desc, [7], vocab)
    with pytest.raises(ValueError, match="one entry per descriptor row"):
        ctx.words_host(desc, [7, 3], vocab, defined=np.ones(13, np.uint8))
    ctx.rec.calls.clear()
    r = ctx.place_host(np.zeros((4, 9), np.uint32), max_candidates=2, want_scores=False)
    (name, args), = ctx.rec.calls
    assert name == "vslam_place_host" and args[2] == args[5] == 4 and args[7] == 9 and r["scores"] is None
    assert r["candidates"].shape == (4, 2) and r["candidates"].dtype == capi.PLACE_CAND_DTYPE and (r["candidates"]["frame"] == -1).all()


# ---- the C++ wrappers

def build_cxx_driver(tmp_path):
    """tests/place_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_place.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "place_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "place_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrappers_refuse_bad_lists_and_answer_no_hip_device_without_a_gpu(tmp_path):
    import torch

    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = build_cxx_driver(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = subprocess.run([exe, "--valid"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"status {0 if torch.cuda.is_available() else HIP}", r.stdout + r.stderr
    assert os.path.exists(os.path.join(ROOT, "visualslam_amd", "bin", "Place"))


# ---- the rules, on hand-made histograms: what each case must give, worked out by hand

def cands(r, i):
    return [tuple(int(v) for v in c) for c in r["candidates"][i, : r["cand_counts"][i]]]


def run_case(name):
    return placeref.place(**placeref.rule_cases()[name])


def test_rule_document_frequency_0_1_and_nd():
    r = run_case("df")
    assert r["weights"].tolist() == [0, 3, 1]  # in no frame; in 1 of 4: bitlen(4) = 3; in all 4: bitlen(1) = 1
    assert r["self_q"].tolist() == [2 * 3 + 1, 1, 5, 1] and r["scores"].tolist() == [[7, 1, 1, 1], [1, 1, 1, 1], [1, 1, 5, 1], [1, 1, 1, 1]]
    assert cands(r, 3) == [(1, 1, 1), (2, 1, 5), (0, 1, 7)]  # 1/1 > 1/5 > 1/7


def test_rule_a_tie_goes_to_the_lower_frame_and_c_cuts_the_list():
    r = run_case("tie")
    assert cands(r, 2) == [(0, 6, 20), (1, 6, 20)] and cands(r, 1) == [(0, 6, 6)] and cands(r, 0) == []
    assert [cands(run_case("c1"), i) for i in (3, 5)] == [[(0, 10, 10)], [(0, 10, 10)]]


def test_rule_acceptance_boundary_and_min_score():
    r = run_case("boundary")  # num / den = 2 / 5
    assert cands(r, 3) == [(0, 10, 10), (1, 4, 10)]  # 4 * 5 == 2 * 10 is in; frame 2 with 3 * 5 < 2 * 10 is not
    assert cands(r, 5) == [(0, 10, 10), (3, 10, 10), (1, 4, 10)] and cands(r, 2) == [(1, 3, 4)] and cands(r, 4) == []
    r = run_case("min_score")
    assert cands(r, 2) == [] and cands(r, 3) == [(0, 10, 10), (1, 4, 10)]  # S = 3 < 4 although 3 / 4 is high; S = 4 is in


def test_rule_an_empty_frame_has_no_candidate_and_divides_nothing():
    r = run_case("empty")
    assert r["self_q"].tolist() == [0, 0, 9, 0]
    assert cands(r, 1) == []                      # N = max(0, 0) = 0: not accepted, whatever num is
    assert cands(r, 2) == [(0, 0, 9), (1, 0, 9)]  # N = 9 > 0 and num = 0: accepted with score 0, the lower frame first
    assert cands(r, 3) == [(2, 0, 9)]


def test_rule_min_gap_regimes_and_fewer_eligible_than_c():
    g0, g1, gl, few = run_case("gap0"), run_case("gap1"), run_case("gap_large"), run_case("few_eligible")
    assert g0["cand_counts"].tolist() == [1, 2, 3, 4, 4, 6] and cands(g0, 0) == [(0, 10, 10)]  # min_gap 0: a frame is its own best candidate
    assert g0["cand_counts"][4] == 4                        # the empty frame against itself: N = 0
    assert g1["cand_counts"].tolist() == [0, 1, 2, 3, 4, 5] and gl["cand_counts"].tolist() == [0] * 6
    assert few["cand_counts"].tolist() == [0, 0, 0, 0, 1, 2] and cands(few, 5) == [(0, 10, 10), (1, 4, 10)]
    assert all(g0[k].tobytes() == gl[k].tobytes() for k in ("weights", "self_q", "self_db", "scores"))  # scores are written for every pair


def test_rule_saturation_with_entries_of_2_to_32_minus_1():
    r = run_case("saturation")
    top = 2 ** 31 - 1
    assert (r["scores"] == top).all() and (r["self_q"] == top).all() and cands(r, 3) == [(0, top, top), (1, top, top), (2, top, top)]


def test_rule_two_buffers_with_their_own_offsets():
    r = run_case("two_buffers")  # db frames 96 .. 100, query frames 100, 101, min_gap 3: eligible 96, 97 / 96, 97, 98
    assert r["weights"].tolist() == [1, 1, 1, 1] and r["self_db"].tolist() == [7, 4, 5, 36, 8]
    assert cands(r, 0) == [(96, 7, 8), (97, 3, 8)] and cands(r, 1) == [(98, 5, 6), (97, 2, 6), (96, 2, 7)]
    assert run_case("db_after")["cand_counts"].tolist() == [0, 0]
    e = run_case("empty_db")
    assert e["cand_counts"].tolist() == [0] and e["weights"].tolist() == [0] * 4 and e["self_q"].tolist() == [0] and e["scores"].shape == (1, 0)


def test_rule_the_nan_row_and_the_dead_word():
    rng = np.random.default_rng(3)
    vocab = matchref.crafted(rng, 20)
    d = np.stack([vocab[4], vocab[4], vocab[7], np.full(128, np.nan, np.float32), vocab[9], vocab[11]])
    vocab[9, 100] = np.nan  # a dead word: row 4 was its exact copy
    vocab[12] = vocab[4]    # a duplicate: never selected
    vdef = np.ones(20, np.uint8)
    vdef[11] = 0
    w, dist, hist = placeref.words(d[None], [6], vocab, np.ones((1, 6), np.uint8), vdef)
    assert w[0].tolist()[:4] == [4, 4, 7, -1] and np.isposinf(dist[0, 3]) and dist[0, 0] == 0.0
    assert w[0, 4] not in (-1, 9) and w[0, 5] not in (-1, 11) and hist[0, [9, 11, 12]].sum() == 0 and hist[0, 4] == 2 and hist[0].sum() == 5


# ---- the restatement against a plain float bag of words

def float_bow(hq, hd, min_gap):
    """idf = the integer weights as floats; histogram intersection over max of the two self-scores, in f64."""
    hq, hd = hq.astype(np.float64), hd.astype(np.float64)
    df = (hd > 0).sum(axis=0)
    w = np.array([0.0 if x == 0 else float(int(len(hd) // x).bit_length()) for x in df])
    S = np.minimum(hq[:, None, :], hd[None, :, :]) @ w
    N = np.maximum((hq @ w)[:, None], (hd @ w)[None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(N > 0, S / N, -1.0)
    for i in range(len(hq)):
        ratio[i, max(i - min_gap + 1, 0):] = -1.0
    return ratio


def test_restatement_ranks_like_a_float_bag_of_words_where_the_margin_exceeds_rounding():
    rng = np.random.default_rng(21)
    h = (rng.integers(1, 9, (30, 200)) * (rng.random((30, 200)) < 0.25)).astype(np.uint32)
    h[20:] = np.maximum(h[:10] // 2, (rng.random((10, 200)) < 0.05).astype(np.uint32))  # revisits
    r = placeref.place(h, None, min_gap=3, max_candidates=8, num=0, den=1)
    ratio = float_bow(h, h, 3)
    compared = 0
    for i in range(30):
        got = [c[0] for c in cands(r, i)]
        order = np.argsort(-ratio[i], kind="stable")
        order = [int(j) for j in order if ratio[i, j] >= 0][:8]
        assert len(got) == len(order)
        # S and N are integers below 2^20 here: the f64 quotients are within 2^-52 relative, so two frames whose quotients differ by more
        # than 1e-12 are ordered alike on both sides; closer ones (exact ties) go to the lower frame in the restatement
        for a, b in zip(got, order):
            if a != b:
                assert abs(ratio[i, a] - ratio[i, b]) <= 1e-12, (i, got, order)
            compared += 1
    assert compared > 150


# ---- planted revisits

def test_planted_revisits_separate_at_4096_words_over_16_seeds():
    """32 frames of 12 places (placeref.revisit_scene), K = 4096 words sampled by the vocabulary rule, min_gap 4, c = 2.  Measured
    with the restatement over the 16 seeds: the lowest S / N of a true first candidate is 0.2672, of any true eligible pair
    0.2434; the highest of any untrue eligible pair is 0.1360.  num / den = 1 / 5 lies between them."""
    lo_first, lo_true, hi_false = 9.0, 9.0, 0.0
    for seed in range(16):
        desc, counts, seq = placeref.revisit_scene(seed)
        assert len(seq) == 32 and seq[24:] == [0, 0, 1, 1, 2, 2, 3, 3]
        vocab, vdef = placeref.vocab_sample(desc, counts, 4096)
        _, _, hist = placeref.words(desc, counts, vocab, None, vdef)
        r = placeref.place(hist, None, min_gap=4, max_candidates=2, num=1, den=5)
        sq, sd, sc = r["self_q"], r["self_db"], r["scores"]
        for i in range(32):
            truth = [j for j in range(32) if j + 4 <= i and seq[j] == seq[i]]
            for j in range(32):
                if j + 4 <= i and max(sq[i], sd[j]) > 0:
                    x = int(sc[i, j]) / max(int(sq[i]), int(sd[j]))
                    if j in truth:
                        lo_true = min(lo_true, x)
                    else:
                        hi_false = max(hi_false, x)
            got = cands(r, i)
            assert sorted(c[0] for c in got) == truth, (seed, i, got, truth)  # at this threshold the accepted set is exactly the true set
            if i >= 24:
                assert len(truth) == 2 and seq[got[0][0]] == seq[i]
                lo_first = min(lo_first, got[0][1] / got[0][2])
    print("planted revisits, K = 4096, 16 seeds: lowest true first candidate %.4f, lowest true pair %.4f, highest untrue eligible pair %.4f" % (lo_first, lo_true, hi_false))
    assert lo_first > hi_false and lo_true > 0.2 > hi_false


# ---- real images through the CPU oracle

CROPS = [("building", 0, 0), ("building", 24, 24), ("building", 48, 48), ("home", 0, 0), ("home", 24, 24), ("home", 48, 48), ("blox", 0, 0), ("blox", 24, 24),
         ("blox", 48, 48), ("chessboard", 400, 400), ("chessboard", 424, 424), ("chessboard", 448, 448), ("building", 8, 40), ("building", 40, 8),
         ("building", 64, 64), ("home", 8, 40), ("home", 40, 8)]
REVISITS = {12: [0, 1, 2], 13: [0, 1, 2], 14: [0, 1, 2], 15: [3, 4, 5], 16: [3, 4, 5]}


def crop_sequence():
    return [np.ascontiguousarray(refimg.load(name)[r:r + 384, c:c + 384]) for name, r, c in CROPS]


@functools.lru_cache(maxsize=None)
def crop_descriptors():
    from tests.test_gpu_match import oracle_chain

    got = [oracle_chain(img) for img in crop_sequence()]
    cap = max(len(d) for _, d, _ in got)
    desc, defined = np.zeros((len(got), cap, 128), np.float32), np.zeros((len(got), cap), np.uint8)
    for f, (_, d, ok) in enumerate(got):
        desc[f, : len(d)], defined[f, : len(d)] = d.reshape(-1, 128), ok
    return desc, defined, np.array([len(d) for _, d, _ in got], np.uint32)


def expect_revisits(r):
    """Every revisit frame has exactly its three earlier frames of the same image, every other frame has no candidate."""
    for i in range(len(CROPS)):
        assert sorted(c[0] for c in cands(r, i)) == REVISITS.get(i, []), (i, cands(r, i))


VOCAB_FRAMES = 12  # the vocabulary of the crop sequence comes from the frames before the first revisit


def test_seventeen_crops_each_revisit_gets_exactly_its_three_earlier_frames():
    """K = 256, min_gap 4, the max norm, num / den = 1 / 5, c = 8 (so that "exactly" is shown, not cut).  The vocabulary is sampled
    by the header's rule from the 12 frames that precede the revisits: a vocabulary exists before the frame that is looked up
    arrives, and a frame of 85 descriptors whose own rows are a sixth of the words mostly finds itself.  Measured with the
    restatement: building 0.542-0.645, home 0.218-0.301, the best untrue candidate of a revisit frame 0.150, the best pair of any
    other frame 0.093.  Sampled from all 17 frames instead, the home revisits score 0.167-0.174 (best untrue 0.141): still first
    in rank, but below 1 / 5 - the second half of the test holds that figure."""
    desc, defined, counts = crop_descriptors()
    assert (counts[9:12] == 0).all() and (counts[:9] > 0).all()  # the chessboard crops are the empty frames
    nan_rows = int((np.isnan(desc[0, : counts[0]]).all(axis=1) & (defined[0, : counts[0]] != 0)).sum())
    assert counts[0] == 607 and nan_rows == 4  # all-NaN rows that are flagged defined: real descriptors contain them
    V = VOCAB_FRAMES
    vocab, vdef = placeref.vocab_sample(desc[:V], counts[:V], 256, defined[:V])
    w, _, hist = placeref.words(desc, counts, vocab, defined, vdef)
    assert (w[0, : counts[0]] == -1).sum() >= nan_rows and hist[9:12].sum() == 0
    r = placeref.place(hist, None, min_gap=4, max_candidates=8, num=1, den=5)
    expect_revisits(r)

    def figures(r):
        sq, sc = r["self_q"], r["scores"]
        true, untrue_rev, other = [], 0.0, 0.0
        for i in range(17):
            for j in range(17):
                if j + 4 <= i and max(sq[i], sq[j]) > 0:
                    x = int(sc[i, j]) / max(int(sq[i]), int(sq[j]))
                    if j in REVISITS.get(i, []):
                        true.append((i, round(x, 3)))
                    elif i in REVISITS:
                        untrue_rev = max(untrue_rev, x)
                    else:
                        other = max(other, x)
        return true, untrue_rev, other

    true, untrue_rev, other = figures(r)
    print("17 crops, K = 256, vocabulary from the first 12 frames: true pairs", true,
          "best untrue candidate of a revisit frame %.3f, best of any other frame %.3f" % (untrue_rev, other))
    assert min(x for _, x in true) > 0.2 > max(untrue_rev, other)
    # the same frames with the SMALLER self-score as the norm: an unrelated frame with many descriptors swallows one with few
    sq, sc = r["self_q"], r["scores"]
    worst = max(int(sc[i, j]) / min(int(sq[i]), int(sq[j])) for i in range(17) for j in range(17)
                if j + 4 <= i and min(sq[i], sq[j]) > 0 and CROPS[i][0] != CROPS[j][0])
    print("under min(Sq, Sd) the best pair of two different images scores %.3f" % worst)
    assert worst > 0.5
    # the vocabulary sampled from all 17 frames, the revisits' own rows among the words: the order still holds, the threshold does not
    vocab, vdef = placeref.vocab_sample(desc, counts, 256, defined)
    _, _, hist = placeref.words(desc, counts, vocab, defined, vdef)
    true, untrue_rev, other = figures(placeref.place(hist, None, min_gap=4, max_candidates=8, num=0, den=1))
    print("vocabulary from all 17 frames: true pairs", true, "best untrue %.3f, other %.3f" % (untrue_rev, other))
    home = [x for i, x in true if i >= 15]
    assert min(x for _, x in true) > max(untrue_rev, other) and max(home) < 0.2 < min(x for i, x in true if i < 15)

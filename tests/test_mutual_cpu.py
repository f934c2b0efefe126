"""Mutual matching without a GPU: the C ABI's new symbols, struct layout and argument checks, the host sizing under the
sanitizers, the Python and C++ wrappers' own checks, and the CPU restatement of the rule (tests/mutualref.py), which the GPU tests
compare against byte for byte: its two forms held against each other, what the mutual list is by construction, the ordered key
the device takes its minimum over, and the figures that say what the cross-check is worth."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import guidedref, matchref, mutualref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- ABI

def test_mutual_symbols_kernel_names_and_version(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ("vslam_match_mutual_dev", "vslam_match_mutual_host"):
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in (b"k_match_nn2_mutual", b"k_match_mutual_merge", b"k_match_rnn_write", b"k_match_nn2", b"k_match_merge"):
        assert k in names
    assert lib.vslam_version() == 200


def test_mutual_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {"]
    want = []
    for cname, ct in (("vslam_rnn", capi.Rnn), ("vslam_match_mutual_out", capi.MatchMutualOut)):
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
    assert rows[0][0] == 8 and capi.RNN_DTYPE.itemsize == 8 and [capi.RNN_DTYPE.fields[n][1] for n in ("index", "dist2")] == rows[0][1:]
    assert rows[1][0] == 80


class Args:
    """A valid vslam_match_mutual_dev call over host arrays (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self, n_pairs=2, qcap=50, tcap=60, match_cap=10):
        self.keep = [np.zeros((n_pairs, max(qcap, tcap), 128), np.float32), np.zeros(n_pairs, np.uint32), np.zeros((n_pairs, max(qcap, tcap)), capi.POINT_DTYPE),
                     np.zeros((n_pairs, qcap), capi.NN2_DTYPE), np.zeros((n_pairs, tcap), capi.RNN_DTYPE), np.zeros((n_pairs, match_cap), capi.MATCH_DTYPE),
                     np.zeros(n_pairs, np.uint32)]
        d, cnt, pts, nn, rnn, m, mc = self.keep
        assert d.ctypes.data % 16 == 0
        self.Q = capi.DescSets(d.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, qcap)
        self.T = capi.DescSets(d.ctypes.data, None, pts.ctypes.data, cnt.ctypes.data, tcap)
        self.n_pairs, self.ratio2, self.same_octave = n_pairs, 0.64, 0
        self.out = capi.MatchMutualOut(C.sizeof(capi.MatchMutualOut), nn.ctypes.data, nn.nbytes, rnn.ctypes.data, rnn.nbytes, m.ctypes.data, m.nbytes,
                                       mc.ctypes.data, mc.nbytes, match_cap)

    def call(self, lib, Q="Q", T="T", out="out"):
        ref = lambda x: None if x is None else C.byref(getattr(self, x))
        return lib.vslam_match_mutual_dev(None, ref(Q), ref(T), self.n_pairs, self.ratio2, self.same_octave, ref(out))


def test_mutual_dev_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    gpu = torch.cuda.is_available()
    # a valid call: no context can exist without a GPU, and the answer is the ABI's "no HIP device"; with one, a null context is invalid
    assert Args().call(lib) == (INVALID if gpu else HIP)
    for name in ("Q", "T", "out"):
        assert Args().call(lib, **{name: None}) == INVALID, name

    def bad(**change):
        a = Args()
        for k, v in change.items():
            obj, field = k.split("__")
            setattr(getattr(a, obj), field, v) if obj != "a" else setattr(a, field, v)
        return a.call(lib)

    assert bad(out__struct_size=C.sizeof(capi.MatchOut)) == INVALID  # the matcher's out struct is not this one
    assert bad(a__n_pairs=-1) == INVALID and bad(a__n_pairs=65536) == INVALID
    for r in (0.0, -0.64, float("nan"), float("inf")):
        assert bad(a__ratio2=r) == INVALID
    for s in ("Q", "T"):
        assert bad(**{s + "__desc": None}) == INVALID and bad(**{s + "__counts": None}) == INVALID and bad(**{s + "__cap": 0}) == INVALID
        assert bad(**{s + "__desc": Args().keep[0].ctypes.data + 4}) == INVALID  # misaligned
        assert bad(**{s + "__points": None, "a__same_octave": 1}) == INVALID
    assert bad(out__nn=None, out__rnn=None, out__matches=None, out__match_counts=None) == INVALID
    assert bad(out__nn_bytes=2 * 50 * 12 - 1) == INVALID and bad(out__rnn_bytes=2 * 60 * 8 - 1) == INVALID
    assert bad(out__match_counts=None) == INVALID and bad(out__match_cap=0) == INVALID
    assert bad(out__matches_bytes=2 * 10 * 12 - 1) == INVALID and bad(out__match_counts_bytes=7) == INVALID
    if not gpu:  # the optional outputs may be absent, points are needed with same_octave only, no pairs is a valid call
        assert bad(a__same_octave=1) == HIP and bad(Q__points=None, T__points=None) == HIP
        assert bad(out__nn=None) == HIP and bad(out__rnn=None) == HIP and bad(out__matches=None, out__match_cap=0) == HIP and bad(a__n_pairs=0) == HIP
        assert bad(out__nn=None, out__matches=None, out__match_counts=None, out__match_cap=0) == HIP  # rnn alone


def test_mutual_host_rejects_bad_arguments_before_it_needs_a_gpu(lib):
    import torch

    q, t = np.zeros((5, 128), np.float32), np.zeros((6, 128), np.float32)
    qp, tp = np.zeros(5, capi.POINT_DTYPE), np.zeros(6, capi.POINT_DTYPE)
    nn, rnn, m, total = np.zeros(5, capi.NN2_DTYPE), np.zeros(6, capi.RNN_DTYPE), np.zeros(5, capi.MATCH_DTYPE), C.c_size_t()

    def call(ratio2=0.64, same=0, qd=q.ctypes.data, qpp=qp.ctypes.data, tpp=tp.ctypes.data, nnp=nn.ctypes.data, rp=rnn.ctypes.data, mp=m.ctypes.data, cap=5,
             tot=C.byref(total)):
        return lib.vslam_match_mutual_host(None, qd, None, qpp, 5, t.ctypes.data, None, tpp, 6, ratio2, same, nnp, rp, mp, cap, tot)

    assert call() == (INVALID if torch.cuda.is_available() else HIP)
    assert call(qd=None) == INVALID
    assert call(same=1, qpp=None) == INVALID and call(same=1, tpp=None) == INVALID
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(ratio2=r) == INVALID
    assert call(nnp=None, rp=None, tot=None, mp=None) == INVALID and call(tot=None) == INVALID and call(cap=0) == INVALID
    if not torch.cuda.is_available():
        assert call(mp=None, tot=None) == HIP and call(nnp=None) == HIP and call(rp=None) == HIP and call(qpp=None, tpp=None) == HIP
        assert call(nnp=None, mp=None, tot=None) == HIP  # rnn alone


SIZES_BY_HAND = {  # (query cap, train cap, pairs) -> qtiles, ttiles, nsplit, fwords, qrow_blocks, trow_blocks, part_elems, flag_words, rev_bytes
    (1, 1, 1): (1, 1, 1, 1, 1, 1, 1, 1, 8),
    (64, 64, 1): (1, 1, 1, 1, 1, 1, 64, 1, 512),
    (65, 65, 1): (1, 2, 2, 2, 1, 1, 130, 2, 520),                           # two train tiles: both splits
    (65536, 65536, 1): (512, 1024, 4, 1024, 256, 256, 4 * 65536, 1024, 8 * 65536),  # 512 workgroups: ceil(2048 / 512) splits
    (1, 65, 65535): (1, 2, 1, 1, 1, 1, 65535, 65535, 65535 * 65 * 8),
    (65536, 64, 65535): (512, 1, 1, 1024, 256, 1, 65535 * 65536, 65535 * 1024, 65535 * 64 * 8),
    (1000, 777, 40): (8, 13, 7, 16, 4, 4, 40 * 7 * 1000, 40 * 16, 40 * 777 * 8),   # 320 workgroups: ceil(2048 / 320) = 7 splits
}


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "mutual_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines() if not l.startswith("size")}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) == 21 * 21 * 13 * 10, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) == 54, rows["args"]   # (29 messages and the order of the checks are among them)
    sizes = {}
    for l in out.stdout.splitlines():
        if l.startswith("size"):
            w = l.split()
            sizes[tuple(int(v) for v in w[1:4])] = tuple(int(x.split("=")[1]) for x in w[4:])
    assert sizes == SIZES_BY_HAND
    src = open(os.path.join(CSRC, "vslam_mutual_plan.h")).read()  # the header under test is plain host code
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


def test_python_wrapper_passes_a_valid_call_on_and_refuses_bad_tensors(ctx):
    import torch

    n, qcap, tcap, mcap = 3, 50, 60, 10
    Q, T = capi.DescSets(0, None, None, 0, qcap), capi.DescSets(0, None, None, 0, tcap)
    Q.n = T.n = n
    t = dict(nn=torch.zeros(n, qcap, 3, dtype=torch.int32), rnn=torch.zeros(n, tcap, 2, dtype=torch.int32), matches=torch.zeros(n, mcap, 3, dtype=torch.int32),
             match_counts=torch.zeros(n, dtype=torch.int32))
    ctx.match_mutual(Q, T, None, 0.49, True, **t)
    (name, args), = ctx.rec.calls
    assert name == "vslam_match_mutual_dev" and args[3] == n and args[4] == 0.49 and args[5] == 1
    out = args[-1]._obj
    want = {"struct_size": C.sizeof(capi.MatchMutualOut), "match_cap": mcap}
    for k, v in t.items():
        want[k], want[k + "_bytes"] = v.data_ptr(), v.numel() * 4
    assert {f: getattr(out, f) for f, _ in out._fields_} == want
    ctx.rec.calls.clear()
    ctx.match_mutual(Q, T, 2, rnn=t["rnn"])  # one optional output alone
    out = ctx.rec.calls[0][1][-1]._obj
    assert (out.nn, out.nn_bytes, out.matches, out.match_counts, out.match_cap) == (None, 0, None, None, 0) and out.rnn == t["rnn"].data_ptr()
    assert ctx.rec.calls[0][1][3] == 2
    ctx.rec.calls.clear()
    with pytest.raises(ValueError, match="match_mutual: rnn must be a contiguous tensor on cpu"):
        ctx.match_mutual(Q, T, rnn=t["rnn"][:, ::2])
    with pytest.raises(ValueError, match="match_mutual: nn must have 4-byte elements"):
        ctx.match_mutual(Q, T, nn=torch.zeros(n, qcap, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="match_mutual: no output requested"):
        ctx.match_mutual(Q, T)
    with pytest.raises(ValueError, match="needs match_counts"):
        ctx.match_mutual(Q, T, nn=t["nn"], matches=t["matches"])
    assert ctx.rec.calls == []


def test_python_host_wrapper_shapes_its_buffers(ctx):
    q, t = np.zeros((5, 128), np.float32), np.zeros((7, 128), np.float32)
    nn, rnn, m, total = ctx.match_mutual_host(q, t, 0.64, False, q_defined=np.ones(5, np.uint8))
    (name, args), = ctx.rec.calls
    assert name == "vslam_match_mutual_host" and (args[4], args[8], args[14]) == (5, 7, 5) and args[2] is not None and args[6] is None
    assert (nn.dtype, len(nn), rnn.dtype, len(rnn), len(m), total) == (capi.NN2_DTYPE, 5, capi.RNN_DTYPE, 7, 0, 0)
    with pytest.raises(ValueError, match="one entry per descriptor row"):
        ctx.match_mutual_host(q, t, t_defined=np.ones(6, np.uint8))


# ---- the C++ wrapper

def build_cxx_driver(tmp_path):
    """tests/mutual_cxx_driver.cpp against the C++ wrapper library -> the executable (tests/test_gpu_mutual.py runs it too)."""
    capi.build()
    cxx, lib_dir = os.path.join(ROOT, "visualslam_amd", "cxx"), os.path.dirname(capi.LIB_PATH)
    r = subprocess.run(["make", "-C", cxx], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = str(tmp_path / "mutual_cxx_driver")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", cxx, os.path.join(ROOT, "tests", "mutual_cxx_driver.cpp"),
                        os.path.join(ROOT, "visualslam_amd", "bin", "libvslam_cxx.a"), "-L" + lib_dir, "-lvslam", "-Wl,-rpath," + lib_dir,
                        "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_cxx_wrapper_refuses_bad_lists_and_answers_no_hip_device_without_a_gpu(tmp_path):
    import torch

    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = build_cxx_driver(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = subprocess.run([exe, "--valid"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"status {0 if torch.cuda.is_available() else HIP}", r.stdout + r.stderr


# ---- the restatement: two forms against each other

def near_copy(rng, t):
    """t * (1 + U(-1, 1) * 2^-20), formed in f64 and rounded to f32: d2 of the pair is below the rounding noise of its chains."""
    return (t.astype(np.float64) * (1.0 + rng.uniform(-1.0, 1.0, t.shape) * 2.0 ** -20)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def crafted_sets(seed, nq=230, nt=190):
    """Sets with everything the reverse rule names: `defined` holes on both sides (some would be the best), NaN rows, exact copies
    and duplicates (ties), near copies (negative d2) and three octaves."""
    rng = np.random.default_rng(seed)
    t = matchref.crafted(rng, nt)
    q = matchref.crafted(rng, nq, t)
    q[40:80] = near_copy(rng, t[20:60])
    t[100:110] = near_copy(rng, q[40:50])
    t[nt // 2], t[nt - 1] = t[1], t[1]         # three equal train rows
    q[0], q[9], q[120] = t[1], t[1], t[1]      # ... and three query rows equal to them: every tie goes to the lowest index
    t[3], q[5] = np.nan, np.nan
    qdf, tdf = np.ones(nq, np.uint8), np.ones(nt, np.uint8)
    qdf[[0, 4, 41]], tdf[[2, 21, 101]] = 0, 0  # q[0] is the lowest of a tie, q[41] / t[21] a near copy's partner
    q[6] = t[2]
    t[7] = q[4]
    qo, to = rng.integers(0, 3, nq).astype(np.int32), rng.integers(0, 3, nt).astype(np.int32)
    qo[40:80] = to[20:60]                      # the near copies share an octave with their partner
    to[100:110] = qo[40:50]
    return q, t, qdf, tdf, qo, to


@pytest.mark.parametrize("same_octave", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_column_walk_equals_the_swapped_matcher_bytes_equal(seed, same_octave):
    q, t, qdf, tdf, qo, to = crafted_sets(seed)
    walk = mutualref.rnn_walk(q, t, same_octave, qdf, tdf, qo, to)
    swapped = mutualref.rnn_swapped(q, t, same_octave, qdf, tdf, qo, to)
    assert walk.tobytes() == swapped.tobytes()
    # the sets show what they are for: negative distances, rows without a candidate, the undefined rows never chosen, ties low
    assert (walk["dist2"] < 0).sum() >= 5 and not np.isnan(walk["dist2"]).any()
    assert walk["index"][3] == -1 and np.isposinf(walk["dist2"][3]) and (walk["index"][[2, 21, 101]] == -1).all()
    assert not np.isin(walk["index"], [0, 4, 5, 41]).any()
    assert ((walk["index"] >= 0) == (walk["dist2"] < np.inf)).all()
    if not same_octave:
        assert walk["index"][1] == 9 and walk["index"][len(t) // 2] == 9 and walk["dist2"][1] == 0.0  # q[0] is undefined: the next of the tie
        assert walk["index"][7] != 4
    else:
        d2 = matchref.d2_all(q, t)
        has = np.flatnonzero(walk["index"] >= 0)
        assert (qo[walk["index"][has]] == to[has]).all() and (walk["dist2"][has] == d2[walk["index"][has], has]).all()


def test_d2_is_symmetric_bit_for_bit():
    q, t = crafted_sets(1)[:2]
    assert matchref.d2_all(q, t).tobytes() == np.ascontiguousarray(matchref.d2_all(t, q).T).tobytes()


@pytest.mark.parametrize("same_octave", [False, True])
def test_mutual_list_is_one_to_one_and_a_subset_of_the_forward_list(same_octave):
    q, t, qdf, tdf, qo, to = crafted_sets(2)
    nn, rnn, m = mutualref.mutual(q, t, 0.64, same_octave, qdf, tdf, qo, to)
    wnn, fwd = matchref.match(q, t, 0.64, same_octave, qdf, tdf, qo, to)
    assert nn.tobytes() == wnn.tobytes()
    assert len(np.unique(m["train"])) == len(m) and len(np.unique(m["query"])) == len(m) and (np.diff(m["query"]) > 0).all()
    fset = {r.tobytes() for r in fwd}
    assert all(r.tobytes() in fset for r in m) and 20 < len(m) < len(fwd)
    # the definition, record by record
    acc = np.zeros(len(q), bool)
    acc[fwd["query"]] = True
    want = [i for i in range(len(q)) if acc[i] and rnn["index"][nn["index"][i]] == i]
    assert m["query"].tolist() == want and (m["train"] == nn["index"][want]).all() and (m["dist2"] == nn["dist2"][want]).all()
    assert (rnn["dist2"][m["train"]] == m["dist2"]).all()  # both sides name the same distance


def test_key_map_is_strictly_monotone_and_invertible():
    f = np.finfo(np.float32)
    rng = np.random.default_rng(5)
    sample = np.concatenate([np.float32([-np.inf, -f.max, -1.0, -f.tiny, -f.smallest_subnormal * 3, -f.smallest_subnormal, 0.0, f.smallest_subnormal,
                                          f.smallest_subnormal * 3, f.tiny, 1.0, f.max, np.inf]),
                             rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    sample = np.unique(sample[~np.isnan(sample)])  # sorted ascending; -0 and +0 are one value
    k = mutualref.key(sample).astype(np.int64)
    assert (np.diff(k) > 0).all()
    assert sample[0] == -np.inf and sample[-1] == np.inf and k[-1] == 0xff800000 and k.max() < 2 ** 32 - 1  # every d2 < +inf lies below +inf's key
    assert mutualref.key(np.float32(-0.0)) == mutualref.key(np.float32(0.0)) == 0x80000000
    assert mutualref.unkey(mutualref.key(sample)).tobytes() == (sample + np.float32(0.0)).tobytes()
    # the lexicographic (key, q) word: the smaller distance wins whatever the indices, equal distances give the lower index
    word = lambda d, i: (int(mutualref.key(np.float32(d))) << 32) | i
    assert word(-1.0, 900) < word(-0.5, 0) < word(0.0, 7) < word(1e-40, 3) < word(1.0, 0) and word(2.0, 3) < word(2.0, 35) < 2 ** 64 - 1


# ---- what the cross-check is worth: the figures, held exactly

def test_building_crops_mutual_keeps_every_exact_translation_and_no_train_row_twice():
    from tests.test_gpu_match import building_crops, exact_translations, oracle_chain

    a, b = building_crops()
    (qp, qd, qk), (tp, td, tk) = oracle_chain(a), oracle_chain(b)
    rows = {}
    for ratio in (0.8, 0.9, 0.95):
        r2 = float(np.float32(ratio) * np.float32(ratio))
        _, fwd = matchref.match(qd, td, r2, False, qk, tk)
        _, _, m = mutualref.mutual(qd, td, r2, False, qk, tk)
        rows[ratio] = (len(fwd), len(m), exact_translations(fwd, qp, tp, 24), exact_translations(m, qp, tp, 24), mutualref.multiply_claimed(fwd),
                       mutualref.multiply_claimed(m))
        print("building crops, ratio", ratio, "forward, mutual, exact forward, exact mutual, (train rows claimed twice, by records):", rows[ratio])
    assert rows[0.8] == (730, 717, 710, 710, (9, 22), (0, 0))
    assert rows[0.9][:4] == (756, 718, 710, 710) and rows[0.95][:4] == (791, 718, 710, 710)


def test_repeated_structure_scenes_precision_from_0_848_to_0_943():
    tot = np.zeros(4, np.int64)
    for seed in range(16):
        s = guidedref.repeated_scene(seed)
        _, fwd = matchref.match(s["q"], s["t"], 0.64)
        _, _, m = mutualref.mutual(s["q"], s["t"], 0.64)
        tot += (len(fwd), guidedref.correct(fwd, s), len(m), guidedref.correct(m, s))
    print("16 repeated-structure scenes: forward accepted, correct, mutual accepted, correct:", tot.tolist())
    assert tuple(tot) == (4294, 3643, 3653, 3443)
    assert round(tot[1] / tot[0], 3) == 0.848 and round(tot[3] / tot[2], 3) == 0.943

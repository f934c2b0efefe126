"""Vocabulary training without a GPU: the C ABI's new symbols, struct layouts and argument checks, the host sizing under the
sanitizers, the Python and C++ wrappers' own checks, and the CPU restatement of the section (tests/kmeansref.py), which the GPU
tests compare against byte for byte: the rule on hand-made rows, the means against independent arithmetic, the distortion from
round to round, and what training does to the loop candidates of the planted scenes and of the 17 crops of the reference's images."""
import ctypes as C
import fractions
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import kmeansref, matchref, placeref
from visualslam_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visualslam_amd", "csrc")
INVALID, HIP = -1, -2
ENTRY_POINTS = ("vslam_vocab_kmeans_dev", "vslam_vocab_kmeans_host")
KERNELS = (b"k_kmeans_init", b"k_kmeans_count", b"k_kmeans_columns", b"k_kmeans_scan", b"k_kmeans_members", b"k_kmeans_block_sums", b"k_kmeans_update")


@pytest.fixture(scope="module")
def lib():
    capi.build()
    return capi.lib()


# ---- ABI

def test_kmeans_symbols_kernel_names_and_version(lib):
    for path in (capi.LIB_PATH, capi.DIAG_LIB_PATH):
        L = C.CDLL(path)
        for name in ENTRY_POINTS:
            assert hasattr(L, name), (path, name)
            assert name in capi.SIGNATURES
    names = lib.vslam_kernel_names().split(b"\n")
    for k in KERNELS:
        assert k in names
    assert lib.vslam_version() == 200


def test_kmeans_struct_layouts_match_a_c99_compile_of_the_header(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "vslam.h"', "int main(void) {"]
    want = []
    structs = (("vslam_kmeans_params", capi.KmeansParams), ("vslam_kmeans_round", capi.KmeansRound), ("vslam_kmeans_out", capi.KmeansOut))
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
    assert [r[0] for r in rows] == [8, 16, 56]
    assert capi.KMEANS_ROUND_DTYPE.itemsize == 16 and [capi.KMEANS_ROUND_DTYPE.fields[n][1] for n in ("assigned", "changed", "empty", "ran")] == rows[1][1:]


class Mem:
    """Host arrays a valid call points at (nothing is launched without a GPU: the pointers are never followed)."""

    def __init__(self):
        self.desc = np.zeros((3, 50, 128), np.float32)
        self.vocab = np.zeros((200, 128), np.float32)
        self.u32 = np.zeros(400, np.uint32)
        assert self.desc.ctypes.data % 16 == 0 and self.vocab.ctypes.data % 16 == 0


def test_kmeans_dev_and_host_reject_bad_arguments_before_they_need_a_gpu(lib):
    import torch

    m = Mem()
    gpu = torch.cuda.is_available()
    v, u, d = m.vocab.ctypes.data, m.u32.ctypes.data, m.desc.ctypes.data

    def out(**change):
        o = capi.KmeansOut(C.sizeof(capi.KmeansOut), v, 100 * 512, u, 400, u, 5 * 16)
        for k, x in change.items():
            setattr(o, k, x)
        return o

    def dev(sets=True, n_sets=3, vocab_in=v, K=100, params=True, rounds=5, reserved=0, o=True, s={}, **change):
        S = capi.DescSets(d, None, None, u, 50)
        for k, x in s.items():
            setattr(S, k, x)
        P = capi.KmeansParams(rounds, reserved)
        return lib.vslam_vocab_kmeans_dev(None, C.byref(S) if sets else None, n_sets, vocab_in, None, K, C.byref(P) if params else None,
                                          C.byref(out(**change)) if o else None)

    def host(desc=d, counts=u, cap=50, n_sets=3, vocab_in=v, K=100, params=True, rounds=5, reserved=0, o=True, **change):
        P = capi.KmeansParams(rounds, reserved)
        return lib.vslam_vocab_kmeans_host(None, desc, None, counts, cap, n_sets, vocab_in, None, K, C.byref(P) if params else None,
                                           C.byref(out(**change)) if o else None)

    assert dev() == (INVALID if gpu else HIP) and host() == (INVALID if gpu else HIP)
    assert dev(sets=False) == INVALID and dev(vocab_in=None) == INVALID and dev(params=False) == INVALID and dev(o=False) == INVALID
    assert dev(struct_size=48) == INVALID and dev(rounds=0) == INVALID and dev(rounds=65, report_bytes=65 * 16) == INVALID and dev(reserved=1) == INVALID
    assert dev(n_sets=-1) == INVALID and dev(n_sets=65536) == INVALID and dev(K=0) == INVALID and dev(K=65537, vocab_bytes=2 ** 40, sizes_bytes=2 ** 40) == INVALID
    assert dev(s=dict(desc=None)) == INVALID and dev(s=dict(counts=None)) == INVALID and dev(s=dict(cap=0)) == INVALID and dev(s=dict(desc=d + 4)) == INVALID
    assert dev(n_sets=65535, s=dict(cap=65538)) == INVALID  # a row id past 32 bits
    assert dev(vocab_in=v + 4, vocab=v + 4) == INVALID and dev(vocab=None) == INVALID and dev(vocab=v + 100 * 512 + 4) == INVALID
    assert dev(vocab_bytes=100 * 512 - 1) == INVALID and dev(sizes_bytes=399) == INVALID and dev(report_bytes=79) == INVALID
    assert dev(vocab=v + 512) == INVALID and dev(vocab_in=v + 512) == INVALID and dev(vocab=v + 99 * 512 + 496) == INVALID  # overlap other than exactly
    assert host(desc=None) == INVALID and host(counts=None) == INVALID and host(cap=0) == INVALID and host(vocab_in=None) == INVALID
    assert host(params=False) == INVALID and host(o=False) == INVALID and host(struct_size=0) == INVALID and host(rounds=65) == INVALID
    assert host(reserved=7) == INVALID and host(n_sets=-1) == INVALID and host(K=0) == INVALID and host(vocab=None) == INVALID
    assert host(vocab_bytes=0) == INVALID and host(sizes_bytes=0) == INVALID and host(report_bytes=0) == INVALID and host(vocab=v + 4) == INVALID
    # (a null context keeps no message: the wording and the order of the rejections are the plan driver's to check, below)
    if not gpu:  # each optional output may be absent, no sets is a valid call, a separate output, the extremes, host arrays need no alignment
        assert dev(sizes=None) == HIP and dev(report=None) == HIP and dev(sizes=None, report=None) == HIP and dev(n_sets=0) == HIP
        assert dev(vocab=v + 100 * 512) == HIP and dev(rounds=1) == HIP and dev(rounds=64, report_bytes=64 * 16) == HIP
        assert dev(n_sets=65535, s=dict(cap=65537), K=65536, vocab_bytes=65536 * 512, sizes_bytes=65536 * 4) == HIP
        assert host(desc=d + 4, vocab_in=v + 4, vocab=v + 4) == HIP and host(n_sets=0) == HIP and host(vocab=v + 100 * 512 + 4) == HIP


SIZES_BY_HAND = {  # (cap, K, sets) -> rows, max_blocks, bsum_bytes, init, count, columns, sums
    (1, 1, 1): (1, 1, 1024, 1, 1, 1, 1),
    (700, 64, 3): (2100, 8 + 64, 72 * 1024, 1, 3, 1, 18),
    (2000, 4096, 1): (2000, 7 + 4096, 4103 * 1024, 1, 8, 16, 1026),
    (65536, 1024, 256): (2 ** 24, 65536 + 1024, 66560 * 1024, 1, 256, 4, 16640),                      # the benchmark's call: 65 MiB of block sums
    (65537, 65536, 65535): (2 ** 32 - 1, 2 ** 24 - 1 + 65536, (2 ** 24 - 1 + 65536) * 1024, 256, 257, 256, 4210688),  # the largest row id: 2^32 - 2
}


def test_host_sizing_and_checks_are_clean_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "plan_driver"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "kmeans_plan_driver.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("this g++ has no sanitizer runtime: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    rows = {l.split()[0]: dict(x.split("=", 1) for x in l.split()[1:]) for l in out.stdout.splitlines() if not l.startswith("size")}
    assert rows["plan"]["bad"] == "0" and int(rows["plan"]["checked"]) > 10000, rows["plan"]
    assert rows["args"]["bad"] == "0" and int(rows["args"]["checked"]) == 56, rows["args"]  # (every message and the order of the checks are among them)
    sizes = {}
    for l in out.stdout.splitlines():
        if l.startswith("size"):
            w = l.split()
            sizes[tuple(int(v) for v in w[1:4])] = tuple(int(x.split("=")[1]) for x in w[4:])
    assert sizes == SIZES_BY_HAND
    src = open(os.path.join(CSRC, "vslam_kmeans_plan.h")).read()  # the header under test is plain host code
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
    vin, vout, vdef = torch.zeros(K, 128), torch.zeros(K, 128), torch.zeros(K, dtype=torch.uint8)
    sizes, report = torch.zeros(K, dtype=torch.int32), torch.zeros(5, 4, dtype=torch.int32)
    ctx.vocab_kmeans(S, vin, 5, vdef, vocab=vout, sizes=sizes, report=report)
    (name, args), = ctx.rec.calls
    assert name == "vslam_vocab_kmeans_dev" and args[2:6] == (n, vin.data_ptr(), vdef.data_ptr(), K)
    P, O = args[6]._obj, args[7]._obj
    assert (P.rounds, P.reserved) == (5, 0)
    assert {f: getattr(O, f) for f, _ in O._fields_} == dict(struct_size=C.sizeof(capi.KmeansOut), vocab=vout.data_ptr(), vocab_bytes=K * 512, sizes=sizes.data_ptr(),
                                                            sizes_bytes=K * 4, report=report.data_ptr(), report_bytes=80)
    ctx.rec.calls.clear()
    ctx.vocab_kmeans(S, vin, 2, n_sets=2)  # in place, no optional output, no vocab_defined
    args = ctx.rec.calls[0][1]
    O = args[7]._obj
    assert args[2] == 2 and args[4] is None and (O.vocab, O.sizes, O.report) == (vin.data_ptr(), None, None)
    ctx.rec.calls.clear()
    with pytest.raises(ValueError, match="vocab_kmeans: vocab_in is required"):
        ctx.vocab_kmeans(S, None, 2)
    with pytest.raises(ValueError, match=r"vocab_kmeans: vocab_in must be float32 \[K, 128\]"):
        ctx.vocab_kmeans(S, torch.zeros(K, 64), 2)
    with pytest.raises(ValueError, match=r"vocab_kmeans: vocab must be float32 \[K, 128\]"):
        ctx.vocab_kmeans(S, vin, 2, vocab=torch.zeros(K, 128, dtype=torch.float64))
    with pytest.raises(ValueError, match="vocab_kmeans: vocab must have vocab_in's K rows"):
        ctx.vocab_kmeans(S, vin, 2, vocab=torch.zeros(K + 1, 128))
    with pytest.raises(ValueError, match="vocab_kmeans: vocab must be a contiguous tensor on cpu"):
        ctx.vocab_kmeans(S, vin, 2, vocab=torch.zeros(K, 256)[:, ::2])
    with pytest.raises(ValueError, match=r"vocab_kmeans: vocab_defined must be uint8 \[K\]"):
        ctx.vocab_kmeans(S, vin, 2, vdef[:-1])
    with pytest.raises(ValueError, match="vocab_kmeans: sizes must have 4-byte elements"):
        ctx.vocab_kmeans(S, vin, 2, sizes=torch.zeros(K, dtype=torch.int64))
    with pytest.raises(ValueError, match="vocab_kmeans: fewer sets than pairs"):
        ctx.vocab_kmeans(S, vin, 6, report=report)
    with pytest.raises(ValueError, match="vocab_kmeans: fewer sets than pairs"):
        ctx.vocab_kmeans(S, vin, 2, sizes=sizes[:-1])
    assert ctx.rec.calls == []


def test_python_host_wrapper_shapes_its_buffers(ctx):
    desc, vocab = np.zeros((2, 7, 128), np.float32), np.ones((9, 128), np.float32)
    v, s, r = ctx.vocab_kmeans_host(desc, [7, 3], vocab, 4, vocab_defined=np.ones(9, np.uint8))
    (name, args), = ctx.rec.calls
    assert name == "vslam_vocab_kmeans_host" and args[4:6] == (7, 2) and args[2] is None and args[7] is not None and args[8] == 9 and args[9]._obj.rounds == 4
    assert (v.shape, v.dtype, s.shape, s.dtype, r.shape, r.dtype) == ((9, 128), np.float32, (9,), np.uint32, (4,), capi.KMEANS_ROUND_DTYPE)
    v, s, r = ctx.vocab_kmeans_host(desc, [7, 3], vocab, 4, want_sizes=False, want_report=False)
    assert s is None and r is None and ctx.rec.calls[-1][1][10]._obj.sizes is None
    with pytest.raises(ValueError, match="one count per set"):
        ctx.vocab_kmeans_host(desc, [7], vocab, 4)
    with pytest.raises(ValueError, match="one entry per descriptor row"):
        ctx.vocab_kmeans_host(desc, [7, 3], vocab, 4, defined=np.ones(13, np.uint8))


# ---- the C++ wrapper

def test_cxx_wrapper_refuses_bad_lists_and_answers_no_hip_device_without_a_gpu(tmp_path):
    import torch

    from tests.test_gpu_kmeans import build_cxx_driver

    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = build_cxx_driver(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    r = subprocess.run([exe, "--valid"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == f"status {0 if torch.cuda.is_available() else HIP}", r.stdout + r.stderr
    assert os.path.exists(os.path.join(ROOT, "visualslam_amd", "bin", "Place"))


# ---- the rule, on hand-made rows

def axis_words(K, scale=8.0):
    """Word k = scale * e_k: far apart, and a row near scale * e_k goes to word k."""
    v = np.zeros((K, 128), np.float32)
    v[np.arange(K), np.arange(K)] = scale
    return v


def rows_of(word, m, rng, spread=0.25):
    """m rows within `spread` of a word, entries on a grid of 1 / 64: sums of thousands of them are exact in f64."""
    return (word[None, :] + np.round(rng.uniform(-spread, spread, (m, 128)) * 64) / 64).astype(np.float32)


def one_set(rows, cap=None):
    cap = cap or max(len(rows), 1)
    desc = np.zeros((1, cap, 128), np.float32)
    desc[0, : len(rows)] = rows
    return desc, [len(rows)]


def exact_mean(rows):
    """The exact rational mean of f32 rows, rounded once to f32 per entry (through the nearest f64 of a Fraction: the quotient of
    two integers below 2^53 after scaling, so float(Fraction) is the correctly rounded f64 and the double rounding is checked)."""
    n = len(rows)
    out = np.zeros(128, np.float32)
    for d in range(128):
        q = sum((fractions.Fraction(float(x)) for x in rows[:, d]), fractions.Fraction(0)) / n
        f64 = float(q)  # correctly rounded (CPython rounds Fraction -> float exactly once)
        out[d] = np.float32(f64)
        lo, hi = np.nextafter(out[d], np.float32(-np.inf)), np.nextafter(out[d], np.float32(np.inf))
        assert abs(fractions.Fraction(float(out[d])) - q) <= min(abs(fractions.Fraction(float(lo)) - q), abs(fractions.Fraction(float(hi)) - q))
    return out


def test_rule_member_counts_0_1_255_256_257_513_over_three_sets_with_an_empty_one_between():
    rng = np.random.default_rng(1)
    counts = [0, 1, 255, 256, 257, 513]
    V = axis_words(6)
    # set 0 holds the first part of every word's rows, set 1 is empty, set 2 holds the rest: 513 = 200 + 313, 257 = 256 + 1
    first = [0, 1, 100, 256, 256, 200]
    parts = [[rows_of(V[k], first[k], rng) for k in range(6)], [], [rows_of(V[k], counts[k] - first[k], rng) for k in range(6)]]
    sets = [np.concatenate(p) if p else np.zeros((0, 128), np.float32) for p in parts]
    for s in (0, 2):
        sets[s] = sets[s][rng.permutation(len(sets[s]))]
    cap = max(len(s) for s in sets)
    desc = np.zeros((3, cap, 128), np.float32)
    for f, s in enumerate(sets):
        desc[f, : len(s)] = s
    r = kmeansref.kmeans(desc, [len(s) for s in sets], V, 1, history=True)
    assert r["sizes"].tolist() == counts and r["report"].tolist() == [(sum(counts), sum(counts), 1, 1)]
    assert r["vocab"][0].tobytes() == V[0].tobytes()  # no member: the bytes stay
    w = r["words"][0]
    for k in range(1, 6):
        mine = np.concatenate([desc[f, : len(sets[f])][w[f, : len(sets[f])] == k] for f in range(3)])  # set ascending, row ascending
        assert len(mine) == counts[k]
        assert r["vocab"][k].tobytes() == exact_mean(mine).tobytes(), k  # every f64 sum is exact here, so any order gives the exact mean ...
    # ... and on rows where it is not, the blocks matter: one sum over all 513 members differs from the rule's in some entry
    big = (rng.random((513, 128)) * np.float32(2.0) ** rng.integers(-20, 20, (513, 128))).astype(np.float32)
    rows = [x.tolist() for x in big]
    straight = [0.0] * 128
    for x in rows:
        straight = [s + v for s, v in zip(straight, x)]
    rule = kmeansref.ordered_sum(rows)
    assert rule != straight and max(abs(a - b) / abs(b) for a, b in zip(rule, straight)) < 1e-13
    assert kmeansref.ordered_sum(rows[:256]) == [sum_in_order(c) for c in zip(*rows[:256])]  # one block: the plain sequential sum


def sum_in_order(xs):
    s = 0.0
    for x in xs:
        s = s + x
    return s


def test_rule_equal_words_undefined_words_nan_rows_and_infinite_rows():
    rng = np.random.default_rng(2)
    V = axis_words(5)
    V[3] = V[1]                      # the second of two equal words gets no member in that round
    vdef = np.array([1, 1, 0, 1, 1], np.uint8)  # word 2 is undefined: its rows go elsewhere
    rows = np.concatenate([rows_of(V[0], 5, rng), rows_of(V[1], 7, rng), rows_of(axis_words(5)[2], 3, rng), rows_of(V[4], 4, rng)])
    rows[2] = np.nan                 # an all-NaN row, flagged defined: no word, counted as changed in round 1, never assigned
    rows[6, 9] = np.inf              # a row holding +inf: every distance is +inf or NaN, so it gets no word either
    rows[13, 3] = -np.inf
    desc, counts = one_set(rows)
    r = kmeansref.kmeans(desc, counts, V, 1, None, vdef, history=True)
    w = r["words"][0][0]
    assert w[2] == -1 and w[6] == -1 and w[13] == -1 and not (w == 2).any() and not (w == 3).any()
    assert r["report"][0].tolist() == (19 - 3, 19, 1, 1)  # empty: word 3 (defined, no member); word 2 is not defined
    assert r["sizes"][[2, 3]].tolist() == [0, 0] and r["vocab"][2].tobytes() == V[2].tobytes() and r["vocab"][3].tobytes() == V[3].tobytes()
    assert np.isfinite(r["vocab"]).all()  # a member's distance is finite, so its entries are: no sum is ever NaN or infinite
    # once word 1 has moved to its mean, word 3 - still where both were - is a word of its own: the next round may give it rows
    r3 = kmeansref.kmeans(desc, counts, V, 3, None, vdef)
    assert r3["vocab"][1].tobytes() != V[1].tobytes() and r3["sizes"][2] == 0 and r3["sizes"][1] + r3["sizes"][3] == 6 and np.isfinite(r3["vocab"]).all()
    # the arithmetic of steps 4 and 5 on such rows all the same: plain IEEE
    m = kmeansref.mean_word([[1.0] * 128, [np.inf] + [2.0] * 127, [-np.inf] + [3.0] * 127])
    assert np.isnan(m[0]) and m[1] == 2.0
    # a vocabulary that comes in with a dead word: no row gets it in any round and it keeps its bytes
    V2 = axis_words(5)
    V2[1, 7] = np.inf
    V2[4] = np.nan
    r = kmeansref.kmeans(desc, counts, V2, 2, history=True)
    assert r["sizes"][[1, 4]].tolist() == [0, 0] and r["vocab"][[1, 4]].tobytes() == V2[[1, 4]].tobytes() and r["report"]["empty"].tolist() == [2, 2]


def test_rule_negative_zero_and_subnormal_entries():
    f = np.finfo(np.float32)
    V = np.zeros((2, 128), np.float32)
    V[1] = 1.0
    rows = np.zeros((4, 128), np.float32)
    rows[0], rows[1] = -0.0, -0.0
    rows[:, 1] = [f.smallest_subnormal, f.smallest_subnormal, f.smallest_subnormal, 0.0]  # mean 3/4 of the smallest subnormal: rounds to it
    rows[:, 2] = [f.smallest_subnormal, 0.0, 0.0, 0.0]                                      # mean 1/4: rounds to +0
    rows[:, 3] = [-f.smallest_subnormal, -f.smallest_subnormal, 0.0, 0.0]                   # mean -1/2: a tie, to even: -0
    rows[:, 4] = [-0.0, -0.0, -0.0, -0.0]                                                   # B starts at +0.0: the sum of -0s is +0
    rows[:, 5] = [f.smallest_normal, -f.smallest_subnormal, 0.0, 0.0]
    desc, counts = one_set(rows)
    r = kmeansref.kmeans(desc, counts, V, 1)
    got = r["vocab"][0]
    assert r["sizes"].tolist() == [4, 0]
    assert got[1] == f.smallest_subnormal and got[2] == 0 and not np.signbit(got[2]) and got[3] == 0 and np.signbit(got[3])
    assert got[4] == 0 and not np.signbit(got[4]) and not np.signbit(got[0])
    assert got[5] == np.float32((float(f.smallest_normal) - float(f.smallest_subnormal)) / 4) and 0 < got[5] < f.smallest_normal


def test_rule_convergence_in_round_2_of_5():
    rng = np.random.default_rng(3)
    V = axis_words(4)
    rows = np.concatenate([rows_of(V[k], m, rng) for k, m in ((0, 10), (1, 300), (3, 5))])
    desc, counts = one_set(rows[rng.permutation(len(rows))])
    five, one = kmeansref.kmeans(desc, counts, V, 5, history=True), kmeansref.kmeans(desc, counts, V, 1)
    assert five["report"].tolist() == [(315, 315, 1, 1), (315, 0, 1, 1), (0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)]
    assert five["vocab"].tobytes() == one["vocab"].tobytes() and five["sizes"].tobytes() == one["sizes"].tobytes() and len(five["vocabs"]) == 2
    none = kmeansref.kmeans(desc[:0], [], V, 3)  # no sets: nothing runs
    assert none["vocab"].tobytes() == V.tobytes() and not none["sizes"].any() and none["report"].tobytes() == bytes(48)


# ---- against independent arithmetic

def test_means_of_random_rows_are_within_the_derived_bound_of_a_float64_mean():
    """|sum_rule - sum_exact| <= gamma * sum |x| with gamma = (255 + ceil(N / 256)) * 2^-53 / (1 - that): at most 255 additions inside a
    block and one per block after it, each within 2^-53 relative.  numpy's pairwise f64 sum obeys a smaller bound of the same form, so
    the two sums differ by at most 2 gamma sum |x|; the division adds 2^-53 relative and the rounding to f32 2^-24 relative."""
    rng = np.random.default_rng(4)
    K = 8
    V = matchref.crafted(rng, K)
    desc = np.stack([matchref.crafted(rng, 900, V, signed=True) for _ in range(2)])
    r = kmeansref.kmeans(desc, [900, 900], V, 1, history=True)
    w = r["words"][0]
    checked = 0
    for k in range(K):
        mine = desc[w == k].astype(np.float64)
        if len(mine) == 0:
            continue
        n = len(mine)
        u = 2.0 ** -53
        gamma = (255 + -(-n // 256)) * u / (1 - (255 + -(-n // 256)) * u)
        mean64 = mine.sum(axis=0) / n
        bound = (2 * gamma + 2 * u) * np.abs(mine).sum(axis=0) / n + 2.0 ** -24 * np.abs(mean64) + np.finfo(np.float32).smallest_subnormal
        assert (np.abs(r["vocab"][k].astype(np.float64) - mean64) <= bound).all(), k
        checked += 1
    assert checked >= 4 and r["sizes"].max() > 256


def test_distortion_does_not_rise_from_round_to_round():
    """J(w, V) = sum over the assigned rows of |x - V[w]|^2, in f64.  The update lowers J exactly (the mean minimises it, up to the
    rounding of the mean); the assignment lowers it up to the f32 error of d2: a row moves from word a to word b when d2_b < d2_a
    in f32, so its exact distance rises by at most B(x, a) + B(x, b) with matchref.d2_bound's B = 264 * 2^-24 * (|x|^2 + |v|^2).
    The slack allowed is that, summed over the rows, plus the mean's rounding: 2^-23 |x - c| |c| per entry, summed likewise."""
    rng = np.random.default_rng(6)
    K = 24
    V0 = matchref.crafted(rng, K)
    desc = np.stack([matchref.crafted(rng, 400, V0) for _ in range(3)])
    counts = [400, 250, 400]
    r = kmeansref.kmeans(desc, counts, V0, 6, history=True)
    assert len(r["words"]) >= 4

    def J(w, V):
        total, slack = 0.0, 0.0
        for f in range(3):
            for q in range(counts[f]):
                k = w[f, q]
                if k >= 0:
                    x, c = desc[f, q].astype(np.float64), V[k].astype(np.float64)
                    total += float(((x - c) ** 2).sum())
                    slack += 2 * 264.0 * 2.0 ** -24 * float((x * x).sum() + (c * c).sum()) + 2.0 ** -23 * float((np.abs(x - c) * np.abs(c)).sum())
        return total, slack

    js = []
    for t, w in enumerate(r["words"]):          # after the assignment of round t + 1, against V_t
        js.append(J(w, r["vocabs"][t]))
        if t + 1 < len(r["vocabs"]):            # after its update
            js.append(J(w, r["vocabs"][t + 1]))
    for (a, _), (b, slack) in zip(js, js[1:]):
        assert b <= a + slack, (a, b, slack)
    assert js[-1][0] < 0.9 * js[0][0]


# ---- what training does to the loop candidates: measured with the restatement, then held

def pair_scores(hist, truth, min_gap=4):
    """-> (S / N of every true eligible pair as (i, x), the highest S / N of an untrue eligible pair)."""
    r = placeref.place(hist, None, min_gap=min_gap, max_candidates=8, num=0, den=1)
    sq, sc = r["self_q"], r["scores"]
    true, untrue = [], 0.0
    for i in range(len(hist)):
        for j in range(len(hist)):
            if j + min_gap <= i and max(sq[i], sq[j]) > 0:
                x = int(sc[i, j]) / max(int(sq[i]), int(sq[j]))
                if truth(i, j):
                    true.append((i, x))
                else:
                    untrue = max(untrue, x)
    return true, untrue


def test_planted_revisits_at_256_words_training_separates_what_sampling_does_not():
    """placeref.revisit_scene, seeds 0 - 3, K = 256 words from all 32 frames (12 places of 400 landmarks: far too few words, chosen
    so that the vocabulary matters), min_gap 4.  Measured with the restatement, over the four seeds:
        sampled vocabulary          lowest true pair 0.6035, highest untrue pair 0.6148: no threshold separates them
        after 2 rounds of k-means   lowest true pair 0.6325, highest untrue pair 0.5897
        (after 4 rounds             lowest true pair 0.6291, highest untrue pair 0.6033: the margin narrows again)
    Two rounds are held: every true pair above 0.62, every untrue pair below 0.60."""
    lo_s, hi_s, lo_k, hi_k = 9.0, 0.0, 9.0, 0.0
    for seed in range(4):
        desc, counts, seq = placeref.revisit_scene(seed)
        vocab, vdef = placeref.vocab_sample(desc, counts, 256)
        trained = kmeansref.kmeans(desc, counts, vocab, 2, None, vdef)
        assert trained["report"]["ran"].tolist() == [1, 1] and trained["report"]["empty"][1] <= trained["report"]["empty"][0] + 8
        for V, which in ((vocab, "s"), (trained["vocab"], "k")):
            _, _, hist = placeref.words(desc, counts, V, None, vdef)
            true, untrue = pair_scores(hist, lambda i, j: seq[i] == seq[j])
            if which == "s":
                lo_s, hi_s = min(lo_s, min(x for _, x in true)), max(hi_s, untrue)
            else:
                lo_k, hi_k = min(lo_k, min(x for _, x in true)), max(hi_k, untrue)
    print("planted revisits, K = 256, 4 seeds: sampled lowest true %.4f highest untrue %.4f; 2 rounds lowest true %.4f highest untrue %.4f" % (lo_s, hi_s, lo_k, hi_k))
    assert lo_s < hi_s           # the parent's vocabulary: the two ranges overlap
    assert lo_k > 0.62 and hi_k < 0.60


def test_seventeen_crops_training_does_not_lift_the_home_revisits_over_the_threshold():
    """The 17 crops of tests/test_place_cpu.py, K = 256 words sampled from all 17 frames, then 8 rounds of k-means on those frames.
    Measured with the restatement (lowest true score / highest untrue score / the home revisits, frames 15 and 16):
        sampled    0.1667 / 0.1405 / 0.167 - 0.174   (the parent: below 1 / 5)
        1 round    0.1438 / 0.1332 / 0.144 - 0.155
        2 rounds   0.1419 / 0.1413 / 0.142 - 0.155
        4 rounds   0.1429 / 0.1429 / 0.143 - 0.185
        8 rounds   0.1613 / 0.1401 / 0.161 - 0.191   (changed 45 of 3949 rows in the last round)
        16 rounds  0.1613 / 0.1385 / 0.161 - 0.191   (changed 5)
    K-MEANS DOES NOT LIFT THE HOME REVISITS OVER 1 / 5.  The best of them rises from 0.174 to 0.191, the worst falls from 0.167 to
    0.161; the building revisits fall from 0.47 - 0.65 to 0.41 - 0.60 and stay far above.  The order holds (every true pair above
    every untrue one) but not after 2 or 4 rounds, where a true pair ties with an untrue one.  A frame of 85 descriptors among 3949
    rows owns about five of 256 centroids whatever the training does; the vocabulary from the frames before the revisits
    (tests/test_place_cpu.py: 0.218 - 0.301) remains the answer for such frames.  The 8-round figures are held."""
    from tests.test_place_cpu import REVISITS, crop_descriptors

    desc, defined, counts = crop_descriptors()
    vocab, vdef = placeref.vocab_sample(desc, counts, 256, defined)
    trained = kmeansref.kmeans(desc, counts, vocab, 8, defined, vdef)
    rep = trained["report"]
    assert rep["ran"].all() and rep["assigned"].tolist() == [3823] * 8 and rep["changed"][0] == 3949 and 0 < rep["changed"][7] < 100
    assert rep["empty"][0] == 36 and rep["empty"][7] == 16  # sampled words that no row is nearest to; training halves them
    _, _, hist = placeref.words(desc, counts, trained["vocab"], defined, vdef)
    true, untrue = pair_scores(hist, lambda i, j: j in REVISITS.get(i, []))
    home = [x for i, x in true if i >= 15]
    print("17 crops, K = 256 from all frames, 8 rounds: true pairs", [(i, round(x, 4)) for i, x in true], "highest untrue %.4f" % untrue)
    assert len(true) == 15 and len(home) == 6
    assert 0.155 < min(home) and max(home) < 0.2          # measured 0.1613 .. 0.1905: still below the threshold
    assert untrue < 0.15 < min(home)                      # measured 0.1401: the order holds
    assert min(x for i, x in true if i < 15) > 0.40       # measured 0.4137

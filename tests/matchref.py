"""CPU restatement of the descriptor matcher's arithmetic (include/vslam.h, "descriptor matching"), bit for bit:

  s(a, b)  = acc = +0.0f; acc = fmaf(a[k], b[k], acc), k = 0 .. 127 ascending
  n(a)     = s(a, a)
  d2(a, b) = (n(a) + n(b)) - 2 s(a, b), every operation rounded to f32

and the sequential nearest-two selection with the ratio test.  A few lines of C, compiled once per process with
gcc -O2 -ffp-contract=off (-mfma where the CPU has it: glibc's fmaf and the instruction agree bit for bit) - this is the
checker, not the product: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from visualslam_amd import capi

_SRC = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
typedef struct { int32_t index; float dist2, second_dist2; } nn2;
static float chain(const float* a, const float* b) {
    float acc = 0.0f;
    for (int k = 0; k < 128; ++k) acc = fmaf(a[k], b[k], acc);
    return acc;
}
void ref_norms(const float* d, size_t n, float* out) {
    for (size_t i = 0; i < n; ++i) out[i] = chain(d + 128 * i, d + 128 * i);
}
void ref_d2(const float* a, const float* b, float* out) {
    const float na = chain(a, a), nb = chain(b, b), sum = na + nb, twice = 2.0f * chain(a, b);
    *out = sum - twice;
}
/* query rows q0 .. q1-1 against every train row */
void ref_match(const float* q, const uint8_t* qdef, const int32_t* qoct, size_t q0, size_t q1, const float* qn,
               const float* t, const uint8_t* tdef, const int32_t* toct, size_t nt, const float* tn,
               int same_octave, float ratio2, nn2* nn, uint8_t* accepted) {
    for (size_t i = q0; i < q1; ++i) {
        float best = INFINITY, second = INFINITY;
        int32_t index = -1;
        if (!qdef || qdef[i]) {
            for (size_t j = 0; j < nt; ++j) {
                if (tdef && !tdef[j]) continue;
                if (same_octave && toct[j] != qoct[i]) continue;
                const float sum = qn[i] + tn[j], twice = 2.0f * chain(q + 128 * i, t + 128 * j);
                const float d2 = sum - twice;
                if (d2 < best) { second = best; best = d2; index = (int32_t)j; }
                else if (d2 < second) second = d2;
            }
        }
        nn[i].index = index; nn[i].dist2 = best; nn[i].second_dist2 = second;
        const float lim = ratio2 * second;
        accepted[i] = index >= 0 && (second == INFINITY || best < lim);
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="matchref_")
        src, so = os.path.join(d, "matchref.c"), os.path.join(d, "matchref.so")
        with open(src, "w") as f:
            f.write(_SRC)
        flags = ["-O2", "-ffp-contract=off", "-shared", "-fPIC"]
        try:
            if " fma " in open("/proc/cpuinfo").read().replace("\n", " "):
                flags.append("-mfma")
        except OSError:
            pass
        subprocess.run(["gcc", *flags, src, "-o", so, "-lm"], check=True, capture_output=True)
        _lib = C.CDLL(so)
    return _lib


def _rows(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 128)


def norms(d):
    d = _rows(d)
    out = np.zeros(len(d), np.float32)
    lib().ref_norms(C.c_void_p(d.ctypes.data), C.c_size_t(len(d)), C.c_void_p(out.ctypes.data))
    return out


def d2(a, b):
    a, b = _rows(a), _rows(b)
    out = np.zeros(1, np.float32)
    lib().ref_d2(C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data), C.c_void_p(out.ctypes.data))
    return out[0]


def match(q, t, ratio2=0.64, same_octave=False, q_defined=None, t_defined=None, q_octave=None, t_octave=None):
    """-> (nn [nq] capi.NN2_DTYPE, matches capi.MATCH_DTYPE in ascending query order)."""
    q, t = _rows(q), _rows(t)
    nq, nt = len(q), len(t)
    opt = [None if a is None else np.ascontiguousarray(a, dtype=dt) for a, dt in
           ((q_defined, np.uint8), (q_octave, np.int32), (t_defined, np.uint8), (t_octave, np.int32))]
    ptr = [C.c_void_p(None if a is None else a.ctypes.data) for a in opt]
    if same_octave:
        assert opt[1] is not None and opt[3] is not None
    qn, tn = norms(q), norms(t)
    nn = np.zeros(nq, capi.NN2_DTYPE)
    acc = np.zeros(nq, np.uint8)
    L = lib()

    def run(lo, hi):
        L.ref_match(C.c_void_p(q.ctypes.data), ptr[0], ptr[1], C.c_size_t(lo), C.c_size_t(hi), C.c_void_p(qn.ctypes.data),
                    C.c_void_p(t.ctypes.data), ptr[2], ptr[3], C.c_size_t(nt), C.c_void_p(tn.ctypes.data),
                    C.c_int(int(bool(same_octave))), C.c_float(ratio2), C.c_void_p(nn.ctypes.data), C.c_void_p(acc.ctypes.data))

    step = max(64, (nq + 15) // 16)
    with ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL; the chunks write disjoint rows
        list(ex.map(lambda lo: run(lo, min(lo + step, nq)), range(0, nq, step)))
    idx = np.flatnonzero(acc)
    m = np.zeros(len(idx), capi.MATCH_DTYPE)
    m["query"], m["train"], m["dist2"] = idx, nn["index"][idx], nn["dist2"][idx]
    return nn, m


def reference_like_descriptors(rng, n):
    """Rows shaped like the reference's descriptors (SIFT(), Diff_of_Gauss.cpp): non-negative histograms divided by their
    maximum, clamped at 0.2 and divided by the new maximum - so many entries are exactly 1."""
    h = rng.gamma(0.6, 1.0, (n, 128)).astype(np.float32)
    h[rng.random((n, 128)) < 0.15] = 0.0
    h[:, 0] += np.float32(1e-3)  # no all-zero row
    h = h / h.max(axis=1, keepdims=True)
    h = np.minimum(h, np.float32(0.2))
    return (h / h.max(axis=1, keepdims=True)).astype(np.float32)

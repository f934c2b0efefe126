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
/* d2 of every query row against every train row, out [nq][nt] */
void ref_d2_all(const float* q, size_t nq, const float* t, size_t nt, float* out) {
    for (size_t i = 0; i < nq; ++i)
        for (size_t j = 0; j < nt; ++j) ref_d2(q + 128 * i, t + 128 * j, out + i * nt + j);
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


def d2_all(q, t):
    """[nq, nt] f32: the restatement's d2 of every query row against every train row."""
    q, t = _rows(q), _rows(t)
    out = np.zeros((len(q), len(t)), np.float32)
    lib().ref_d2_all(C.c_void_p(q.ctypes.data), C.c_size_t(len(q)), C.c_void_p(t.ctypes.data), C.c_size_t(len(t)), C.c_void_p(out.ctypes.data))
    return out


def exact_d2(q, t):
    """[nq, nt] f64: sum over k of (a_k - b_k)^2 of the f32 rows, formed in f64 - NOT the matcher's arithmetic but the quantity
    it stands for.  A difference of two f32 and its square are exact or correctly rounded in f64, and the 128-term f64 sum is
    accurate to about 1e-14 relative."""
    q, t = _rows(q).astype(np.float64), _rows(t).astype(np.float64)
    out = np.zeros((len(q), len(t)), np.float64)
    for lo in range(0, len(q), 32):
        d = q[lo:lo + 32, None, :] - t[None, :, :]
        out[lo:lo + 32] = (d * d).sum(axis=2)
    return out


def d2_bound(q, t):
    """[nq, nt] f64: B = 264 * 2^-24 * (|a|^2 + |b|^2), a bound on |d2 - exact_d2| that is derived, not measured.  With
    u = 2^-24, a 128-term fmaf chain errs by at most gamma_128 ~ 128 u times sum |a_k b_k|; the three chains of d2 contribute at
    most 128 u (n(a) + n(b) + 2 sum |a b|) <= 256 u (n(a) + n(b)), and the two remaining roundings (the sum, the difference)
    fewer than 8 u more of the same quantity."""
    q, t = _rows(q).astype(np.float64), _rows(t).astype(np.float64)
    return 264.0 * 2.0 ** -24 * ((q * q).sum(axis=1)[:, None] + (t * t).sum(axis=1)[None, :])


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


def crafted(rng, n, base=None, signed=False):
    """n rows like the reference's descriptors; with `base`, a quarter of them are exact copies of base rows (distance exactly 0)
    and a quarter are copies with sigma = 0.02 noise.  signed: every entry gets a random sign (cancellation in every chain) and
    the noisy copies keep theirs; otherwise all entries are non-negative."""
    d = reference_like_descriptors(rng, n)
    if signed:
        d = d * rng.choice(np.float32([-1.0, 1.0]), (n, 128))
    if base is not None and len(base) and n:
        k = rng.integers(0, len(base), n)
        noisy = base[k] + rng.normal(0, 0.02, (n, 128)).astype(np.float32)
        noisy = (noisy if signed else np.abs(noisy)).astype(np.float32)
        pick = rng.random(n)
        d[pick < 0.25] = base[k][pick < 0.25]
        d[(pick >= 0.25) & (pick < 0.5)] = noisy[(pick >= 0.25) & (pick < 0.5)]
    return d

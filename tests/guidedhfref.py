"""CPU restatement of guided matching under H or F (include/vslam.h, "guided matching under H or F"), bit for bit: the guided
pass of tests/guidedref.py with the candidate predicate chosen by the pair's kind - IN BAND under F (guidedref's in_band, as it
is), IN WINDOW under H (written out again from the header text), nothing without a model.  The C sources of matchref, epiref and
guidedref are compiled in front of the few lines here, gcc -O2 -ffp-contract=off: every f64 operation rounded on its own.  This
is the checker, not the product: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import epiref, guidedref, homref, matchref
from visualslam_amd import capi

NONE, F, H = 0, 1, 2  # the kind of a pair

_SRC = guidedref._SRC + r"""
/* train row (x', y') IN WINDOW of query row (x, y) under the homography Hm (row-major) */
static int in_window(const double* Hm, const double* q, const double* t, double max_transfer2) {
    if (q[0] != q[0] || t[0] != t[0]) return 0; /* not trusted */
    const double x = q[0], y = q[1], xp = t[0], yp = t[1];
    const double p0 = (Hm[0] * x + Hm[1] * y) + Hm[2], p1 = (Hm[3] * x + Hm[4] * y) + Hm[5], p2 = (Hm[6] * x + Hm[7] * y) + Hm[8];
    const double L = max_transfer2 * (p2 * p2);
    const double dx = p0 - xp * p2, dy = p1 - yp * p2;
    return p2 > 0 && dx * dx + dy * dy < L;
}
/* out [nq][nt] bytes */
void ref_window(const double* Hm, const double* qxy, size_t nq, const double* txy, size_t nt, double max_transfer2, uint8_t* out) {
    for (size_t i = 0; i < nq; ++i)
        for (size_t j = 0; j < nt; ++j) out[i * nt + j] = (uint8_t)in_window(Hm, qxy + 2 * i, txy + 2 * j, max_transfer2);
}

/* query rows q0 .. q1-1 against every train row; kind 0: no model, 1: F = m->F (m->best >= 0), 2: H = Hm */
void ref_guided_hf(const float* q, const uint8_t* qdef, const point* qp, const double* qxy, size_t q0, size_t q1, const float* qn,
                   const float* t, const uint8_t* tdef, const point* tp, const double* txy, size_t nt, const float* tn,
                   int kind, const model* m, const double* Hm, int same_octave, float ratio2, float max_desc_dist2, double max_dist2,
                   double max_transfer2, nn2* nn, uint8_t* accepted) {
    for (size_t i = q0; i < q1; ++i) {
        float best = INFINITY, second = INFINITY;
        int32_t index = -1;
        if (kind != 0 && (!qdef || qdef[i]) && qxy[2 * i] == qxy[2 * i]) {
            for (size_t j = 0; j < nt; ++j) {
                if (tdef && !tdef[j]) continue;
                if (same_octave && tp[j].octave != qp[i].octave) continue;
                if (kind == 1 ? !in_band(m, qxy + 2 * i, txy + 2 * j, max_dist2) : !in_window(Hm, qxy + 2 * i, txy + 2 * j, max_transfer2)) continue;
                const float sum = qn[i] + tn[j], twice = 2.0f * chain(q + 128 * i, t + 128 * j);
                const float d2 = sum - twice;
                if (d2 < best) { second = best; best = d2; index = (int32_t)j; }
                else if (d2 < second) second = d2;
            }
        }
        nn[i].index = index; nn[i].dist2 = best; nn[i].second_dist2 = second;
        const float lim = ratio2 * second;
        accepted[i] = index >= 0 && (second == INFINITY || best < lim) && best < max_desc_dist2;
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="guidedhfref_")
        src, so = os.path.join(d, "guidedhfref.c"), os.path.join(d, "guidedhfref.so")
        with open(src, "w") as f:
            f.write(_SRC)
        flags = ["-O2", "-ffp-contract=off", "-shared", "-fPIC"]
        try:  # as matchref: glibc's fmaf and the instruction agree bit for bit, the instruction is much faster
            if " fma " in open("/proc/cpuinfo").read().replace("\n", " "):
                flags.append("-mfma")
        except OSError:
            pass
        subprocess.run(["gcc", *flags, src, "-o", so, "-lm"], check=True, capture_output=True)
        _lib = C.CDLL(so)
    return _lib


_p = guidedref._p


def homography_record(Hm, best=0):
    """One capi.HOMOGRAPHY_DTYPE record with the given H (9 values) and `best` (G, which the rule does not read, stays zero)."""
    m = np.zeros(1, capi.HOMOGRAPHY_DTYPE)
    m["H"][0] = np.asarray(Hm, np.float64).reshape(9)
    m["best"] = best
    return m


def kind(epipolar_model, homography_model):
    """The kind of one pair from its two records (each an array of one record, or None)."""
    if epipolar_model is not None and int(np.asarray(epipolar_model).reshape(-1)["best"][0]) >= 0:
        return F
    if homography_model is not None and int(np.asarray(homography_model).reshape(-1)["best"][0]) >= 0:
        return H
    return NONE


def in_window(Hm, q_xy, t_xy, max_transfer2):
    """The predicate on one pair of (x, y) coordinates."""
    return bool(window(homography_record(Hm), None, None, max_transfer2, qxy=np.asarray([q_xy], np.float64), txy=np.asarray([t_xy], np.float64))[0, 0])


def window(homography_model, q_points, t_points, max_transfer2, qxy=None, txy=None):
    """bool [nq, nt]: train row j is in window of query row i under the record's H (its `best` is not looked at: that is kind()'s)."""
    m = np.ascontiguousarray(homography_model, dtype=capi.HOMOGRAPHY_DTYPE).reshape(-1)[:1]
    qxy = guidedref.rows_xy(q_points) if qxy is None else np.ascontiguousarray(qxy, dtype=np.float64)
    txy = guidedref.rows_xy(t_points) if txy is None else np.ascontiguousarray(txy, dtype=np.float64)
    out = np.zeros((len(qxy), len(txy)), np.uint8)
    Hm = np.ascontiguousarray(m["H"][0])
    lib().ref_window(_p(Hm), _p(qxy), C.c_size_t(len(qxy)), _p(txy), C.c_size_t(len(txy)), C.c_double(max_transfer2), _p(out))
    return out.astype(bool)


def guided_hf(q, t, q_points, t_points, epipolar_model=None, homography_model=None, ratio2=0.64, max_desc_dist2=np.inf, max_dist2=4.0,
              max_transfer2=4.0, same_octave=False, q_defined=None, t_defined=None):
    """-> (nn [nq] capi.NN2_DTYPE, matches capi.MATCH_DTYPE in ascending query order)."""
    assert epipolar_model is not None or homography_model is not None
    q, t = matchref._rows(q), matchref._rows(t)
    nq, nt = len(q), len(t)
    qp = np.ascontiguousarray(q_points, dtype=capi.POINT_DTYPE).reshape(-1)
    tp = np.ascontiguousarray(t_points, dtype=capi.POINT_DTYPE).reshape(-1)
    assert len(qp) == nq and len(tp) == nt
    k = kind(epipolar_model, homography_model)
    m = np.zeros(1, capi.EPIPOLAR_DTYPE) if k != F else np.ascontiguousarray(epipolar_model, dtype=capi.EPIPOLAR_DTYPE).reshape(-1)[:1]
    Hm = np.zeros(9) if k != H else np.ascontiguousarray(np.asarray(homography_model, dtype=capi.HOMOGRAPHY_DTYPE).reshape(-1)["H"][0])
    qdef = None if q_defined is None else np.ascontiguousarray(q_defined, dtype=np.uint8)
    tdef = None if t_defined is None else np.ascontiguousarray(t_defined, dtype=np.uint8)
    qxy, txy = guidedref.rows_xy(qp), guidedref.rows_xy(tp)
    qn, tn = matchref.norms(q), matchref.norms(t)
    nn = np.zeros(nq, capi.NN2_DTYPE)
    acc = np.zeros(nq, np.uint8)
    L = lib()

    def run(lo, hi):
        L.ref_guided_hf(_p(q), _p(qdef), _p(qp), _p(qxy), C.c_size_t(lo), C.c_size_t(hi), _p(qn), _p(t), _p(tdef), _p(tp), _p(txy), C.c_size_t(nt),
                        _p(tn), C.c_int(k), _p(m), _p(Hm), C.c_int(int(bool(same_octave))), C.c_float(ratio2), C.c_float(max_desc_dist2),
                        C.c_double(max_dist2), C.c_double(max_transfer2), _p(nn), _p(acc))

    step = max(64, (nq + 15) // 16)
    with ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL; the chunks write disjoint rows
        list(ex.map(lambda lo: run(lo, min(lo + step, nq)), range(0, nq, step)))
    idx = np.flatnonzero(acc)
    out = np.zeros(len(idx), capi.MATCH_DTYPE)
    out["query"], out["train"], out["dist2"] = idx, nn["index"][idx], nn["dist2"][idx]
    return nn, out


# ---- the fixture that shows what the pass is for (no library involved)

def repeated_scene(seed, kind, n=600, outliers=0.3, width=1920, height=1080):
    """guidedref.repeated_scene over homref.cameras(kind) ("plane", "rotation"; "general" is guidedref's scene itself): the same
    draws in the same order, so only the geometry differs."""
    rng = np.random.default_rng(seed)
    xq, xt = homref.cameras(rng, n, kind, width, height)
    planted = rng.random(n) >= outliers
    noise = np.stack([rng.uniform(0, width - 1, n), rng.uniform(0, height - 1, n)], axis=1)
    xt = np.where(planted[:, None], xt, noise)
    octave = rng.integers(0, 3, n).astype(np.int32)
    padding = rng.integers(0, 2, n).astype(np.int32)
    qp, tp = epiref.to_points(xq, octave, padding), epiref.to_points(xt, octave, padding)
    half = n // 2
    group = np.concatenate([np.arange(half), half + np.arange(n - half) // 3])
    base = matchref.reference_like_descriptors(rng, int(group.max()) + 1)
    q = np.abs(base[group] + rng.normal(0, 0.02, (n, 128)).astype(np.float32)).astype(np.float32)
    t = np.abs(base[group] + rng.normal(0, 0.02, (n, 128)).astype(np.float32)).astype(np.float32)
    fresh = matchref.reference_like_descriptors(rng, n)
    t[~planted] = fresh[~planted]
    perm = rng.permutation(n)
    ts, tps = np.zeros_like(t), np.zeros(n, capi.POINT_DTYPE)
    ts[perm], tps[perm] = t, tp
    return dict(q=q, t=ts, qp=qp, tp=tps, perm=perm, planted=planted)

"""CPU restatement of guided matching (include/vslam.h, "guided matching"), bit for bit: the matcher's d2 and sequential
nearest-two selection with one more skipped case - a train row outside the query row's epipolar band under the pair's F - and
the acceptance with its absolute bound.  d2 is matchref's chain and the coordinates are epiref's (the C sources of both are
compiled in front of the few lines here); the band predicate is written out again from the header text.  gcc -O2
-ffp-contract=off: every f64 operation rounded on its own.  This is the checker, not the product: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from tests import epiref, matchref
from visualslam_amd import capi

_SRC = matchref._SRC + epiref._SRC + r"""
/* (x, y) of one point by the two-view section's rule; NaN: the row is not trusted (octave outside 0 .. 31) */
static void row_xy(const point* p, double* xy) {
    const match self = {0, 0, 0.0f};
    double c[4];
    coords(&self, p, 1, p, 1, c);
    xy[0] = c[0]; xy[1] = c[1];
}
void ref_rows_xy(const point* p, size_t n, double* xy) {
    for (size_t i = 0; i < n; ++i) row_xy(p + i, xy + 2 * i);
}

/* train row (x', y') IN BAND of query row (x, y) under model m */
static int in_band(const model* m, const double* q, const double* t, double max_dist2) {
    if (m->best < 0) return 0;
    if (q[0] != q[0] || t[0] != t[0]) return 0; /* not trusted */
    const double* F = m->F;
    const double x = q[0], y = q[1], xp = t[0], yp = t[1];
    const double a0 = (F[0] * x + F[1] * y) + F[2], a1 = (F[3] * x + F[4] * y) + F[5], a2 = (F[6] * x + F[7] * y) + F[8];
    const double b0 = (F[0] * xp + F[3] * yp) + F[6], b1 = (F[1] * xp + F[4] * yp) + F[7];
    const double e = (xp * a0 + yp * a1) + a2;
    return e * e < max_dist2 * (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1);
}
/* out [nq][nt] bytes */
void ref_band(const model* m, const double* qxy, size_t nq, const double* txy, size_t nt, double max_dist2, uint8_t* out) {
    for (size_t i = 0; i < nq; ++i)
        for (size_t j = 0; j < nt; ++j) out[i * nt + j] = (uint8_t)in_band(m, qxy + 2 * i, txy + 2 * j, max_dist2);
}

/* query rows q0 .. q1-1 against every train row */
void ref_guided(const float* q, const uint8_t* qdef, const point* qp, const double* qxy, size_t q0, size_t q1, const float* qn,
                const float* t, const uint8_t* tdef, const point* tp, const double* txy, size_t nt, const float* tn,
                const model* m, int same_octave, float ratio2, float max_desc_dist2, double max_dist2, nn2* nn, uint8_t* accepted) {
    for (size_t i = q0; i < q1; ++i) {
        float best = INFINITY, second = INFINITY;
        int32_t index = -1;
        if ((!qdef || qdef[i]) && qxy[2 * i] == qxy[2 * i]) {
            for (size_t j = 0; j < nt; ++j) {
                if (tdef && !tdef[j]) continue;
                if (same_octave && tp[j].octave != qp[i].octave) continue;
                if (!in_band(m, qxy + 2 * i, txy + 2 * j, max_dist2)) continue;
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
        d = tempfile.mkdtemp(prefix="guidedref_")
        src, so = os.path.join(d, "guidedref.c"), os.path.join(d, "guidedref.so")
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


def _p(a):
    return C.c_void_p(None if a is None else a.ctypes.data)


def model_record(F, best=0):
    """One capi.EPIPOLAR_DTYPE record with the given F (9 values) and `best`."""
    m = np.zeros(1, capi.EPIPOLAR_DTYPE)
    m["F"][0] = np.asarray(F, np.float64).reshape(9)
    m["best"] = best
    return m


def rows_xy(points):
    """[n, 2] f64 (x, y) of POINT_DTYPE records; NaN rows are not trusted."""
    p = np.ascontiguousarray(points, dtype=capi.POINT_DTYPE).reshape(-1)
    out = np.zeros((len(p), 2), np.float64)
    lib().ref_rows_xy(_p(p), C.c_size_t(len(p)), _p(out))
    return out


def band(model, q_points, t_points, max_dist2):
    """bool [nq, nt]: train row j is in band of query row i."""
    m = np.ascontiguousarray(model, dtype=capi.EPIPOLAR_DTYPE).reshape(-1)[:1]
    qxy, txy = rows_xy(q_points), rows_xy(t_points)
    out = np.zeros((len(qxy), len(txy)), np.uint8)
    lib().ref_band(_p(m), _p(qxy), C.c_size_t(len(qxy)), _p(txy), C.c_size_t(len(txy)), C.c_double(max_dist2), _p(out))
    return out.astype(bool)


def guided(q, t, q_points, t_points, model, ratio2=0.64, max_desc_dist2=np.inf, max_dist2=4.0, same_octave=False, q_defined=None,
           t_defined=None):
    """-> (nn [nq] capi.NN2_DTYPE, matches capi.MATCH_DTYPE in ascending query order)."""
    q, t = matchref._rows(q), matchref._rows(t)
    nq, nt = len(q), len(t)
    qp = np.ascontiguousarray(q_points, dtype=capi.POINT_DTYPE).reshape(-1)
    tp = np.ascontiguousarray(t_points, dtype=capi.POINT_DTYPE).reshape(-1)
    assert len(qp) == nq and len(tp) == nt
    m = np.ascontiguousarray(model, dtype=capi.EPIPOLAR_DTYPE).reshape(-1)[:1]
    qdef = None if q_defined is None else np.ascontiguousarray(q_defined, dtype=np.uint8)
    tdef = None if t_defined is None else np.ascontiguousarray(t_defined, dtype=np.uint8)
    qxy, txy = rows_xy(qp), rows_xy(tp)
    qn, tn = matchref.norms(q), matchref.norms(t)
    nn = np.zeros(nq, capi.NN2_DTYPE)
    acc = np.zeros(nq, np.uint8)
    L = lib()

    def run(lo, hi):
        L.ref_guided(_p(q), _p(qdef), _p(qp), _p(qxy), C.c_size_t(lo), C.c_size_t(hi), _p(qn), _p(t), _p(tdef), _p(tp), _p(txy), C.c_size_t(nt),
                     _p(tn), _p(m), C.c_int(int(bool(same_octave))), C.c_float(ratio2), C.c_float(max_desc_dist2), C.c_double(max_dist2), _p(nn),
                     _p(acc))

    step = max(64, (nq + 15) // 16)
    with ThreadPoolExecutor(8) as ex:  # ctypes releases the GIL; the chunks write disjoint rows
        list(ex.map(lambda lo: run(lo, min(lo + step, nq)), range(0, nq, step)))
    idx = np.flatnonzero(acc)
    out = np.zeros(len(idx), capi.MATCH_DTYPE)
    out["query"], out["train"], out["dist2"] = idx, nn["index"][idx], nn["dist2"][idx]
    return nn, out


# ---- the fixture that shows what the pass is for (no library involved)

def repeated_scene(seed, n=600, outliers=0.3, width=1920, height=1080):
    """A planted two-view scene with repeated structure -> dict: q, t (f32 [n, 128]), qp, tp (POINT_DTYPE [n]), perm (train row of
    query row i's partner), planted (bool [n]).  Geometry as epiref.planted_scene; descriptors: points 0 .. n/2-1 each have a group
    of their own, points n/2 .. n-1 share one group per three consecutive points, both sides are |base[group] + N(0, 0.02)| drawn
    independently, unplanted train rows get a fresh descriptor, and the train side is permuted."""
    rng = np.random.default_rng(seed)
    xq, xt = epiref.two_cameras(rng, n, width, height)
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


def correct(matches, scene):
    """Number of records whose query is planted and whose train is the permuted partner."""
    m = np.asarray(matches)
    return int((scene["planted"][m["query"]] & (scene["perm"][m["query"]] == m["train"])).sum())

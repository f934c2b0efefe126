"""CPU restatement of the two-view geometry arithmetic (include/vslam.h, "two-view geometry"), bit for bit: the counter-hash
sampling, the normalised 8-point model with Gauss-Jordan elimination under full pivoting, the Jacobi rank-2 projection, the
Sampson inlier test without a division, and the selection.  A few lines of C, compiled once per process with
gcc -O2 -ffp-contract=off - every + - * / sqrt rounded on its own, sums left to right as the header writes them.  This is
the checker, not the product: the library has no CPU path.
"""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from visualslam_amd import capi

# The 3 x 3 pieces that the relative-pose restatement (tests/poseref.py) needs too: both C sources begin with this fragment.
GEOM3_SRC = r"""
#include <math.h>
/* S = M^T M; six sweeps of cyclic Jacobi with the eigenvectors accumulated in V: d [3] = diag S, V [3][3] */
void ref_gram_jacobi(const double* M, double* d, double* Vout) {
    double S[3][3], (*V)[3] = (double (*)[3])Vout;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { V[i][j] = i == j; S[i][j] = (M[i] * M[j] + M[3 + i] * M[3 + j]) + M[6 + i] * M[6 + j]; }
    static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2}, R[3] = {2, 1, 0};
    for (int sweep = 0; sweep < 6; ++sweep)
        for (int e = 0; e < 3; ++e) {
            const int p = P[e], q = Q[e], r = R[e];
            const double apq = S[p][q];
            if (apq == 0.0) continue;
            const double theta = (S[q][q] - S[p][p]) / (2.0 * apq);
            const double den = fabs(theta) + sqrt(theta * theta + 1.0);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / den;
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            const double app = S[p][p] - t * apq, aqq = S[q][q] + t * apq;
            const double arp = c * S[r][p] - s * S[r][q], arq = s * S[r][p] + c * S[r][q];
            S[p][p] = app; S[q][q] = aqq; S[p][q] = S[q][p] = 0.0;
            S[r][p] = S[p][r] = arp; S[r][q] = S[q][r] = arq;
            for (int i = 0; i < 3; ++i) {
                const double vp = c * V[i][p] - s * V[i][q], vq = s * V[i][p] + c * V[i][q];
                V[i][p] = vp; V[i][q] = vq;
            }
        }
    for (int i = 0; i < 3; ++i) d[i] = S[i][i];
}

/* H = L^T F R; L, R = {sx, sy, ax, ay} stand for [[sx, 0, ax], [0, sy, ay], [0, 0, 1]] */
void ref_lt_f_r(const double* L, const double* F, const double* R, double* H) {
    double G[9];
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = F[3 * i] * R[0]; G[3 * i + 1] = F[3 * i + 1] * R[1];
        G[3 * i + 2] = (F[3 * i] * R[2] + F[3 * i + 1] * R[3]) + F[3 * i + 2];
    }
    for (int j = 0; j < 3; ++j) {
        H[j] = L[0] * G[j]; H[3 + j] = L[1] * G[3 + j];
        H[6 + j] = (L[2] * G[j] + L[3] * G[3 + j]) + G[6 + j];
    }
}

double ref_frobenius(const double* M) {
    double n2 = M[0] * M[0];
    for (int i = 1; i < 9; ++i) n2 = n2 + M[i] * M[i];
    return sqrt(n2);
}
"""

_SRC = GEOM3_SRC + r"""
#include <stddef.h>
#include <stdint.h>
#include <string.h>
typedef struct { int32_t row, col, value, padding, octave, level; } point;
typedef struct { int32_t query, train; float dist2; } match;
typedef struct { double F[9]; uint32_t inliers; int32_t valid; } hyp;
typedef struct { double F[9]; uint32_t n_matches, n_inliers; int32_t best; uint32_t n_valid; } model;

uint32_t ref_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

int ref_sample(uint32_t seed, uint32_t j, uint32_t h, uint32_t m, uint32_t* idx) {
    if (m < 8) return 0;
    const uint32_t base = ref_mix(ref_mix(seed + j) + h);
    int n = 0;
    for (uint32_t t = 0; t < 64 && n < 8; ++t) {
        const uint32_t r = ref_mix(base + t);
        const uint32_t i = (uint32_t)(((uint64_t)r * m) >> 32);
        int seen = 0;
        for (int k = 0; k < n; ++k) seen |= idx[k] == i;
        if (!seen) idx[n++] = i;
    }
    return n == 8;
}

/* {x, y, x', y'} of one record; NaN for a record that is not trusted */
static void coords(const match* mt, const point* qp, uint32_t qcap, const point* tp, uint32_t tcap, double* c) {
    c[0] = c[1] = c[2] = c[3] = NAN;
    if ((uint32_t)mt->query >= qcap || (uint32_t)mt->train >= tcap) return;
    const point* q = qp + (uint32_t)mt->query;
    const point* t = tp + (uint32_t)mt->train;
    if ((uint32_t)q->octave > 31u || (uint32_t)t->octave > 31u) return;
    const double sq = q->octave == 0 ? 0.5 : (double)(1u << (q->octave - 1));
    const double st = t->octave == 0 ? 0.5 : (double)(1u << (t->octave - 1));
    c[0] = (double)((int64_t)q->col - (int64_t)q->padding) * sq;
    c[1] = (double)((int64_t)q->row - (int64_t)q->padding) * sq;
    c[2] = (double)((int64_t)t->col - (int64_t)t->padding) * st;
    c[3] = (double)((int64_t)t->row - (int64_t)t->padding) * st;
}
void ref_coords(const match* mt, size_t m, const point* qp, uint32_t qcap, const point* tp, uint32_t tcap, double* out) {
    for (size_t i = 0; i < m; ++i) coords(mt + i, qp, qcap, tp, tcap, out + 4 * i);
}

/* centroid, scale: 0 = degenerate */
static int normalise(const double* x, const double* y, double* cx, double* cy, double* s) {
    double sx = x[0], sy = y[0];
    for (int i = 1; i < 8; ++i) { sx = sx + x[i]; sy = sy + y[i]; }
    *cx = sx / 8.0; *cy = sy / 8.0;
    double d = 0.0;
    for (int i = 0; i < 8; ++i) {
        const double dx = x[i] - *cx, dy = y[i] - *cy;
        const double r = sqrt(dx * dx + dy * dy);
        d = i == 0 ? r : d + r;
    }
    d = d / 8.0;
    if (d == 0.0) return 0;
    *s = 1.4142135623730951 / d;
    return 1;
}

/* pts: 8 x {x, y, x', y'}; F row-major; 0 = invalid (F untouched) */
int ref_model_from_8(const double* pts, double* F, int rank2) {
    double qx[8], qy[8], tx[8], ty[8];
    for (int i = 0; i < 8; ++i) {
        qx[i] = pts[4 * i]; qy[i] = pts[4 * i + 1]; tx[i] = pts[4 * i + 2]; ty[i] = pts[4 * i + 3];
        if (qx[i] != qx[i] || tx[i] != tx[i]) return 0;
    }
    double cqx, cqy, sq, ctx, cty, st;
    if (!normalise(qx, qy, &cqx, &cqy, &sq)) return 0;
    if (!normalise(tx, ty, &ctx, &cty, &st)) return 0;
    double a[8][9];
    for (int i = 0; i < 8; ++i) {
        const double x = (qx[i] - cqx) * sq, y = (qy[i] - cqy) * sq, u = (tx[i] - ctx) * st, v = (ty[i] - cty) * st;
        a[i][0] = u * x; a[i][1] = u * y; a[i][2] = u; a[i][3] = v * x; a[i][4] = v * y; a[i][5] = v; a[i][6] = x; a[i][7] = y; a[i][8] = 1.0;
    }
    int used[9] = {0}, pc[8];
    for (int k = 0; k < 8; ++k) {
        double best = 0.0;
        int pr = -1, pcol = -1;
        for (int r = k; r < 8; ++r)
            for (int c = 0; c < 9; ++c) {
                if (used[c]) continue;
                const double v = fabs(a[r][c]);
                if (v > best) { best = v; pr = r; pcol = c; }
            }
        if (pr < 0 || !(best < INFINITY)) return 0;
        if (pr != k)
            for (int c = 0; c < 9; ++c) { const double t = a[k][c]; a[k][c] = a[pr][c]; a[pr][c] = t; }
        const double p = a[k][pcol];
        for (int c = 0; c < 9; ++c) a[k][c] = a[k][c] / p;
        for (int r = 0; r < 8; ++r) {
            if (r == k) continue;
            const double f = a[r][pcol];
            for (int c = 0; c < 9; ++c) a[r][c] = a[r][c] - f * a[k][c];
        }
        used[pcol] = 1; pc[k] = pcol;
    }
    int fr = 0;
    while (used[fr]) ++fr;
    double f[9];
    f[fr] = 1.0;
    for (int k = 0; k < 8; ++k) f[pc[k]] = -a[k][fr];
    if (rank2) {
        double S[3], V[9];
        ref_gram_jacobi(f, S, V);
        int k = 0;
        if (S[1] < S[k]) k = 1;
        if (S[2] < S[k]) k = 2;
        const double v0 = V[k], v1 = V[3 + k], v2 = V[6 + k];
        for (int i = 0; i < 3; ++i) {
            const double g = (f[3 * i] * v0 + f[3 * i + 1] * v1) + f[3 * i + 2] * v2;
            f[3 * i] = f[3 * i] - g * v0; f[3 * i + 1] = f[3 * i + 1] - g * v1; f[3 * i + 2] = f[3 * i + 2] - g * v2;
        }
    }
    /* F <- Tt^T F Tq, T = [[s, 0, -(s cx)], [0, s, -(s cy)], [0, 0, 1]] */
    const double Tq[4] = {sq, sq, -(sq * cqx), -(sq * cqy)}, Tt[4] = {st, st, -(st * ctx), -(st * cty)};
    double H[9];
    ref_lt_f_r(Tt, f, Tq, H);
    const double n = ref_frobenius(H);
    if (n == 0.0 || !(n < INFINITY)) return 0;
    for (int i = 0; i < 9; ++i) F[i] = H[i] / n;
    return 1;
}

static int inlier(const double* F, const double* c, double max_dist2) {
    const double x = c[0], y = c[1], u = c[2], v = c[3];
    const double a0 = (F[0] * x + F[1] * y) + F[2], a1 = (F[3] * x + F[4] * y) + F[5], a2 = (F[6] * x + F[7] * y) + F[8];
    const double b0 = (F[0] * u + F[3] * v) + F[6], b1 = (F[1] * u + F[4] * v) + F[7];
    const double e = (u * a0 + v * a1) + a2;
    const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    return e * e < max_dist2 * den;
}

/* inlier flags (one byte per record) of F over m coordinate records; returns the count */
uint32_t ref_score(const double* F, const double* xy, size_t m, double max_dist2, uint8_t* flags) {
    uint32_t n = 0;
    for (size_t i = 0; i < m; ++i) {
        const int in = inlier(F, xy + 4 * i, max_dist2);
        if (flags) flags[i] = (uint8_t)in;
        n += (uint32_t)in;
    }
    return n;
}

/* one pair; hyps [H]; flags [m] bytes */
void ref_ransac(const match* mt, uint32_t m, const point* qp, uint32_t qcap, const point* tp, uint32_t tcap, uint32_t seed, uint32_t j,
                uint32_t H, double max_dist2, double* xy, hyp* hyps, model* out, uint8_t* flags) {
    ref_coords(mt, m, qp, qcap, tp, tcap, xy);
    int best = -1;
    uint32_t nvalid = 0;
    for (uint32_t h = 0; h < H; ++h) {
        memset(&hyps[h], 0, sizeof(hyp));
        uint32_t idx[8];
        double pts[32];
        if (!ref_sample(seed, j, h, m, idx)) continue;
        for (int i = 0; i < 8; ++i) memcpy(pts + 4 * i, xy + 4 * (size_t)idx[i], 32);
        if (!ref_model_from_8(pts, hyps[h].F, 1)) { memset(&hyps[h], 0, sizeof(hyp)); continue; }
        hyps[h].valid = 1;
        hyps[h].inliers = ref_score(hyps[h].F, xy, m, max_dist2, NULL);
        ++nvalid;
        if (best < 0 || hyps[h].inliers > hyps[best].inliers) best = (int)h;
    }
    memset(out, 0, sizeof(model));
    out->n_matches = m; out->best = best; out->n_valid = nvalid;
    memset(flags, 0, m);
    if (best >= 0) {
        memcpy(out->F, hyps[best].F, sizeof out->F);
        out->n_inliers = ref_score(out->F, xy, m, max_dist2, flags);
    }
}
"""

_lib = None


def compile_c(name, text):
    """-> the C source `text` as a ctypes library, built the way every restatement is."""
    d = tempfile.mkdtemp(prefix=name + "_")
    src, so = os.path.join(d, name + ".c"), os.path.join(d, name + ".so")
    with open(src, "w") as f:
        f.write(text)
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so, "-lm"], check=True, capture_output=True)
    return C.CDLL(so)


def lib():
    global _lib
    if _lib is None:
        L = compile_c("epiref", _SRC)
        L.ref_mix.restype = C.c_uint32
        L.ref_score.restype = C.c_uint32
        L.ref_frobenius.restype = C.c_double
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def mix(x):
    return int(lib().ref_mix(C.c_uint32(x & 0xFFFFFFFF)))


def sample(seed, j, h, m):
    """The 8 distinct record indices of hypothesis h of pair j over m records, or None (invalid sample)."""
    idx = np.zeros(8, np.uint32)
    ok = lib().ref_sample(C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(j), C.c_uint32(h), C.c_uint32(m), _p(idx))
    return [int(i) for i in idx] if ok else None


def coords(matches, query_points, train_points):
    """[m, 4] f64 {x, y, x', y'} in image pixels; NaN rows for records that are not trusted."""
    mt = np.ascontiguousarray(matches, dtype=capi.MATCH_DTYPE).reshape(-1)
    qp = np.ascontiguousarray(query_points, dtype=capi.POINT_DTYPE).reshape(-1)
    tp = np.ascontiguousarray(train_points, dtype=capi.POINT_DTYPE).reshape(-1)
    out = np.zeros((len(mt), 4), np.float64)
    lib().ref_coords(_p(mt), C.c_size_t(len(mt)), _p(qp), C.c_uint32(len(qp)), _p(tp), C.c_uint32(len(tp)), _p(out))
    return out


def model_from_8(pts, rank2=True):
    """pts [8, 4] f64 {x, y, x', y'} -> F [3, 3] (x'^T F x = 0, Frobenius norm 1) or None.  rank2=False leaves out step 4
    (only to show what the step is for)."""
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(8, 4)
    F = np.zeros(9, np.float64)
    return F.reshape(3, 3) if lib().ref_model_from_8(_p(p), _p(F), C.c_int(int(rank2))) else None


def score(F, xy, max_dist2):
    """-> (count, flags bool [m]) of the Sampson test of F over coordinate records xy [m, 4]."""
    F = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 4)
    flags = np.zeros(len(xy), np.uint8)
    n = lib().ref_score(_p(F), _p(xy), C.c_size_t(len(xy)), C.c_double(max_dist2), _p(flags))
    return int(n), flags.astype(bool)


def exact_inlier(F, xy, max_dist2):
    """The Sampson predicate e^2 < max_dist2 * den of F over coordinate records xy [m, 4] in exact rational arithmetic (the
    inputs are doubles, so fractions.Fraction loses nothing) - NOT the header's rounded operations but the inequality they
    stand for.  -> (inlier bool [m], near bool [m], trusted bool [m]); `near`: the two sides differ by no more than
    2^-40 * (T^2 + max_dist2 * den), T = |x' a0| + |y' a1| + |a2|, about 2^12 roundings of the quantities being compared, where
    the rounded test may fall on either side.  Records with NaN coordinates are not trusted and are never inliers."""
    from fractions import Fraction as Q

    f = [Q(float(v)) for v in np.asarray(F, np.float64).reshape(9)]
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 4)
    md, eps = Q(float(max_dist2)), Q(1, 2 ** 40)
    inl, near, trusted = (np.zeros(len(xy), bool) for _ in range(3))
    for i, rec in enumerate(xy):
        if np.isnan(rec).any():
            continue
        x, y, u, v = (Q(float(c)) for c in rec)
        a0, a1, a2 = f[0] * x + f[1] * y + f[2], f[3] * x + f[4] * y + f[5], f[6] * x + f[7] * y + f[8]
        b0, b1 = f[0] * u + f[3] * v + f[6], f[1] * u + f[4] * v + f[7]
        e = u * a0 + v * a1 + a2
        rhs = md * (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1)
        T = abs(u * a0) + abs(v * a1) + abs(a2)
        trusted[i], inl[i], near[i] = True, e * e < rhs, abs(e * e - rhs) <= eps * (T * T + rhs)
    return inl, near, trusted


def ransac(matches, query_points, train_points, n_hypotheses, seed, max_dist2, pair=0):
    """One pair -> (model [1] capi.EPIPOLAR_DTYPE, flags bool [m], hypotheses [H] capi.EPIPOLAR_HYP_DTYPE).  `pair`: the index j
    the pair has inside a batched call (it enters the sampling hash)."""
    mt = np.ascontiguousarray(matches, dtype=capi.MATCH_DTYPE).reshape(-1)
    qp = np.ascontiguousarray(query_points, dtype=capi.POINT_DTYPE).reshape(-1)
    tp = np.ascontiguousarray(train_points, dtype=capi.POINT_DTYPE).reshape(-1)
    m, H = len(mt), int(n_hypotheses)
    xy = np.zeros((max(m, 1), 4), np.float64)
    hyps = np.zeros(H, capi.EPIPOLAR_HYP_DTYPE)
    out = np.zeros(1, capi.EPIPOLAR_DTYPE)
    flags = np.zeros(max(m, 1), np.uint8)
    lib().ref_ransac(_p(mt), C.c_uint32(m), _p(qp), C.c_uint32(len(qp)), _p(tp), C.c_uint32(len(tp)), C.c_uint32(seed & 0xFFFFFFFF),
                     C.c_uint32(pair), C.c_uint32(H), C.c_double(max_dist2), _p(xy), _p(hyps), _p(out), _p(flags))
    return out, flags[:m].astype(bool), hyps


def bits(flags, words):
    """The ballot words of a flag vector: bit i % 64 of word i / 64, `words` words."""
    b = np.zeros(words * 64, np.uint8)
    b[: len(flags)] = flags
    return np.packbits(b, bitorder="little").view(np.uint64)


# ---- planted data (no library involved)

def two_cameras(rng, n, width=1920, height=1080, f=800.0, yaw=0.05, baseline=0.5):
    """n random 3-D points seen by two cameras (focal length f, the second yawed and moved along x): pixel coordinates
    (xq [n, 2], xt [n, 2]) as exact f64, every point inside both images."""
    K = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1.0]])
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.array([-baseline, 0, 0])
    q, tr = [], []
    while len(q) < n:
        X = np.array([rng.uniform(-6, 6), rng.uniform(-3.5, 3.5), rng.uniform(4, 12)])
        a, b = K @ X, K @ (R @ X + t)
        a, b = a[:2] / a[2], b[:2] / b[2]
        if 0 <= a[0] < width - 1 and 0 <= a[1] < height - 1 and 0 <= b[0] < width - 1 and 0 <= b[1] < height - 1:
            q.append(a), tr.append(b)
    return np.array(q), np.array(tr)


def to_points(xy, octave, padding):
    """Pixel coordinates -> POINT_DTYPE records at each point's octave pitch 2^(octave - 1), rounded to the lattice."""
    p = np.zeros(len(xy), capi.POINT_DTYPE)
    pitch = 2.0 ** (np.asarray(octave) - 1)
    p["col"] = np.rint(xy[:, 0] / pitch).astype(np.int32) + padding
    p["row"] = np.rint(xy[:, 1] / pitch).astype(np.int32) + padding
    p["padding"], p["octave"], p["level"] = padding, octave, 1
    return p


def planted_scene(seed, n=300, outliers=0.3, width=1920, height=1080):
    """-> (matches [n], query points [n], train points [n], planted inlier flags [n]): matches of a two-camera scene, octaves 0 .. 2
    and paddings 0 / 1 mixed, coordinates rounded to the octave pitch, the train list shuffled, and a fraction `outliers` of the
    train points replaced by uniform noise."""
    rng = np.random.default_rng(seed)
    xq, xt = two_cameras(rng, n, width, height)
    planted = rng.random(n) >= outliers
    noise = np.stack([rng.uniform(0, width - 1, n), rng.uniform(0, height - 1, n)], axis=1)
    xt = np.where(planted[:, None], xt, noise)
    octave = rng.integers(0, 3, n).astype(np.int32)
    padding = rng.integers(0, 2, n).astype(np.int32)
    qp, tp = to_points(xq, octave, padding), to_points(xt, octave, padding)
    perm = rng.permutation(n)
    tps = np.zeros(n, capi.POINT_DTYPE)
    tps[perm] = tp
    m = np.zeros(n, capi.MATCH_DTYPE)
    m["query"], m["train"], m["dist2"] = np.arange(n), perm, rng.random(n).astype(np.float32)
    return m, qp, tps, planted

"""CPU restatement of the resection arithmetic (include/vslam.h, "resection"), bit for bit, written from the header text alone:
the link by index is a Python dictionary (the first live record of pair j - 1 per train index, chainref.live_records); the
gather, the 6-record counter-hash sample, the calibrated DLT with Gauss-Jordan elimination under full pivoting, the rotation by
Jacobi sweeps, the reprojection test without a division and the selection are a few lines of C, compiled like every
restatement (epiref.compile_c: gcc -O2 -ffp-contract=off).  This is the checker, not the product: the library has no CPU path.
"""
import ctypes as C

import numpy as np

from tests import chainref, epiref
from visualslam_amd import capi

_SRC = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
typedef struct { double R[9], t[3]; uint32_t inliers; int32_t valid; } hyp;
typedef struct { double Y[3], u, v; uint32_t b, reserved; } corr;
typedef struct { double R[9], t[3]; uint32_t n_obs, n_corr, n_inliers; int32_t best; uint32_t n_valid, reserved; } model;
typedef struct { double R[9]; double t[3]; uint32_t n_matches, n_front; int32_t best; int32_t valid; } pose;
typedef struct { int32_t row, col, value, padding, octave, level; } point;
typedef struct { int32_t query, train; float dist2; } match;

static uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
static int fin(double x) { return x == x && x != INFINITY && x != -INFINITY; }

/* step 2: m observation records of pair j >= 1 with their links a [m] (-1: none); X = points of pair j - 1, tp the train
   points of pair j (tcap of them), K = {fx, fy, cx, cy}.  out: the dense list; usable [m] bytes; returns n_corr */
uint32_t res_gather(const pose* prev, const double* X, const int32_t* a, const match* obs, uint32_t m, const point* tp, uint32_t tcap,
                    const double* K, corr* out, uint8_t* usable) {
    uint32_t n = 0;
    const double* R = prev->R;
    const double* t = prev->t;
    for (uint32_t b = 0; b < m; ++b) {
        usable[b] = 0;
        const uint32_t tr = (uint32_t)obs[b].train;
        if (a[b] < 0 || tr >= tcap) continue;
        const point p = tp[tr];
        if (p.octave < 0 || p.octave > 31) continue;
        const double s = ldexp(1.0, p.octave - 1);
        const double xp = (double)((int64_t)p.col - (int64_t)p.padding) * s, yp = (double)((int64_t)p.row - (int64_t)p.padding) * s;
        corr c;
        memset(&c, 0, sizeof c);
        c.u = (xp - K[2]) / K[0];
        c.v = (yp - K[3]) / K[1];
        const double* x = X + 3 * (size_t)a[b];
        for (int i = 0; i < 3; ++i) c.Y[i] = ((R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2]) + t[i];
        if (!fin(c.Y[0]) || !fin(c.Y[1]) || !fin(c.Y[2])) continue;
        c.b = b;
        usable[b] = 1;
        out[n++] = c;
    }
    return n;
}

int res_sample6(uint32_t seed, uint32_t j, uint32_t h, uint32_t m, uint32_t* idx) {
    if (m < 6) return 0;
    const uint32_t base = mix(mix(seed + j) + h);
    int n = 0;
    for (uint32_t d = 0; d < 64 && n < 6; ++d) {
        const uint32_t i = (uint32_t)(((uint64_t)mix(base + d) * m) >> 32);
        int k = 0;
        while (k < n && idx[k] != i) ++k;
        if (k == n) idx[n++] = i;
    }
    return n == 6;
}

/* the pose section's sweeps: S = M^T M, V = I, six sweeps over (0,1), (0,2), (1,2) */
static void jacobi(const double* M, double S[3][3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            S[i][j] = (M[i] * M[j] + M[3 + i] * M[3 + j]) + M[6 + i] * M[6 + j];
            V[i][j] = i == j;
        }
    static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2}, Rr[3] = {2, 1, 0};
    for (int sweep = 0; sweep < 6; ++sweep)
        for (int e = 0; e < 3; ++e) {
            const int p = P[e], q = Q[e], r = Rr[e];
            if (S[p][q] == 0.0) continue;
            const double theta = (S[q][q] - S[p][p]) / (2.0 * S[p][q]);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
            const double spp = S[p][p] - t * S[p][q], sqq = S[q][q] + t * S[p][q];
            const double srp = c * S[r][p] - s * S[r][q], srq = s * S[r][p] + c * S[r][q];
            S[p][p] = spp; S[q][q] = sqq; S[p][q] = S[q][p] = 0.0;
            S[r][p] = S[p][r] = srp; S[r][q] = S[q][r] = srq;
            for (int i = 0; i < 3; ++i) {
                const double vp = c * V[i][p] - s * V[i][q], vq = s * V[i][p] + c * V[i][q];
                V[i][p] = vp; V[i][q] = vq;
            }
        }
}
static void cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
static void mulv(const double* M, const double* v, double* w) {
    for (int i = 0; i < 3; ++i) w[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}
static double norm3(const double* w) { return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }
static int bad_norm(double n) { return n == 0.0 || !(n < INFINITY); }

/* c6: 6 x {Y0, Y1, Y2, u, v}; 0 = invalid (R, t untouched).  Mm (12 doubles, may be NULL): M and m of step 4 */
int res_model_from_6(const double* c6, double* R, double* t, double* Mm) {
    double cen[3], r[6];
    for (int k = 0; k < 3; ++k) cen[k] = (((((c6[k] + c6[5 + k]) + c6[10 + k]) + c6[15 + k]) + c6[20 + k]) + c6[25 + k]) / 6.0;
    for (int i = 0; i < 6; ++i) {
        const double e0 = c6[5 * i] - cen[0], e1 = c6[5 * i + 1] - cen[1], e2 = c6[5 * i + 2] - cen[2];
        r[i] = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    }
    const double d = (((((r[0] + r[1]) + r[2]) + r[3]) + r[4]) + r[5]) / 6.0;
    if (d == 0.0) return 0;
    const double s = 1.7320508075688772 / d;
    double a[12][12];
    for (int i = 0; i < 6; ++i) {
        const double N0 = (c6[5 * i] - cen[0]) * s, N1 = (c6[5 * i + 1] - cen[1]) * s, N2 = (c6[5 * i + 2] - cen[2]) * s;
        const double u = c6[5 * i + 3], v = c6[5 * i + 4];
        double* e = a[2 * i]; double* o = a[2 * i + 1];
        e[0] = N0; e[1] = N1; e[2] = N2; e[3] = 1.0; e[4] = e[5] = e[6] = e[7] = 0.0;
        e[8] = -(u * N0); e[9] = -(u * N1); e[10] = -(u * N2); e[11] = -u;
        o[0] = o[1] = o[2] = o[3] = 0.0; o[4] = N0; o[5] = N1; o[6] = N2; o[7] = 1.0;
        o[8] = -(v * N0); o[9] = -(v * N1); o[10] = -(v * N2); o[11] = -v;
    }
    int chosen[12] = {0}, col[11];
    for (int k = 0; k < 11; ++k) {
        double big = 0.0;
        int br = -1, bc = -1;
        for (int rr = k; rr < 12; ++rr)
            for (int c = 0; c < 12; ++c)
                if (!chosen[c] && fabs(a[rr][c]) > big) { big = fabs(a[rr][c]); br = rr; bc = c; }
        if (br < 0 || big == INFINITY) return 0;
        for (int c = 0; c < 12; ++c) { const double x = a[k][c]; a[k][c] = a[br][c]; a[br][c] = x; }
        const double piv = a[k][bc];
        for (int c = 0; c < 12; ++c) a[k][c] = a[k][c] / piv;
        for (int i = 0; i < 12; ++i)
            if (i != k) {
                const double g = a[i][bc];
                for (int c = 0; c < 12; ++c) a[i][c] = a[i][c] - g * a[k][c];
            }
        chosen[bc] = 1; col[k] = bc;
    }
    int fr = 0;
    while (chosen[fr]) ++fr;
    double p[12];
    p[fr] = 1.0;
    for (int k = 0; k < 11; ++k) p[col[k]] = -a[k][fr];
    double M[9], m[3];
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) M[3 * i + k] = p[4 * i + k] * s;
        m[i] = p[4 * i + 3] - ((M[3 * i] * cen[0] + M[3 * i + 1] * cen[1]) + M[3 * i + 2] * cen[2]);
    }
    const double det = (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
    if (det == 0.0 || !fin(det)) return 0;
    if (det < 0.0) {
        for (int i = 0; i < 9; ++i) M[i] = -M[i];
        for (int i = 0; i < 3; ++i) m[i] = -m[i];
    }
    if (Mm) { memcpy(Mm, M, sizeof M); memcpy(Mm + 9, m, sizeof m); }
    double S[3][3], V[3][3];
    jacobi(M, S, V);
    int k = 0;
    if (S[1][1] < S[k][k]) k = 1;
    if (S[2][2] < S[k][k]) k = 2;
    const int pi = k == 0 ? 1 : 0, qi = k == 2 ? 1 : 2;
    double v1[3], v2[3], v3[3], w1[3], w2[3], w3[3], u1[3], u2[3], u3[3];
    for (int i = 0; i < 3; ++i) { v1[i] = V[i][pi]; v2[i] = V[i][qi]; }
    cross(v1, v2, v3);
    mulv(M, v1, w1);
    const double n1 = norm3(w1);
    if (bad_norm(n1)) return 0;
    for (int i = 0; i < 3; ++i) u1[i] = w1[i] / n1;
    mulv(M, v2, w2);
    const double g = (u1[0] * w2[0] + u1[1] * w2[1]) + u1[2] * w2[2];
    for (int i = 0; i < 3; ++i) w2[i] = w2[i] - g * u1[i];
    const double n2 = norm3(w2);
    if (bad_norm(n2)) return 0;
    for (int i = 0; i < 3; ++i) u2[i] = w2[i] / n2;
    cross(u1, u2, u3);
    mulv(M, v3, w3);
    const double n3 = norm3(w3);
    const double lam = ((n1 + n2) + n3) / 3.0;
    if (bad_norm(lam)) return 0;
    double Rc[9], tc[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            Rc[3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
            if (!fin(Rc[3 * i + j])) return 0;
        }
        tc[i] = m[i] / lam;
        if (!fin(tc[i])) return 0;
    }
    memcpy(R, Rc, sizeof Rc); memcpy(t, tc, sizeof tc);
    return 1;
}

static int inlier(const double* R, const double* t, double fx, double fy, const corr* c, double md) {
    const double* Y = c->Y;
    const double Z0 = ((R[0] * Y[0] + R[1] * Y[1]) + R[2] * Y[2]) + t[0];
    const double Z1 = ((R[3] * Y[0] + R[4] * Y[1]) + R[5] * Y[2]) + t[1];
    const double Z2 = ((R[6] * Y[0] + R[7] * Y[1]) + R[8] * Y[2]) + t[2];
    const double ex = (c->u * Z2 - Z0) * fx, ey = (c->v * Z2 - Z1) * fy;
    return Z2 > 0.0 && (ex * ex + ey * ey) < md * (Z2 * Z2);
}

uint32_t res_score(const double* R, const double* t, double fx, double fy, const corr* cs, size_t n, double md, uint8_t* flags) {
    uint32_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        const int in = inlier(R, t, fx, fy, cs + i, md);
        if (flags) flags[i] = (uint8_t)in;
        k += (uint32_t)in;
    }
    return k;
}

/* one pair over its dense list cs [n]; hyps [NH]; flags [n] bytes (per correspondence) */
void res_ransac(const corr* cs, uint32_t n, uint32_t n_obs, uint32_t seed, uint32_t j, uint32_t NH, double md, double fx, double fy, hyp* hyps,
                model* out, uint8_t* flags) {
    int best = -1;
    uint32_t nvalid = 0;
    for (uint32_t h = 0; h < NH; ++h) {
        memset(&hyps[h], 0, sizeof(hyp));
        uint32_t idx[6];
        double c6[30];
        if (!res_sample6(seed, j, h, n, idx)) continue;
        for (int i = 0; i < 6; ++i) memcpy(c6 + 5 * i, &cs[idx[i]], 40);
        if (!res_model_from_6(c6, hyps[h].R, hyps[h].t, NULL)) continue;
        hyps[h].valid = 1;
        hyps[h].inliers = res_score(hyps[h].R, hyps[h].t, fx, fy, cs, n, md, NULL);
        ++nvalid;
        if (best < 0 || hyps[h].inliers > hyps[best].inliers) best = (int)h;
    }
    memset(out, 0, sizeof(model));
    out->n_obs = n_obs; out->n_corr = n; out->best = best; out->n_valid = nvalid;
    memset(flags, 0, n);
    if (best >= 0) {
        memcpy(out->R, hyps[best].R, sizeof out->R); memcpy(out->t, hyps[best].t, sizeof out->t);
        out->n_inliers = res_score(out->R, out->t, fx, fy, cs, n, md, flags);
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = epiref.compile_c("resectref", _SRC)
        L.res_gather.restype = C.c_uint32
        L.res_score.restype = C.c_uint32
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def sample6(seed, j, h, m):
    """The 6 distinct dense-list indices of hypothesis h of pair j over m correspondences, or None (invalid sample)."""
    idx = np.zeros(6, np.uint32)
    ok = lib().res_sample6(C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(j), C.c_uint32(h), C.c_uint32(m), _p(idx))
    return [int(i) for i in idx] if ok else None


def model_from_6(c6, want_M=False):
    """c6 [6, 5] f64 {Y0, Y1, Y2, u, v} -> (R [3, 3], t [3]) or None; with want_M also (M [3, 3], m [3]) of step 4."""
    c = np.ascontiguousarray(c6, dtype=np.float64).reshape(6, 5)
    R, t, Mm = np.zeros(9), np.zeros(3), np.zeros(12)
    if not lib().res_model_from_6(_p(c), _p(R), _p(t), _p(Mm)):
        return None
    return (R.reshape(3, 3), t, Mm[:9].reshape(3, 3), Mm[9:]) if want_M else (R.reshape(3, 3), t)


def as_corr(Y, u, v):
    """A RESECT_CORR_DTYPE list from Y [n, 3], u [n], v [n] (b = the row)."""
    Y = np.asarray(Y, np.float64).reshape(-1, 3)
    c = np.zeros(len(Y), capi.RESECT_CORR_DTYPE)
    c["Y"], c["u"], c["v"], c["b"] = Y, u, v, np.arange(len(Y))
    return c


def score(R, t, K, corr, max_dist2):
    """-> (count, flags bool [n]) of the reprojection test of (R, t) over a RESECT_CORR_DTYPE list."""
    R, t = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    cs = np.ascontiguousarray(corr, dtype=capi.RESECT_CORR_DTYPE).reshape(-1)
    n = len(cs)
    buf = cs if n else np.zeros(1, capi.RESECT_CORR_DTYPE)
    flags = np.zeros(max(n, 1), np.uint8)
    k = lib().res_score(_p(R), _p(t), C.c_double(K[0]), C.c_double(K[1]), _p(buf), C.c_size_t(n), C.c_double(max_dist2), _p(flags))
    return int(k), flags[:n].astype(bool)


def exact_inlier(R, t, K, corr, max_dist2):
    """The reprojection predicate in exact rational arithmetic (the inputs are doubles, so fractions.Fraction loses nothing): NOT
    the header's rounded operations but the inequality they stand for, with the stored (R, t).  -> (inlier bool [n], near bool
    [n]).  With A_k = |R[k][0] Y0| + |R[k][1] Y1| + |R[k][2] Y2| + |t_k| (Z_k with every term in absolute value) and T = fx *
    (|u| A2 + A0) + fy * (|v| A2 + A1):  `near`: the two sides of the distance inequality differ by no more than 2^-40 * (T^2 +
    max_dist2 * A2^2) - about 2^12 roundings of the quantities compared -, or |Z2| <= 2^-40 * A2: there the rounded test may
    fall on either side."""
    from fractions import Fraction as Q

    r, tt = [Q(float(x)) for x in np.asarray(R, np.float64).reshape(9)], [Q(float(x)) for x in np.asarray(t, np.float64).reshape(3)]
    fx, fy, md, eps = Q(float(K[0])), Q(float(K[1])), Q(float(max_dist2)), Q(1, 2 ** 40)
    cs = np.ascontiguousarray(corr, dtype=capi.RESECT_CORR_DTYPE).reshape(-1)
    inl, near = np.zeros(len(cs), bool), np.zeros(len(cs), bool)
    for i, c in enumerate(cs):
        Y, u, v = [Q(float(x)) for x in c["Y"]], Q(float(c["u"])), Q(float(c["v"]))
        Z = [r[3 * k] * Y[0] + r[3 * k + 1] * Y[1] + r[3 * k + 2] * Y[2] + tt[k] for k in range(3)]
        A = [abs(r[3 * k] * Y[0]) + abs(r[3 * k + 1] * Y[1]) + abs(r[3 * k + 2] * Y[2]) + abs(tt[k]) for k in range(3)]
        ex, ey = (u * Z[2] - Z[0]) * fx, (v * Z[2] - Z[1]) * fy
        lhs, rhs = ex * ex + ey * ey, md * Z[2] * Z[2]
        T = fx * (abs(u) * A[2] + A[0]) + fy * (abs(v) * A[2] + A[1])
        inl[i] = Z[2] > 0 and lhs < rhs
        near[i] = abs(lhs - rhs) <= eps * (T * T + md * A[2] * A[2]) or abs(Z[2]) <= eps * A[2]
    return inl, near


ARGS = ("poses", "matches", "match_counts", "points", "front_bits", "point_cap", "obs_matches", "obs_counts", "train_points", "K")


def run(inputs, n_hypotheses, seed, max_dist2):
    """resect() over a dict of its inputs (synthetic(), or a test's own)."""
    return resect(*(inputs[k] for k in ARGS), n_hypotheses, seed, max_dist2)


def synthetic(n_pairs, n_pts, seed, K=(800.0, 800.0, 960.0, 540.0), no_pose=()):
    """Planted inputs (no library involved): n_pts points of a rigid scene seen by n_pairs + 1 cameras, x_{j+1} = R_j x_j + s_j t_j
    with |t_j| = 1; point i has index i in every frame.  Structure side as vslam_pose_dev would leave it: poses (R_j, t_j) with
    best = 0 (-1 for the pairs in no_pose), record i = (query i, train i), all in front, points[j] = x_j / s_j (pair j's unit).
    Observation side: the same records, and frame j + 1's pixels at mixed octaves and paddings (epiref.to_points).  -> a dict of
    the arrays resect() takes, with the true (R_j, s_j t_j / s_{j-1}) under "truth"."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-4, 4, n_pts), rng.uniform(-2.5, 2.5, n_pts), rng.uniform(6, 12, n_pts)], 1)
    poses, mt = np.zeros(n_pairs, capi.POSE_DTYPE), np.zeros((n_pairs, n_pts), capi.MATCH_DTYPE)
    pts, bits = np.zeros((n_pairs, n_pts, 3)), np.zeros((n_pairs, (n_pts + 63) // 64), np.uint64)
    tp = np.zeros((n_pairs, n_pts), capi.POINT_DTYPE)
    truth, s_prev = [], 1.0
    for j in range(n_pairs):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = rng.uniform(-0.05, 0.05)
        A = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        R = np.eye(3) + np.sin(ang) * A + (1 - np.cos(ang)) * A @ A
        t = rng.normal(size=3) * [1.0, 0.2, 0.2]
        t /= np.linalg.norm(t)
        s = rng.uniform(0.3, 0.9)
        valid = j not in no_pose
        poses["R"][j], poses["t"][j], poses["best"][j], poses["valid"][j], poses["n_matches"][j] = R.reshape(9), t, 0 if valid else -1, 1, n_pts
        mt["query"][j] = mt["train"][j] = np.arange(n_pts)
        pts[j] = x / s
        if valid:
            bits[j] = epiref.bits(np.ones(n_pts, bool), bits.shape[1])
        x = x @ R.T + s * t
        pix = np.stack([K[0] * x[:, 0] / x[:, 2] + K[2], K[1] * x[:, 1] / x[:, 2] + K[3]], 1)
        tp[j] = epiref.to_points(pix, rng.integers(0, 3, n_pts).astype(np.int32), rng.integers(0, 2, n_pts).astype(np.int32))
        truth.append((R, s * t / s_prev))
        s_prev = s
    cnt = np.full(n_pairs, n_pts, np.uint32)
    return dict(poses=poses, matches=mt, match_counts=cnt, points=pts, front_bits=bits, point_cap=n_pts, obs_matches=mt.copy(), obs_counts=cnt.copy(),
                train_points=tp, K=tuple(float(v) for v in K), truth=truth)


def links_of(prev_live, prev_matches, obs, n_obs, point_cap):
    """Step 2's link of every observation record: the lowest live record of pair j - 1 per train index, looked up by query."""
    first = {}
    for i in np.flatnonzero(prev_live):
        first.setdefault(int(prev_matches["train"][i]) & 0xFFFFFFFF, int(i))
    a = np.full(n_obs, -1, np.int32)
    for b in range(n_obs):
        q = int(obs["query"][b]) & 0xFFFFFFFF
        if q < point_cap:
            a[b] = first.get(q, -1)
    return a


def resect(poses, matches, match_counts, points, front_bits, point_cap, obs_matches, obs_counts, train_points, K, n_hypotheses, seed, max_dist2,
           first_pair=0):
    """The whole step over n pairs: the structure side as chainref.chain takes it, obs_matches [n, obs_cap] capi.MATCH_DTYPE,
    obs_counts [n], train_points [n, train_cap] capi.POINT_DTYPE, K = (fx, fy, cx, cy) -> (models [n] capi.RESECT_DTYPE, and per
    pair: links int32 [n_obs], correspondences [n_corr] capi.RESECT_CORR_DTYPE, inlier flags bool [n_obs], hypotheses [NH]
    capi.RESECT_HYP_DTYPE).  `first_pair` is added to the pair index where it enters the sampling hash (the same as seed +
    first_pair: a call whose pair 0 is pair s of a longer one)."""
    ps = np.ascontiguousarray(poses, dtype=capi.POSE_DTYPE).reshape(-1)
    n, NH = len(ps), int(n_hypotheses)
    mt = np.ascontiguousarray(matches, dtype=capi.MATCH_DTYPE).reshape(n, -1)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(n, mt.shape[1], 3)
    fb = np.ascontiguousarray(front_bits).view(np.uint64).reshape(n, -1)
    ob = np.ascontiguousarray(obs_matches, dtype=capi.MATCH_DTYPE).reshape(n, -1)
    tp = np.ascontiguousarray(train_points, dtype=capi.POINT_DTYPE).reshape(n, -1)
    Kc = np.array([float(v) for v in K], np.float64)
    models = np.zeros(n, capi.RESECT_DTYPE)
    links, corrs, flags, hyps = [], [], [], []
    live_prev = None
    for j in range(n):
        _, live = chainref.live_records(ps[j], mt[j], match_counts[j], fb[j], point_cap)
        n_obs = min(int(obs_counts[j]), ob.shape[1])
        a = links_of(live_prev, mt[j - 1], ob[j], n_obs, point_cap) if j >= 1 else np.full(n_obs, -1, np.int32)
        dense = np.zeros(max(n_obs, 1), capi.RESECT_CORR_DTYPE)
        usable = np.zeros(max(n_obs, 1), np.uint8)
        nc = 0
        if j >= 1 and n_obs:
            ab, obj = np.ascontiguousarray(a), np.ascontiguousarray(ob[j])
            nc = lib().res_gather(_p(ps[j - 1:j]), _p(np.ascontiguousarray(pts[j - 1])), _p(ab), _p(obj), C.c_uint32(n_obs),
                                  _p(np.ascontiguousarray(tp[j])), C.c_uint32(tp.shape[1]), _p(Kc), _p(dense), _p(usable))
        hy = np.zeros(NH, capi.RESECT_HYP_DTYPE)
        cf = np.zeros(max(nc, 1), np.uint8)
        lib().res_ransac(_p(dense), C.c_uint32(nc), C.c_uint32(n_obs), C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(j + first_pair), C.c_uint32(NH),
                         C.c_double(max_dist2), C.c_double(Kc[0]), C.c_double(Kc[1]), _p(hy), _p(models[j:j + 1]), _p(cf))
        fl = np.zeros(n_obs, bool)
        fl[dense["b"][:nc]] = cf[:nc].astype(bool)
        links.append(a), corrs.append(dense[:nc].copy()), flags.append(fl), hyps.append(hy)
        live_prev = live
    return models, links, corrs, flags, hyps

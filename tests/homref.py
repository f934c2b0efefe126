"""CPU restatement of the homography arithmetic and the degeneracy verdict (include/vslam.h, "homography and the degeneracy
verdict"), bit for bit: the 4-record counter-hash sample, the normalised DLT with Gauss-Jordan elimination under full
pivoting, the sign rules, the adjugate, the symmetric-transfer inlier test without a division, the selection, the integer
verdict and the gate.  A few lines of C written from the header's text, compiled like every restatement
(epiref.compile_c: gcc -O2 -ffp-contract=off).  This is the checker, not the product: the library has no CPU path.
"""
import ctypes as C

import numpy as np

from tests import epiref
from visualslam_amd import capi

_SRC = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
typedef struct { double H[9], G[9]; uint32_t inliers; int32_t valid; } hyp;
typedef struct { double H[9], G[9]; uint32_t n_matches, n_inliers; int32_t best; uint32_t n_valid, n_epipolar; int32_t degenerate; } model;

static uint32_t mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

int hom_sample4(uint32_t seed, uint32_t j, uint32_t h, uint32_t m, uint32_t* idx) {
    if (m < 4) return 0;
    const uint32_t base = mix(mix(seed + j) + h);
    int n = 0;
    for (uint32_t t = 0; t < 64 && n < 4; ++t) {
        const uint32_t i = (uint32_t)(((uint64_t)mix(base + t) * m) >> 32);
        int k = 0;
        while (k < n && idx[k] != i) ++k;
        if (k == n) idx[n++] = i;
    }
    return n == 4;
}

/* step 1 for one side: v = {x, y} pairs with stride 4 doubles */
static int side(const double* v, double* cx, double* cy, double* s) {
    *cx = (((v[0] + v[4]) + v[8]) + v[12]) / 4.0;
    *cy = (((v[1] + v[5]) + v[9]) + v[13]) / 4.0;
    double r[4];
    for (int i = 0; i < 4; ++i) {
        const double dx = v[4 * i] - *cx, dy = v[4 * i + 1] - *cy;
        r[i] = sqrt(dx * dx + dy * dy);
    }
    const double d = (((r[0] + r[1]) + r[2]) + r[3]) / 4.0;
    if (d == 0.0) return 0;
    *s = 1.4142135623730951 / d;
    return 1;
}

/* pts: 4 x {x, y, x', y'}; 0 = invalid (H, G untouched) */
int hom_model_from_4(const double* pts, double* H, double* G) {
    for (int i = 0; i < 16; ++i) if (pts[i] != pts[i]) return 0;
    double cqx, cqy, sq, ctx, cty, st;
    if (!side(pts, &cqx, &cqy, &sq)) return 0;
    if (!side(pts + 2, &ctx, &cty, &st)) return 0;
    double a[8][9];
    for (int i = 0; i < 4; ++i) {
        const double x = (pts[4 * i] - cqx) * sq, y = (pts[4 * i + 1] - cqy) * sq;
        const double xp = (pts[4 * i + 2] - ctx) * st, yp = (pts[4 * i + 3] - cty) * st;
        double* e = a[2 * i]; double* o = a[2 * i + 1];
        e[0] = x; e[1] = y; e[2] = 1.0; e[3] = 0.0; e[4] = 0.0; e[5] = 0.0; e[6] = -(xp * x); e[7] = -(xp * y); e[8] = -xp;
        o[0] = 0.0; o[1] = 0.0; o[2] = 0.0; o[3] = x; o[4] = y; o[5] = 1.0; o[6] = -(yp * x); o[7] = -(yp * y); o[8] = -yp;
    }
    int chosen[9] = {0}, col[8];
    for (int k = 0; k < 8; ++k) {
        double big = 0.0;
        int br = -1, bc = -1;
        for (int r = k; r < 8; ++r)
            for (int c = 0; c < 9; ++c)
                if (!chosen[c] && fabs(a[r][c]) > big) { big = fabs(a[r][c]); br = r; bc = c; }
        if (br < 0 || big == INFINITY) return 0;
        for (int c = 0; c < 9; ++c) { const double t = a[k][c]; a[k][c] = a[br][c]; a[br][c] = t; }
        const double piv = a[k][bc];
        for (int c = 0; c < 9; ++c) a[k][c] = a[k][c] / piv;
        for (int i = 0; i < 8; ++i)
            if (i != k) {
                const double g = a[i][bc];
                for (int c = 0; c < 9; ++c) a[i][c] = a[i][c] - g * a[k][c];
            }
        chosen[bc] = 1; col[k] = bc;
    }
    int fr = 0;
    while (chosen[fr]) ++fr;
    double hn[9];
    hn[fr] = 1.0;
    for (int k = 0; k < 8; ++k) hn[col[k]] = -a[k][fr];
    const double aq = -(sq * cqx), bq = -(sq * cqy), r = 1.0 / st;
    double G1[3][3], M[9];
    for (int i = 0; i < 3; ++i) {
        G1[i][0] = hn[3 * i] * sq; G1[i][1] = hn[3 * i + 1] * sq;
        G1[i][2] = (hn[3 * i] * aq + hn[3 * i + 1] * bq) + hn[3 * i + 2];
    }
    for (int j = 0; j < 3; ++j) {
        M[j] = r * G1[0][j] + ctx * G1[2][j];
        M[3 + j] = r * G1[1][j] + cty * G1[2][j];
        M[6 + j] = G1[2][j];
    }
    double n2 = M[0] * M[0];
    for (int i = 1; i < 9; ++i) n2 = n2 + M[i] * M[i];
    const double n = sqrt(n2);
    if (n == 0.0 || !(n < INFINITY)) return 0;
    double h[9], g[9];
    for (int i = 0; i < 9; ++i) h[i] = M[i] / n;
    const double w = (h[6] * pts[0] + h[7] * pts[1]) + h[8];
    if (w < 0.0) { for (int i = 0; i < 9; ++i) h[i] = -h[i]; }
    else if (!(w > 0.0)) return 0;
#define AD(a_, b_, c_, d_) (h[a_] * h[b_] - h[c_] * h[d_])
    g[0] = AD(4, 8, 5, 7); g[1] = AD(2, 7, 1, 8); g[2] = AD(1, 5, 2, 4);
    g[3] = AD(5, 6, 3, 8); g[4] = AD(0, 8, 2, 6); g[5] = AD(2, 3, 0, 5);
    g[6] = AD(3, 7, 4, 6); g[7] = AD(1, 6, 0, 7); g[8] = AD(0, 4, 1, 3);
    const double wg = (g[6] * pts[2] + g[7] * pts[3]) + g[8];
    if (wg != wg || wg == 0.0 || wg == INFINITY || wg == -INFINITY) return 0;
    if (wg < 0.0) for (int i = 0; i < 9; ++i) g[i] = -g[i];
    memcpy(H, h, sizeof h); memcpy(G, g, sizeof g);
    return 1;
}

static int transfer(const double* A, double x, double y, double u, double v, double md) {
    const double p0 = (A[0] * x + A[1] * y) + A[2], p1 = (A[3] * x + A[4] * y) + A[5], p2 = (A[6] * x + A[7] * y) + A[8];
    const double dx = p0 - u * p2, dy = p1 - v * p2;
    return p2 > 0.0 && dx * dx + dy * dy < md * (p2 * p2);
}

uint32_t hom_score(const double* H, const double* G, const double* xy, size_t m, double md, uint8_t* flags) {
    uint32_t n = 0;
    for (size_t i = 0; i < m; ++i) {
        const double* c = xy + 4 * i;
        const int in = transfer(H, c[0], c[1], c[2], c[3], md) && transfer(G, c[2], c[3], c[0], c[1], md);
        if (flags) flags[i] = (uint8_t)in;
        n += (uint32_t)in;
    }
    return n;
}

/* one pair over its coordinate records xy [m][4]; hyps [NH]; flags [m] bytes */
void hom_ransac(const double* xy, uint32_t m, uint32_t seed, uint32_t j, uint32_t NH, double md, hyp* hyps, model* out, uint8_t* flags) {
    int best = -1;
    uint32_t nvalid = 0;
    for (uint32_t h = 0; h < NH; ++h) {
        memset(&hyps[h], 0, sizeof(hyp));
        uint32_t idx[4];
        double pts[16];
        if (!hom_sample4(seed, j, h, m, idx)) continue;
        for (int i = 0; i < 4; ++i) memcpy(pts + 4 * i, xy + 4 * (size_t)idx[i], 32);
        if (!hom_model_from_4(pts, hyps[h].H, hyps[h].G)) continue;
        hyps[h].valid = 1;
        hyps[h].inliers = hom_score(hyps[h].H, hyps[h].G, xy, m, md, NULL);
        ++nvalid;
        if (best < 0 || hyps[h].inliers > hyps[best].inliers) best = (int)h;
    }
    memset(out, 0, sizeof(model));
    out->n_matches = m; out->best = best; out->n_valid = nvalid;
    memset(flags, 0, m);
    if (best >= 0) {
        memcpy(out->H, hyps[best].H, sizeof out->H); memcpy(out->G, hyps[best].G, sizeof out->G);
        out->n_inliers = hom_score(out->H, out->G, xy, m, md, flags);
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = epiref.compile_c("homref", _SRC)
        L.hom_score.restype = C.c_uint32
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def sample4(seed, j, h, m):
    """The 4 distinct record indices of hypothesis h of pair j over m records, or None (invalid sample)."""
    idx = np.zeros(4, np.uint32)
    ok = lib().hom_sample4(C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(j), C.c_uint32(h), C.c_uint32(m), _p(idx))
    return [int(i) for i in idx] if ok else None


def model_from_4(pts):
    """pts [4, 4] f64 {x, y, x', y'} -> (H [3, 3] query -> train with Frobenius norm 1, G [3, 3] train -> query) or None."""
    p = np.ascontiguousarray(pts, dtype=np.float64).reshape(4, 4)
    H, G = np.zeros(9, np.float64), np.zeros(9, np.float64)
    return (H.reshape(3, 3), G.reshape(3, 3)) if lib().hom_model_from_4(_p(p), _p(H), _p(G)) else None


def score(H, G, xy, max_dist2):
    """-> (count, flags bool [m]) of the symmetric-transfer test of (H, G) over coordinate records xy [m, 4]."""
    H, G = (np.ascontiguousarray(a, dtype=np.float64).reshape(9) for a in (H, G))
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 4)
    flags = np.zeros(max(len(xy), 1), np.uint8)
    n = lib().hom_score(_p(H), _p(G), _p(xy), C.c_size_t(len(xy)), C.c_double(max_dist2), _p(flags))
    return int(n), flags[: len(xy)].astype(bool)


def exact_inlier(H, G, xy, max_dist2):
    """The two transfer predicates in exact rational arithmetic (the inputs are doubles, so fractions.Fraction loses nothing):
    NOT the header's rounded operations but the inequalities they stand for, with the stored (H, G).  -> (inlier bool [m],
    near bool [m], trusted bool [m]).  `near`: in either direction the two sides of the distance inequality differ by no more
    than 2^-40 * (T^2 + max_dist2 * p2^2), T = |p0| + |p1| + (|x'| + |y'|) * |p2| - about 2^12 roundings of the quantities
    compared -, or |p2| <= 2^-40 * (|H20 x| + |H21 y| + |H22|): there the rounded test may fall on either side."""
    from fractions import Fraction as Q

    h, g = ([Q(float(v)) for v in np.asarray(a, np.float64).reshape(9)] for a in (H, G))
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 4)
    md, eps = Q(float(max_dist2)), Q(1, 2 ** 40)
    inl, near, trusted = (np.zeros(len(xy), bool) for _ in range(3))

    def one(A, x, y, u, v):
        p0, p1, p2 = A[0] * x + A[1] * y + A[2], A[3] * x + A[4] * y + A[5], A[6] * x + A[7] * y + A[8]
        dx, dy = p0 - u * p2, p1 - v * p2
        lhs, rhs = dx * dx + dy * dy, md * p2 * p2
        T = abs(p0) + abs(p1) + (abs(u) + abs(v)) * abs(p2)
        close = abs(lhs - rhs) <= eps * (T * T + rhs) or abs(p2) <= eps * (abs(A[6] * x) + abs(A[7] * y) + abs(A[8]))
        return p2 > 0 and lhs < rhs, close

    for i, rec in enumerate(xy):
        if np.isnan(rec).any():
            continue
        x, y, u, v = (Q(float(c)) for c in rec)
        (f, fn), (b, bn) = one(h, x, y, u, v), one(g, u, v, x, y)
        trusted[i], inl[i], near[i] = True, f and b, fn or bn
    return inl, near, trusted


def ransac(matches, query_points, train_points, n_hypotheses, seed, max_dist2, pair=0):
    """One pair -> (model [1] capi.HOMOGRAPHY_DTYPE with n_epipolar = degenerate = 0, flags bool [m], hypotheses [H]
    capi.HOMOGRAPHY_HYP_DTYPE).  `pair`: the index j the pair has inside a batched call (it enters the sampling hash)."""
    xy = epiref.coords(matches, query_points, train_points)
    m, NH = len(xy), int(n_hypotheses)
    xy = np.ascontiguousarray(xy if m else np.zeros((1, 4)))
    hyps = np.zeros(NH, capi.HOMOGRAPHY_HYP_DTYPE)
    out = np.zeros(1, capi.HOMOGRAPHY_DTYPE)
    flags = np.zeros(max(m, 1), np.uint8)
    lib().hom_ransac(_p(xy), C.c_uint32(m), C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(pair), C.c_uint32(NH), C.c_double(max_dist2), _p(hyps),
                     _p(out), _p(flags))
    return out, flags[:m].astype(bool), hyps


def verdict(model, epipolar, num=1, den=2, min_inliers=16):
    """The header's verdict, Python integers (no width to overflow): -> a copy of the HOMOGRAPHY_DTYPE record(s) `model` with
    n_epipolar and degenerate set from the EPIPOLAR_DTYPE record(s) `epipolar` (None: no verdict, both 0)."""
    out = np.array(model, dtype=capi.HOMOGRAPHY_DTYPE, copy=True).reshape(-1)
    out["n_epipolar"], out["degenerate"] = 0, 0
    if epipolar is None:
        return out
    epi = np.asarray(epipolar, dtype=capi.EPIPOLAR_DTYPE).reshape(-1)
    for j in range(len(out)):
        ne = int(epi["n_inliers"][j]) if int(epi["best"][j]) >= 0 else 0
        nh = int(out["n_inliers"][j])
        out["n_epipolar"][j] = ne
        out["degenerate"][j] = int(int(out["best"][j]) >= 0 and int(epi["best"][j]) >= 0 and nh >= int(min_inliers) and nh * int(den) >= int(num) * ne)
    return out


def gate(epipolar, judged):
    """-> the gated copy of the EPIPOLAR_DTYPE record(s): a degenerate pair becomes the "no model" record."""
    out = np.array(epipolar, dtype=capi.EPIPOLAR_DTYPE, copy=True).reshape(-1)
    deg = np.asarray(judged).reshape(-1)["degenerate"] != 0
    out["F"][deg], out["n_inliers"][deg], out["best"][deg] = 0.0, 0, -1
    return out


# ---- planted data (no library involved): epiref.two_cameras' construction, with the two degenerate variants

KINDS = ("general", "plane", "rotation")


def cameras(rng, n, kind, width=1920, height=1080, f=800.0, yaw=0.05, baseline=0.5):
    """kind "general": epiref.two_cameras itself.  "plane": the same cameras, every point on Z = 8 + 0.3 X - 0.2 Y.
    "rotation": the same cameras with the baseline set to zero (pure yaw)."""
    if kind == "general":
        return epiref.two_cameras(rng, n, width, height, f, yaw, baseline)
    K = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1.0]])
    R = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    t = np.array([0.0 if kind == "rotation" else -baseline, 0, 0])
    q, tr = [], []
    while len(q) < n:
        X = np.array([rng.uniform(-6, 6), rng.uniform(-3.5, 3.5), rng.uniform(4, 12)])
        if kind == "plane":
            X[2] = 8 + 0.3 * X[0] - 0.2 * X[1]
        a, b = K @ X, K @ (R @ X + t)
        a, b = a[:2] / a[2], b[:2] / b[2]
        if 0 <= a[0] < width - 1 and 0 <= a[1] < height - 1 and 0 <= b[0] < width - 1 and 0 <= b[1] < height - 1:
            q.append(a), tr.append(b)
    return np.array(q), np.array(tr)


def planted_scene(seed, n=300, kind="general", outliers=0.3, width=1920, height=1080):
    """epiref.planted_scene's construction over cameras(kind): -> (matches [n], query points [n], train points [n], planted
    inlier flags [n])."""
    rng = np.random.default_rng(seed)
    xq, xt = cameras(rng, n, kind, width, height)
    planted = rng.random(n) >= outliers
    noise = np.stack([rng.uniform(0, width - 1, n), rng.uniform(0, height - 1, n)], axis=1)
    xt = np.where(planted[:, None], xt, noise)
    octave = rng.integers(0, 3, n).astype(np.int32)
    padding = rng.integers(0, 2, n).astype(np.int32)
    qp, tp = epiref.to_points(xq, octave, padding), epiref.to_points(xt, octave, padding)
    perm = rng.permutation(n)
    tps = np.zeros(n, capi.POINT_DTYPE)
    tps[perm] = tp
    m = np.zeros(n, capi.MATCH_DTYPE)
    m["query"], m["train"], m["dist2"] = np.arange(n), perm, rng.random(n).astype(np.float32)
    return m, qp, tps, planted

"""CPU restatement of the refinement of the resected pose (include/vslam.h, "resection: Gauss-Newton refinement over all
inliers"), bit for bit, written from the header text alone: the member test, the ordered sum over the dense rows, the residual
and the two Jacobian rows of a member, the 29 sums, the 6 x 7 Gauss-Jordan under full pivoting, the Cayley update and the
acceptance rule.  A few lines of C compiled like every restatement (epiref.compile_c: gcc -O2 -ffp-contract=off); it shares
nothing with the kernels.  This is the checker, not the product: the library has no CPU path.
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
typedef struct { double Y[3], u, v; uint32_t b, reserved; } corr;
typedef struct { double R[9], t[3]; uint32_t n_obs, n_corr, n_inliers; int32_t best; uint32_t n_valid, reserved; } model;
typedef struct { uint32_t n_before, n_after, accepted; int32_t stop; double cost_before, cost_after; } info;

static int fin(double x) { return x == x && x != INFINITY && x != -INFINITY; }
static double canon(double x) {
    if (x == x) return x;
    const uint64_t q = 0x7ff8000000000000ull;
    double d;
    memcpy(&d, &q, 8);
    return d;
}

static int member(const double* R, const double* t, double fx, double fy, const corr* c, double md, double* Z) {
    const double* Y = c->Y;
    Z[0] = ((R[0] * Y[0] + R[1] * Y[1]) + R[2] * Y[2]) + t[0];
    Z[1] = ((R[3] * Y[0] + R[4] * Y[1]) + R[5] * Y[2]) + t[1];
    Z[2] = ((R[6] * Y[0] + R[7] * Y[1]) + R[8] * Y[2]) + t[2];
    const double ex = (c->u * Z[2] - Z[0]) * fx, ey = (c->v * Z[2] - Z[1]) * fy;
    return Z[2] > 0.0 && (ex * ex + ey * ey) < md * (Z[2] * Z[2]);
}

/* the ordered sum of term[r], r < m; a row with flag[r] == 0 contributes +0.0 */
double rr_ordered_sum(const double* term, const uint8_t* flag, size_t m) {
    double total = 0.0;
    const size_t blocks = (m + 4095) / 4096;
    for (size_t b = 0; b < blocks; ++b) {
        double s[256];
        for (int l = 0; l < 256; ++l) {
            s[l] = 0.0;
            for (int k = 0; k < 16; ++k) {
                const size_t r = 4096 * b + 256 * (size_t)k + (size_t)l;
                if (r >= m) continue;
                s[l] = s[l] + (flag[r] ? term[r] : 0.0);
            }
        }
        for (int h = 128; h >= 1; h >>= 1)
            for (int l = 0; l < h; ++l) s[l] = s[l] + s[l + h];
        total = b == 0 ? s[0] : total + s[0];
    }
    return total;
}

/* EVALUATE: sums [29] = H's upper triangle row-major, g, cost, n.  terms [29][m] and flag [m] are scratch */
void rr_evaluate(const double* R, const double* t, double fx, double fy, const corr* cs, size_t m, double md, double* terms, uint8_t* flag,
                 double* sums) {
    for (size_t r = 0; r < m; ++r) {
        double Z[3];
        flag[r] = (uint8_t)member(R, t, fx, fy, cs + r, md, Z);
        if (!flag[r]) {
            for (int e = 0; e < 29; ++e) terms[(size_t)e * m + r] = 0.0;
            continue;
        }
        const double u = cs[r].u, v = cs[r].v;
        const double iz = 1.0 / Z[2];
        const double px = Z[0] * iz, py = Z[1] * iz;
        const double rx = (px - u) * fx, ry = (py - v) * fy;
        const double pxy = px * py;
        const double Jx[6] = {fx * (-pxy), fx * (1.0 + px * px), fx * (-py), fx * iz, fx * 0.0, fx * (-(px * iz))};
        const double Jy[6] = {fy * (-(1.0 + py * py)), fy * pxy, fy * px, fy * 0.0, fy * iz, fy * (-(py * iz))};
        int e = 0;
        for (int p = 0; p < 6; ++p)
            for (int q = p; q < 6; ++q, ++e) terms[(size_t)e * m + r] = Jx[p] * Jx[q] + Jy[p] * Jy[q];
        for (int p = 0; p < 6; ++p) terms[(size_t)(21 + p) * m + r] = Jx[p] * rx + Jy[p] * ry;
        terms[(size_t)27 * m + r] = rx * rx + ry * ry;
        terms[(size_t)28 * m + r] = 1.0;
    }
    for (int e = 0; e < 29; ++e) sums[e] = rr_ordered_sum(terms + (size_t)e * m, flag, m);
}

/* STEP: 0 = invalid; delta [6] (may be NULL) gets d */
int rr_step(const double* R, const double* t, const double* sums, double* Rn, double* tn, double* delta) {
    double a[6][7];
    int e = 0;
    for (int p = 0; p < 6; ++p) {
        for (int q = p; q < 6; ++q, ++e) a[p][q] = a[q][p] = sums[e];
        a[p][6] = -sums[21 + p];
    }
    int chosen[6] = {0}, col[6];
    for (int k = 0; k < 6; ++k) {
        double big = 0.0;
        int br = -1, bc = -1;
        for (int r = k; r < 6; ++r)
            for (int c = 0; c < 6; ++c)
                if (!chosen[c] && fabs(a[r][c]) > big) { big = fabs(a[r][c]); br = r; bc = c; }
        if (br < 0 || big == INFINITY) return 0;
        for (int c = 0; c < 7; ++c) { const double x = a[k][c]; a[k][c] = a[br][c]; a[br][c] = x; }
        const double piv = a[k][bc];
        for (int c = 0; c < 7; ++c) a[k][c] = a[k][c] / piv;
        for (int i = 0; i < 6; ++i)
            if (i != k) {
                const double g = a[i][bc];
                for (int c = 0; c < 7; ++c) a[i][c] = a[i][c] - g * a[k][c];
            }
        chosen[bc] = 1; col[k] = bc;
    }
    double d[6];
    for (int k = 0; k < 6; ++k) d[col[k]] = a[k][6];
    if (delta) memcpy(delta, d, sizeof d);
    for (int k = 0; k < 6; ++k) if (!fin(d[k])) return 0;
    const double a0 = d[0] / 2.0, a1 = d[1] / 2.0, a2 = d[2] / 2.0;
    const double q = (a0 * a0 + a1 * a1) + a2 * a2;
    const double ee = 1.0 - q, den = 1.0 + q;
    double D[3][3];
    D[0][0] = (ee + 2.0 * (a0 * a0)) / den;
    D[1][1] = (ee + 2.0 * (a1 * a1)) / den;
    D[2][2] = (ee + 2.0 * (a2 * a2)) / den;
    D[0][1] = (2.0 * (a0 * a1) - 2.0 * a2) / den;
    D[1][0] = (2.0 * (a1 * a0) + 2.0 * a2) / den;
    D[0][2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
    D[2][0] = (2.0 * (a2 * a0) - 2.0 * a1) / den;
    D[1][2] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
    D[2][1] = (2.0 * (a2 * a1) + 2.0 * a0) / den;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            Rn[3 * i + j] = (D[i][0] * R[j] + D[i][1] * R[3 + j]) + D[i][2] * R[6 + j];
            if (!fin(Rn[3 * i + j])) return 0;
        }
        tn[i] = ((D[i][0] * t[0] + D[i][1] * t[1]) + D[i][2] * t[2]) + d[3 + i];
        if (!fin(tn[i])) return 0;
    }
    return 1;
}

/* one pair: cs [obs_cap] (the first min(in->n_corr, obs_cap) rows are read); flags [obs_cap] bytes per observation record;
   terms [29][obs_cap], work [obs_cap]: scratch; trace [rounds + 1][12] (may be NULL): the pose kept after the input's evaluation
   and after every round that ran to its end */
void rr_refine(const model* in, const corr* cs, uint32_t obs_cap, uint32_t rounds, double md, double fx, double fy, double* terms, uint8_t* work,
               model* out, info* inf, uint8_t* flags, double* trace) {
    const uint32_t m = in->n_corr < obs_cap ? in->n_corr : obs_cap, n_obs = in->n_obs < obs_cap ? in->n_obs : obs_cap;
    *out = *in;
    memset(inf, 0, sizeof *inf);
    memset(flags, 0, obs_cap);
    if (in->best < 0) { inf->stop = 5; return; }
    double Rc[9], tc[3], Rn[9], tn[3], sc[29], sn[29];
    memcpy(Rc, in->R, sizeof Rc); memcpy(tc, in->t, sizeof tc);
    rr_evaluate(Rc, tc, fx, fy, cs, m, md, terms, work, sc);
    uint32_t n_cur = (uint32_t)sc[28];
    double cost_cur = sc[27];
    inf->n_before = n_cur; inf->cost_before = canon(cost_cur);
    if (trace) { memcpy(trace, Rc, sizeof Rc); memcpy(trace + 9, tc, sizeof tc); }
    int stop = 0;
    for (uint32_t r = 1; r <= rounds; ++r) {
        if (n_cur < 6) { stop = 1; break; }
        if (!rr_step(Rc, tc, sc, Rn, tn, NULL)) { stop = 3; break; }
        rr_evaluate(Rn, tn, fx, fy, cs, m, md, terms, work, sn);
        const uint32_t n_new = (uint32_t)sn[28];
        if (n_new > n_cur || (n_new == n_cur && sn[27] < cost_cur)) {
            memcpy(Rc, Rn, sizeof Rc); memcpy(tc, tn, sizeof tc); memcpy(sc, sn, sizeof sc);
            n_cur = n_new; cost_cur = sn[27]; inf->accepted += 1;
            if (trace) { memcpy(trace + 12 * r, Rc, sizeof Rc); memcpy(trace + 12 * r + 9, tc, sizeof tc); }
        } else { stop = 4; break; }
    }
    inf->stop = stop; inf->n_after = n_cur; inf->cost_after = canon(cost_cur);
    for (int k = 0; k < 9; ++k) out->R[k] = canon(Rc[k]);
    for (int k = 0; k < 3; ++k) out->t[k] = canon(tc[k]);
    out->n_inliers = n_cur;
    for (uint32_t r = 0; r < m; ++r) {
        double Z[3];
        if (cs[r].b < n_obs && member(out->R, out->t, fx, fy, cs + r, md, Z)) flags[cs[r].b] = 1;
    }
}
"""

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = epiref.compile_c("resectrefineref", _SRC)
        L.rr_ordered_sum.restype = C.c_double
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _corr(corr):
    cs = np.ascontiguousarray(corr, dtype=capi.RESECT_CORR_DTYPE).reshape(-1)
    return cs if len(cs) else np.zeros(1, capi.RESECT_CORR_DTYPE), len(cs)


def ordered_sum(terms, flags=None):
    """The header's ordered sum of terms [m] f64 over the rows with flags [m] set (default: all)."""
    t = np.ascontiguousarray(terms, dtype=np.float64).reshape(-1)
    f = np.ones(len(t), np.uint8) if flags is None else np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    assert len(f) == len(t)
    buf = t if len(t) else np.zeros(1)
    return float(lib().rr_ordered_sum(_p(buf), _p(f if len(f) else np.zeros(1, np.uint8)), C.c_size_t(len(t))))


def evaluate(R, t, K, corr, max_dist2):
    """EVALUATE (R, t) over a RESECT_CORR_DTYPE list -> (H [6, 6], g [6], cost, n)."""
    R, t = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    cs, m = _corr(corr)
    terms, flag, sums = np.zeros(29 * max(m, 1)), np.zeros(max(m, 1), np.uint8), np.zeros(29)
    lib().rr_evaluate(_p(R), _p(t), C.c_double(K[0]), C.c_double(K[1]), _p(cs), C.c_size_t(m), C.c_double(max_dist2), _p(terms), _p(flag), _p(sums))
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = sums[:21]
    H = H + np.triu(H, 1).T
    return H, sums[21:27].copy(), float(sums[27]), int(sums[28])


def step(R, t, H, g):
    """STEP from (R, t) with H [6, 6] and g [6] -> (R_new [3, 3], t_new [3], d [6]) or None (invalid)."""
    R, t = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)
    sums = np.zeros(29)
    sums[:21], sums[21:27] = np.asarray(H, np.float64)[np.triu_indices(6)], g
    Rn, tn, d = np.zeros(9), np.zeros(3), np.zeros(6)
    if not lib().rr_step(_p(R), _p(t), _p(sums), _p(Rn), _p(tn), _p(d)):
        return None
    return Rn.reshape(3, 3), tn, d


def refine_pair(model, corr, rounds, max_dist2, K, obs_cap=None):
    """One pair: model one RESECT_DTYPE record, corr its dense list (at least min(n_corr, obs_cap) rows; obs_cap defaults to
    len(corr)) -> (model [1] RESECT_DTYPE, info [1] RESECT_REFINE_DTYPE, flags bool [obs_cap] per observation record, trace
    [rounds + 1, 12]: R, t kept after the input's evaluation and after every accepted round, zero otherwise)."""
    mod = np.ascontiguousarray(model, dtype=capi.RESECT_DTYPE).reshape(-1)[:1].copy()
    cs, m = _corr(corr)
    cap = m if obs_cap is None else int(obs_cap)
    if len(cs) < cap:
        cs = np.concatenate([cs, np.zeros(cap - len(cs), capi.RESECT_CORR_DTYPE)])
    out, inf = np.zeros(1, capi.RESECT_DTYPE), np.zeros(1, capi.RESECT_REFINE_DTYPE)
    terms, work, flags = np.zeros(29 * max(cap, 1)), np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
    trace = np.zeros((int(rounds) + 1, 12))
    lib().rr_refine(_p(mod), _p(cs), C.c_uint32(cap), C.c_uint32(int(rounds)), C.c_double(max_dist2), C.c_double(K[0]), C.c_double(K[1]), _p(terms),
                    _p(work), _p(out), _p(inf), _p(flags), _p(trace))
    return out, inf, flags[:cap].astype(bool), trace


def refine(models, corrs, rounds, max_dist2, K, obs_cap):
    """n pairs: models [n] RESECT_DTYPE, corrs a list of n dense lists (or an array [n, obs_cap]) -> (models [n], info [n], bits
    uint64 [n, (obs_cap + 63) // 64] with the words past (n_obs + 63) // 64 zero)."""
    ms = np.ascontiguousarray(models, dtype=capi.RESECT_DTYPE).reshape(-1)
    n, words = len(ms), (obs_cap + 63) // 64
    out, inf, bits = np.zeros(n, capi.RESECT_DTYPE), np.zeros(n, capi.RESECT_REFINE_DTYPE), np.zeros((n, words), np.uint64)
    for j in range(n):
        o, i, fl, _ = refine_pair(ms[j:j + 1], corrs[j], rounds, max_dist2, K, obs_cap)
        out[j], inf[j], bits[j] = o[0], i[0], epiref.bits(fl, words)
    return out, inf, bits


def dense(corrs, obs_cap, fill=None):
    """The [n, obs_cap] RESECT_CORR_DTYPE array of a list of dense lists; the rows past each list are `fill` bytes (default 0)."""
    a = np.zeros((len(corrs), obs_cap), capi.RESECT_CORR_DTYPE)
    if fill is not None:
        a.view(np.uint8)[...] = fill
    for j, c in enumerate(corrs):
        k = min(len(c), obs_cap)
        a[j, :k] = c[:k]
    return a

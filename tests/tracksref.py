"""CPU restatement of the tracks arithmetic (include/vslam.h, "tracks"), bit for bit, written from the header text alone: the
two tables are Python dictionaries (prev: the lowest live record of pair j - 1 per train index; next: the lowest candidate per
record of pair j - 1), a track is a Python list of views, and the arithmetic of steps 2 - 5 - the train camera, the normal
equations, the cofactor solve, the reprojection test - is a few lines of C, compiled once per process with
gcc -O2 -ffp-contract=off: every + - * / rounded on its own, sums left to right as the header writes them.  This is the
checker, not the product: the library has no CPU path.
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
typedef struct { double R[9]; double t[3]; uint32_t n_matches, n_front; int32_t best; int32_t valid; } pose;
typedef struct { double W[9], w[3], C[3], Ct[3]; double scale, ratio; uint32_t n_links; int32_t segment, linked, valid; } chain;
typedef struct { double W[9], w[3], C[3], x, y; } view;
typedef struct { double X[3], det; uint32_t n_views, n_ok, status, reserved; } track;

static double canonical(double x) {
    if (x == x) return x;
    const uint64_t qnan = 0x7ff8000000000000ull;
    memcpy(&x, &qnan, 8);
    return x;
}

/* step 2: the query view of a record of pair j */
void ref_query_view(const chain* c, double x, double y, view* o) {
    memcpy(o->W, c->W, sizeof o->W);
    memcpy(o->w, c->w, sizeof o->w);
    memcpy(o->C, c->C, sizeof o->C);
    o->x = x, o->y = y;
}

/* step 2: the train view of the last record, pair j */
void ref_train_view(const pose* p, const chain* c, double x, double y, view* o) {
    const double* R = p->R;
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) o->W[3 * i + k] = (R[3 * i] * c->W[k] + R[3 * i + 1] * c->W[3 + k]) + R[3 * i + 2] * c->W[6 + k];
        o->w[i] = ((R[3 * i] * c->w[0] + R[3 * i + 1] * c->w[1]) + R[3 * i + 2] * c->w[2]) + c->scale * p->t[i];
        o->C[i] = c->Ct[i];
    }
    o->x = x, o->y = y;
}

/* steps 3 - 5 over the n views of one track, in order */
void ref_track(const view* v, uint32_t n, double fx, double fy, double cx, double cy, double max_dist2, uint32_t min_views, track* out) {
    double A00 = 0.0, A01 = 0.0, A02 = 0.0, A11 = 0.0, A12 = 0.0, A22 = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
    for (uint32_t p = 0; p < n; ++p) {
        const double* W = v[p].W;
        const double* Cc = v[p].C;
        const double q0 = (v[p].x - cx) / fx, q1 = (v[p].y - cy) / fy;
        const double d0 = (W[0] * q0 + W[3] * q1) + W[6];
        const double d1 = (W[1] * q0 + W[4] * q1) + W[7];
        const double d2 = (W[2] * q0 + W[5] * q1) + W[8];
        const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
        const double e0 = d0 / dd, e1 = d1 / dd, e2 = d2 / dd;
        const double P00 = 1.0 - e0 * d0, P11 = 1.0 - e1 * d1, P22 = 1.0 - e2 * d2;
        const double P01 = 0.0 - e0 * d1, P02 = 0.0 - e0 * d2, P12 = 0.0 - e1 * d2;
        A00 = A00 + P00; A01 = A01 + P01; A02 = A02 + P02; A11 = A11 + P11; A12 = A12 + P12; A22 = A22 + P22;
        g0 = g0 + ((P00 * Cc[0] + P01 * Cc[1]) + P02 * Cc[2]);
        g1 = g1 + ((P01 * Cc[0] + P11 * Cc[1]) + P12 * Cc[2]);
        g2 = g2 + ((P02 * Cc[0] + P12 * Cc[1]) + P22 * Cc[2]);
    }
    const double c00 = A11 * A22 - A12 * A12, c01 = A02 * A12 - A01 * A22, c02 = A01 * A12 - A02 * A11;
    const double c11 = A00 * A22 - A02 * A02, c12 = A01 * A02 - A00 * A12, c22 = A00 * A11 - A01 * A01;
    const double det = (A00 * c00 + A01 * c01) + A02 * c02;
    double X[3];
    X[0] = ((c00 * g0 + c01 * g1) + c02 * g2) / det;
    X[1] = ((c01 * g0 + c11 * g1) + c12 * g2) / det;
    X[2] = ((c02 * g0 + c12 * g1) + c22 * g2) / det;
    const int solved = det > 0.0 && det < INFINITY && isfinite(X[0]) && isfinite(X[1]) && isfinite(X[2]);
    uint32_t n_ok = 0;
    for (uint32_t p = 0; p < n; ++p) {
        const double* W = v[p].W;
        const double* w = v[p].w;
        const double u = (v[p].x - cx) / fx, vv = (v[p].y - cy) / fy;
        const double Z0 = ((W[0] * X[0] + W[1] * X[1]) + W[2] * X[2]) + w[0];
        const double Z1 = ((W[3] * X[0] + W[4] * X[1]) + W[5] * X[2]) + w[1];
        const double Z2 = ((W[6] * X[0] + W[7] * X[1]) + W[8] * X[2]) + w[2];
        const double ex = (u * Z2 - Z0) * fx, ey = (vv * Z2 - Z1) * fy;
        if (Z2 > 0.0 && (ex * ex + ey * ey) < max_dist2 * (Z2 * Z2)) ++n_ok;
    }
    const int good = solved && n_ok == n && n >= min_views;
    for (int k = 0; k < 3; ++k) out->X[k] = canonical(X[k]);
    out->det = canonical(det);
    out->n_views = n;
    out->n_ok = n_ok;
    out->status = (solved ? 1u : 0u) | (good ? 2u : 0u);
    out->reserved = 0;
}
"""

_lib = None
QNAN = chainref.QNAN
NONE = 0xFFFFFFFF
VIEW_DTYPE = np.dtype([("W", "<f8", (9,)), ("w", "<f8", (3,)), ("C", "<f8", (3,)), ("x", "<f8"), ("y", "<f8")], align=True)


def lib():
    global _lib
    if _lib is None:
        _lib = epiref.compile_c("tracksref", _SRC)
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def pixel(p):
    """The exact coordinate (x, y) of one capi.POINT_DTYPE record; NaN, NaN for an octave outside 0 .. 31."""
    o = int(p["octave"])
    if not 0 <= o <= 31:
        return QNAN, QNAN
    s = 0.5 if o == 0 else float(1 << (o - 1))
    return float(int(p["col"]) - int(p["padding"])) * s, float(int(p["row"]) - int(p["padding"])) * s


def empty_track():
    t = np.zeros(1, capi.TRACK_DTYPE)
    t["X"], t["det"] = QNAN, QNAN
    return t[0]


def solve(views, intrinsics, max_dist2, min_views):
    """Steps 3 - 5 of one track: views [n] VIEW_DTYPE in the track's order -> one capi.TRACK_DTYPE record."""
    v = np.ascontiguousarray(views, dtype=VIEW_DTYPE).reshape(-1)
    out = np.zeros(1, capi.TRACK_DTYPE)
    fx, fy, cx, cy = (float(a) for a in intrinsics)
    lib().ref_track(_p(v), C.c_uint32(len(v)), C.c_double(fx), C.c_double(fy), C.c_double(cx), C.c_double(cy), C.c_double(float(max_dist2)),
                    C.c_uint32(int(min_views)), _p(out))
    return out[0]


def views_of(path, poses, matches, chain, frames):
    """The views of the track whose records are path = [(j, i), ...]: a query view per record, then the last record's train view."""
    v = np.zeros(len(path) + 1, VIEW_DTYPE)
    for p, (j, i) in enumerate(path):
        x, y = pixel(frames[j, int(matches[j]["query"][i]) & NONE])
        lib().ref_query_view(_p(chain[j:j + 1]), C.c_double(x), C.c_double(y), _p(v[p:p + 1]))
    j, i = path[-1]
    x, y = pixel(frames[j + 1, int(matches[j]["train"][i]) & NONE])
    lib().ref_train_view(_p(poses[j:j + 1]), _p(chain[j:j + 1]), C.c_double(x), C.c_double(y), _p(v[len(path):]))
    return v


def paths(poses, matches, match_counts, front_bits, point_cap, chain):
    """Steps 1 and 2 -> (m [n], live [n] of bool [m], tracks: {(j0, i0): [(j0, i0), (j0 + 1, i1), ...]} in head order)."""
    n = len(poses)
    ms, lives, nxt = [], [], [dict() for _ in range(max(n - 1, 0))]
    cont = [set() for _ in range(n)]        # the records that continue one of the pair before
    for j in range(n):
        m, live = chainref.live_records(poses[j], matches[j], match_counts[j], front_bits[j], point_cap)
        ms.append(m), lives.append(live)
        if j >= 1 and int(chain["linked"][j]) != 0:
            prev = {}                       # train index -> the lowest live record of pair j - 1
            for i in np.flatnonzero(lives[j - 1]):
                prev.setdefault(int(matches[j - 1]["train"][i]) & NONE, int(i))
            for b in np.flatnonzero(live):  # ascending: the first candidate for a is the lowest
                a = prev.get(int(matches[j]["query"][b]) & NONE)
                if a is not None and a not in nxt[j - 1]:
                    nxt[j - 1][a] = int(b)
                    cont[j].add(int(b))
    tracks = {}
    for j in range(n):
        for i in np.flatnonzero(lives[j]):
            if int(i) in cont[j]:
                continue
            path, jj, ii = [(j, int(i))], j, int(i)
            while jj + 1 < n and ii in nxt[jj]:
                ii = nxt[jj][ii]
                jj += 1
                path.append((jj, ii))
            tracks[(j, int(i))] = path
    return ms, lives, tracks


def tracks(poses, matches, match_counts, front_bits, point_cap, chain, frame_points, intrinsics, max_dist2, min_views, cut=None):
    """The whole step over n pairs: poses [n] capi.POSE_DTYPE, matches [n, match_cap] capi.MATCH_DTYPE, match_counts [n], front_bits
    uint64 [n, words], chain [n] capi.CHAIN_DTYPE, frame_points [n + 1, point_cap] capi.POINT_DTYPE -> (m [n], and per pair: tracks
    [m] capi.TRACK_DTYPE, refs [m] capi.TRACK_REF_DTYPE, good bool [m]; summary [n] capi.TRACK_SUMMARY_DTYPE; the paths).
    cut: every track's views are cut to its first `cut` (a test's means: the device has no such parameter)."""
    ps = np.ascontiguousarray(poses, dtype=capi.POSE_DTYPE).reshape(-1)
    n = len(ps)
    summary = np.zeros(n, capi.TRACK_SUMMARY_DTYPE)
    if n == 0:
        return [], [], [], [], summary, {}
    mt = np.ascontiguousarray(matches, dtype=capi.MATCH_DTYPE).reshape(n, -1)
    fb = np.ascontiguousarray(front_bits).view(np.uint64).reshape(n, -1)
    ch = np.ascontiguousarray(chain, dtype=capi.CHAIN_DTYPE).reshape(-1)
    fp = np.ascontiguousarray(frame_points, dtype=capi.POINT_DTYPE).reshape(n + 1, point_cap)
    ms, lives, pth = paths(ps, mt, match_counts, fb, point_cap, ch)
    rows, refs, goods = [], [], []
    for j in range(n):
        r = np.zeros(ms[j], capi.TRACK_DTYPE)
        r["X"], r["det"] = QNAN, QNAN
        rows.append(r)
        refs.append(np.full(ms[j], NONE, np.uint32).repeat(2).view(capi.TRACK_REF_DTYPE).copy())
        goods.append(np.zeros(ms[j], bool))
    for (j0, i0), path in pth.items():
        v = views_of(path, ps, mt, ch, fp)
        if cut is not None:
            v = v[:cut]
        t = solve(v, intrinsics, max_dist2, min_views)
        rows[j0][i0] = t
        goods[j0][i0] = bool(int(t["status"]) & 2)
        for pos, (j, i) in enumerate(path):
            refs[j][i] = (i0, pos)
        summary["n_heads"][j0] += 1
        summary["n_good"][j0] += int(goods[j0][i0])
        summary["max_views"][j0] = max(int(summary["max_views"][j0]), int(t["n_views"]))
    return ms, rows, refs, goods, summary, pth

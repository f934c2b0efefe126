"""CPU restatement of the trajectory arithmetic (include/vslam.h, "trajectory"), bit for bit, written from the header text
alone: the link by index is a Python dictionary (the first live record of pair j - 1 per train index), the ratios, the median
(qsort on the uint64 keys), the sequential walk and the map are a few lines of C, compiled once per process with
gcc -O2 -ffp-contract=off - every + - * / sqrt rounded on its own, sums left to right as the header writes them.  This is
the checker, not the product: the library has no CPU path.
"""
import ctypes as C

import numpy as np

from tests import epiref
from visualslam_amd import capi

_SRC = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
typedef struct { double R[9]; double t[3]; uint32_t n_matches, n_front; int32_t best; int32_t valid; } pose;
typedef struct { double W[9], w[3], C[3], Ct[3]; double scale, ratio; uint32_t n_links; int32_t segment, linked, valid; } chain;

static double canonical(double x) {
    if (x == x) return x;
    const uint64_t qnan = 0x7ff8000000000000ull;
    memcpy(&x, &qnan, 8);
    return x;
}

/* step 2: m records of pair j, a [m] the linked record of pair j - 1 or -1; X = points of pair j - 1, Z = points of pair j.
   r [m]: the ratio as computed (canonical NaN when not linked); returns the number of usable ratios */
uint32_t ref_ratios(const pose* prev, const double* X, const double* Z, const int32_t* a, uint32_t m, double* r, uint8_t* usable) {
    uint32_t n = 0;
    const double* R = prev->R;
    const double* t = prev->t;
    for (uint32_t b = 0; b < m; ++b) {
        usable[b] = 0;
        r[b] = canonical(NAN);
        if (a[b] < 0) continue;
        const double* x = X + 3 * (size_t)a[b];
        const double* z = Z + 3 * (size_t)b;
        double Y[3];
        for (int i = 0; i < 3; ++i) Y[i] = ((R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2]) + t[i];
        const double dY = sqrt((Y[0] * Y[0] + Y[1] * Y[1]) + Y[2] * Y[2]);
        const double dZ = sqrt((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
        const double q = dY / dZ;
        usable[b] = q > 0.0 && q < INFINITY;
        n += usable[b];
        r[b] = canonical(q);
    }
    return n;
}

static int by_key(const void* a, const void* b) {
    const uint64_t x = *(const uint64_t*)a, y = *(const uint64_t*)b;
    return x < y ? -1 : x > y;
}

/* step 3: the lower median of n usable ratios (their bit patterns are sorted in place), 0.0 for none */
double ref_median(uint64_t* keys, uint32_t n) {
    if (n == 0) return 0.0;
    qsort(keys, n, sizeof(uint64_t), by_key);
    double out;
    memcpy(&out, &keys[(n - 1) >> 1], 8);
    return out;
}

static void compose(const double* R, const double* W, double* out) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) out[3 * i + k] = (R[3 * i] * W[k] + R[3 * i + 1] * W[3 + k]) + R[3 * i + 2] * W[6 + k];
}
static void apply(const double* R, const double* w, double s, const double* t, double* out) {
    for (int i = 0; i < 3; ++i) out[i] = ((R[3 * i] * w[0] + R[3 * i + 1] * w[1]) + R[3 * i + 2] * w[2]) + s * t[i];
}
static void centre(const double* W, const double* w, double* c) {
    for (int i = 0; i < 3; ++i) c[i] = canonical(-((W[i] * w[0] + W[3 + i] * w[1]) + W[6 + i] * w[2]));
}

/* step 4 */
void ref_walk(const pose* poses, const uint32_t* n_links, const double* ratio, int n_pairs, uint32_t min_links, chain* out) {
    double W[9], w[3], scale = 1.0;
    int segment = 0;
    for (int j = 0; j < n_pairs; ++j) {
        const int valid = poses[j].best >= 0;
        const int linked = j >= 1 && poses[j - 1].best >= 0 && valid && n_links[j] >= min_links;
        if (linked) {
            double nW[9], nw[3];
            compose(poses[j - 1].R, W, nW);
            apply(poses[j - 1].R, w, scale, poses[j - 1].t, nw);
            memcpy(W, nW, sizeof W);
            memcpy(w, nw, sizeof w);
            scale = scale * ratio[j];
        } else {
            segment = j;
            scale = 1.0;
            for (int k = 0; k < 9; ++k) W[k] = k % 4 == 0;
            w[0] = w[1] = w[2] = 0.0;
        }
        chain* o = out + j;
        memset(o, 0, sizeof *o);
        for (int k = 0; k < 9; ++k) o->W[k] = canonical(W[k]);
        for (int k = 0; k < 3; ++k) o->w[k] = canonical(w[k]);
        if (valid) {
            double Wt[9], wt[3];
            centre(W, w, o->C);
            compose(poses[j].R, W, Wt);
            apply(poses[j].R, w, scale, poses[j].t, wt);
            centre(Wt, wt, o->Ct);
        }
        o->scale = canonical(scale);
        o->ratio = ratio[j];
        o->n_links = n_links[j];
        o->segment = segment;
        o->linked = linked;
        o->valid = valid;
    }
}

/* step 5 for one valid pair: m records, live [m] bytes; M [m][3] */
void ref_map(const chain* c, const double* X, const uint8_t* live, uint32_t m, double* M) {
    for (uint32_t i = 0; i < m; ++i) {
        const double* x = X + 3 * (size_t)i;
        double d[3];
        for (int k = 0; k < 3; ++k) d[k] = c->scale * x[k] - c->w[k];
        for (int k = 0; k < 3; ++k)
            M[3 * (size_t)i + k] = live[i] ? canonical((c->W[k] * d[0] + c->W[3 + k] * d[1]) + c->W[6 + k] * d[2]) : canonical(NAN);
    }
}
"""

_lib = None
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def lib():
    global _lib
    if _lib is None:
        L = epiref.compile_c("chainref", _SRC)
        L.ref_ratios.restype = C.c_uint32
        L.ref_median.restype = C.c_double
        _lib = L
    return _lib


def _p(a):
    return C.c_void_p(a.ctypes.data)


def median(r):
    """The lower median of the usable ratios r (positive, finite), by qsort on their bit patterns; 0.0 for none."""
    keys = np.ascontiguousarray(r, dtype=np.float64).view(np.uint64).copy()
    return float(lib().ref_median(_p(keys) if len(keys) else None, C.c_uint32(len(keys))))


def walk(poses, n_links, ratio, min_links):
    """Step 4 alone -> [n] capi.CHAIN_DTYPE."""
    ps = np.ascontiguousarray(poses, dtype=capi.POSE_DTYPE).reshape(-1)
    n = len(ps)
    nl, rt = np.ascontiguousarray(n_links, dtype=np.uint32), np.ascontiguousarray(ratio, dtype=np.float64)
    out = np.zeros(max(n, 1), capi.CHAIN_DTYPE)
    lib().ref_walk(_p(ps), _p(nl), _p(rt), C.c_int(n), C.c_uint32(min_links), _p(out))
    return out[:n]


def map_points(record, X, live):
    """Step 5 of one valid pair: its chain record [1], X [m, 3], live bool [m] -> M [m, 3]."""
    rec = np.ascontiguousarray(record, dtype=capi.CHAIN_DTYPE).reshape(-1)[:1]
    m = len(live)
    Xc = np.zeros((max(m, 1), 3), np.float64)
    Xc[:m] = np.asarray(X, np.float64).reshape(-1, 3)[:m]
    lv = np.zeros(max(m, 1), np.uint8)
    lv[:m] = live
    M = np.zeros((max(m, 1), 3), np.float64)
    lib().ref_map(_p(rec), _p(Xc), _p(lv), C.c_uint32(m), _p(M))
    return M[:m]


def live_records(pose, matches, count, bits, point_cap):
    """-> (m, live bool [m]) of one pair: min(count, capacity) records; in front under a winner, both indices below point_cap."""
    cap = len(matches)
    m = min(int(count), cap)
    if int(pose["best"]) < 0 or m == 0:
        return m, np.zeros(m, bool)
    front = np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), bitorder="little")[:m].astype(bool)
    q, t = matches["query"][:m].astype(np.int64) & 0xFFFFFFFF, matches["train"][:m].astype(np.int64) & 0xFFFFFFFF
    return m, front & (q < point_cap) & (t < point_cap)


def chain(poses, matches, match_counts, points, front_bits, point_cap, min_links):
    """The whole step over n pairs: poses [n] capi.POSE_DTYPE, matches [n, match_cap] capi.MATCH_DTYPE, match_counts [n], points
    float64 [n, match_cap, 3], front_bits uint64 [n, words] -> (chain [n] capi.CHAIN_DTYPE, m [n], and per pair: map [m, 3] or
    None for an invalid pair, links int32 [m], ratios [m], usable bool [m])."""
    ps = np.ascontiguousarray(poses, dtype=capi.POSE_DTYPE).reshape(-1)
    n = len(ps)
    if n == 0:
        return np.zeros(0, capi.CHAIN_DTYPE), [], [], [], [], []
    mt = np.ascontiguousarray(matches, dtype=capi.MATCH_DTYPE).reshape(n, -1)
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(n, mt.shape[1], 3)
    fb = np.ascontiguousarray(front_bits).view(np.uint64).reshape(n, -1)
    ms, lives, links, ratios, usables = [], [], [], [], []
    n_links, ratio = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.float64)
    for j in range(n):
        m, live = live_records(ps[j], mt[j], match_counts[j], fb[j], point_cap)
        ms.append(m), lives.append(live)
        a = np.full(max(m, 1), -1, np.int32)
        if j >= 1:
            first = {}                                      # train index -> the lowest live record of pair j - 1
            for i in np.flatnonzero(lives[j - 1]):
                first.setdefault(int(mt[j - 1]["train"][i]), int(i))
            for b in np.flatnonzero(live):
                a[b] = first.get(int(mt[j]["query"][b]), -1)
        r, use = np.zeros(max(m, 1), np.float64), np.zeros(max(m, 1), np.uint8)
        X = np.ascontiguousarray(pts[j - 1]) if j >= 1 else np.zeros((1, 3))
        Z = np.ascontiguousarray(pts[j])
        n_links[j] = lib().ref_ratios(_p(ps[max(j - 1, 0):]), _p(X), _p(Z), _p(a), C.c_uint32(m), _p(r), _p(use))
        use = use[:m].astype(bool)
        ratio[j] = median(r[:m][use])
        links.append(a[:m]), ratios.append(r[:m]), usables.append(use)
    out = walk(ps, n_links, ratio, min_links)
    maps = []
    for j in range(n):
        if not out["valid"][j]:
            maps.append(None)
            continue
        maps.append(map_points(out[j:j + 1], pts[j, :ms[j]], lives[j]))
    return out, ms, maps, links, ratios, usables

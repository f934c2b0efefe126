"""CPU restatement of the bundle adjustment (include/vslam.h, "bundle adjustment"), bit for bit, written from the header text
alone.  The paths are tracksref.paths' (steps 1 and 2 of the tracks section, "verbatim"), EVALUATE and STEP of a camera are
resectrefineref's over the dense rows rows_of() builds (a row that does not count is a row of NaN: never a member, so it adds
+0.0 in its slot); the views, the point step, the rows, the sweeps and the outputs are a few lines of C compiled like every
restatement (epiref.compile_c: gcc -O2 -ffp-contract=off).  It shares nothing with the kernels.  This is the checker, not the
product: the library has no CPU path.
"""
import ctypes as C

import numpy as np

from tests import epiref, resectrefineref, tracksref
from visualslam_amd import capi

_SRC = r"""
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
typedef struct { double R[9]; double t[3]; uint32_t n_matches, n_front; int32_t best; int32_t valid; } pose;
typedef struct { double W[9], w[3], C[3], Ct[3]; double scale, ratio; uint32_t n_links; int32_t segment, linked, valid; } chain;
typedef struct { int32_t row, col, value, padding, octave, level; } point;
typedef struct { int32_t query, train; float dist2; } match;
typedef struct { double X[3], det; uint32_t n_views, n_ok, status, reserved; } track;
typedef struct { uint32_t head, pos; } ref;
typedef struct { double W[9], w[3], C[3]; uint32_t n_before, n_after, accepted, rejected, invalid, skipped; double cost_before, cost_after; } cam;
typedef struct { uint32_t n_before, n_after, accepted, rejected, invalid, skipped; double cost_before, cost_after; } pinfo;
typedef struct { double Y[3], u, v; uint32_t b, reserved; } corr;
typedef void (*eval_fn)(const double*, const double*, double, double, const corr*, size_t, double, double*, uint8_t*, double*);
typedef int (*step_fn)(const double*, const double*, const double*, double*, double*, double*);

typedef struct {
    const pose* poses; const match* matches; const uint32_t* ms; const uint8_t* live; const chain* ch; const point* frames; const ref* refs;
    track* tracks;            /* [n][cap]: the output rows, X as the sweeps leave it, status as tracks_in had it until the end */
    double* W; double* w;     /* [n][9], [n][3]: T_j as kept so far */
    const uint8_t* valid;     /* [n] */
    const int32_t* path_j0; const uint32_t* path_off; const uint32_t* path_len; const uint32_t* path_rec; uint32_t n_paths;
    uint32_t cap, pcap; int32_t n; uint32_t min_views;
    double fx, fy, cx, cy, md;
    eval_fn evaluate; step_fn step;
    corr* rows; double* terms; uint8_t* flag;   /* scratch: 2 * cap rows, 29 * 2 * cap terms, 2 * cap flags */
} ctx;

static double qnan(void) { const uint64_t q = 0x7ff8000000000000ull; double d; memcpy(&d, &q, 8); return d; }
static double canon(double x) { return x == x ? x : qnan(); }
static int fin(double x) { return x == x && x != INFINITY && x != -INFINITY; }

static void pixel(const ctx* c, const point* p, double* u, double* v) {
    double x = qnan(), y = x;
    if (p->octave >= 0 && p->octave <= 31) {
        const double s = p->octave == 0 ? 0.5 : (double)(1u << (p->octave - 1));
        x = (double)((int64_t)p->col - (int64_t)p->padding) * s;
        y = (double)((int64_t)p->row - (int64_t)p->padding) * s;
    }
    *u = (x - c->cx) / c->fx; *v = (y - c->cy) / c->fy;
}

static const double EYE[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
static const double ZERO[3] = {0.0, 0.0, 0.0};
/* camera j, or the held camera for j < 0 */
static void camera(const ctx* c, int j, const double** W, const double** w) {
    if (j < 0) { *W = EYE; *w = ZERO; } else { *W = c->W + 9 * (size_t)j; *w = c->w + 3 * (size_t)j; }
}
static int query_cam(const ctx* c, int j) { return j >= 1 && c->ch[j].linked != 0 ? j - 1 : -1; }

static int member(const double* W, const double* w, const double* X, double u, double v, double fx, double fy, double md, double* Z) {
    Z[0] = ((W[0] * X[0] + W[1] * X[1]) + W[2] * X[2]) + w[0];
    Z[1] = ((W[3] * X[0] + W[4] * X[1]) + W[5] * X[2]) + w[1];
    Z[2] = ((W[6] * X[0] + W[7] * X[1]) + W[8] * X[2]) + w[2];
    const double ex = (u * Z[2] - Z[0]) * fx, ey = (v * Z[2] - Z[1]) * fy;
    return Z[2] > 0.0 && (ex * ex + ey * ey) < md * (Z[2] * Z[2]);
}

/* view p of path k: its camera and its pixel */
static void view(const ctx* c, uint32_t k, uint32_t p, const double** W, const double** w, double* u, double* v) {
    const int j0 = c->path_j0[k];
    const uint32_t L = c->path_len[k];
    const uint32_t* rec = c->path_rec + c->path_off[k];
    if (p < L) {
        const int j = j0 + (int)p;
        camera(c, p == 0 ? query_cam(c, j0) : j - 1, W, w);
        pixel(c, c->frames + (size_t)j * c->pcap + (uint32_t)c->matches[(size_t)j * c->cap + rec[p]].query, u, v);
    } else {
        const int j = j0 + (int)L - 1;
        camera(c, j, W, w);
        pixel(c, c->frames + (size_t)(j + 1) * c->pcap + (uint32_t)c->matches[(size_t)j * c->cap + rec[L - 1]].train, u, v);
    }
}

/* EVALUATE-POINT (X) of path k: out = H00 H01 H02 H11 H12 H22 g0 g1 g2 cost; returns n.  flags [L + 1] (may be NULL): members */
uint32_t ba_point_eval(const ctx* c, uint32_t k, const double* X, double* out, uint8_t* flags) {
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, cost = 0.0;
    uint32_t n = 0;
    const double fx = c->fx, fy = c->fy;
    for (uint32_t p = 0; p <= c->path_len[k]; ++p) {
        const double *W, *w;
        double u, v, Z[3];
        view(c, k, p, &W, &w, &u, &v);
        const int mem = member(W, w, X, u, v, fx, fy, c->md, Z);
        if (flags) flags[p] = (uint8_t)mem;
        if (!mem) continue;
        const double iz = 1.0 / Z[2];
        const double px = Z[0] * iz, py = Z[1] * iz;
        const double rx = (px - u) * fx, ry = (py - v) * fy;
        const double sx = fx * iz, sy = fy * iz;
        double ax[3], ay[3];
        for (int q = 0; q < 3; ++q) { ax[q] = sx * (W[q] - px * W[6 + q]); ay[q] = sy * (W[3 + q] - py * W[6 + q]); }
        int e = 0;
        for (int a = 0; a < 3; ++a)
            for (int b = a; b < 3; ++b, ++e) H[e] = H[e] + (ax[a] * ax[b] + ay[a] * ay[b]);
        for (int a = 0; a < 3; ++a) g[a] = g[a] + (ax[a] * rx + ay[a] * ry);
        cost = cost + (rx * rx + ry * ry);
        n += 1;
    }
    memcpy(out, H, sizeof H); memcpy(out + 6, g, sizeof g); out[9] = cost;
    return n;
}

/* step A.3: 0 = invalid */
int ba_point_delta(const double* s, double* delta) {
    const double H00 = s[0], H01 = s[1], H02 = s[2], H11 = s[3], H12 = s[4], H22 = s[5], g0 = s[6], g1 = s[7], g2 = s[8];
    const double c00 = H11 * H22 - H12 * H12, c01 = H02 * H12 - H01 * H22, c02 = H01 * H12 - H02 * H11;
    const double c11 = H00 * H22 - H02 * H02, c12 = H01 * H02 - H00 * H12, c22 = H00 * H11 - H01 * H01;
    const double det = (H00 * c00 + H01 * c01) + H02 * c02;
    delta[0] = -(((c00 * g0 + c01 * g1) + c02 * g2) / det);
    delta[1] = -(((c01 * g0 + c11 * g1) + c12 * g2) / det);
    delta[2] = -(((c02 * g0 + c12 * g1) + c22 * g2) / det);
    return det > 0.0 && det < INFINITY && fin(delta[0]) && fin(delta[1]) && fin(delta[2]);
}

static int active_row(const ctx* c, const track* t) { return (t->status & 1u) && t->n_views >= c->min_views; }

/* the row "one side of record i of pair jj" counts: -> its head's track row, or NULL */
static const track* row_track(const ctx* c, int jj, uint32_t i, int need_head) {
    if (!c->live[(size_t)jj * c->cap + i]) return NULL;
    const ref r = c->refs[(size_t)jj * c->cap + i];
    if (r.pos > (uint32_t)jj || (need_head && r.pos != 0)) return NULL;
    const int jh = jj - (int)r.pos;
    if (r.head >= c->ms[jh]) return NULL;
    const track* t = c->tracks + (size_t)jh * c->cap + r.head;
    return active_row(c, t) ? t : NULL;
}

static uint32_t head_rows(const ctx* c, int j) { return j + 1 < c->n && c->ch[j + 1].linked != 0 ? c->ms[j + 1] : 0u; }

/* the dense rows of camera T_j; a row that does not count is NaN throughout.  Returns n_rows */
size_t ba_rows(const ctx* c, int j, corr* out) {
    const uint32_t m0 = c->ms[j];
    const size_t n_rows = (size_t)m0 + head_rows(c, j);
    for (size_t r = 0; r < n_rows; ++r) {
        const int train = r < m0;
        const int jj = train ? j : j + 1;
        const uint32_t i = (uint32_t)(train ? r : r - m0);
        const track* t = row_track(c, jj, i, !train);
        corr* o = out + r;
        o->b = (uint32_t)r; o->reserved = 0;
        if (!t) { o->Y[0] = o->Y[1] = o->Y[2] = o->u = o->v = qnan(); continue; }
        memcpy(o->Y, t->X, sizeof o->Y);
        const match* mt = c->matches + (size_t)jj * c->cap + i;
        pixel(c, c->frames + (size_t)(j + 1) * c->pcap + (uint32_t)(train ? mt->train : mt->query), &o->u, &o->v);
    }
    return n_rows;
}

static void cam_eval(const ctx* c, int j, const double* W, const double* w, double* sums) {
    const size_t n_rows = ba_rows(c, j, c->rows);
    c->evaluate(W, w, c->fx, c->fy, c->rows, n_rows, c->md, c->terms, c->flag, sums);
}

/* the initial T_j */
void ba_init_cam(const pose* p, const chain* ch, const cam* in, int valid, double* W, double* w) {
    if (!valid) { memcpy(W, EYE, sizeof EYE); memcpy(w, ZERO, sizeof ZERO); return; }
    if (in) { memcpy(W, in->W, sizeof in->W); memcpy(w, in->w, sizeof in->w); return; }
    const double* R = p->R;
    for (int i = 0; i < 3; ++i) {
        for (int k = 0; k < 3; ++k) W[3 * i + k] = (R[3 * i] * ch->W[k] + R[3 * i + 1] * ch->W[3 + k]) + R[3 * i + 2] * ch->W[6 + k];
        w[i] = ((R[3 * i] * ch->w[0] + R[3 * i + 1] * ch->w[1]) + R[3 * i + 2] * ch->w[2]) + ch->scale * p->t[i];
    }
}

/* the whole call.  cams [n], info [n][cap] (zeroed by the caller; written at the head slots of active tracks), mbits [n][2][cap] bytes (zeroed) */
void ba_run(ctx* c, uint32_t sweeps, cam* cams, pinfo* info, uint8_t* written, uint8_t* mbits) {
    for (int j = 0; j < c->n; ++j) memset(cams + j, 0, sizeof(cam));
    for (uint32_t sweep = 0; sweep < sweeps; ++sweep) {
        /* A */
        for (uint32_t k = 0; k < c->n_paths; ++k) {
            const size_t o = (size_t)c->path_j0[k] * c->cap + c->path_rec[c->path_off[k]];
            track* t = c->tracks + o;
            if (!active_row(c, t)) continue;
            pinfo* pi = info + o;
            written[o] = 1;
            double s[10], sn[10], d[3];
            const uint32_t n = ba_point_eval(c, k, t->X, s, NULL);
            if (sweep == 0) { pi->n_before = n; pi->cost_before = s[9]; }
            if (n < 2) { pi->skipped += 1; continue; }
            if (!ba_point_delta(s, d)) { pi->invalid += 1; continue; }
            const double Xn[3] = {t->X[0] + d[0], t->X[1] + d[1], t->X[2] + d[2]};
            const uint32_t nn = ba_point_eval(c, k, Xn, sn, NULL);
            if (nn > n || (nn == n && sn[9] < s[9])) { memcpy(t->X, Xn, sizeof Xn); pi->accepted += 1; } else pi->rejected += 1;
        }
        /* B: every candidate from the cameras and points as A left them, then all kept or dropped */
        for (int j = 0; j < c->n; ++j) {
            if (!c->valid[j]) continue;
            double *W = c->W + 9 * (size_t)j, *w = c->w + 3 * (size_t)j, sc[29], sn[29], Wn[9], wn[3];
            cam_eval(c, j, W, w, sc);
            const uint32_t n = (uint32_t)sc[28];
            if (sweep == 0) { cams[j].n_before = n; cams[j].cost_before = sc[27]; }
            if (n < 6) { cams[j].skipped += 1; continue; }
            if (!c->step(W, w, sc, Wn, wn, NULL)) { cams[j].invalid += 1; continue; }
            cam_eval(c, j, Wn, wn, sn);
            const uint32_t nn = (uint32_t)sn[28];
            if (nn > n || (nn == n && sn[27] < sc[27])) { memcpy(W, Wn, sizeof Wn); memcpy(w, wn, sizeof wn); cams[j].accepted += 1; } else cams[j].rejected += 1;
        }
    }
    for (int j = 0; j < c->n; ++j) {
        cam* o = cams + j;
        if (!c->valid[j]) {
            memcpy(o->W, EYE, sizeof EYE);
            o->skipped = sweeps;
            continue;
        }
        const double *W = c->W + 9 * (size_t)j, *w = c->w + 3 * (size_t)j;
        double sc[29];
        cam_eval(c, j, W, w, sc);
        o->n_after = (uint32_t)sc[28]; o->cost_after = canon(sc[27]); o->cost_before = canon(o->cost_before);
        for (int k = 0; k < 9; ++k) o->W[k] = canon(W[k]);
        for (int k = 0; k < 3; ++k) o->w[k] = canon(w[k]);
        for (int k = 0; k < 3; ++k) o->C[k] = canon(-((W[k] * w[0] + W[3 + k] * w[1]) + W[6 + k] * w[2]));
    }
    /* member bits, under the output, by the status bits tracks_in had */
    for (int j = 0; j < c->n; ++j)
        for (uint32_t i = 0; i < c->ms[j]; ++i) {
            const track* t = row_track(c, j, i, 0);
            if (!t) continue;
            const match* mt = c->matches + (size_t)j * c->cap + i;
            const double *W, *w;
            double u, v, Z[3];
            camera(c, query_cam(c, j), &W, &w);
            pixel(c, c->frames + (size_t)j * c->pcap + (uint32_t)mt->query, &u, &v);
            mbits[((size_t)j * 2) * c->cap + i] = (uint8_t)member(W, w, t->X, u, v, c->fx, c->fy, c->md, Z);
            camera(c, j, &W, &w);
            pixel(c, c->frames + (size_t)(j + 1) * c->pcap + (uint32_t)mt->train, &u, &v);
            mbits[((size_t)j * 2 + 1) * c->cap + i] = (uint8_t)member(W, w, t->X, u, v, c->fx, c->fy, c->md, Z);
        }
    /* the head rows of active tracks */
    for (uint32_t k = 0; k < c->n_paths; ++k) {
        const size_t o = (size_t)c->path_j0[k] * c->cap + c->path_rec[c->path_off[k]];
        track* t = c->tracks + o;
        if (!active_row(c, t)) continue;
        double s[10];
        const uint32_t n = ba_point_eval(c, k, t->X, s, NULL);
        const int solved = t->det > 0.0 && t->det < INFINITY && fin(t->X[0]) && fin(t->X[1]) && fin(t->X[2]);
        const int good = solved && n == t->n_views && t->n_views >= c->min_views;
        for (int q = 0; q < 3; ++q) t->X[q] = canon(t->X[q]);
        t->n_ok = n;
        t->status = (solved ? 1u : 0u) | (good ? 2u : 0u);
        info[o].n_after = n; info[o].cost_after = canon(s[9]); info[o].cost_before = canon(info[o].cost_before);
        written[o] = 1;
    }
}
"""

_lib = None
NONE = 0xFFFFFFFF


def lib():
    global _lib
    if _lib is None:
        L = epiref.compile_c("bundleref", _SRC)
        L.ba_point_eval.restype = C.c_uint32
        L.ba_rows.restype = C.c_size_t
        _lib = L
    return _lib


class _Ctx(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("poses", "matches", "ms", "live", "ch", "frames", "refs", "tracks", "W", "w", "valid", "path_j0", "path_off",
                                          "path_len", "path_rec")] + \
               [("n_paths", C.c_uint32), ("cap", C.c_uint32), ("pcap", C.c_uint32), ("n", C.c_int32), ("min_views", C.c_uint32)] + \
               [(n, C.c_double) for n in ("fx", "fy", "cx", "cy", "md")] + \
               [(n, C.c_void_p) for n in ("evaluate", "step", "rows", "terms", "flag")]


def _p(a):
    return a.ctypes.data


class Problem:
    """One call's inputs, and the state the sweeps carry: tracks [n, cap] (the output rows), W [n, 9], w [n, 3].  poses [n]
    POSE_DTYPE, matches [n, cap] MATCH_DTYPE, match_counts [n], front_bits uint64 [n, words], chain [n] CHAIN_DTYPE, frame_points [n +
    1, point_cap] POINT_DTYPE, tracks_in [n, cap] TRACK_DTYPE, refs [n, cap] TRACK_REF_DTYPE, cams_in [n] BUNDLE_CAM_DTYPE or None."""

    def __init__(self, poses, matches, match_counts, front_bits, point_cap, chain, frame_points, tracks_in, refs, intrinsics, max_dist2, min_views,
                 cams_in=None):
        self.poses = np.ascontiguousarray(poses, dtype=capi.POSE_DTYPE).reshape(-1).copy()
        n = self.n = len(self.poses)
        self.matches = np.ascontiguousarray(matches, dtype=capi.MATCH_DTYPE).reshape(n, -1).copy()
        cap = self.cap = self.matches.shape[1] if n else 1
        self.pcap = int(point_cap)
        self.bits = np.ascontiguousarray(front_bits).view(np.uint64).reshape(n, -1)
        self.chain = np.ascontiguousarray(chain, dtype=capi.CHAIN_DTYPE).reshape(-1).copy()
        self.frames = np.ascontiguousarray(frame_points, dtype=capi.POINT_DTYPE).reshape(n + 1, self.pcap).copy()
        self.tracks_in = np.ascontiguousarray(tracks_in, dtype=capi.TRACK_DTYPE).reshape(n, cap).copy()
        self.refs = np.ascontiguousarray(refs, dtype=capi.TRACK_REF_DTYPE).reshape(n, cap).copy()
        self.K, self.max_dist2, self.min_views = tuple(float(v) for v in intrinsics), float(max_dist2), int(min_views)
        ms, lives, self.paths = tracksref.paths(self.poses, self.matches, match_counts, self.bits, self.pcap, self.chain) if n else ([], [], {})
        self.ms = np.array(ms, np.uint32).reshape(n)
        self.live = np.zeros((n, cap), np.uint8)
        for j in range(n):
            self.live[j, :ms[j]] = lives[j]
        self.heads = list(self.paths)
        self.index = {h: k for k, h in enumerate(self.heads)}
        lens = np.array([len(self.paths[h]) for h in self.heads], np.uint32)
        self.path_j0 = np.array([h[0] for h in self.heads], np.int32)
        self.path_len = lens
        self.path_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32) if len(lens) else np.zeros(0, np.uint32)
        self.path_rec = np.array([i for h in self.heads for (_, i) in self.paths[h]], np.uint32)
        self.valid = (self.poses["best"] >= 0).astype(np.uint8)
        self.tracks = self.tracks_in.copy()
        self.W, self.w = np.zeros((n, 9)), np.zeros((n, 3))
        ci = None if cams_in is None else np.ascontiguousarray(cams_in, dtype=capi.BUNDLE_CAM_DTYPE).reshape(-1).copy()
        for j in range(n):
            lib().ba_init_cam(C.c_void_p(_p(self.poses[j:j + 1])), C.c_void_p(_p(self.chain[j:j + 1])), None if ci is None else C.c_void_p(_p(ci[j:j + 1])),
                              C.c_int(int(self.valid[j])), C.c_void_p(_p(self.W[j:j + 1])), C.c_void_p(_p(self.w[j:j + 1])))
        self._rows = np.zeros(2 * cap + 1, capi.RESECT_CORR_DTYPE)
        self._terms, self._flag = np.zeros(29 * (2 * cap + 1)), np.zeros(2 * cap + 1, np.uint8)
        rl = resectrefineref.lib()
        c = self._c = _Ctx()
        for name, a in (("poses", self.poses), ("matches", self.matches), ("ms", self.ms), ("live", self.live), ("ch", self.chain), ("frames", self.frames),
                        ("refs", self.refs), ("tracks", self.tracks), ("W", self.W), ("w", self.w), ("valid", self.valid), ("path_j0", self.path_j0),
                        ("path_off", self.path_off), ("path_len", self.path_len), ("path_rec", self.path_rec), ("rows", self._rows),
                        ("terms", self._terms), ("flag", self._flag)):
            setattr(c, name, _p(a))
        c.n_paths, c.cap, c.pcap, c.n, c.min_views = len(self.heads), cap, self.pcap, n, self.min_views
        c.fx, c.fy, c.cx, c.cy = self.K
        c.md = self.max_dist2
        c.evaluate, c.step = C.cast(rl.rr_evaluate, C.c_void_p).value, C.cast(rl.rr_step, C.c_void_p).value

    def active(self, head):
        t = self.tracks[head]
        return bool(int(t["status"]) & 1) and int(t["n_views"]) >= self.min_views

    def active_heads(self):
        return [h for h in self.heads if self.active(h)]

    def rows_of(self, j):
        """The dense rows {Y, u, v, b} of camera T_j under the points as they stand (RESECT_CORR_DTYPE; NaN: the row does not count)."""
        out = np.zeros(2 * self.cap + 1, capi.RESECT_CORR_DTYPE)
        k = lib().ba_rows(C.byref(self._c), C.c_int(j), C.c_void_p(_p(out)))
        return out[:k]

    def point_eval(self, head, X=None):
        """EVALUATE-POINT of the track headed by `head` at X (default: its point as it stands) -> (H [3, 3], g [3], cost, n, member flags [L + 1])."""
        X = np.ascontiguousarray(self.tracks[head]["X"] if X is None else X, dtype=np.float64).copy()
        s, fl = np.zeros(10), np.zeros(len(self.paths[head]) + 1, np.uint8)
        n = lib().ba_point_eval(C.byref(self._c), C.c_uint32(self.index[head]), C.c_void_p(_p(X)), C.c_void_p(_p(s)), C.c_void_p(_p(fl)))
        H = np.zeros((3, 3))
        H[np.triu_indices(3)] = s[:6]
        return H + np.triu(H, 1).T, s[6:9].copy(), float(s[9]), int(n), fl.astype(bool)

    def point_delta(self, H, g):
        s, d = np.zeros(10), np.zeros(3)
        s[:6], s[6:9] = np.asarray(H)[np.triu_indices(3)], g
        return d if lib().ba_point_delta(C.c_void_p(_p(s)), C.c_void_p(_p(d))) else None

    def views(self, head):
        """[(camera index or -1 for the held camera, frame, point index)] of the track's views, in order."""
        path = self.paths[head]
        j0 = head[0]
        out = [(j0 - 1 if j0 >= 1 and int(self.chain["linked"][j0]) != 0 else -1, j0, int(self.matches[j0]["query"][path[0][1]]) & NONE)]
        for p in range(1, len(path)):
            j, i = path[p]
            out.append((j - 1, j, int(self.matches[j]["query"][i]) & NONE))
        j, i = path[-1]
        out.append((j, j + 1, int(self.matches[j]["train"][i]) & NONE))
        return out

    def run(self, sweeps):
        """The call: `sweeps` sweeps from the state as it stands, then the outputs -> dict(tracks [n, cap] TRACK_DTYPE (rows past m_j:
        tracks_in's), cams [n] BUNDLE_CAM_DTYPE, point_info [n, cap] BUNDLE_POINT_DTYPE with written bool [n, cap], member bool [n, 2, cap])."""
        n, cap = self.n, self.cap
        cams, info = np.zeros(max(n, 1), capi.BUNDLE_CAM_DTYPE), np.zeros((n, cap), capi.BUNDLE_POINT_DTYPE)
        written, mb = np.zeros((n, cap), np.uint8), np.zeros((n, 2, cap), np.uint8)
        if n:
            lib().ba_run(C.byref(self._c), C.c_uint32(int(sweeps)), C.c_void_p(_p(cams)), C.c_void_p(_p(info)), C.c_void_p(_p(written)), C.c_void_p(_p(mb)))
        return dict(tracks=self.tracks.copy(), cams=cams[:n].copy(), point_info=info, written=written.astype(bool), member=mb.astype(bool), ms=self.ms.copy())


def bundle(poses, matches, match_counts, front_bits, point_cap, chain, frame_points, tracks_in, refs, intrinsics, max_dist2, min_views, sweeps,
           cams_in=None):
    """The whole call -> Problem.run()'s dict."""
    if len(np.ascontiguousarray(poses).reshape(-1)) == 0:                              # no pairs: nothing is written
        cap = np.asarray(matches).shape[-1] if np.asarray(matches).ndim == 2 else 0
        return dict(tracks=np.zeros((0, cap), capi.TRACK_DTYPE), cams=np.zeros(0, capi.BUNDLE_CAM_DTYPE), point_info=np.zeros((0, cap), capi.BUNDLE_POINT_DTYPE),
                    written=np.zeros((0, cap), bool), member=np.zeros((0, 2, cap), bool), ms=np.zeros(0, np.uint32))
    return Problem(poses, matches, match_counts, front_bits, point_cap, chain, frame_points, tracks_in, refs, intrinsics, max_dist2, min_views,
                   cams_in).run(sweeps)


def dense_tracks(ms, rows, refs, cap, fill=0):
    """tracksref.tracks' per-pair rows and refs as the [n, cap] arrays the entry point reads (rows past m_j: `fill` bytes)."""
    n = len(ms)
    t, r = np.zeros((n, cap), capi.TRACK_DTYPE), np.zeros((n, cap), capi.TRACK_REF_DTYPE)
    t.view(np.uint8)[...] = fill
    r.view(np.uint8)[...] = fill
    for j in range(n):
        t[j, :ms[j]], r[j, :ms[j]] = rows[j], refs[j]
    return t, r

// Gauss-Newton refinement of the resected pose (include/vslam.h, "resection: Gauss-Newton refinement over all inliers").
//   k_rr_init       : one lane per pair: models_in -> RrState; the first candidate is the input pose
//   k_rr_pass       : the hot path, grid = (blocks of 4096 rows, pairs), 256 lanes = the 256 slots of the header's ordered sum, 16
//                     rows per lane, each 48-byte row loaded as three 16-byte loads: EVALUATE of the candidate pose - membership,
//                     the residual, the two Jacobian rows and all 29 sums in one walk; the pose and fx, fy are wave-uniform
//                     (the state is read through blockIdx.y alone).  The tree is refit_tree<29>: h = 128, 64 through 29696
//                     bytes of LDS, h <= 32 by __shfl_down in wave 0; the block's sums go to the scratch with plain stores
//   k_rr_step       : one lane per pair, after each pass: the block sums added left to right, the candidate kept or stop 4,
//                     then stop 1 or STEP - the 6 x 7 Gauss-Jordan in LDS, lane-strided, because the pivot is data-dependent -
//                     and the next candidate, or stop 3; the launch with r == rounds writes models and info
//   k_rr_flags_zero : one lane per word of inlier_bits below (n_obs + 63) / 64
//   k_rr_flags      : one lane per dense row: a member under the output pose sets bit corr.b (an integer atomicOr: the word is
//                     the same in any order)
// No floating-point atomics, no flags or fences between workgroups: kernel boundaries order everything.  A workgroup of a
// stopped pair, or of a block past the pair's n_corr, leaves before its first barrier (workgroup-uniform).  The arithmetic is
// the header's, operation for operation, under the rules of kernels_epipolar.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_resect_refine_plan.h"

namespace vslam {

struct __attribute__((aligned(16))) RrRow {  // vslam_resect_corr as three 16-byte loads
    double2 a, b, c;                         // {Y0, Y1}, {Y2, u}, {v, b | reserved}
};
static_assert(sizeof(RrRow) == sizeof(vslam_resect_corr), "a row is 48 bytes");

__device__ __forceinline__ unsigned int rr_ncorr(const RrState& st, unsigned int ocap) { return st.in.n_corr < ocap ? st.in.n_corr : ocap; }

// Z = R Y + t and the member test of one row (step 6 of the resection section).
__device__ __forceinline__ bool rr_member(const double (&R)[9], const double (&t)[3], double fx, double fy, double Y0, double Y1, double Y2, double u,
                                          double v, double max_dist2, double (&Z)[3]) {
    Z[0] = ((R[0] * Y0 + R[1] * Y1) + R[2] * Y2) + t[0];
    Z[1] = ((R[3] * Y0 + R[4] * Y1) + R[5] * Y2) + t[1];
    Z[2] = ((R[6] * Y0 + R[7] * Y1) + R[8] * Y2) + t[2];
    const double ex = (u * Z[2] - Z[0]) * fx, ey = (v * Z[2] - Z[1]) * fy;
    return Z[2] > 0.0 && (ex * ex + ey * ey) < max_dist2 * (Z[2] * Z[2]);
}

__global__ __launch_bounds__(RR_PAIR_WG) void k_rr_init(const vslam_resect* __restrict__ models_in, int n_pairs, RrState* __restrict__ state) {
    const int j = blockIdx.x * RR_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    RrState s;
    s.in = models_in[j];
#pragma unroll
    for (int k = 0; k < 9; ++k) s.Rcur[k] = s.Rcand[k] = s.in.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s.tcur[k] = s.tcand[k] = s.in.t[k];
    s.cost_cur = s.cost_before = 0.0;
    s.n_cur = s.n_before = s.accepted = 0;
    s.stop = s.in.best < 0 ? 5 : RR_RUNNING;
    state[j] = s;
}

// partial [n_pairs][sum_blocks][RR_SUMS]: H's upper triangle row-major, g, cost, n.
__global__ __launch_bounds__(REFIT_WG) void k_rr_pass(const vslam_resect_corr* __restrict__ corr, unsigned int ocap, const RrState* __restrict__ state,
                                                       double fx, double fy, double max_dist2, double* __restrict__ partial,
                                                       unsigned int sum_blocks) {
    __shared__ double lds[RR_SUMS * 128];  // 29696 bytes
    const int j = blockIdx.y;
    const RrState* st = state + j;
    if (st->stop != RR_RUNNING) return;
    const unsigned int m = rr_ncorr(*st, ocap);
    const size_t first = (size_t)blockIdx.x * REFIT_BLOCK;
    if (first >= m) return;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = st->Rcand[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = st->tcand[k];
    const RrRow* src = reinterpret_cast<const RrRow*>(corr + (size_t)j * ocap);
    double s[RR_SUMS];
#pragma unroll
    for (int k = 0; k < (int)RR_SUMS; ++k) s[k] = 0.0;
#pragma unroll 2
    for (unsigned int k = 0; k < REFIT_PER_LANE; ++k) {
        const size_t i = first + (size_t)k * REFIT_WG + threadIdx.x;
        if (i < m) {
            const RrRow row = src[i];
            const double u = row.b.y, v = row.c.x;
            double Z[3];
            if (rr_member(R, t, fx, fy, row.a.x, row.a.y, row.b.x, u, v, max_dist2, Z)) {  // (a row that is not a member adds +0.0: nothing)
                const double iz = 1.0 / Z[2];
                const double px = Z[0] * iz, py = Z[1] * iz;
                const double rx = (px - u) * fx, ry = (py - v) * fy;
                const double pxy = px * py;
                const double Jx[6] = {fx * (-pxy), fx * (1.0 + px * px), fx * (-py), fx * iz, fx * 0.0, fx * (-(px * iz))};
                const double Jy[6] = {fy * (-(1.0 + py * py)), fy * pxy, fy * px, fy * 0.0, fy * iz, fy * (-(py * iz))};
                int e = 0;
#pragma unroll
                for (int p = 0; p < 6; ++p) {
#pragma unroll
                    for (int q = p; q < 6; ++q, ++e) s[e] = s[e] + (Jx[p] * Jx[q] + Jy[p] * Jy[q]);
                }
#pragma unroll
                for (int p = 0; p < 6; ++p) s[21 + p] = s[21 + p] + (Jx[p] * rx + Jy[p] * ry);
                s[27] = s[27] + (rx * rx + ry * ry);
                s[28] = s[28] + 1.0;
            }
        }
    }
    refit_tree<(int)RR_SUMS>(s, lds);
    if (threadIdx.x == 0) {
        double* out = partial + ((size_t)j * sum_blocks + blockIdx.x) * RR_SUMS;
#pragma unroll
        for (int k = 0; k < (int)RR_SUMS; ++k) out[k] = s[k];
    }
}

__device__ __forceinline__ double rr_canonical(double x) { return x == x ? x : __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool rr_finite(double x) { return fabs(x) < __builtin_huge_val(); }

// `models` may be the buffer k_rr_init read: it is written by the last launch only (r == rounds), so it is not __restrict__.
__global__ __launch_bounds__(RR_PAIR_WG) void k_rr_step(const double* __restrict__ partial, unsigned int sum_blocks, unsigned int ocap, int n_pairs,
                                                         unsigned int r, unsigned int rounds, RrState* __restrict__ state, vslam_resect* models,
                                                         vslam_resect_refine* __restrict__ info) {
    __shared__ double a[42][RR_PAIR_WG];  // the 6 x 7 matrix of STEP, element e of lane l at a[e][l]: 21504 bytes
    const int j = blockIdx.x * RR_PAIR_WG + threadIdx.x, l = threadIdx.x;
    if (j >= n_pairs) return;  // (no barrier below: every lane works on its own column of a)
    RrState* st = state + j;
    if (st->stop == RR_RUNNING) {
        // the pair's sums: ((B_0 + B_1) + B_2) + ...
        const unsigned int m = rr_ncorr(*st, ocap);
        const unsigned int nb = (unsigned int)(((size_t)m + REFIT_BLOCK - 1) / REFIT_BLOCK);
        const double* src = partial + (size_t)j * sum_blocks * RR_SUMS;
        double s[RR_SUMS];
#pragma unroll
        for (int k = 0; k < (int)RR_SUMS; ++k) s[k] = nb ? src[k] : 0.0;
        for (unsigned int b = 1; b < nb; ++b) {
#pragma unroll
            for (int k = 0; k < (int)RR_SUMS; ++k) s[k] = s[k] + src[(size_t)b * RR_SUMS + k];
        }
        const unsigned int n = (unsigned int)s[28];
        const double cost = s[27];
        bool running = true;
        if (r == 0) {
            st->n_before = st->n_cur = n;
            st->cost_before = st->cost_cur = cost;
        } else if (n > st->n_cur || (n == st->n_cur && cost < st->cost_cur)) {  // round step 3
#pragma unroll
            for (int k = 0; k < 9; ++k) st->Rcur[k] = st->Rcand[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) st->tcur[k] = st->tcand[k];
            st->n_cur = n, st->cost_cur = cost;
            st->accepted += 1;
        } else {
            st->stop = 4;
            running = false;
        }
        if (running) {
            if (r == rounds) {
                st->stop = 0;
            } else if (st->n_cur < 6) {  // round step 1
                st->stop = 1;
            } else {  // round step 2: STEP from the pose just evaluated (it is the current one)
                // a. [H | -g]
                {
                    int e = 0;
#pragma unroll
                    for (int p = 0; p < 6; ++p) {
#pragma unroll
                        for (int q = p; q < 6; ++q, ++e) a[7 * p + q][l] = s[e], a[7 * q + p][l] = s[e];
                        a[7 * p + 6][l] = -s[21 + p];
                    }
                }
                unsigned int used = 0, pcs = 0;  // chosen columns: bit mask, and 3 bits per step
                bool ok = true;
                for (int k = 0; k < 6; ++k) {
                    double best = 0.0;
                    int pr = -1, pc = -1;
                    for (int rr = k; rr < 6; ++rr)
                        for (int c = 0; c < 6; ++c) {
                            if (used >> c & 1u) continue;
                            const double x = fabs(a[7 * rr + c][l]);
                            if (x > best) best = x, pr = rr, pc = c;
                        }
                    if (pr < 0 || !(best < __builtin_huge_val())) {
                        ok = false;
                        break;
                    }
                    if (pr != k)
                        for (int c = 0; c < 7; ++c) {
                            const double x = a[7 * k + c][l];
                            a[7 * k + c][l] = a[7 * pr + c][l];
                            a[7 * pr + c][l] = x;
                        }
                    const double p = a[7 * k + pc][l];
                    double rowk[7];
#pragma unroll
                    for (int c = 0; c < 7; ++c) {
                        rowk[c] = a[7 * k + c][l] / p;
                        a[7 * k + c][l] = rowk[c];
                    }
                    for (int i = 0; i < 6; ++i) {
                        if (i == k) continue;
                        const double g = a[7 * i + pc][l];
#pragma unroll
                        for (int c = 0; c < 7; ++c) a[7 * i + c][l] = a[7 * i + c][l] - g * rowk[c];
                    }
                    used |= 1u << pc;
                    pcs |= (unsigned int)pc << (3 * k);
                }
                double Rn[9], tn[3];
                if (ok) {
                    // d lives in row 0's slots from here on (the matrix is no longer needed once the last column is read out)
                    double dk[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) dk[k] = a[7 * k + 6][l];
#pragma unroll
                    for (int k = 0; k < 6; ++k) a[(pcs >> (3 * k)) & 7u][l] = dk[k];
                    double d[6];
#pragma unroll
                    for (int k = 0; k < 6; ++k) {
                        d[k] = a[k][l];
                        ok &= rr_finite(d[k]);
                    }
                    // b. the Cayley rotation
                    const double a0 = d[0] / 2.0, a1 = d[1] / 2.0, a2 = d[2] / 2.0;
                    const double q = (a0 * a0 + a1 * a1) + a2 * a2;
                    const double e = 1.0 - q, den = 1.0 + q;
                    double D[9];
                    D[0] = (e + 2.0 * (a0 * a0)) / den;
                    D[4] = (e + 2.0 * (a1 * a1)) / den;
                    D[8] = (e + 2.0 * (a2 * a2)) / den;
                    D[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den;
                    D[3] = (2.0 * (a1 * a0) + 2.0 * a2) / den;
                    D[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
                    D[6] = (2.0 * (a2 * a0) - 2.0 * a1) / den;
                    D[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;
                    D[7] = (2.0 * (a2 * a1) + 2.0 * a0) / den;
                    // c. the new pose
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            Rn[3 * i + c] = (D[3 * i] * st->Rcur[c] + D[3 * i + 1] * st->Rcur[3 + c]) + D[3 * i + 2] * st->Rcur[6 + c];
                            ok &= rr_finite(Rn[3 * i + c]);
                        }
                        tn[i] = ((D[3 * i] * st->tcur[0] + D[3 * i + 1] * st->tcur[1]) + D[3 * i + 2] * st->tcur[2]) + d[3 + i];
                        ok &= rr_finite(tn[i]);
                    }
                }
                if (ok) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) st->Rcand[k] = Rn[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) st->tcand[k] = tn[k];
                } else {
                    st->stop = 3;
                }
            }
        }
    }
    if (r == rounds) {
        vslam_resect out = st->in;
        double cb = 0.0, ca = 0.0;
        if (st->stop != 5) {
#pragma unroll
            for (int k = 0; k < 9; ++k) out.R[k] = rr_canonical(st->Rcur[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) out.t[k] = rr_canonical(st->tcur[k]);
            out.n_inliers = st->n_cur;
            cb = rr_canonical(st->cost_before), ca = rr_canonical(st->cost_cur);
        }
        models[j] = out;
        if (info) info[j] = vslam_resect_refine{st->n_before, st->n_cur, st->accepted, st->stop, cb, ca};
    }
}

// grid = (word blocks of 256, pairs): the words of inlier_bits that hold an observation record below n_obs.
__global__ __launch_bounds__(REFIT_WG) void k_rr_flags_zero(const vslam_resect* __restrict__ models, unsigned int ocap, unsigned long long* __restrict__ flags,
                                                             unsigned int fwords) {
    const int j = blockIdx.y;
    const unsigned int n_obs = models[j].n_obs < ocap ? models[j].n_obs : ocap;
    const size_t w = (size_t)blockIdx.x * REFIT_WG + threadIdx.x;
    if (w < ((size_t)n_obs + 63) / 64) flags[(size_t)j * fwords + w] = 0ull;
}

// grid = (row blocks of 256, pairs): the members under the output pose, by observation record.  The rows of a wave come from
// consecutive observation records, so their bits fall into one or two words: the lanes of one word OR their bits across the
// wave and one lane issues the atomic (one per lane made 64 lanes queue on one address: 0.94 ms on full lists against 0.13).
__global__ __launch_bounds__(REFIT_WG) void k_rr_flags(const vslam_resect_corr* __restrict__ corr, unsigned int ocap, const vslam_resect* __restrict__ models,
                                                        double fx, double fy, double max_dist2, unsigned long long* __restrict__ flags,
                                                        unsigned int fwords) {
    const int j = blockIdx.y;
    const vslam_resect* mo = models + j;
    if (mo->best < 0) return;
    const unsigned int m = mo->n_corr < ocap ? mo->n_corr : ocap, n_obs = mo->n_obs < ocap ? mo->n_obs : ocap;
    const size_t i = (size_t)blockIdx.x * REFIT_WG + threadIdx.x;
    if (!g3_wave_has_record(i, m)) return;  // (wave-uniform)
    bool set = false;
    unsigned int b = 0;
    if (i < m) {
        const RrRow row = reinterpret_cast<const RrRow*>(corr + (size_t)j * ocap)[i];
        b = (unsigned int)(unsigned long long)__double_as_longlong(row.c.y);  // the low word: corr.b
        if (b < n_obs) {  // (the words past (n_obs + 63) / 64 are not this call's)
            double R[9], t[3], Z[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = mo->R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = mo->t[k];
            set = rr_member(R, t, fx, fy, row.a.x, row.a.y, row.b.x, row.b.y, row.c.x, max_dist2, Z);
        }
    }
    const unsigned int word = b >> 6, lane = threadIdx.x & 63u;
    unsigned long long pending = __ballot(set);
    while (pending) {  // (wave-uniform)
        const unsigned int leader = (unsigned int)__ffsll((long long)pending) - 1u;
        const unsigned int w = (unsigned int)__shfl((int)word, (int)leader);
        const bool mine = set && word == w;
        unsigned long long bits = mine ? 1ull << (b & 63u) : 0ull;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) bits |= (unsigned long long)__shfl_xor((long long)bits, off);
        if (lane == leader) atomicOr(flags + (size_t)j * fwords + w, bits);  // w < (n_obs + 63) / 64 <= fwords
        pending &= ~__ballot(mine);
    }
}

}  // namespace vslam

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
// the header's, operation for operation, under the rules of kernels_epipolar.hip.h.  The member test, EVALUATE of one row and
// STEP are kernels_resect_refine_step.hip.h's: the bundle adjustment's camera step runs the same lines.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_resect_refine_step.hip.h"

namespace vslam {

struct __attribute__((aligned(16))) RrRow {  // vslam_resect_corr as three 16-byte loads
    double2 a, b, c;                         // {Y0, Y1}, {Y2, u}, {v, b | reserved}
};
static_assert(sizeof(RrRow) == sizeof(vslam_resect_corr), "a row is 48 bytes");

__device__ __forceinline__ unsigned int rr_ncorr(const RrState& st, unsigned int ocap) { return st.in.n_corr < ocap ? st.in.n_corr : ocap; }

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
            RR_ROW_SUMS(R, t, fx, fy, row.a.x, row.a.y, row.b.x, u, v, max_dist2, s);
        }
    }
    refit_tree<(int)RR_SUMS>(s, lds);
    if (threadIdx.x == 0) {
        double* out = partial + ((size_t)j * sum_blocks + blockIdx.x) * RR_SUMS;
#pragma unroll
        for (int k = 0; k < (int)RR_SUMS; ++k) out[k] = s[k];
    }
}

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
                RR_STEP_SOLVE(a, l, s, st->Rcur, st->tcur);
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

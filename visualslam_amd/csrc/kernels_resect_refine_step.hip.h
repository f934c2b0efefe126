// What the kernels of the resection's refinement (kernels_resect_refine.hip.h) and of the bundle adjustment's camera step
// (kernels_bundle.hip.h) share, each stated once: the member test, EVALUATE of one row and STEP (include/vslam.h, "resection:
// Gauss-Newton refinement over all inliers").  No kernel, so two translation units include it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_resect_refine_plan.h"

namespace vslam {

// Z = R Y + t and the member test of one row (step 6 of the resection section).
__device__ __forceinline__ bool rr_member(const double (&R)[9], const double (&t)[3], double fx, double fy, double Y0, double Y1, double Y2, double u,
                                          double v, double max_dist2, double (&Z)[3]) {
    Z[0] = ((R[0] * Y0 + R[1] * Y1) + R[2] * Y2) + t[0];
    Z[1] = ((R[3] * Y0 + R[4] * Y1) + R[5] * Y2) + t[1];
    Z[2] = ((R[6] * Y0 + R[7] * Y1) + R[8] * Y2) + t[2];
    const double ex = (u * Z[2] - Z[0]) * fx, ey = (v * Z[2] - Z[1]) * fy;
    return Z[2] > 0.0 && (ex * ex + ey * ey) < max_dist2 * (Z[2] * Z[2]);
}

__device__ __forceinline__ double rr_canonical(double x) { return x == x ? x : __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ bool rr_finite(double x) { return fabs(x) < __builtin_huge_val(); }

// STEP from (Rcur, tcur) with the 29 sums s of its evaluation, as text: the 6 x 7 Gauss-Jordan in the lane's column l of a [42][RR_PAIR_WG]
// (LDS), the Cayley rotation and the new pose; it declares `bool ok` (false: invalid) and `double Rn[9], tn[3]`.  A macro, like
// RR_ROW_SUMS below and for its reason: k_ba_cam_step (kernels_bundle.hip.h) runs the same lines.
#define RR_STEP_SOLVE(a, l, s, Rcur, tcur) \
                                                                                                                             \
                {                                                                                                            \
                    int e = 0;                                                                                               \
_Pragma("unroll")                                                                                                            \
                    for (int p = 0; p < 6; ++p) {                                                                            \
_Pragma("unroll")                                                                                                            \
                        for (int q = p; q < 6; ++q, ++e) a[7 * p + q][l] = s[e], a[7 * q + p][l] = s[e];                     \
                        a[7 * p + 6][l] = -s[21 + p];                                                                        \
                    }                                                                                                        \
                }                                                                                                            \
                unsigned int used = 0, pcs = 0;                                                                              \
                bool ok = true;                                                                                              \
                for (int k = 0; k < 6; ++k) {                                                                                \
                    double best = 0.0;                                                                                       \
                    int pr = -1, pc = -1;                                                                                    \
                    for (int rr = k; rr < 6; ++rr)                                                                           \
                        for (int c = 0; c < 6; ++c) {                                                                        \
                            if (used >> c & 1u) continue;                                                                    \
                            const double x = fabs(a[7 * rr + c][l]);                                                         \
                            if (x > best) best = x, pr = rr, pc = c;                                                         \
                        }                                                                                                    \
                    if (pr < 0 || !(best < __builtin_huge_val())) {                                                          \
                        ok = false;                                                                                          \
                        break;                                                                                               \
                    }                                                                                                        \
                    if (pr != k)                                                                                             \
                        for (int c = 0; c < 7; ++c) {                                                                        \
                            const double x = a[7 * k + c][l];                                                                \
                            a[7 * k + c][l] = a[7 * pr + c][l];                                                              \
                            a[7 * pr + c][l] = x;                                                                            \
                        }                                                                                                    \
                    const double p = a[7 * k + pc][l];                                                                       \
                    double rowk[7];                                                                                          \
_Pragma("unroll")                                                                                                            \
                    for (int c = 0; c < 7; ++c) {                                                                            \
                        rowk[c] = a[7 * k + c][l] / p;                                                                       \
                        a[7 * k + c][l] = rowk[c];                                                                           \
                    }                                                                                                        \
                    for (int i = 0; i < 6; ++i) {                                                                            \
                        if (i == k) continue;                                                                                \
                        const double g = a[7 * i + pc][l];                                                                   \
_Pragma("unroll")                                                                                                            \
                        for (int c = 0; c < 7; ++c) a[7 * i + c][l] = a[7 * i + c][l] - g * rowk[c];                         \
                    }                                                                                                        \
                    used |= 1u << pc;                                                                                        \
                    pcs |= (unsigned int)pc << (3 * k);                                                                      \
                }                                                                                                            \
                double Rn[9], tn[3];                                                                                         \
                if (ok) {                                                                                                    \
                                                                                                                             \
                    double dk[6];                                                                                            \
_Pragma("unroll")                                                                                                            \
                    for (int k = 0; k < 6; ++k) dk[k] = a[7 * k + 6][l];                                                     \
_Pragma("unroll")                                                                                                            \
                    for (int k = 0; k < 6; ++k) a[(pcs >> (3 * k)) & 7u][l] = dk[k];                                         \
                    double d[6];                                                                                             \
_Pragma("unroll")                                                                                                            \
                    for (int k = 0; k < 6; ++k) {                                                                            \
                        d[k] = a[k][l];                                                                                      \
                        ok &= rr_finite(d[k]);                                                                               \
                    }                                                                                                        \
                                                                                                                             \
                    const double a0 = d[0] / 2.0, a1 = d[1] / 2.0, a2 = d[2] / 2.0;                                          \
                    const double q = (a0 * a0 + a1 * a1) + a2 * a2;                                                          \
                    const double e = 1.0 - q, den = 1.0 + q;                                                                 \
                    double D[9];                                                                                             \
                    D[0] = (e + 2.0 * (a0 * a0)) / den;                                                                      \
                    D[4] = (e + 2.0 * (a1 * a1)) / den;                                                                      \
                    D[8] = (e + 2.0 * (a2 * a2)) / den;                                                                      \
                    D[1] = (2.0 * (a0 * a1) - 2.0 * a2) / den;                                                               \
                    D[3] = (2.0 * (a1 * a0) + 2.0 * a2) / den;                                                               \
                    D[2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;                                                               \
                    D[6] = (2.0 * (a2 * a0) - 2.0 * a1) / den;                                                               \
                    D[5] = (2.0 * (a1 * a2) - 2.0 * a0) / den;                                                               \
                    D[7] = (2.0 * (a2 * a1) + 2.0 * a0) / den;                                                               \
                                                                                                                             \
_Pragma("unroll")                                                                                                            \
                    for (int i = 0; i < 3; ++i) {                                                                            \
_Pragma("unroll")                                                                                                            \
                        for (int c = 0; c < 3; ++c) {                                                                        \
                            Rn[3 * i + c] = (D[3 * i] * Rcur[c] + D[3 * i + 1] * Rcur[3 + c]) + D[3 * i + 2] * Rcur[6 + c];  \
                            ok &= rr_finite(Rn[3 * i + c]);                                                                  \
                        }                                                                                                    \
                        tn[i] = ((D[3 * i] * tcur[0] + D[3 * i + 1] * tcur[1]) + D[3 * i + 2] * tcur[2]) + d[3 + i];         \
                        ok &= rr_finite(tn[i]);                                                                              \
                    }                                                                                                        \
                }                                                                                                            \
    (void)0

// EVALUATE of one row, as text: a member under (R, t) adds its 29 terms to the slot's sums s (a row that is not a member adds
// +0.0: nothing).  A macro, not a function: the bundle adjustment's camera pass (kernels_bundle.hip.h) states the same lines over
// rows it gathers itself, and k_rr_pass keeps the very instructions it had when the lines stood in its body.
#define RR_ROW_SUMS(R, t, fx, fy, Y0, Y1, Y2, u, v, max_dist2, s) \
            double Z[3];                                                                                                     \
            if (rr_member(R, t, fx, fy, Y0, Y1, Y2, u, v, max_dist2, Z)) {                                                   \
                const double iz = 1.0 / Z[2];                                                                                \
                const double px = Z[0] * iz, py = Z[1] * iz;                                                                 \
                const double rx = (px - u) * fx, ry = (py - v) * fy;                                                         \
                const double pxy = px * py;                                                                                  \
                const double Jx[6] = {fx * (-pxy), fx * (1.0 + px * px), fx * (-py), fx * iz, fx * 0.0, fx * (-(px * iz))};  \
                const double Jy[6] = {fy * (-(1.0 + py * py)), fy * pxy, fy * px, fy * 0.0, fy * iz, fy * (-(py * iz))};     \
                int e = 0;                                                                                                   \
_Pragma("unroll")                                                                                                            \
                for (int p = 0; p < 6; ++p) {                                                                                \
_Pragma("unroll")                                                                                                            \
                    for (int q = p; q < 6; ++q, ++e) s[e] = s[e] + (Jx[p] * Jx[q] + Jy[p] * Jy[q]);                          \
                }                                                                                                            \
_Pragma("unroll")                                                                                                            \
                for (int p = 0; p < 6; ++p) s[21 + p] = s[21 + p] + (Jx[p] * rx + Jy[p] * ry);                               \
                s[27] = s[27] + (rx * rx + ry * ry);                                                                         \
                s[28] = s[28] + 1.0;                                                                                         \
            }                                                                                                                \
    (void)0

}  // namespace vslam

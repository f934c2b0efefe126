// The host arithmetic of vslam_resect_refine_dev (include/vslam.h, "resection: Gauss-Newton refinement over all inliers") that
// needs no HIP: the argument checks in the ABI's order, and the grids and scratch sizes, all from the capacity (the counts
// live on the device).  Stated once, here, so that a host program can run it under the sanitizers with extreme capacities
// (tests/resect_refine_plan_driver.cpp).  The ordered sum is the refit's: its block, slots and lanes are vslam_refit_plan.h's.
#pragma once
#include "vslam_refit_plan.h"

namespace vslam {

constexpr unsigned int RR_SUMS = 29;     // one pass: the 21 sums of H's upper triangle, the 6 of g, the cost, the member count
constexpr unsigned int RR_PAIR_WG = 64;  // pairs (lanes) per workgroup of the per-pair kernels: one wave, 42 f64 of LDS per lane
constexpr int RR_RUNNING = -1;           // RrState::stop of a pair that has not stopped

// The per-pair record of the scratch: what the rounds carry from kernel to kernel.
struct RrState {
    vslam_resect in;                // models_in[j], read once (models may be the same buffer)
    double Rcur[9], tcur[3];        // the pose kept so far
    double Rcand[9], tcand[3];      // the pose the next pass evaluates: the input's, then each round's (R, t)_new
    double cost_cur, cost_before;
    unsigned int n_cur, n_before, accepted;
    int stop;
};
static_assert(sizeof(RrState) == 344, "the header states the scratch per pair");

// The message of the first failed check, without the stage in front, in the order of vslam_resect_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.  `aligned`: the device entry point loads the
// rows with 16-byte loads.
inline const char* resect_refine_check_args(const vslam_resect* models_in, const vslam_resect_corr* corr, uint32_t obs_cap, int n_pairs,
                                            const vslam_resect_refine_params* prm, const vslam_resect_refine_out* out, bool aligned) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_resect_refine_out)) return "out->struct_size is not sizeof(vslam_resect_refine_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->rounds < 1 || prm->rounds > 8) return "1 .. 8 rounds";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = check_intrinsics(prm->K, "an intrinsic is not finite")) return why;
    if (const char* why = twoview_check_inputs(models_in && corr, obs_cap, 1, 1)) return why;
    if (aligned && (reinterpret_cast<uintptr_t>(corr) & 15u)) return "correspondences must be 16-byte aligned";
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(obs_cap);
    OUT_NEEDS(out, models, vslam_resect, np);
    OUT_FITS(out, info, vslam_resect_refine, np);
    // np * fwords < 2^42: no element count wraps, and the byte counts are compared by division
    OUT_FITS(out, inlier_bits, uint64_t, np * fwords);
    const uintptr_t a = reinterpret_cast<uintptr_t>(models_in), b = reinterpret_cast<uintptr_t>(out->models), span = np * sizeof(vslam_resect);
    if (a != b && (a < b ? b - a : a - b) < span) return "models overlaps models_in without being equal to it";
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, at most 2^20 blocks per pair, 29 f64 per block - below 2^44 bytes.
struct ResectRefinePlan {
    unsigned int fwords;       // ballot words per pair of inlier_bits
    unsigned int sum_blocks;   // grid.x of the streaming kernel: blocks of the ordered sum per pair, from the capacity
    unsigned int row_blocks;   // grid.x of the flag kernels: REFIT_WG rows (or words) per workgroup
    unsigned int pair_blocks;  // grid.x of the per-pair kernels
    size_t partial_elems;      // scratch: [n_pairs][sum_blocks][RR_SUMS] f64 block sums
    size_t state_elems;        // scratch: RrState [n_pairs]
};

inline ResectRefinePlan resect_refine_plan(uint32_t obs_cap, int n_pairs) {
    ResectRefinePlan p{};
    const size_t np = (size_t)n_pairs;
    p.fwords = (unsigned int)twoview_fwords(obs_cap);
    p.sum_blocks = (unsigned int)(((size_t)obs_cap + REFIT_BLOCK - 1) / REFIT_BLOCK);
    p.row_blocks = (unsigned int)(((size_t)obs_cap + REFIT_WG - 1) / REFIT_WG);
    p.pair_blocks = (unsigned int)((np + RR_PAIR_WG - 1) / RR_PAIR_WG);
    p.partial_elems = np * p.sum_blocks * RR_SUMS;
    p.state_elems = np;
    return p;
}

}  // namespace vslam

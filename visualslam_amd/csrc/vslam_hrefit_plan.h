// The host arithmetic of vslam_hrefit_dev (include/vslam.h, "homography: least-squares refit over the inliers") that needs no
// HIP: the argument checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on
// the device).  Stated once, here, so that a host program can run it under the sanitizers with extreme capacities
// (tests/hrefit_plan_driver.cpp).  The block of the ordered sum and the per-pair workgroup are the refit of F's
// (vslam_refit_plan.h): the two stages sum the same way.
#pragma once
#include "vslam_refit_plan.h"

namespace vslam {

constexpr unsigned int HREFIT_SUMS = 24;  // the widest pass: A_k, B_k, C_k, D_k for the six index pairs of a symmetric 3 x 3 block

// The per-pair record of the scratch (520 bytes), a type of its own as RefitState is.
struct HRefitState : RefitRounds<vslam_homography, HomModel, vslam_hrefit, 4, HREFIT_SUMS> {};

// The message of the first failed check, without the stage in front, in the order of refit_check_args (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* hrefit_check_args(const vslam_homography* models_in, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                     const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                     int n_pairs, const vslam_epipolar* epipolar_models, const vslam_hrefit_params* prm, const vslam_hrefit_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_hrefit_out)) return "out->struct_size is not sizeof(vslam_hrefit_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->rounds < 1 || prm->rounds > 8) return "1 .. 8 rounds";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (epipolar_models && prm->degenerate_den == 0) return "degenerate_den must be positive";
    if (const char* why = twoview_check_inputs(models_in && matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, models, vslam_homography, np);
    OUT_FITS(out, info, vslam_hrefit, np);
    if (const char* why = twoview_check_lists(out, np, fwords)) return why;
    if (out->gated_models && !epipolar_models) return "gated_models needs epipolar_models";
    OUT_FITS(out, gated_models, vslam_epipolar, np);
    return nullptr;
}

// Grids and scratch: the refit of F's, 24 f64 per block (below 2^44 bytes).
using HRefitPlan = RefitPlan;
inline HRefitPlan hrefit_plan(uint32_t match_cap, int n_pairs) { return refit_plan(match_cap, n_pairs, HREFIT_SUMS); }

}  // namespace vslam

// The host arithmetic of vslam_match_guided_hf_dev (include/vslam.h, "guided matching under H or F") that needs no HIP: the
// argument checks in the ABI's order; the grids and scratch sizes are the guided plan's (vslam_guided_plan.h), all in size_t
// from the capacities (the counts and both model arrays live on the device, so a pair's kind is not known here).  Stated once,
// here, so that a host program can run it under the sanitizers with extreme capacities (tests/guided_hf_plan_driver.cpp).
#pragma once
#include "vslam_guided_plan.h"

namespace vslam {

// The kind of a pair, read on the device: F where the epipolar record has a model, else H where the homography record has one.
enum GuidedKind : int { GUIDED_KIND_NONE = 0, GUIDED_KIND_F = 1, GUIDED_KIND_H = 2 };

// The message of the first failed check - the entry point puts "match_guided_hf: " in front -, vslam_match_guided_dev's checks
// in its order where they coincide (guided_check_args), max_transfer2 after max_dist2, each looked at only when its model array
// is given; nullptr: the call is valid.
inline const char* guided_hf_check_args(const vslam_desc_sets* Q, const vslam_desc_sets* T, const vslam_epipolar* epipolar_models,
                                        const vslam_homography* homography_models, int n_pairs, const vslam_guided_hf_params* prm,
                                        const vslam_match_out* out) {
    if (!Q || !T || !out || !prm) return "null argument";
    if (!epipolar_models && !homography_models) return "epipolar_models and homography_models are both null";
    if (out->struct_size != sizeof(vslam_match_out)) return "out->struct_size is not sizeof(vslam_match_out)";
    if (n_pairs < 0 || n_pairs > 65535) return "0 .. 65535 pairs per call";
    if (prm->reserved != 0) return "params->reserved must be 0";
    if (!std::isfinite(prm->ratio2) || !(prm->ratio2 > 0.0f)) return "ratio2 must be finite and positive";
    if (!(prm->max_desc_dist2 > 0.0f)) return "max_desc_dist2 must be positive (+inf: no bound)";
    if (epipolar_models)
        if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (homography_models && (!std::isfinite(prm->max_transfer2) || !(prm->max_transfer2 > 0.0))) return "max_transfer2 must be finite and positive";
    if (const char* why = match_check_sets(Q, T, "the points of both sets are required")) return why;
    return match_check_out(out, n_pairs, Q->cap);
}

// Grids and scratch of one valid call with n_pairs >= 1: the search has k_match_guided's tiling, one GuidedRow per row and one
// partial result per (pair, split, query row), so the plan - nsplit included - is guided_plan's, whatever the pairs' kinds.
using GuidedHfPlan = GuidedPlan;
inline GuidedHfPlan guided_hf_plan(uint32_t query_cap, uint32_t train_cap, int n_pairs) { return guided_plan(query_cap, train_cap, n_pairs); }
// Scratch of a call with both model arrays: the pairs sorted by kind, u32 [2][n_pairs], and the two counts behind them (k_guided_hf_kinds).
inline size_t guided_hf_list_elems(int n_pairs) { return 2 * (size_t)n_pairs + 2; }

}  // namespace vslam

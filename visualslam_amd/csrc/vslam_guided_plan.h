// The host arithmetic of vslam_match_guided_dev (include/vslam.h, "guided matching") that needs no HIP: the argument checks in
// the ABI's order; the grids and scratch sizes are the matcher family's (vslam_match_plan.h), all from the capacities (the counts
// and the models live on the device).  Stated once, here, so that a host program can run it under the sanitizers with extreme
// capacities (tests/guided_plan_driver.cpp).
#pragma once
#include "vslam_epipolar_plan.h"
#include "vslam_match_plan.h"

namespace vslam {

// One row of the per-row pass (k_guided_rows).  A query row: {a0, a1, a2, a0*a0 + a1*a1}; a train row: {x', y', b0*b0, b1*b1};
// NaN in every field: the row is not trusted (or, on the query side, its pair has no model).
struct __attribute__((aligned(16))) GuidedRow {
    double v[4];
};

// The message of the first failed check - the entry point puts "match_guided: " in front -, vslam_match_dev's checks in its
// order with the new ones beside their kind (null, struct_size, n_pairs, the parameters, the sets, the buffers); nullptr: the
// call is valid.
inline const char* guided_check_args(const vslam_desc_sets* Q, const vslam_desc_sets* T, const vslam_epipolar* models, int n_pairs,
                                     const vslam_guided_params* prm, const vslam_match_out* out) {
    if (!Q || !T || !out || !models || !prm) return "null argument";
    if (out->struct_size != sizeof(vslam_match_out)) return "out->struct_size is not sizeof(vslam_match_out)";
    if (n_pairs < 0 || n_pairs > 65535) return "0 .. 65535 pairs per call";
    if (prm->reserved != 0) return "params->reserved must be 0";
    if (!std::isfinite(prm->ratio2) || !(prm->ratio2 > 0.0f)) return "ratio2 must be finite and positive";
    if (!(prm->max_desc_dist2 > 0.0f)) return "max_desc_dist2 must be positive (+inf: no bound)";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = match_check_sets(Q, T, "the points of both sets are required")) return why;
    return match_check_out(out, n_pairs, Q->cap);
}

// Grids and scratch of one valid call with n_pairs >= 1: the search has the matcher's tiling, and q_elems / t_elems count the
// GuidedRows as they count the norms.
using GuidedPlan = MatchPlan;
inline GuidedPlan guided_plan(uint32_t query_cap, uint32_t train_cap, int n_pairs) { return match_plan(query_cap, train_cap, n_pairs); }

}  // namespace vslam

// The host arithmetic of vslam_pose_dev (include/vslam.h, "relative pose and triangulation") that needs no HIP: the argument
// checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated
// once, here, so that a host program can run it under the sanitizers with extreme capacities (tests/pose_plan_driver.cpp).
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int POSE_PAIR_WG = 64;  // pairs (lanes) per k_pose_candidates / k_pose_select workgroup: one wave
constexpr unsigned int POSE_REC_WG = TWOVIEW_REC_WG;  // match records (lanes) per k_pose_vote / k_pose_points workgroup

// The message of the first failed check, without the stage in front, in the order of vslam_epipolar_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* pose_check_args(const vslam_epipolar* models, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                   const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                   int n_pairs, const vslam_pose_params* prm, const vslam_pose_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_pose_out)) return "out->struct_size is not sizeof(vslam_pose_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (const char* why = check_intrinsics(*prm)) return why;
    if (const char* why = twoview_check_inputs(models && matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, poses, vslam_pose, np);
    OUT_FITS(out, candidates, vslam_pose_cand[4], np);
    // np * match_cap < 2^48: the element count cannot wrap, and the byte count is compared by division
    OUT_FITS(out, points, double[3], np * match_cap);
    OUT_FITS(out, front_bits, uint64_t, np * fwords);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a record <= 104 bytes.
struct PosePlan : TwoViewPlan {  // (rec_blocks: grid.x of k_pose_vote and k_pose_points, and of k_epi_coords)
    unsigned int pair_blocks;  // grid.x of k_pose_candidates and k_pose_select
    size_t cand_elems;         // scratch when the caller gives no candidates buffer
};

inline PosePlan pose_plan(uint32_t match_cap, int n_pairs) {
    PosePlan p{};
    static_cast<TwoViewPlan&>(p) = twoview_plan(match_cap, n_pairs);
    const size_t np = (size_t)n_pairs;
    p.pair_blocks = (unsigned int)((np + POSE_PAIR_WG - 1) / POSE_PAIR_WG);
    p.cand_elems = np * 4;
    return p;
}

}  // namespace vslam

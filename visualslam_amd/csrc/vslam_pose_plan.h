// The host arithmetic of vslam_pose_dev (include/vslam.h, "relative pose and triangulation") that needs no HIP: the argument
// checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated
// once, here, so that a host program can run it under the sanitizers with extreme capacities (tests/pose_plan_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/vslam.h"

namespace vslam {

constexpr unsigned int POSE_PAIR_WG = 64;  // pairs (lanes) per k_pose_candidates / k_pose_select workgroup: one wave
constexpr unsigned int POSE_REC_WG = 256;  // match records (lanes) per k_pose_vote / k_pose_points workgroup

// The message of the first failed check, in the order of vslam_epipolar_dev's (null, struct_size, n_pairs, the parameters, the
// inputs, the buffers); nullptr: the call is valid.
inline const char* pose_check_args(const vslam_epipolar* models, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                   const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                   int n_pairs, const vslam_pose_params* prm, const vslam_pose_out* out) {
    if (!prm || !out) return "pose: null argument";
    if (out->struct_size != sizeof(vslam_pose_out)) return "pose: out->struct_size is not sizeof(vslam_pose_out)";
    if (n_pairs < 0 || n_pairs > 65535) return "pose: 0 .. 65535 pairs per call";
    if (!std::isfinite(prm->fx) || !std::isfinite(prm->fy) || !std::isfinite(prm->cx) || !std::isfinite(prm->cy))
        return "pose: the intrinsics must be finite";
    if (!(prm->fx > 0.0) || !(prm->fy > 0.0)) return "pose: fx and fy must be positive";
    if (!models || !matches || !match_counts || !query_points || !train_points) return "pose: null input";
    if (match_cap == 0 || query_cap == 0 || train_cap == 0) return "pose: a capacity is zero";
    const size_t np = (size_t)n_pairs, fwords = ((size_t)match_cap + 63) / 64;
    if (!out->poses) return "pose: poses is required";
    if (out->poses_bytes / sizeof(vslam_pose) < np) return "pose: poses buffer too small";
    if (out->candidates && out->candidates_bytes / (4 * sizeof(vslam_pose_cand)) < np) return "pose: candidates buffer too small";
    // np * match_cap < 2^48: the element count cannot wrap, and the byte count is compared by division
    if (out->points && out->points_bytes / (3 * sizeof(double)) < np * match_cap) return "pose: points buffer too small";
    if (out->front_bits && out->front_bits_bytes / sizeof(uint64_t) < np * fwords) return "pose: front_bits buffer too small";
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a record <= 104 bytes.
struct PosePlan {
    unsigned int fwords;       // ballot words per pair
    unsigned int rec_blocks;   // POSE_REC_WG-record blocks per pair: grid.x of k_pose_vote and k_pose_points (and of k_epi_coords)
    unsigned int pair_blocks;  // grid.x of k_pose_candidates and k_pose_select
    size_t coords_elems;       // scratch: {x, y, x', y'} f64 records
    size_t cand_elems;         // scratch when the caller gives no candidates buffer
};

inline PosePlan pose_plan(uint32_t match_cap, int n_pairs) {
    PosePlan p{};
    const size_t np = (size_t)n_pairs;
    p.fwords = (unsigned int)(((size_t)match_cap + 63) / 64);
    p.rec_blocks = (unsigned int)(((size_t)match_cap + POSE_REC_WG - 1) / POSE_REC_WG);
    p.pair_blocks = (unsigned int)((np + POSE_PAIR_WG - 1) / POSE_PAIR_WG);
    p.coords_elems = np * match_cap;
    p.cand_elems = np * 4;
    return p;
}

}  // namespace vslam

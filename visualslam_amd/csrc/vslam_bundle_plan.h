// The host arithmetic of vslam_bundle_dev (include/vslam.h, "bundle adjustment") that needs no HIP: the argument checks in the
// ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once, here,
// so that a host program can run it under the sanitizers with extreme capacities (tests/bundle_plan_driver.cpp).  The tables
// are the tracks stage's (vslam_tracks_plan.h), the ordered sum and the per-pair workgroup the resection refinement's.
#pragma once
#include "vslam_resect_refine_plan.h"
#include "vslam_tracks_plan.h"

namespace vslam {

// The per-camera record of the scratch: what the sweeps carry from kernel to kernel.
struct BaCam {
    double Wcur[9], wcur[3];    // T_j as kept so far
    double Wcand[9], wcand[3];  // the candidate the second pass of a sweep evaluates
    double cost_cur, cost_before;
    unsigned int n_cur, n_before, accepted, rejected, invalid, skipped;
    int valid;     // poses[j].best >= 0
    int has_cand;  // this sweep's STEP gave a candidate
};
static_assert(sizeof(BaCam) == 240, "the header states the scratch per camera");

// The message of the first failed check, without the stage in front, in the order of vslam_tracks_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* bundle_check_args(const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                     const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain,
                                     const vslam_point* frame_points, const vslam_track* tracks_in, const vslam_track_ref* refs,
                                     const vslam_bundle_params* prm, const vslam_bundle_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_bundle_out)) return "out->struct_size is not sizeof(vslam_bundle_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->sweeps < 1 || prm->sweeps > 64) return "1 .. 64 sweeps";
    if (prm->min_views < 2) return "min_views must be at least 2";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = check_intrinsics(prm->K)) return why;
    if (const char* why = twoview_check_inputs(poses && matches && match_counts && front_bits && chain && frame_points && tracks_in && refs, match_cap,
                                               point_cap, point_cap))
        return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    // np * match_cap < 2^48: no element count wraps, and the byte counts are compared by division
    OUT_NEEDS(out, tracks, vslam_track, np * match_cap);
    OUT_NEEDS(out, cams, vslam_bundle_cam, np);
    OUT_FITS(out, point_info, vslam_bundle_point, np * match_cap);
    OUT_FITS(out, member_bits, uint64_t, np * 2 * fwords);
    // (np * match_cap * 48 < 2^54)
    const uintptr_t a = reinterpret_cast<uintptr_t>(tracks_in), b = reinterpret_cast<uintptr_t>(out->tracks), span = np * match_cap * sizeof(vslam_track);
    if (a != b && (a < b ? b - a : a - b) < span) return "tracks overlaps tracks_in without being equal to it";
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, a camera has at most 2 * match_cap < 2^33 rows - at most 2^21 blocks of 29 f64 -,
// so the block sums stay below 2^45 bytes.
struct BundlePlan {
    TracksPlan trk;            // the tables and the record grid (rec_blocks, fwords, link_pairs, prev_elems, next_elems)
    unsigned int sum_blocks;   // grid.x of k_ba_cam_pass: blocks of the ordered sum per camera, from the capacity
    unsigned int pair_blocks;  // grid.x of k_ba_cam_step
    size_t partial_elems;      // scratch: [n_pairs][sum_blocks][RR_SUMS] f64 block sums
    size_t state_elems;        // scratch: BaCam [n_pairs]
};

inline BundlePlan bundle_plan(uint32_t match_cap, uint32_t point_cap, int n_pairs) {
    BundlePlan p{};
    const size_t np = (size_t)n_pairs;
    p.trk = tracks_plan(match_cap, point_cap, n_pairs);
    p.sum_blocks = (unsigned int)((2 * (size_t)match_cap + REFIT_BLOCK - 1) / REFIT_BLOCK);
    p.pair_blocks = (unsigned int)((np + RR_PAIR_WG - 1) / RR_PAIR_WG);
    p.partial_elems = np * p.sum_blocks * RR_SUMS;
    p.state_elems = np;
    return p;
}

}  // namespace vslam

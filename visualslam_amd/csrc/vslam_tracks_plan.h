// The host arithmetic of vslam_tracks_dev (include/vslam.h, "tracks") that needs no HIP: the argument checks in the ABI's
// order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once, here, so
// that a host program can run it under the sanitizers with extreme capacities (tests/tracks_plan_driver.cpp).
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int TRK_REC_WG = TWOVIEW_REC_WG;  // match records (lanes) per k_trk_next / k_trk_walk / k_trk_rows workgroup

// The message of the first failed check, without the stage in front, in the order of vslam_chain_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* tracks_check_args(const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                     const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain,
                                     const vslam_point* frame_points, const vslam_tracks_params* prm, const vslam_tracks_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_tracks_out)) return "out->struct_size is not sizeof(vslam_tracks_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (const char* why = check_intrinsics(prm->K)) return why;
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (prm->min_views < 2) return "min_views must be at least 2";
    if (const char* why = twoview_check_inputs(poses && matches && match_counts && front_bits && chain && frame_points, match_cap, point_cap, point_cap))
        return why;
    const size_t np = (size_t)n_pairs;
    // np * match_cap < 2^48: the element count cannot wrap, and the byte count is compared by division
    OUT_NEEDS(out, tracks, vslam_track, np * match_cap);
    OUT_FITS(out, refs, vslam_track_ref, np * match_cap);
    OUT_FITS(out, good_bits, uint64_t, np * twoview_fwords(match_cap));
    OUT_FITS(out, summary, vslam_track_summary, np);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, an element 4 bytes.
struct TracksPlan {
    unsigned int fwords;      // ballot words per pair of front_bits and good_bits
    unsigned int rec_blocks;  // grid.x of k_trk_next, k_trk_walk and k_trk_rows
    unsigned int link_pairs;  // n_pairs - 1: grid.y of k_chain_link and k_trk_next (0: neither is launched)
    size_t prev_elems;        // scratch: the link table, uint32 [link_pairs][point_cap]
    size_t next_elems;        // scratch: the continuation table, uint32 [link_pairs][match_cap]
    size_t frame_elems;       // the records of frame_points: (n_pairs + 1) * point_cap
};

inline TracksPlan tracks_plan(uint32_t match_cap, uint32_t point_cap, int n_pairs) {
    const TwoViewPlan tv = twoview_plan(match_cap, n_pairs);
    TracksPlan p{};
    p.fwords = tv.fwords, p.rec_blocks = tv.rec_blocks;
    const LinkTable lt = link_table(point_cap, n_pairs);
    p.link_pairs = lt.link_pairs, p.prev_elems = lt.elems;
    p.next_elems = (size_t)p.link_pairs * match_cap;
    p.frame_elems = ((size_t)n_pairs + 1) * point_cap;
    return p;
}

}  // namespace vslam

// The host arithmetic of vslam_match_mutual_dev (include/vslam.h, "mutual matching") that needs no HIP: the argument checks in
// the ABI's order, and the matcher family's grids and scratch sizes (vslam_match_plan.h) with the reverse table beside them, all
// from the capacities (the counts live on the device).  Stated once, here, so that a host program can run it under the
// sanitizers with extreme capacities (tests/mutual_plan_driver.cpp).
#pragma once
#include "vslam_match_plan.h"

namespace vslam {

// The message of the first failed check - the entry point puts "match_mutual: " in front -, vslam_match_dev's checks in its
// order with the rnn buffer beside the nn buffer; nullptr: the call is valid.
inline const char* mutual_check_args(const vslam_desc_sets* Q, const vslam_desc_sets* T, int n_pairs, float ratio2, int same_octave,
                                     const vslam_match_mutual_out* out) {
    if (!Q || !T || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_match_mutual_out)) return "out->struct_size is not sizeof(vslam_match_mutual_out)";
    if (n_pairs < 0 || n_pairs > 65535) return "0 .. 65535 pairs per call";
    if (!std::isfinite(ratio2) || !(ratio2 > 0.0f)) return "ratio2 must be finite and positive";
    if (const char* why = match_check_sets(Q, T, same_octave ? "same_octave needs the points of both sets" : nullptr)) return why;
    const bool rnn_small = out->rnn && out->rnn_bytes / sizeof(vslam_rnn) < (size_t)n_pairs * T->cap;
    return match_check_out(out, n_pairs, Q->cap, out->rnn != nullptr, rnn_small ? "rnn buffer too small" : nullptr);
}

// Grids and scratch of one valid call with n_pairs >= 1: the matcher's, and the reverse table (8-byte records: no size wraps).
struct MutualPlan : MatchPlan {
    size_t rev_elems, rev_bytes;  // scratch: the reverse table, one 64-bit (key, query) word per (pair, train row)
};

inline MutualPlan mutual_plan(uint32_t query_cap, uint32_t train_cap, int n_pairs) {
    const MatchPlan m = match_plan(query_cap, train_cap, n_pairs);
    return {m, m.t_elems, m.t_elems * 8};
}

}  // namespace vslam

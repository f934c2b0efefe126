// The host arithmetic of vslam_match_mutual_dev (include/vslam.h, "mutual matching") that needs no HIP: the argument checks in
// the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once,
// here, so that a host program can run it under the sanitizers with extreme capacities (tests/mutual_plan_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/vslam.h"

namespace vslam {

// The tiling of the search is k_match_nn2's (kernels_match.hip.h; vslam_match_mutual.hip asserts that the two agree).
constexpr unsigned int MUTUAL_Q = 128;         // query rows per workgroup
constexpr unsigned int MUTUAL_T = 64;          // train rows per LDS tile, and per 64-lane atomic of the reverse table
constexpr unsigned int MUTUAL_MAX_SPLIT = 16;  // workgroups that share the train tiles of one query tile
constexpr size_t MUTUAL_WANT_WGS = 2048;       // 8 workgroups per compute unit
constexpr unsigned int MUTUAL_ROW_WG = 256;    // rows (lanes) per workgroup of the per-row kernels

// The message of the first failed check - the entry point puts "match_mutual: " in front -, vslam_match_dev's checks in its
// order with the rnn buffer beside the nn buffer; nullptr: the call is valid.
inline const char* mutual_check_args(const vslam_desc_sets* Q, const vslam_desc_sets* T, int n_pairs, float ratio2, int same_octave,
                                     const vslam_match_mutual_out* out) {
    if (!Q || !T || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_match_mutual_out)) return "out->struct_size is not sizeof(vslam_match_mutual_out)";
    if (n_pairs < 0 || n_pairs > 65535) return "0 .. 65535 pairs per call";
    if (!std::isfinite(ratio2) || !(ratio2 > 0.0f)) return "ratio2 must be finite and positive";
    for (const vslam_desc_sets* s : {Q, T}) {
        if (!s->desc || !s->counts || s->cap == 0) return "a descriptor set needs desc, counts and a capacity";
        if ((reinterpret_cast<uintptr_t>(s->desc) & 15) != 0) return "desc must be 16-byte aligned";
        if (same_octave && !s->points) return "same_octave needs the points of both sets";
    }
    const size_t np = (size_t)n_pairs;
    if (!out->nn && !out->rnn && !out->match_counts) return "no output requested";
    if (out->nn && out->nn_bytes / sizeof(vslam_nn2) < np * Q->cap) return "nn buffer too small";
    if (out->rnn && out->rnn_bytes / sizeof(vslam_rnn) < np * T->cap) return "rnn buffer too small";
    if (out->matches && (!out->match_counts || out->match_cap == 0)) return "matches needs match_counts and a match_cap";
    if (out->matches && out->matches_bytes / sizeof(vslam_match) < np * out->match_cap) return "matches buffer too small";
    if (out->match_counts && out->match_counts_bytes / sizeof(uint32_t) < np) return "match_counts buffer too small";
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a scratch record <= 12 bytes, nsplit <= 16.
struct MutualPlan {
    unsigned int qtiles;                    // grid.x of k_match_nn2_mutual: MUTUAL_Q-row query tiles
    unsigned int ttiles;                    // MUTUAL_T-row train tiles per pair
    unsigned int nsplit;                    // grid.y of k_match_nn2_mutual: the train tiles are dealt round robin to nsplit workgroups
    unsigned int fwords;                    // accepted-query ballot words per pair
    unsigned int qrow_blocks, trow_blocks;  // grid.x of the per-row kernels over the query / train capacity
    size_t q_elems, t_elems;                // scratch: one f32 norm per query / train row
    size_t part_elems;                      // scratch: one partial result per (pair, split, query row)
    size_t flag_words;                      // scratch: ballot words of all pairs
    size_t rev_elems, rev_bytes;            // scratch: the reverse table, one 64-bit (key, query) word per (pair, train row)
};

inline MutualPlan mutual_plan(uint32_t query_cap, uint32_t train_cap, int n_pairs) {
    MutualPlan p{};
    const size_t np = (size_t)n_pairs, qc = query_cap, tc = train_cap;
    p.qtiles = (unsigned int)((qc + MUTUAL_Q - 1) / MUTUAL_Q);
    p.ttiles = (unsigned int)((tc + MUTUAL_T - 1) / MUTUAL_T);
    const size_t wgs = (size_t)p.qtiles * np;
    size_t split = (MUTUAL_WANT_WGS + wgs - 1) / wgs;
    if (split > MUTUAL_MAX_SPLIT) split = MUTUAL_MAX_SPLIT;
    if (split > p.ttiles) split = p.ttiles;
    p.nsplit = (unsigned int)(split < 1 ? 1 : split);
    p.fwords = (unsigned int)((qc + 63) / 64);
    p.qrow_blocks = (unsigned int)((qc + MUTUAL_ROW_WG - 1) / MUTUAL_ROW_WG);
    p.trow_blocks = (unsigned int)((tc + MUTUAL_ROW_WG - 1) / MUTUAL_ROW_WG);
    p.q_elems = np * qc;
    p.t_elems = np * tc;
    p.part_elems = np * p.nsplit * qc;
    p.flag_words = np * p.fwords;
    p.rev_elems = np * tc;
    p.rev_bytes = p.rev_elems * 8;
    return p;
}

}  // namespace vslam

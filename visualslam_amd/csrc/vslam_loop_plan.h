// The host arithmetic of the loop verification entry points (vslam_loop_pairs_dev, vslam_match_pairs_dev / vslam_match_pairs_host,
// vslam_pair_points_dev, vslam_loop_verdict_dev / vslam_loop_verdict_host; include/vslam.h) that needs no HIP: the argument checks,
// in the order the entry points answer them and with their messages, and every grid and scratch size.  The indexed search is
// tiled by the matcher's plan (vslam_match_plan.h) with the table's slots as the pairs; the norms are sized by the SETS.  No size
// wraps for 65535 slots, 65535 sets and capacities up to 2^32 - 1: everything is formed in size_t (64 bits), the largest product is
// 65535 slots * 16 splits * 2^32 rows * 12 bytes < 2^60.  A host program runs all of it under the sanitizers
// (tests/loop_plan_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/vslam.h"
#include "vslam_match_plan.h"

namespace vslam {

constexpr uint32_t LP_MAX_SETS = 65535;    // sets on either side, slots of one table, frames of one verdict
constexpr uint32_t LP_MAX_C = 8;           // slots per query frame (vslam_place_dev's max_candidates)
constexpr unsigned int LP_WG = 256;        // lanes of the per-slot, per-record and verdict workgroups

// The one rule of the pair table, for the kernels and for the host alike: slot `pr` names no pair of sets
#ifdef __HIPCC__
#define LP_HOST_DEVICE __host__ __device__
#else
#define LP_HOST_DEVICE
#endif
LP_HOST_DEVICE inline bool pair_empty(const vslam_set_pair pr, uint32_t n_query_sets, uint32_t n_train_sets) {
    return (uint32_t)pr.query_set >= n_query_sets || (uint32_t)pr.train_set >= n_train_sets;
}

// ---- grids and scratch

struct LoopPairsPlan {
    unsigned int blocks;  // grid.x of k_loop_pairs: one lane per slot
    size_t slots;         // nq * c
};
inline LoopPairsPlan loop_pairs_plan(uint32_t nq, uint32_t c) {
    LoopPairsPlan p{};
    p.slots = (size_t)nq * c;
    p.blocks = (unsigned int)((p.slots + LP_WG - 1) / LP_WG);
    return p;
}

struct MatchPairsPlan {
    MatchPlan m;                      // the search, the merge and the list: query / train capacity, pairs = the table's slots
    size_t qnorm_elems, tnorm_elems;  // scratch: one f32 norm per row of every SET
};
inline MatchPairsPlan match_pairs_plan(uint32_t query_cap, int n_query_sets, uint32_t train_cap, int n_train_sets, int n_pairs) {
    MatchPairsPlan p{};
    p.m = match_plan(query_cap, train_cap, n_pairs);
    p.qnorm_elems = (size_t)n_query_sets * query_cap;
    p.tnorm_elems = (size_t)n_train_sets * train_cap;
    return p;
}

struct PairPointsPlan {
    unsigned int row_blocks;  // grid.x of k_pair_points over match_cap, LP_WG records per workgroup; grid.y = n_pairs
    size_t records;           // n_pairs * match_cap
};
inline PairPointsPlan pair_points_plan(uint32_t match_cap, int n_pairs) {
    PairPointsPlan p{};
    p.row_blocks = (unsigned int)(((size_t)match_cap + LP_WG - 1) / LP_WG);
    p.records = (size_t)n_pairs * match_cap;
    return p;
}

// ---- checks: nullptr, or the message of the first one that fails

inline const char* loop_pairs_check(const vslam_place_cand* candidates, const uint32_t* cand_counts, uint32_t nq, uint32_t c, uint32_t nd,
                                    const vslam_set_pair* pairs, size_t pairs_bytes) {
    if (!candidates || !cand_counts || !pairs) return "null argument";
    if (nq > LP_MAX_SETS || nd > LP_MAX_SETS) return "at most 65535 frames on either side";
    if (c < 1 || c > LP_MAX_C) return "c must be 1 .. 8";
    if (pairs_bytes / sizeof(vslam_set_pair) < loop_pairs_plan(nq, c).slots) return "pairs buffer too small";
    return nullptr;
}

// device: the pointers are device pointers, whose alignment the kernels rely on
inline const char* match_pairs_check(const vslam_desc_sets* Q, int n_query_sets, const vslam_desc_sets* T, int n_train_sets,
                                     const vslam_set_pair* pairs, int n_pairs, float ratio2, int same_octave, const vslam_match_out* out, bool device) {
    if (!Q || !T || !pairs || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_match_out)) return "out->struct_size is not sizeof(vslam_match_out)";
    if (n_pairs < 0 || n_pairs > (int)LP_MAX_SETS) return "0 .. 65535 pairs per call";
    if (n_query_sets < 0 || n_query_sets > (int)LP_MAX_SETS || n_train_sets < 0 || n_train_sets > (int)LP_MAX_SETS) return "0 .. 65535 sets on either side";
    if (!(std::isfinite(ratio2) && ratio2 > 0.0f)) return "ratio2 must be finite and positive";
    for (const vslam_desc_sets* s : {Q, T}) {
        if (!s->desc || !s->counts || s->cap == 0) return "a descriptor set needs desc, counts and a capacity";
        if (device && (reinterpret_cast<uintptr_t>(s->desc) & 15) != 0) return "desc must be 16-byte aligned";
        if (same_octave && !s->points) return "same_octave needs the points of both sets";
    }
    return match_check_out(out, n_pairs, Q->cap);
}

inline const char* pair_points_check(const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap, const vslam_set_pair* pairs, int n_pairs,
                                     const vslam_point* query_points, uint32_t query_cap, int n_query_sets, const vslam_point* train_points,
                                     uint32_t train_cap, int n_train_sets, const vslam_point* qout, size_t qout_bytes, const vslam_point* tout,
                                     size_t tout_bytes, const vslam_match* local, size_t local_bytes) {
    if (!matches || !match_counts || !pairs || !query_points || !train_points || !qout || !tout || !local) return "null argument";
    if (n_pairs < 0 || n_pairs > (int)LP_MAX_SETS) return "0 .. 65535 pairs per call";
    if (n_query_sets < 0 || n_query_sets > (int)LP_MAX_SETS || n_train_sets < 0 || n_train_sets > (int)LP_MAX_SETS) return "0 .. 65535 sets on either side";
    if (match_cap == 0 || query_cap == 0 || train_cap == 0) return "match_cap, query_cap and train_cap must be positive";
    const size_t records = pair_points_plan(match_cap, n_pairs).records;
    if (qout_bytes / sizeof(vslam_point) < records) return "query_points_out buffer too small";
    if (tout_bytes / sizeof(vslam_point) < records) return "train_points_out buffer too small";
    if (local_bytes / sizeof(vslam_match) < records) return "local buffer too small";
    return nullptr;
}

inline const char* loop_verdict_check(const vslam_epipolar* models, const vslam_set_pair* pairs, uint32_t nq, uint32_t c, uint32_t n_train_sets,
                                      const vslam_loop_params* params, const vslam_loop_out* out) {
    if (!models || !pairs || !params || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_loop_out)) return "out->struct_size is not sizeof(vslam_loop_out)";
    if (nq > LP_MAX_SETS || n_train_sets > LP_MAX_SETS) return "at most 65535 frames on either side";
    if (c < 1 || c > LP_MAX_C) return "c must be 1 .. 8";
    if (params->min_inliers == 0) return "min_inliers must be positive";
    if (params->den == 0) return "den must be positive";
    if (params->reserved != 0) return "params->reserved must be 0";
    if (!out->loops && !out->loop_list && !out->n_loops) return "no output requested";
    if (out->loop_list && !out->n_loops) return "loop_list needs n_loops";
    if (out->loops && out->loops_bytes / sizeof(vslam_loop) < nq) return "loops buffer too small";
    if (out->loop_list && out->loop_list_bytes / sizeof(int32_t) < nq) return "loop_list buffer too small";
    if (out->n_loops && out->n_loops_bytes / sizeof(uint32_t) < 1) return "n_loops buffer too small";
    return nullptr;
}

}  // namespace vslam

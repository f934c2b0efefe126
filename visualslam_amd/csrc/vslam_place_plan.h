// The host arithmetic of the place recognition entry points (vslam_vocab_sample_dev, vslam_words_dev / vslam_words_host,
// vslam_place_dev / vslam_place_host; include/vslam.h) that needs no HIP: the argument checks, in the order the entry points
// answer them and with their messages, and every grid and scratch size.  The word search is tiled by the matcher's plan
// (vslam_match_plan.h) with the K vocabulary rows as the train capacity and the sets as the pairs.  No size wraps for K = 65536,
// 65535 sets and capacities up to 2^32 - 1: everything is formed in size_t (64 bits), the largest product is
// 65535 sets * 16 splits * 2^32 rows * 8 bytes < 2^59.  A host program runs all of it under the sanitizers
// (tests/place_plan_driver.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vslam.h"
#include "vslam_match_plan.h"

namespace vslam {

constexpr uint32_t PL_MAX_K = 65536;       // words of a vocabulary
constexpr uint32_t PL_MAX_FRAMES = 65535;  // sets of one words call, frames on either side of one place call
constexpr unsigned int PL_TILE = 16;       // k_place_score: a workgroup owns PL_TILE x PL_TILE (query, db) frames
constexpr unsigned int PL_KC = 128;        // ... and streams K through LDS in chunks of PL_KC words
constexpr unsigned int PL_MAX_C = 8;       // candidates kept per query frame
constexpr unsigned int PL_GATHER_WG = 8;   // k_vocab_gather: words per 256-lane workgroup (32 lanes x 16 bytes = one row)

// ---- grids and scratch

struct VocabPlan {
    unsigned int gather_blocks;  // grid.x of k_vocab_gather
    size_t vocab_bytes, defined_bytes;
};
inline VocabPlan vocab_plan(uint32_t K) {
    VocabPlan p{};
    p.gather_blocks = (K + PL_GATHER_WG - 1) / PL_GATHER_WG;
    p.vocab_bytes = (size_t)K * 128 * sizeof(float);
    p.defined_bytes = K;
    return p;
}

struct WordsPlan {
    MatchPlan m;          // the search: query capacity = the sets' cap, train capacity = K, pairs = n_sets
    size_t row_elems;     // one word / one distance per (set, row)
    size_t hist_elems;    // n_sets * K
    size_t vnorm_elems;   // K
    size_t part_bytes;    // scratch of the partial results: 8 bytes per (set, split, row)
};
inline WordsPlan words_plan(uint32_t cap, uint32_t K, int n_sets) {
    WordsPlan p{};
    p.m = match_plan(cap, K, n_sets);
    p.row_elems = (size_t)n_sets * cap;
    p.hist_elems = (size_t)n_sets * K;
    p.vnorm_elems = K;
    p.part_bytes = p.m.part_elems * 8;
    return p;
}

struct PlacePlan {
    unsigned int df_blocks;         // grid.x of k_place_df: 256 words per workgroup
    unsigned int self_blocks;       // grid.x of k_place_self: one wave per frame, the query frames and then the db frames
    unsigned int tiles_q, tiles_d;  // grid.y, grid.x of k_place_score
    unsigned int top_blocks;        // grid.x of k_place_top: one wave per query frame
    size_t score_elems;             // nq * nd
};
inline PlacePlan place_plan(uint32_t nq, uint32_t nd, uint32_t K) {
    PlacePlan p{};
    p.df_blocks = (K + 255) / 256;
    p.self_blocks = nq + nd;
    p.tiles_q = (nq + PL_TILE - 1) / PL_TILE;
    p.tiles_d = (nd + PL_TILE - 1) / PL_TILE;
    p.top_blocks = nq;
    p.score_elems = (size_t)nq * nd;
    return p;
}

// ---- checks: nullptr, or the message of the first one that fails

inline const char* place_check_set(const vslam_desc_sets* s, bool device) {
    if (!s->desc || !s->counts || s->cap == 0) return "a descriptor set needs desc, counts and a capacity";
    if (device && (reinterpret_cast<uintptr_t>(s->desc) & 15) != 0) return "desc must be 16-byte aligned";
    return nullptr;
}

inline const char* vocab_sample_check(const vslam_desc_sets* sets, int n_sets, uint32_t K, const float* vocab, size_t vocab_bytes,
                                      const uint8_t* vocab_defined, size_t vocab_defined_bytes) {
    if (!sets || !vocab || !vocab_defined) return "null argument";
    if (n_sets < 1 || n_sets > (int)PL_MAX_FRAMES) return "1 .. 65535 sets per call";
    if (K < 1 || K > PL_MAX_K) return "1 .. 65536 words";
    if (const char* why = place_check_set(sets, true)) return why;
    if ((reinterpret_cast<uintptr_t>(vocab) & 15) != 0) return "vocab must be 16-byte aligned";
    const VocabPlan p = vocab_plan(K);
    if (vocab_bytes < p.vocab_bytes) return "vocab buffer too small";
    if (vocab_defined_bytes < p.defined_bytes) return "vocab_defined buffer too small";
    return nullptr;
}

// device: the pointers are device pointers, whose alignment the kernels rely on
inline const char* words_check(const vslam_desc_sets* sets, int n_sets, const float* vocab, uint32_t K, const vslam_words_out* out, bool device) {
    if (!sets || !vocab || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_words_out)) return "out->struct_size is not sizeof(vslam_words_out)";
    if (n_sets < 0 || n_sets > (int)PL_MAX_FRAMES) return "0 .. 65535 sets per call";
    if (K < 1 || K > PL_MAX_K) return "1 .. 65536 words";
    if (const char* why = place_check_set(sets, device)) return why;
    if (device && (reinterpret_cast<uintptr_t>(vocab) & 15) != 0) return "vocab must be 16-byte aligned";
    if (!out->words && !out->word_dist2 && !out->hist) return "no output requested";
    const size_t rows = (size_t)n_sets * sets->cap;
    if (out->words && out->words_bytes / sizeof(int32_t) < rows) return "words buffer too small";
    if (out->word_dist2 && out->word_dist2_bytes / sizeof(float) < rows) return "word_dist2 buffer too small";
    if (out->hist && out->hist_bytes / sizeof(uint32_t) < (size_t)n_sets * K) return "hist buffer too small";
    return nullptr;
}

inline const char* place_check(const uint32_t* hist_q, uint32_t nq, uint32_t q_first, const uint32_t* hist_db, uint32_t nd, uint32_t db_first,
                               uint32_t K, const vslam_place_params* params, const vslam_place_out* out) {
    if (!params || !out || (!hist_q && nq) || (!hist_db && nd)) return "null argument";
    if (out->struct_size != sizeof(vslam_place_out)) return "out->struct_size is not sizeof(vslam_place_out)";
    if (nq > PL_MAX_FRAMES || nd > PL_MAX_FRAMES) return "at most 65535 frames on either side";
    if (K < 1 || K > PL_MAX_K) return "1 .. 65536 words";
    if ((uint64_t)q_first + nq > (1ull << 31) || (uint64_t)db_first + nd > (1ull << 31)) return "a frame id does not fit 31 bits";
    if (params->max_candidates < 1 || params->max_candidates > PL_MAX_C) return "max_candidates must be 1 .. 8";
    if (params->den == 0) return "den must be positive";
    if (params->reserved != 0) return "params->reserved must be 0";
    if (!out->candidates && !out->cand_counts && !out->weights && !out->self_q && !out->self_db && !out->scores) return "no output requested";
    if (out->candidates && !out->cand_counts) return "candidates needs cand_counts";
    if (out->candidates && out->candidates_bytes / sizeof(vslam_place_cand) < (size_t)nq * params->max_candidates) return "candidates buffer too small";
    if (out->cand_counts && out->cand_counts_bytes / sizeof(uint32_t) < nq) return "cand_counts buffer too small";
    if (out->weights && out->weights_bytes / sizeof(uint32_t) < K) return "weights buffer too small";
    if (out->self_q && out->self_q_bytes / sizeof(uint32_t) < nq) return "self_q buffer too small";
    if (out->self_db && out->self_db_bytes / sizeof(uint32_t) < nd) return "self_db buffer too small";
    if (out->scores && out->scores_bytes / sizeof(uint32_t) < (size_t)nq * nd) return "scores buffer too small";
    return nullptr;
}

}  // namespace vslam

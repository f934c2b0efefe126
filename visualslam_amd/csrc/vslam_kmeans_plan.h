// The host arithmetic of vocabulary training (vslam_vocab_kmeans_dev / vslam_vocab_kmeans_host; include/vslam.h, "vocabulary
// training") that needs no HIP: the argument checks, in the order the entry points answer them and with their messages, and every
// grid and scratch size.  The assignment step is the word search, tiled by words_plan (vslam_place_plan.h).  No size wraps: the
// row ids are checked to fit 32 bits, so rows < 2^32, and everything else is formed in size_t (64 bits); the largest product is
// (2^24 + 2^16) blocks * 1 KiB < 2^35.  A host program runs all of it under the sanitizers (tests/kmeans_plan_driver.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/vslam.h"
#include "vslam_place_plan.h"

namespace vslam {

constexpr uint32_t KM_MAX_ROUNDS = 64;
constexpr unsigned int KM_BLOCK = 256;  // members of one block of the ordered sum (the header's rule, not a tuning knob)
constexpr unsigned int KM_CHUNK = 256;  // k_kmeans_members: rows of a set ranked at once by its workgroup
constexpr unsigned int KM_WAVES = 4;    // k_kmeans_block_sums: waves (= blocks of the sum) per workgroup

struct KmeansPlan {
    WordsPlan w;                 // the assignment: the word search of n_sets sets of `cap` rows against K words
    size_t rows;                 // n_sets * cap: one word of this round, one of the last, one member slot per row
    size_t max_blocks;           // rows / 256 + K >= the blocks of all words, whatever the assignment
    size_t bsum_elems;           // max_blocks * 128 f64
    unsigned int init_blocks;    // grid.x of k_kmeans_init: 256 sets per workgroup
    unsigned int count_blocks;   // grid.x of k_kmeans_count (grid.y = n_sets): 256 rows per workgroup
    unsigned int column_blocks;  // grid.x of k_kmeans_columns: 256 words per workgroup
    unsigned int sum_blocks;     // grid.x of k_kmeans_block_sums: KM_WAVES blocks of the sum per workgroup
    size_t vocab_bytes, sizes_bytes, report_bytes;
};
inline KmeansPlan kmeans_plan(uint32_t cap, uint32_t K, int n_sets, uint32_t rounds) {
    KmeansPlan p{};
    if (n_sets > 0) p.w = words_plan(cap, K, n_sets);  // (no sets: no search to tile; the output sizes below are still asked for)
    p.rows = (size_t)n_sets * cap;
    p.max_blocks = p.rows / KM_BLOCK + K;
    p.bsum_elems = p.max_blocks * 128;
    p.init_blocks = (unsigned int)(((size_t)n_sets + 255) / 256);
    p.count_blocks = (unsigned int)(((size_t)cap + 255) / 256);
    p.column_blocks = (K + 255) / 256;
    p.sum_blocks = (unsigned int)((p.max_blocks + KM_WAVES - 1) / KM_WAVES);
    p.vocab_bytes = (size_t)K * 128 * sizeof(float);
    p.sizes_bytes = (size_t)K * sizeof(uint32_t);
    p.report_bytes = (size_t)rounds * sizeof(vslam_kmeans_round);
    return p;
}

// nullptr, or the message of the first check that fails.  device: the pointers are device pointers, whose alignment the kernels
// rely on.
inline const char* kmeans_check(const vslam_desc_sets* sets, int n_sets, const float* vocab_in, uint32_t K, const vslam_kmeans_params* params,
                                const vslam_kmeans_out* out, bool device) {
    static_assert(sizeof(vslam_kmeans_round) == 16 && sizeof(vslam_kmeans_params) == 8, "record layout");
    if (!sets || !vocab_in || !params || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_kmeans_out)) return "out->struct_size is not sizeof(vslam_kmeans_out)";
    if (params->rounds < 1 || params->rounds > KM_MAX_ROUNDS) return "rounds must be 1 .. 64";
    if (params->reserved != 0) return "params->reserved must be 0";
    if (n_sets < 0 || n_sets > (int)PL_MAX_FRAMES) return "0 .. 65535 sets per call";
    if (K < 1 || K > PL_MAX_K) return "1 .. 65536 words";
    if (const char* why = place_check_set(sets, device)) return why;
    if ((uint64_t)n_sets * sets->cap > 0xffffffffull) return "n_sets * cap must fit 32 bits";
    if (device && (reinterpret_cast<uintptr_t>(vocab_in) & 15) != 0) return "vocab_in must be 16-byte aligned";
    if (!out->vocab) return "out->vocab is required";
    if (device && (reinterpret_cast<uintptr_t>(out->vocab) & 15) != 0) return "vocab must be 16-byte aligned";
    const KmeansPlan p = kmeans_plan(sets->cap, K, n_sets, params->rounds);
    if (out->vocab_bytes < p.vocab_bytes) return "vocab buffer too small";
    if (out->sizes && out->sizes_bytes < p.sizes_bytes) return "sizes buffer too small";
    if (out->report && out->report_bytes < p.report_bytes) return "report buffer too small";
    const uintptr_t a = reinterpret_cast<uintptr_t>(vocab_in), b = reinterpret_cast<uintptr_t>(out->vocab);
    if (a != b && a < b + p.vocab_bytes && b < a + p.vocab_bytes) return "vocab overlaps vocab_in without being vocab_in";
    return nullptr;
}

}  // namespace vslam

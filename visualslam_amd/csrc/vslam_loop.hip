// The integer stages of loop verification of the C ABI (include/vslam.h, "loop verification"): argument checks
// (vslam_loop_plan.h) and launches of kernels_loop.hip.h.  No scratch: every kernel reads its inputs and writes its outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_loop.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_loop_plan.h"

using namespace vslam;

extern "C" {

int vslam_loop_pairs_dev(vslam_ctx* c, const vslam_place_cand* candidates, const uint32_t* cand_counts, uint32_t nq, uint32_t cc, uint32_t db_first,
                         uint32_t nd, vslam_set_pair* pairs, size_t pairs_bytes) {
    static_assert(sizeof(vslam_set_pair) == 8 && sizeof(vslam_loop_params) == 16 && sizeof(vslam_loop) == 20, "record layouts");
    if (const char* why = loop_pairs_check(candidates, cand_counts, nq, cc, nd, pairs, pairs_bytes))
        return fail(c, VSLAM_ERR_INVALID, std::string("loop_pairs: ") + why);
    TRY(usable_ctx(c));
    if (nq == 0) return VSLAM_OK;
    const LoopPairsPlan pl = loop_pairs_plan(nq, cc);
    LAUNCH(c, "k_loop_pairs", k_loop_pairs, dim3(pl.blocks), dim3(LP_WG), candidates, cand_counts, nq, cc, db_first, nd, pairs);
    return VSLAM_OK;
}

int vslam_pair_points_dev(vslam_ctx* c, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap, const vslam_set_pair* pairs,
                          int n_pairs, const vslam_point* query_points, uint32_t query_cap, int n_query_sets, const vslam_point* train_points,
                          uint32_t train_cap, int n_train_sets, vslam_point* query_points_out, size_t query_points_out_bytes,
                          vslam_point* train_points_out, size_t train_points_out_bytes, vslam_match* local, size_t local_bytes) {
    if (const char* why = pair_points_check(matches, match_counts, match_cap, pairs, n_pairs, query_points, query_cap, n_query_sets, train_points, train_cap,
                                            n_train_sets, query_points_out, query_points_out_bytes, train_points_out, train_points_out_bytes, local, local_bytes))
        return fail(c, VSLAM_ERR_INVALID, std::string("pair_points: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;
    const PairPointsPlan pl = pair_points_plan(match_cap, n_pairs);
    LAUNCH(c, "k_pair_points", k_pair_points, dim3(pl.row_blocks, n_pairs), dim3(LP_WG), matches, match_counts, match_cap, pairs,
           (unsigned int)n_query_sets, (unsigned int)n_train_sets, query_points, query_cap, train_points, train_cap, query_points_out, train_points_out,
           local);
    return VSLAM_OK;
}

int vslam_loop_verdict_dev(vslam_ctx* c, const vslam_epipolar* models, const vslam_set_pair* pairs, uint32_t nq, uint32_t cc, uint32_t n_train_sets,
                           const vslam_loop_params* params, const vslam_loop_out* out) {
    if (const char* why = loop_verdict_check(models, pairs, nq, cc, n_train_sets, params, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("loop_verdict: ") + why);
    TRY(usable_ctx(c));
    LAUNCH(c, "k_loop_verdict", k_loop_verdict, dim3(1), dim3(LP_WG), models, pairs, nq, cc, n_train_sets, *params, out->loops, out->loop_list, out->n_loops);
    return VSLAM_OK;
}

int vslam_loop_verdict_host(vslam_ctx* c, const vslam_epipolar* models, const vslam_set_pair* pairs, uint32_t nq, uint32_t cc, uint32_t n_train_sets,
                            const vslam_loop_params* params, const vslam_loop_out* out) {
    if (const char* why = loop_verdict_check(models, pairs, nq, cc, n_train_sets, params, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("loop_verdict_host: ") + why);
    TRY(usable_ctx(c));
    HostMirror hm(c);
    const size_t slots = (size_t)nq * cc;
    const vslam_epipolar* d_models = hm.in(models, slots);
    const vslam_set_pair* d_pairs = hm.in(pairs, slots);
    vslam_loop_out o{};
    o.struct_size = sizeof(o);
    hm.out(o.loops, o.loops_bytes, out->loops, (size_t)nq, false);
    hm.out(o.loop_list, o.loop_list_bytes, out->loop_list, (size_t)nq, true);
    hm.out(o.n_loops, o.n_loops_bytes, out->n_loops, (size_t)1, false);
    TRY(hm.status());
    TRY(vslam_loop_verdict_dev(c, d_models, d_pairs, nq, cc, n_train_sets, params, &o));
    return hm.finish();
}

}  // extern "C"

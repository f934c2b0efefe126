// The indexed matcher of the C ABI (include/vslam.h, "loop verification"): argument checks (vslam_loop_plan.h), scratch and
// launches of kernels_match_pairs.hip.h.  The norms are k_desc_norms over the SETS, once per set; the match list is the
// matcher's count -> scan -> scatter over the pairs' flag words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match_pairs.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_loop_plan.h"

using namespace vslam;

namespace {
// one buffer on both sides: its norms are computed once
bool same_sets(const vslam_desc_sets& a, int na, const vslam_desc_sets& b, int nb) {
    return a.desc == b.desc && a.counts == b.counts && a.cap == b.cap && na == nb;
}
}  // namespace

extern "C" {

int vslam_match_pairs_dev(vslam_ctx* c, const vslam_desc_sets* Q, int n_query_sets, const vslam_desc_sets* T, int n_train_sets,
                          const vslam_set_pair* pairs, int n_pairs, float ratio2, int same_octave, const vslam_match_out* out) {
    static_assert(sizeof(vslam_set_pair) == 8 && sizeof(MatchPart) == 12, "record layouts");
    if (const char* why = match_pairs_check(Q, n_query_sets, T, n_train_sets, pairs, n_pairs, ratio2, same_octave, out, true))
        return fail(c, VSLAM_ERR_INVALID, std::string("match_pairs: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const MatchPairsPlan pl = match_pairs_plan(Q->cap, n_query_sets, T->cap, n_train_sets, n_pairs);  // (grids from the capacities)
    const bool one = same_sets(*Q, n_query_sets, *T, n_train_sets);
    float *qnorm = nullptr, *tnorm = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long* flags = nullptr;
    unsigned int* chunk_ws = nullptr;
    WsPlan ws;
    ws.add(qnorm, pl.qnorm_elems);
    if (!one) ws.add(tnorm, pl.tnorm_elems);
    ws.add(part, pl.m.part_elems);
    if (!out->nn) ws.add(nn_ws, pl.m.q_elems);
    ws.add(flags, pl.m.flag_words);
    ws.add(chunk_ws, match_list_ws_elems(pl.m.fwords, n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;
    if (one) tnorm = qnorm;

    if (n_query_sets > 0) TRY(enqueue_desc_norms(c, *Q, n_query_sets, qnorm));
    if (!one && n_train_sets > 0) TRY(enqueue_desc_norms(c, *T, n_train_sets, tnorm));
    const dim3 grid(pl.m.qtiles, pl.m.nsplit, n_pairs);
    const unsigned int nqs = (unsigned int)n_query_sets, nts = (unsigned int)n_train_sets;
    if (same_octave)
        LAUNCH(c, "k_match_nn2_pairs", k_match_nn2_pairs<true>, grid, dim3(256), *Q, *T, pairs, nqs, nts, qnorm, tnorm, (int)pl.m.nsplit, part);
    else
        LAUNCH(c, "k_match_nn2_pairs", k_match_nn2_pairs<false>, grid, dim3(256), *Q, *T, pairs, nqs, nts, qnorm, tnorm, (int)pl.m.nsplit, part);
    LAUNCH(c, "k_match_merge_pairs", k_match_merge_pairs, dim3(pl.m.qrow_blocks, n_pairs), dim3(MT_ROW_WG), *Q, pairs, nqs, nts, part, (int)pl.m.nsplit,
           ratio2, nn, flags, pl.m.fwords);
    if (out->match_counts)
        TRY(enqueue_match_list(c, flags, pl.m.fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_pairs_host(vslam_ctx* c, const vslam_desc_sets* Q, int n_query_sets, const vslam_desc_sets* T, int n_train_sets,
                           const vslam_set_pair* pairs, int n_pairs, float ratio2, int same_octave, const vslam_match_out* out) {
    if (const char* why = match_pairs_check(Q, n_query_sets, T, n_train_sets, pairs, n_pairs, ratio2, same_octave, out, false))
        return fail(c, VSLAM_ERR_INVALID, std::string("match_pairs_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;  // (as the device call: nothing is written)

    HostMirror hm(c);
    auto up = [&](const vslam_desc_sets& h, int n) {
        const size_t rows = (size_t)n * h.cap;
        return vslam_desc_sets{hm.in(h.desc, std::max<size_t>(rows, 1) * 128), hm.in(h.defined, rows), hm.in(h.points, rows), hm.in(h.counts, (size_t)std::max(n, 1)),
                               h.cap};
    };
    // (a side without sets is never read: its desc goes up as one row so that the set has its pointers)
    std::vector<float> none(128, 0.0f);
    const uint32_t zero = 0;
    auto host_side = [&](const vslam_desc_sets& h, int n) { return n > 0 ? h : vslam_desc_sets{none.data(), nullptr, h.points, &zero, h.cap}; };
    const vslam_desc_sets dq = up(host_side(*Q, n_query_sets), n_query_sets);
    const vslam_desc_sets dt = same_sets(*Q, n_query_sets, *T, n_train_sets) && n_query_sets > 0 ? dq : up(host_side(*T, n_train_sets), n_train_sets);
    const vslam_set_pair* d_pairs = hm.in(pairs, (size_t)n_pairs);
    vslam_match_out o{};
    o.struct_size = sizeof(o);
    o.match_cap = out->match_cap;
    hm.out(o.nn, o.nn_bytes, out->nn, (size_t)n_pairs * Q->cap, true);
    hm.out(o.matches, o.matches_bytes, out->matches, (size_t)n_pairs * out->match_cap, true);
    hm.out(o.match_counts, o.match_counts_bytes, out->match_counts, (size_t)n_pairs, false);
    TRY(hm.status());
    TRY(vslam_match_pairs_dev(c, &dq, n_query_sets, &dt, n_train_sets, d_pairs, n_pairs, ratio2, same_octave, &o));
    return hm.finish();
}

}  // extern "C"

// Guided matching of the C ABI (include/vslam.h): argument checks and sizing (vslam_guided_plan.h), scratch and launches of
// kernels_match_guided.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match_guided.hip.h"
#include "vslam_ctx.h"
#include "vslam_guided_plan.h"
#include "vslam_launch.h"

using namespace vslam;

int vslam::enqueue_guided_merge(vslam_ctx* c, const vslam_desc_sets& Q, int n_pairs, const MatchPart* part, unsigned int nsplit, float ratio2,
                                float max_desc_dist2, vslam_nn2* nn, unsigned long long* flags, unsigned int fwords) {
    const unsigned int blocks = (unsigned int)(((size_t)Q.cap + MT_ROW_WG - 1) / MT_ROW_WG);  // MatchPlan::qrow_blocks
    LAUNCH(c, "k_match_guided_merge", k_match_guided_merge, dim3(blocks, n_pairs), dim3(MT_ROW_WG), Q, part, (int)nsplit, ratio2, max_desc_dist2, nn, flags,
           fwords);
    return VSLAM_OK;
}

extern "C" {

int vslam_match_guided_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, const vslam_epipolar* models, int n_pairs,
                           const vslam_guided_params* prm, const vslam_match_out* out) {
    static_assert(sizeof(vslam_guided_params) == 24 && sizeof(GuidedRow) == 32 && sizeof(MatchPart) == 12 && sizeof(GuidedQn) == 8, "record layouts");
    if (const char* why = guided_check_args(Q, T, models, n_pairs, prm, out)) return fail(c, VSLAM_ERR_INVALID, std::string("match_guided: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const GuidedPlan pl = guided_plan(Q->cap, T->cap, n_pairs);
    float *qnorm = nullptr, *tnorm = nullptr;
    GuidedRow *qrows = nullptr, *trows = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long* flags = nullptr;
    unsigned int* chunk_ws = nullptr;
    WsPlan ws;
    ws.add(qnorm, pl.q_elems);
    ws.add(tnorm, pl.t_elems);
    ws.add(qrows, pl.q_elems);
    ws.add(trows, pl.t_elems);
    ws.add(part, pl.part_elems);
    if (!out->nn) ws.add(nn_ws, pl.q_elems);
    ws.add(flags, pl.flag_words);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;

    TRY(enqueue_desc_norms(c, *Q, n_pairs, qnorm));
    TRY(enqueue_desc_norms(c, *T, n_pairs, tnorm));
    LAUNCH(c, "k_guided_rows", k_guided_rows<true>, dim3(pl.qrow_blocks, n_pairs), dim3(MT_ROW_WG), *Q, models, qrows);
    LAUNCH(c, "k_guided_rows", k_guided_rows<false>, dim3(pl.trow_blocks, n_pairs), dim3(MT_ROW_WG), *T, models, trows);
    const dim3 grid(pl.qtiles, pl.nsplit, n_pairs);
    if (prm->same_octave)
        LAUNCH(c, "k_match_guided", k_match_guided<true>, grid, dim3(256), *Q, *T, qnorm, tnorm, qrows, trows, prm->max_dist2, (int)pl.nsplit, part);
    else
        LAUNCH(c, "k_match_guided", k_match_guided<false>, grid, dim3(256), *Q, *T, qnorm, tnorm, qrows, trows, prm->max_dist2, (int)pl.nsplit, part);
    TRY(enqueue_guided_merge(c, *Q, n_pairs, part, pl.nsplit, prm->ratio2, prm->max_desc_dist2, nn, flags, pl.fwords));
    if (out->match_counts)
        TRY(enqueue_match_list(c, flags, pl.fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_guided_host(vslam_ctx* c, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                            const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt,
                            const vslam_epipolar* model, const vslam_guided_params* prm, vslam_nn2* nn, vslam_match* matches, size_t match_cap,
                            size_t* n_matches) {
    ARGCHK(c, model && prm, "match_guided_host: null argument");
    ARGCHK(c, (query || nq == 0) && (train || nt == 0), "match_guided_host: null descriptors");
    ARGCHK(c, nq < (1u << 31) && nt < (1u << 31) && match_cap < (1u << 31), "match_guided_host: too many rows");
    ARGCHK(c, prm->reserved == 0, "match_guided_host: params->reserved must be 0");
    ARGCHK(c, std::isfinite(prm->ratio2) && prm->ratio2 > 0.0f, "match_guided_host: ratio2 must be finite and positive");
    ARGCHK(c, prm->max_desc_dist2 > 0.0f, "match_guided_host: max_desc_dist2 must be positive (+inf: no bound)");
    ARGCHK(c, std::isfinite(prm->max_dist2) && prm->max_dist2 > 0.0, "match_guided_host: max_dist2 must be finite and positive");
    ARGCHK(c, (query_points || nq == 0) && (train_points || nt == 0), "match_guided_host: the points of both sets are required");
    ARGCHK(c, nn || n_matches, "match_guided_host: no output requested");
    ARGCHK(c, !matches || (n_matches && match_cap > 0), "match_guided_host: matches needs n_matches and a match_cap");
    TRY(usable_ctx(c));

    HostSets hs{{query, train}, {query_defined, train_defined}, {query_points, train_points}, {nq, nt}, nn, matches, match_cap, n_matches};
    DevBufs dev;
    vslam_epipolar* d_model = nullptr;
    vslam_match_out out{};
    TRY(hs.upload(c, dev, true));
    TRY(dev.put(c, d_model, model, 1));
    TRY(hs.outputs(c, dev, out));
    TRY(vslam_match_guided_dev(c, &hs.Q, &hs.T, d_model, 1, prm, &out));
    return hs.download(c, out);
}

}  // extern "C"

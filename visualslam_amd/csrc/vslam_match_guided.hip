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
    const unsigned int blocks = (unsigned int)(((size_t)Q.cap + GUIDED_ROW_WG - 1) / GUIDED_ROW_WG);  // GuidedPlan::qrow_blocks
    LAUNCH(c, "k_match_guided_merge", k_match_guided_merge, dim3(blocks, n_pairs), dim3(GUIDED_ROW_WG), Q, part, (int)nsplit, ratio2, max_desc_dist2, nn, flags,
           fwords);
    return VSLAM_OK;
}

extern "C" {

int vslam_match_guided_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, const vslam_epipolar* models, int n_pairs,
                           const vslam_guided_params* prm, const vslam_match_out* out) {
    static_assert(sizeof(vslam_guided_params) == 24 && sizeof(GuidedRow) == 32 && sizeof(MatchPart) == 12 && sizeof(GuidedQn) == 8, "record layouts");
    static_assert(GUIDED_Q == MT_Q && GUIDED_T == MT_T && GUIDED_MAX_SPLIT == MT_MAX_SPLIT && GUIDED_T * 4 == 256, "the plan's tiling is the kernels'");
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
    LAUNCH(c, "k_guided_rows", k_guided_rows<true>, dim3(pl.qrow_blocks, n_pairs), dim3(GUIDED_ROW_WG), *Q, models, qrows);
    LAUNCH(c, "k_guided_rows", k_guided_rows<false>, dim3(pl.trow_blocks, n_pairs), dim3(GUIDED_ROW_WG), *T, models, trows);
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

    DevBufs dev;
    const float* d_desc[2] = {nullptr, nullptr};
    const uint8_t* d_def[2] = {nullptr, nullptr};
    const vslam_point* d_pts[2] = {nullptr, nullptr};
    uint32_t* d_cnt = nullptr;
    vslam_epipolar* d_model = nullptr;
    const float* h_desc[2] = {query, train};
    const uint8_t* h_def[2] = {query_defined, train_defined};
    const vslam_point* h_pts[2] = {query_points, train_points};
    const uint32_t h_cnt[2] = {(uint32_t)nq, (uint32_t)nt};
    for (int i = 0; i < 2; ++i) {
        float* d = nullptr;
        TRY(dev.put(c, d, h_desc[i], (size_t)h_cnt[i] * 128));
        d_desc[i] = d;
        if (h_def[i]) {
            uint8_t* q = nullptr;
            TRY(dev.put(c, q, h_def[i], h_cnt[i]));
            d_def[i] = q;
        }
        vslam_point* q = nullptr;
        TRY(dev.put(c, q, h_pts[i], h_cnt[i]));  // (no rows: one unread record, so that the set has its points)
        d_pts[i] = q;
    }
    TRY(dev.put(c, d_cnt, h_cnt, 2));
    TRY(dev.put(c, d_model, model, 1));
    const vslam_desc_sets Q{d_desc[0], d_def[0], d_pts[0], d_cnt, std::max<uint32_t>(h_cnt[0], 1)};
    const vslam_desc_sets T{d_desc[1], d_def[1], d_pts[1], d_cnt + 1, std::max<uint32_t>(h_cnt[1], 1)};
    vslam_match_out out{};
    out.struct_size = sizeof(out);
    if (nn) {
        TRY(dev.get(c, out.nn, nq));
        out.nn_bytes = std::max<size_t>(nq, 1) * sizeof(vslam_nn2);
    }
    if (n_matches) {
        TRY(dev.get(c, out.match_counts, 1));
        out.match_counts_bytes = sizeof(uint32_t);
        if (matches) {
            TRY(dev.get(c, out.matches, match_cap));
            out.matches_bytes = match_cap * sizeof(vslam_match);
            out.match_cap = (uint32_t)match_cap;
        }
    }
    TRY(vslam_match_guided_dev(c, &Q, &T, d_model, 1, prm, &out));
    uint32_t total = 0;
    if (nn && nq) HIPCHK(c, hipMemcpyAsync(nn, out.nn, nq * sizeof(vslam_nn2), hipMemcpyDeviceToHost, c->stream));
    if (n_matches) HIPCHK(c, hipMemcpyAsync(&total, out.match_counts, sizeof(total), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_matches) {
        *n_matches = total;
        const size_t m = std::min<size_t>(total, match_cap);
        if (matches && m) HIPCHK(c, hipMemcpy(matches, out.matches, m * sizeof(vslam_match), hipMemcpyDeviceToHost));
    }
    return VSLAM_OK;
}

}  // extern "C"

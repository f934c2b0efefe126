// Mutual matching of the C ABI (include/vslam.h): argument checks and sizing (vslam_mutual_plan.h), scratch and launches of
// kernels_match_mutual.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match_mutual.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_mutual_plan.h"

using namespace vslam;

extern "C" {

int vslam_match_mutual_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, int n_pairs, float ratio2, int same_octave,
                           const vslam_match_mutual_out* out) {
    static_assert(sizeof(vslam_rnn) == 8 && sizeof(vslam_nn2) == 12 && sizeof(MatchPart) == 12, "record layouts");
    static_assert(MUTUAL_Q == MT_Q && MUTUAL_T == MT_T && MUTUAL_MAX_SPLIT == MT_MAX_SPLIT && MUTUAL_T == 64, "the plan's tiling is the kernels'");
    if (const char* why = mutual_check_args(Q, T, n_pairs, ratio2, same_octave, out)) return fail(c, VSLAM_ERR_INVALID, std::string("match_mutual: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const MutualPlan pl = mutual_plan(Q->cap, T->cap, n_pairs);
    float *qnorm = nullptr, *tnorm = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long *flags = nullptr, *rev = nullptr;
    unsigned int* chunk_ws = nullptr;
    WsPlan ws;
    ws.add(qnorm, pl.q_elems);
    ws.add(tnorm, pl.t_elems);
    ws.add(part, pl.part_elems);
    if (!out->nn) ws.add(nn_ws, pl.q_elems);
    ws.add(flags, pl.flag_words);
    ws.add(rev, pl.rev_elems);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;

    HIPCHK(c, hipMemsetAsync(rev, 0xff, pl.rev_bytes, c->stream));  // REV_NONE everywhere: nothing offered yet
    TRY(enqueue_desc_norms(c, *Q, n_pairs, qnorm));
    TRY(enqueue_desc_norms(c, *T, n_pairs, tnorm));
    const dim3 grid(pl.qtiles, pl.nsplit, n_pairs);
    if (same_octave)
        LAUNCH(c, "k_match_nn2_mutual", k_match_nn2_mutual<true>, grid, dim3(256), *Q, *T, qnorm, tnorm, (int)pl.nsplit, part, rev);
    else
        LAUNCH(c, "k_match_nn2_mutual", k_match_nn2_mutual<false>, grid, dim3(256), *Q, *T, qnorm, tnorm, (int)pl.nsplit, part, rev);
    LAUNCH(c, "k_match_mutual_merge", k_match_mutual_merge, dim3(pl.qrow_blocks, n_pairs), dim3(MUTUAL_ROW_WG), *Q, part, (int)pl.nsplit, ratio2, rev, T->cap,
           nn, flags, pl.fwords);
    if (out->rnn) LAUNCH(c, "k_match_rnn_write", k_match_rnn_write, dim3(pl.trow_blocks, n_pairs), dim3(MUTUAL_ROW_WG), *T, rev, out->rnn);
    if (out->match_counts)
        TRY(enqueue_match_list(c, flags, pl.fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_mutual_host(vslam_ctx* c, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                            const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt, float ratio2,
                            int same_octave, vslam_nn2* nn, vslam_rnn* rnn, vslam_match* matches, size_t match_cap, size_t* n_matches) {
    ARGCHK(c, (query || nq == 0) && (train || nt == 0), "match_mutual_host: null descriptors");
    ARGCHK(c, nq < (1u << 31) && nt < (1u << 31) && match_cap < (1u << 31), "match_mutual_host: too many rows");
    ARGCHK(c, std::isfinite(ratio2) && ratio2 > 0.0f, "match_mutual_host: ratio2 must be finite and positive");
    ARGCHK(c, !same_octave || ((query_points || nq == 0) && (train_points || nt == 0)), "match_mutual_host: same_octave needs the points of both sets");
    ARGCHK(c, nn || rnn || n_matches, "match_mutual_host: no output requested");
    ARGCHK(c, !matches || (n_matches && match_cap > 0), "match_mutual_host: matches needs n_matches and a match_cap");
    TRY(usable_ctx(c));

    DevBufs dev;
    const float* d_desc[2] = {nullptr, nullptr};
    const uint8_t* d_def[2] = {nullptr, nullptr};
    const vslam_point* d_pts[2] = {nullptr, nullptr};
    uint32_t* d_cnt = nullptr;
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
        if (same_octave) {
            vslam_point* q = nullptr;
            TRY(dev.put(c, q, h_pts[i], h_cnt[i]));
            d_pts[i] = q;
        }
    }
    TRY(dev.put(c, d_cnt, h_cnt, 2));
    const vslam_desc_sets Q{d_desc[0], d_def[0], d_pts[0], d_cnt, std::max<uint32_t>(h_cnt[0], 1)};
    const vslam_desc_sets T{d_desc[1], d_def[1], d_pts[1], d_cnt + 1, std::max<uint32_t>(h_cnt[1], 1)};
    vslam_match_mutual_out out{};
    out.struct_size = sizeof(out);
    if (nn) {
        TRY(dev.get(c, out.nn, nq));
        out.nn_bytes = std::max<size_t>(nq, 1) * sizeof(vslam_nn2);
    }
    if (rnn) {
        TRY(dev.get(c, out.rnn, nt));
        out.rnn_bytes = std::max<size_t>(nt, 1) * sizeof(vslam_rnn);
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
    TRY(vslam_match_mutual_dev(c, &Q, &T, 1, ratio2, same_octave, &out));
    uint32_t total = 0;
    if (nn && nq) HIPCHK(c, hipMemcpyAsync(nn, out.nn, nq * sizeof(vslam_nn2), hipMemcpyDeviceToHost, c->stream));
    if (rnn && nt) HIPCHK(c, hipMemcpyAsync(rnn, out.rnn, nt * sizeof(vslam_rnn), hipMemcpyDeviceToHost, c->stream));
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

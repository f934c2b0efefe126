// Descriptor matching of the C ABI (include/vslam.h): argument checks, scratch and launches of kernels_match.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"

using namespace vslam;

int vslam::enqueue_desc_norms(vslam_ctx* c, const vslam_desc_sets& S, int n_pairs, float* norms) {
    LAUNCH(c, "k_desc_norms", k_desc_norms, dim3((unsigned int)(((size_t)S.cap + 255) / 256), n_pairs), dim3(256), S, norms);
    return VSLAM_OK;
}

extern "C" {

int vslam_match_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, int n_pairs, float ratio2, int same_octave,
                    const vslam_match_out* out) {
    static_assert(sizeof(vslam_nn2) == 12 && sizeof(vslam_match) == 12 && sizeof(MatchPart) == 12, "record layouts");
    ARGCHK(c, Q && T && out, "match: null argument");
    ARGCHK(c, out->struct_size == sizeof(vslam_match_out), "match: out->struct_size is not sizeof(vslam_match_out)");
    ARGCHK(c, n_pairs >= 0 && n_pairs <= 65535, "match: 0 .. 65535 pairs per call");
    ARGCHK(c, std::isfinite(ratio2) && ratio2 > 0.0f, "match: ratio2 must be finite and positive");
    for (const vslam_desc_sets* s : {Q, T}) {
        ARGCHK(c, s->desc && s->counts && s->cap > 0, "match: a descriptor set needs desc, counts and a capacity");
        ARGCHK(c, (reinterpret_cast<uintptr_t>(s->desc) & 15) == 0, "match: desc must be 16-byte aligned");
        ARGCHK(c, !same_octave || s->points, "match: same_octave needs the points of both sets");
    }
    const size_t np = (size_t)n_pairs;
    ARGCHK(c, out->nn || out->match_counts, "match: no output requested");
    ARGCHK(c, !out->nn || out->nn_bytes / sizeof(vslam_nn2) >= np * Q->cap, "match: nn buffer too small");
    ARGCHK(c, !out->matches || (out->match_counts && out->match_cap > 0), "match: matches needs match_counts and a match_cap");
    ARGCHK(c, !out->matches || out->matches_bytes / sizeof(vslam_match) >= np * out->match_cap, "match: matches buffer too small");
    ARGCHK(c, !out->match_counts || out->match_counts_bytes / sizeof(uint32_t) >= np, "match: match_counts buffer too small");
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    // Train tiles are dealt out round robin to nsplit workgroups per query tile, so that one small pair still fills the chip
    // (the counts live on the device: the grid is sized from the capacities).  The merge is exact for any nsplit.
    const unsigned int qtiles = (Q->cap + MT_Q - 1) / MT_Q, ttiles = (T->cap + MT_T - 1) / MT_T;
    const size_t wgs = (size_t)qtiles * np;
    const int nsplit = (int)std::max<size_t>(1, std::min<size_t>({(2048 + wgs - 1) / wgs, (size_t)MT_MAX_SPLIT, (size_t)ttiles}));
    const unsigned int fwords = (Q->cap + 63) / 64;

    float *qnorm = nullptr, *tnorm = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long* flags = nullptr;
    unsigned int* chunk_ws = nullptr;
    WsPlan ws;
    ws.add(qnorm, np * Q->cap);
    ws.add(tnorm, np * T->cap);
    ws.add(part, np * nsplit * Q->cap);
    if (!out->nn) ws.add(nn_ws, np * Q->cap);
    ws.add(flags, np * fwords);
    ws.add(chunk_ws, match_list_ws_elems(fwords, n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;

    TRY(enqueue_desc_norms(c, *Q, n_pairs, qnorm));
    TRY(enqueue_desc_norms(c, *T, n_pairs, tnorm));
    const dim3 grid(qtiles, nsplit, n_pairs);
    if (same_octave)
        LAUNCH(c, "k_match_nn2", k_match_nn2<true>, grid, dim3(256), *Q, *T, qnorm, tnorm, nsplit, part);
    else
        LAUNCH(c, "k_match_nn2", k_match_nn2<false>, grid, dim3(256), *Q, *T, qnorm, tnorm, nsplit, part);
    LAUNCH(c, "k_match_merge", k_match_merge, dim3((Q->cap + 255) / 256, n_pairs), dim3(256), *Q, part, nsplit, ratio2, nn, flags, fwords);
    if (out->match_counts) TRY(enqueue_match_list(c, flags, fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_host(vslam_ctx* c, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                     const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt, float ratio2,
                     int same_octave, vslam_nn2* nn, vslam_match* matches, size_t match_cap, size_t* n_matches) {
    ARGCHK(c, (query || nq == 0) && (train || nt == 0), "match_host: null descriptors");
    ARGCHK(c, nq < (1u << 31) && nt < (1u << 31) && match_cap < (1u << 31), "match_host: too many rows");
    ARGCHK(c, std::isfinite(ratio2) && ratio2 > 0.0f, "match_host: ratio2 must be finite and positive");
    ARGCHK(c, !same_octave || ((query_points || nq == 0) && (train_points || nt == 0)), "match_host: same_octave needs the points of both sets");
    ARGCHK(c, nn || n_matches, "match_host: no output requested");
    ARGCHK(c, !matches || (n_matches && match_cap > 0), "match_host: matches needs n_matches and a match_cap");
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
    TRY(vslam_match_dev(c, &Q, &T, 1, ratio2, same_octave, &out));
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

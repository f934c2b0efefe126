// Vocabulary training of the C ABI (include/vslam.h, "vocabulary training"): argument checks (vslam_kmeans_plan.h), scratch and
// the launches of one call: per round the word search as vslam_words_dev enqueues it (enqueue_words, vslam_words.hip) and the
// kernels of kernels_kmeans.hip.h.  Every round is enqueued; the device decides which of them run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_kmeans.hip.h"
#include "vslam_ctx.h"
#include "vslam_kmeans_plan.h"
#include "vslam_launch.h"

using namespace vslam;

extern "C" {

int vslam_vocab_kmeans_dev(vslam_ctx* c, const vslam_desc_sets* sets, int n_sets, const float* vocab_in, const uint8_t* vocab_defined, uint32_t K,
                           const vslam_kmeans_params* params, const vslam_kmeans_out* out) {
    static_assert(sizeof(KmState) == 16, "record layout");
    if (const char* why = kmeans_check(sets, n_sets, vocab_in, K, params, out, true))
        return fail(c, VSLAM_ERR_INVALID, std::string("vocab_kmeans: ") + why);
    TRY(usable_ctx(c));
    const uint32_t rounds = params->rounds;
    const KmeansPlan pl = kmeans_plan(sets->cap, K, n_sets, rounds);

    if (out->vocab != vocab_in) HIPCHK(c, hipMemcpyAsync(out->vocab, vocab_in, pl.vocab_bytes, hipMemcpyDeviceToDevice, c->stream));
    if (out->report) HIPCHK(c, hipMemsetAsync(out->report, 0, pl.report_bytes, c->stream));
    if (n_sets == 0) {
        if (out->sizes) HIPCHK(c, hipMemsetAsync(out->sizes, 0, pl.sizes_bytes, c->stream));
        return VSLAM_OK;
    }

    WordsScratch s{};
    int* words[2] = {nullptr, nullptr};  // this round's and the last round's, in turns
    uint32_t *vcount = nullptr, *kcounts = nullptr, *hist = nullptr, *N = nullptr, *wstart = nullptr, *bstart = nullptr, *members = nullptr;
    double* bsum = nullptr;
    KmState* state = nullptr;
    WsPlan ws;
    ws.add(s.qnorm, pl.w.m.q_elems);
    ws.add(s.vnorm, pl.w.vnorm_elems);
    ws.add(s.part, pl.w.m.part_elems);
    ws.add(vcount, 1);
    ws.add(kcounts, (size_t)n_sets);
    ws.add(state, 1);
    ws.add(words[0], pl.rows);
    ws.add(words[1], pl.rows);
    ws.add(hist, pl.w.hist_elems);
    ws.add(N, K);
    ws.add(wstart, (size_t)K + 1);
    ws.add(bstart, (size_t)K + 1);
    ws.add(members, pl.rows);
    ws.add(bsum, pl.bsum_elems);
    TRY(ws.commit(c));

    // the call's own counts, clamped: a converged call zeroes them, and the vocabulary's with them
    LAUNCH(c, "k_kmeans_init", k_kmeans_init, dim3(pl.init_blocks), dim3(256), sets->counts, sets->cap, (unsigned int)n_sets, K, kcounts, vcount,
           state);
    const vslam_desc_sets S{sets->desc, sets->defined, nullptr, kcounts, sets->cap};
    const vslam_desc_sets V{out->vocab, vocab_defined, nullptr, vcount, K};
    for (uint32_t t = 0; t < rounds; ++t) {
        int *cur = words[t & 1], *prev = words[(t & 1) ^ 1];
        TRY(enqueue_words(c, S, n_sets, V, pl.w, s, t == 0, cur, nullptr, hist));
        LAUNCH(c, "k_kmeans_count", k_kmeans_count, dim3(pl.count_blocks, n_sets), dim3(256), kcounts, sets->cap, cur, prev, t == 0 ? 1 : 0, state);
        LAUNCH(c, "k_kmeans_columns", k_kmeans_columns, dim3(pl.column_blocks), dim3(256), hist, (unsigned int)n_sets, K, N, state);
        LAUNCH(c, "k_kmeans_scan", k_kmeans_scan, dim3(1), dim3(256), N, vocab_defined, K, (unsigned int)n_sets, t, wstart, bstart, kcounts, vcount,
               out->report, state);
        LAUNCH(c, "k_kmeans_members", k_kmeans_members, dim3(n_sets), dim3(KM_CHUNK), cur, kcounts, sets->cap, K, hist, wstart, members, state);
        LAUNCH(c, "k_kmeans_block_sums", k_kmeans_block_sums, dim3(pl.sum_blocks), dim3(64 * KM_WAVES), sets->desc, members, wstart, bstart, K, bsum,
               state);
        LAUNCH(c, "k_kmeans_update", k_kmeans_update, dim3(K), dim3(128), out->vocab, wstart, bstart, bsum, out->sizes, state);
    }
    return VSLAM_OK;
}

int vslam_vocab_kmeans_host(vslam_ctx* c, const float* desc, const uint8_t* defined, const uint32_t* counts, uint32_t cap, int n_sets,
                            const float* vocab_in, const uint8_t* vocab_defined, uint32_t K, const vslam_kmeans_params* params,
                            const vslam_kmeans_out* out) {
    const vslam_desc_sets host{desc, defined, nullptr, counts, cap};
    if (const char* why = kmeans_check(&host, n_sets, vocab_in, K, params, out, false))
        return fail(c, VSLAM_ERR_INVALID, std::string("vocab_kmeans_host: ") + why);
    TRY(usable_ctx(c));

    const size_t rows = (size_t)n_sets * cap;
    HostMirror hm(c);
    const vslam_desc_sets dev{hm.in(desc, rows * 128), hm.in(defined, rows), nullptr, hm.in(counts, (size_t)n_sets), cap};
    const float* d_vocab = hm.in(vocab_in, (size_t)K * 128);
    const uint8_t* d_vdef = hm.in(vocab_defined, (size_t)K);
    vslam_kmeans_out o{};
    o.struct_size = sizeof(o);
    o.vocab = const_cast<float*>(d_vocab);  // in place over the device copy of vocab_in
    hm.out(o.vocab, o.vocab_bytes, out->vocab, (size_t)K * 128, false);
    hm.out(o.sizes, o.sizes_bytes, out->sizes, (size_t)K, false);
    hm.out(o.report, o.report_bytes, out->report, (size_t)params->rounds, false);
    TRY(hm.status());
    TRY(vslam_vocab_kmeans_dev(c, &dev, n_sets, d_vocab, d_vdef, K, params, &o));
    return hm.finish();
}

}  // extern "C"

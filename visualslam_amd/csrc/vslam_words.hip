// Vocabulary and visual words of the C ABI (include/vslam.h, "place recognition"): argument checks (vslam_place_plan.h),
// scratch and launches of kernels_words.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_words.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_place_plan.h"

using namespace vslam;

namespace vslam {
int enqueue_words(vslam_ctx* c, const vslam_desc_sets& sets, int n_sets, const vslam_desc_sets& V, const WordsPlan& pl, const WordsScratch& ws,
                  bool row_norms, int* words, float* dist2, unsigned int* hist) {
    static_assert(sizeof(WordPart) == sizeof(*ws.part), "record layout");
    WordPart* part = reinterpret_cast<WordPart*>(ws.part);
    if (hist) HIPCHK(c, hipMemsetAsync(hist, 0, pl.hist_elems * sizeof(uint32_t), c->stream));
    if (row_norms) TRY(enqueue_desc_norms(c, sets, n_sets, ws.qnorm));
    TRY(enqueue_desc_norms(c, V, 1, ws.vnorm));
    LAUNCH(c, "k_words_nn", k_words_nn, dim3(pl.m.qtiles, pl.m.nsplit, n_sets), dim3(256), sets, V, ws.qnorm, ws.vnorm, (int)pl.m.nsplit, part);
    LAUNCH(c, "k_words_merge", k_words_merge, dim3(pl.m.qrow_blocks, n_sets), dim3(MT_ROW_WG), sets, part, (int)pl.m.nsplit, V.cap, words, dist2, hist);
    return VSLAM_OK;
}
}  // namespace vslam

extern "C" {

int vslam_vocab_sample_dev(vslam_ctx* c, const vslam_desc_sets* sets, int n_sets, uint32_t K, float* vocab, size_t vocab_bytes,
                           uint8_t* vocab_defined, size_t vocab_defined_bytes) {
    if (const char* why = vocab_sample_check(sets, n_sets, K, vocab, vocab_bytes, vocab_defined, vocab_defined_bytes))
        return fail(c, VSLAM_ERR_INVALID, std::string("vocab_sample: ") + why);
    TRY(usable_ctx(c));
    const VocabPlan pl = vocab_plan(K);
    LAUNCH(c, "k_vocab_gather", k_vocab_gather, dim3(pl.gather_blocks), dim3(256), *sets, (unsigned int)n_sets, K, vocab, vocab_defined);
    return VSLAM_OK;
}

int vslam_words_dev(vslam_ctx* c, const vslam_desc_sets* sets, int n_sets, const float* vocab, const uint8_t* vocab_defined, uint32_t K,
                    const vslam_words_out* out) {
    if (const char* why = words_check(sets, n_sets, vocab, K, out, true)) return fail(c, VSLAM_ERR_INVALID, std::string("words: ") + why);
    TRY(usable_ctx(c));
    if (n_sets == 0) return VSLAM_OK;

    const WordsPlan pl = words_plan(sets->cap, K, n_sets);  // (the counts live on the device: the grid is sized from the capacities)
    WordsScratch s{};
    uint32_t* vcount = nullptr;
    WsPlan ws;
    ws.add(s.qnorm, pl.m.q_elems);
    ws.add(s.vnorm, pl.vnorm_elems);
    ws.add(s.part, pl.m.part_elems);
    ws.add(vcount, 1);
    TRY(ws.commit(c));

    // the vocabulary as one descriptor set of K rows, all in use
    HIPCHK(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(vcount), (int)K, 1, c->stream));
    const vslam_desc_sets V{vocab, vocab_defined, nullptr, vcount, K};
    return enqueue_words(c, *sets, n_sets, V, pl, s, true, out->words, out->word_dist2, out->hist);
}

int vslam_words_host(vslam_ctx* c, const float* desc, const uint8_t* defined, const uint32_t* counts, uint32_t cap, int n_sets, const float* vocab,
                     const uint8_t* vocab_defined, uint32_t K, const vslam_words_out* out) {
    const vslam_desc_sets host{desc, defined, nullptr, counts, cap};
    if (const char* why = words_check(&host, n_sets, vocab, K, out, false)) return fail(c, VSLAM_ERR_INVALID, std::string("words_host: ") + why);
    TRY(usable_ctx(c));

    const size_t rows = (size_t)n_sets * cap;
    HostMirror hm(c);
    const vslam_desc_sets dev{hm.in(desc, rows * 128), hm.in(defined, rows), nullptr, hm.in(counts, (size_t)n_sets), cap};
    const float* d_vocab = hm.in(vocab, (size_t)K * 128);
    const uint8_t* d_vdef = hm.in(vocab_defined, (size_t)K);
    vslam_words_out o{};
    o.struct_size = sizeof(o);
    hm.out(o.words, o.words_bytes, out->words, rows, true);
    hm.out(o.word_dist2, o.word_dist2_bytes, out->word_dist2, rows, true);
    hm.out(o.hist, o.hist_bytes, out->hist, (size_t)n_sets * K, false);
    TRY(hm.status());
    TRY(vslam_words_dev(c, &dev, n_sets, d_vocab, d_vdef, K, &o));
    return hm.finish();
}

}  // extern "C"

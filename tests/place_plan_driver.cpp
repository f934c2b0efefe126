// Host driver of tests/test_place_cpu.py: the argument checks and the grid and scratch sizing of the place recognition entry
// points (visualslam_amd/csrc/vslam_place_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities,
// vocabulary sizes and set counts up to their extremes and checks every size against its product formed in 128 bits and every
// grid dimension against HIP's limits; then every rejection of the three checks over pointers they never follow, with its message
// byte for byte, each output one element short at the largest call, and the order of the checks.
//   driver          "plan checked=N bad=B first=...", "args checked=N bad=B first=...", and one "size ..." line per plan the
//                   test works out by hand
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_place_plan.h"

using namespace vslam;

namespace {
struct Mem {
    alignas(16) float desc[8];
    uint32_t counts[1];
    uint8_t bytes[1];
    int32_t i32[1];
    uint32_t u32[1];
    vslam_place_cand cand[1];
};

struct Vocab : Mem {  // a valid vslam_vocab_sample_dev call: 40 sets, K = 100
    vslam_desc_sets S{desc, nullptr, nullptr, counts, 50};
    const vslam_desc_sets* s = &S;
    int n_sets = 40;
    uint32_t K = 100;
    float* vocab = desc;
    size_t vocab_bytes = 100 * 512, defined_bytes = 100;
    uint8_t* vdef = bytes;
    const char* why() const { return vocab_sample_check(s, n_sets, K, vocab, vocab_bytes, vdef, defined_bytes); }
};

struct Words : Mem {  // a valid vslam_words_dev call: 3 sets of capacity 50, K = 100
    vslam_desc_sets S{desc, nullptr, nullptr, counts, 50};
    const vslam_desc_sets* s = &S;
    int n_sets = 3;
    uint32_t K = 100;
    const float* vocab = desc;
    bool device = true;
    vslam_words_out out{};
    const vslam_words_out* o = &out;
    Words() {
        out.struct_size = sizeof(out);
        out.words = i32, out.words_bytes = 3 * 50 * 4;
        out.word_dist2 = desc, out.word_dist2_bytes = 3 * 50 * 4;
        out.hist = u32, out.hist_bytes = 3 * 100 * 4;
    }
    const char* why() const { return words_check(s, n_sets, vocab, K, o, device); }
};

struct Place : Mem {  // a valid vslam_place_dev call: 20 query frames from 7, 30 db frames from 0, K = 100, c = 3
    const uint32_t *hq = u32, *hd = u32;
    uint32_t nq = 20, q_first = 7, nd = 30, db_first = 0, K = 100;
    vslam_place_params P{4, 3, 1, 5, 0, 0};
    const vslam_place_params* p = &P;
    vslam_place_out out{};
    const vslam_place_out* o = &out;
    Place() {
        out.struct_size = sizeof(out);
        out.candidates = cand, out.candidates_bytes = 20 * 3 * 12;
        out.cand_counts = u32, out.cand_counts_bytes = 20 * 4;
        out.weights = u32, out.weights_bytes = 100 * 4;
        out.self_q = u32, out.self_q_bytes = 20 * 4;
        out.self_db = u32, out.self_db_bytes = 30 * 4;
        out.scores = u32, out.scores_bytes = 20 * 30 * 4;
    }
    const char* why() const { return place_check(hq, nq, q_first, hd, nd, db_first, K, p, o); }
};

// a valid call of `Type`, one change to it, and the whole message it must be refused with (nullptr: it stays valid)
#define EXPECT(Type, what, message, stmt)                                                                              \
    {                                                                                                                  \
        Type c;                                                                                                        \
        stmt;                                                                                                          \
        const char *why = c.why(), *want = message;                                                                    \
        args.expect(want ? (why && std::strcmp(why, want) == 0) : why == nullptr, #Type " " what);                      \
    }
}  // namespace

int main() {
    static_assert(sizeof(vslam_place_cand) == 12 && sizeof(vslam_place_params) == 24, "record layouts");
    static_assert(sizeof(vslam_words_out) == 7 * sizeof(size_t) && sizeof(vslam_place_out) == 13 * sizeof(size_t), "out layouts");
    typedef unsigned __int128 u128;
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff81u, 0xffffffffu};
    const uint32_t Ks[] = {1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096, 65535, 65536};
    const int sets[] = {1, 2, 7, 8, 9, 127, 128, 129, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t cap : caps)
        for (uint32_t K : Ks)
            for (int n : sets) {
                const WordsPlan p = words_plan(cap, K, n);
                const u128 q = cap, k = K, s = (unsigned)n;
                plan.expect((u128)p.m.qtiles * MT_Q >= q && ((u128)p.m.qtiles - 1) * MT_Q < q && p.m.qtiles < (1u << 31), "qtiles", cap, K, n);
                plan.expect((u128)p.m.ttiles * MT_T >= k && ((u128)p.m.ttiles - 1) * MT_T < k, "ttiles", cap, K, n);
                plan.expect(p.m.nsplit >= 1 && p.m.nsplit <= (unsigned int)MT_MAX_SPLIT && p.m.nsplit <= p.m.ttiles, "nsplit", cap, K, n);
                plan.expect((u128)p.m.qrow_blocks * MT_ROW_WG >= q && ((u128)p.m.qrow_blocks - 1) * MT_ROW_WG < q && p.m.qrow_blocks < (1u << 31), "qrow_blocks", cap, K, n);
                plan.expect((u128)p.m.q_elems == s * q && (u128)p.row_elems == s * q && (u128)p.vnorm_elems == k, "row elems", cap, K, n);
                plan.expect((u128)p.m.part_elems == s * p.m.nsplit * q && (u128)p.part_bytes == s * p.m.nsplit * q * 8 && (u128)p.part_bytes < ((u128)1 << 63), "part", cap, K, n);
                plan.expect((u128)p.hist_elems == s * k && (u128)p.hist_elems * 4 < ((u128)1 << 63), "hist", cap, K, n);
            }
    for (uint32_t K : Ks) {
        const VocabPlan v = vocab_plan(K);
        plan.expect((u128)v.gather_blocks * PL_GATHER_WG >= K && ((u128)v.gather_blocks - 1) * PL_GATHER_WG < K, "gather_blocks", K);
        plan.expect(v.vocab_bytes == (size_t)K * 512 && v.defined_bytes == K, "vocab bytes", K);
        const uint32_t frames[] = {0, 1, 2, 15, 16, 17, 40, 255, 256, 257, 65534, 65535};
        for (uint32_t nq : frames)
            for (uint32_t nd : frames) {
                const PlacePlan p = place_plan(nq, nd, K);
                plan.expect((u128)p.df_blocks * 256 >= K && ((u128)p.df_blocks - 1) * 256 < K, "df_blocks", nq, nd, K);
                plan.expect(p.self_blocks == nq + nd && p.top_blocks == nq, "wave grids", nq, nd, K);
                plan.expect((u128)p.tiles_q * PL_TILE >= nq && (nq == 0 ? p.tiles_q == 0 : ((u128)p.tiles_q - 1) * PL_TILE < nq) && p.tiles_q <= 65535, "tiles_q", nq, nd, K);
                plan.expect((u128)p.tiles_d * PL_TILE >= nd && (nd == 0 ? p.tiles_d == 0 : ((u128)p.tiles_d - 1) * PL_TILE < nd), "tiles_d", nq, nd, K);
                plan.expect((u128)p.score_elems == (u128)nq * nd, "score_elems", nq, nd, K);
            }
    }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);
    const struct {
        uint32_t cap, K;
        int n;
    } shown[] = {{1, 1, 1}, {129, 65, 1}, {2000, 4096, 1}, {4000, 1024, 256}, {0xffffffffu, 65536, 65535}};
    for (const auto& s : shown) {
        const WordsPlan p = words_plan(s.cap, s.K, s.n);
        std::printf("size %u %u %d qtiles=%u ttiles=%u nsplit=%u qrow_blocks=%u part_bytes=%zu hist_elems=%zu\n", s.cap, s.K, s.n, p.m.qtiles, p.m.ttiles,
                    p.m.nsplit, p.m.qrow_blocks, p.part_bytes, p.hist_elems);
    }

    Tally args;
    // ---- vslam_vocab_sample_dev
    EXPECT(Vocab, "valid", nullptr, (void)0)
    EXPECT(Vocab, "largest", nullptr, (c.n_sets = 65535, c.K = 65536, c.S.cap = 0xffffffffu, c.vocab_bytes = (size_t)65536 * 512, c.defined_bytes = 65536))
    EXPECT(Vocab, "largest vocab - 1", "vocab buffer too small", (c.K = 65536, c.vocab_bytes = (size_t)65536 * 512 - 1, c.defined_bytes = 65536))
    EXPECT(Vocab, "null sets", "null argument", c.s = nullptr)
    EXPECT(Vocab, "null vocab", "null argument", c.vocab = nullptr)
    EXPECT(Vocab, "null vocab_defined", "null argument", c.vdef = nullptr)
    EXPECT(Vocab, "sets 0", "1 .. 65535 sets per call", c.n_sets = 0)
    EXPECT(Vocab, "sets 65536", "1 .. 65535 sets per call", c.n_sets = 65536)
    EXPECT(Vocab, "K 0", "1 .. 65536 words", c.K = 0)
    EXPECT(Vocab, "K 65537", "1 .. 65536 words", (c.K = 65537, c.vocab_bytes = (size_t)1 << 40, c.defined_bytes = (size_t)1 << 40))
    EXPECT(Vocab, "desc", "a descriptor set needs desc, counts and a capacity", c.S.desc = nullptr)
    EXPECT(Vocab, "counts", "a descriptor set needs desc, counts and a capacity", c.S.counts = nullptr)
    EXPECT(Vocab, "cap", "a descriptor set needs desc, counts and a capacity", c.S.cap = 0)
    EXPECT(Vocab, "desc misaligned", "desc must be 16-byte aligned", c.S.desc = c.desc + 1)
    EXPECT(Vocab, "vocab misaligned", "vocab must be 16-byte aligned", c.vocab = c.desc + 3)
    EXPECT(Vocab, "vocab small", "vocab buffer too small", c.vocab_bytes -= 1)
    EXPECT(Vocab, "vocab_defined small", "vocab_defined buffer too small", c.defined_bytes -= 1)
    EXPECT(Vocab, "null before sets", "null argument", (c.vocab = nullptr, c.n_sets = 0))
    EXPECT(Vocab, "sets before K", "1 .. 65535 sets per call", (c.n_sets = 0, c.K = 0))
    EXPECT(Vocab, "K before set", "1 .. 65536 words", (c.K = 0, c.S.cap = 0))
    EXPECT(Vocab, "set before vocab alignment", "desc must be 16-byte aligned", (c.S.desc = c.desc + 1, c.vocab = c.desc + 1))
    EXPECT(Vocab, "alignment before sizes", "vocab must be 16-byte aligned", (c.vocab = c.desc + 1, c.vocab_bytes = 0))
    EXPECT(Vocab, "vocab before vocab_defined", "vocab buffer too small", (c.vocab_bytes = 0, c.defined_bytes = 0))
    // ---- vslam_words_dev / vslam_words_host
    EXPECT(Words, "valid", nullptr, (void)0)
    EXPECT(Words, "no sets", nullptr, c.n_sets = 0)
    EXPECT(Words, "no vocab_defined is not looked at, words alone", nullptr, (c.out.word_dist2 = nullptr, c.out.hist = nullptr))
    EXPECT(Words, "word_dist2 alone", nullptr, (c.out.words = nullptr, c.out.hist = nullptr))
    EXPECT(Words, "hist alone", nullptr, (c.out.words = nullptr, c.out.word_dist2 = nullptr))
    EXPECT(Words, "largest", nullptr,
           (c.n_sets = 65535, c.K = 65536, c.S.cap = 0xffffffffu, c.out.words_bytes = c.out.word_dist2_bytes = (size_t)65535 * 0xffffffffu * 4,
            c.out.hist_bytes = (size_t)65535 * 65536 * 4))
    EXPECT(Words, "largest words - 1", "words buffer too small",
           (c.n_sets = 65535, c.K = 65536, c.S.cap = 0xffffffffu, c.out.words_bytes = (size_t)65535 * 0xffffffffu * 4 - 1))
    EXPECT(Words, "largest hist - 1", "hist buffer too small",
           (c.n_sets = 65535, c.K = 65536, c.out.words_bytes = c.out.word_dist2_bytes = (size_t)65535 * 50 * 4, c.out.hist_bytes = (size_t)65535 * 65536 * 4 - 1))
    EXPECT(Words, "null sets", "null argument", c.s = nullptr)
    EXPECT(Words, "null vocab", "null argument", c.vocab = nullptr)
    EXPECT(Words, "null out", "null argument", c.o = nullptr)
    EXPECT(Words, "struct_size", "out->struct_size is not sizeof(vslam_words_out)", c.out.struct_size -= 8)
    EXPECT(Words, "sets < 0", "0 .. 65535 sets per call", c.n_sets = -1)
    EXPECT(Words, "sets 65536", "0 .. 65535 sets per call", c.n_sets = 65536)
    EXPECT(Words, "K 0", "1 .. 65536 words", c.K = 0)
    EXPECT(Words, "K 65537", "1 .. 65536 words", c.K = 65537)
    EXPECT(Words, "desc", "a descriptor set needs desc, counts and a capacity", c.S.desc = nullptr)
    EXPECT(Words, "counts", "a descriptor set needs desc, counts and a capacity", c.S.counts = nullptr)
    EXPECT(Words, "cap", "a descriptor set needs desc, counts and a capacity", c.S.cap = 0)
    EXPECT(Words, "desc misaligned", "desc must be 16-byte aligned", c.S.desc = c.desc + 1)
    EXPECT(Words, "vocab misaligned", "vocab must be 16-byte aligned", c.vocab = c.desc + 2)
    EXPECT(Words, "host arrays need no alignment", nullptr, (c.device = false, c.S.desc = c.desc + 1, c.vocab = c.desc + 2))
    EXPECT(Words, "no output", "no output requested", (c.out.words = nullptr, c.out.word_dist2 = nullptr, c.out.hist = nullptr))
    EXPECT(Words, "words small", "words buffer too small", c.out.words_bytes -= 1)
    EXPECT(Words, "word_dist2 small", "word_dist2 buffer too small", c.out.word_dist2_bytes -= 1)
    EXPECT(Words, "hist small", "hist buffer too small", c.out.hist_bytes -= 1)
    EXPECT(Words, "hist sized by the capacity", "hist buffer too small", c.out.hist_bytes = 3 * 50 * 4)
    EXPECT(Words, "null before struct_size", "null argument", (c.vocab = nullptr, c.out.struct_size = 0))
    EXPECT(Words, "struct_size before sets", "out->struct_size is not sizeof(vslam_words_out)", (c.out.struct_size = 0, c.n_sets = -1))
    EXPECT(Words, "sets before K", "0 .. 65535 sets per call", (c.n_sets = -1, c.K = 0))
    EXPECT(Words, "K before set", "1 .. 65536 words", (c.K = 0, c.S.desc = nullptr))
    EXPECT(Words, "set before vocab", "desc must be 16-byte aligned", (c.S.desc = c.desc + 1, c.vocab = c.desc + 1))
    EXPECT(Words, "vocab before outputs", "vocab must be 16-byte aligned", (c.vocab = c.desc + 1, c.out.words = nullptr, c.out.word_dist2 = nullptr, c.out.hist = nullptr))
    EXPECT(Words, "no output before sizes", "no output requested", (c.out.words = nullptr, c.out.word_dist2 = nullptr, c.out.hist = nullptr, c.out.hist_bytes = 0))
    EXPECT(Words, "words before word_dist2", "words buffer too small", (c.out.words_bytes = 0, c.out.word_dist2_bytes = 0))
    EXPECT(Words, "word_dist2 before hist", "word_dist2 buffer too small", (c.out.word_dist2_bytes = 0, c.out.hist_bytes = 0))
    // ---- vslam_place_dev / vslam_place_host
    EXPECT(Place, "valid", nullptr, (void)0)
    EXPECT(Place, "no query frames", nullptr, (c.nq = 0, c.hq = nullptr))
    EXPECT(Place, "an empty database", nullptr, (c.nd = 0, c.hd = nullptr))
    EXPECT(Place, "cand_counts alone", nullptr, (c.out.candidates = nullptr, c.out.weights = nullptr, c.out.self_q = nullptr, c.out.self_db = nullptr, c.out.scores = nullptr))
    EXPECT(Place, "scores alone", nullptr, (c.out.candidates = nullptr, c.out.cand_counts = nullptr, c.out.weights = nullptr, c.out.self_q = nullptr, c.out.self_db = nullptr))
    EXPECT(Place, "weights alone", nullptr, (c.out.candidates = nullptr, c.out.cand_counts = nullptr, c.out.scores = nullptr, c.out.self_q = nullptr, c.out.self_db = nullptr))
    EXPECT(Place, "c 1 and 8", nullptr, (c.P.max_candidates = 8, c.out.candidates_bytes = 20 * 8 * 12))
    EXPECT(Place, "largest", nullptr,
           (c.nq = c.nd = 65535, c.K = 65536, c.q_first = c.db_first = (1u << 31) - 65535, c.P.max_candidates = 8, c.out.candidates_bytes = (size_t)65535 * 8 * 12,
            c.out.cand_counts_bytes = c.out.self_q_bytes = c.out.self_db_bytes = 65535 * 4, c.out.weights_bytes = 65536 * 4, c.out.scores_bytes = (size_t)65535 * 65535 * 4))
    EXPECT(Place, "largest scores - 1", "scores buffer too small",
           (c.nq = c.nd = 65535, c.out.candidates_bytes = (size_t)65535 * 3 * 12, c.out.cand_counts_bytes = c.out.self_q_bytes = c.out.self_db_bytes = 65535 * 4,
            c.out.scores_bytes = (size_t)65535 * 65535 * 4 - 1))
    EXPECT(Place, "null params", "null argument", c.p = nullptr)
    EXPECT(Place, "null out", "null argument", c.o = nullptr)
    EXPECT(Place, "null hist_q", "null argument", c.hq = nullptr)
    EXPECT(Place, "null hist_db", "null argument", c.hd = nullptr)
    EXPECT(Place, "struct_size", "out->struct_size is not sizeof(vslam_place_out)", c.out.struct_size += 8)
    EXPECT(Place, "nq", "at most 65535 frames on either side", c.nq = 65536)
    EXPECT(Place, "nd", "at most 65535 frames on either side", c.nd = 65536)
    EXPECT(Place, "K 0", "1 .. 65536 words", c.K = 0)
    EXPECT(Place, "K 65537", "1 .. 65536 words", c.K = 65537)
    EXPECT(Place, "query ids", "a frame id does not fit 31 bits", c.q_first = (1u << 31) - 19)
    EXPECT(Place, "db ids", "a frame id does not fit 31 bits", c.db_first = 0xffffffffu)
    EXPECT(Place, "c 0", "max_candidates must be 1 .. 8", c.P.max_candidates = 0)
    EXPECT(Place, "c 9", "max_candidates must be 1 .. 8", c.P.max_candidates = 9)
    EXPECT(Place, "den", "den must be positive", c.P.den = 0)
    EXPECT(Place, "reserved", "params->reserved must be 0", c.P.reserved = 1)
    EXPECT(Place, "no output", "no output requested",
           (c.out.candidates = nullptr, c.out.cand_counts = nullptr, c.out.weights = nullptr, c.out.self_q = nullptr, c.out.self_db = nullptr, c.out.scores = nullptr))
    EXPECT(Place, "candidates without counts", "candidates needs cand_counts", c.out.cand_counts = nullptr)
    EXPECT(Place, "candidates small", "candidates buffer too small", c.out.candidates_bytes -= 1)
    EXPECT(Place, "candidates sized for c = 3 with c = 4", "candidates buffer too small", c.P.max_candidates = 4)
    EXPECT(Place, "cand_counts small", "cand_counts buffer too small", c.out.cand_counts_bytes -= 1)
    EXPECT(Place, "weights small", "weights buffer too small", c.out.weights_bytes -= 1)
    EXPECT(Place, "self_q small", "self_q buffer too small", c.out.self_q_bytes -= 1)
    EXPECT(Place, "self_db small", "self_db buffer too small", c.out.self_db_bytes -= 1)
    EXPECT(Place, "self_db sized by nq", "self_db buffer too small", c.out.self_db_bytes = 20 * 4)
    EXPECT(Place, "scores small", "scores buffer too small", c.out.scores_bytes -= 1)
    EXPECT(Place, "null before struct_size", "null argument", (c.hq = nullptr, c.out.struct_size = 0))
    EXPECT(Place, "struct_size before frames", "out->struct_size is not sizeof(vslam_place_out)", (c.out.struct_size = 0, c.nq = 65536))
    EXPECT(Place, "frames before K", "at most 65535 frames on either side", (c.nd = 65536, c.K = 0))
    EXPECT(Place, "K before ids", "1 .. 65536 words", (c.K = 0, c.db_first = 0xffffffffu))
    EXPECT(Place, "ids before c", "a frame id does not fit 31 bits", (c.db_first = 0xffffffffu, c.P.max_candidates = 0))
    EXPECT(Place, "c before den", "max_candidates must be 1 .. 8", (c.P.max_candidates = 0, c.P.den = 0))
    EXPECT(Place, "den before reserved", "den must be positive", (c.P.den = 0, c.P.reserved = 1))
    EXPECT(Place, "reserved before outputs", "params->reserved must be 0", (c.P.reserved = 1, c.out.cand_counts = nullptr))
    EXPECT(Place, "counts before sizes", "candidates needs cand_counts", (c.out.cand_counts = nullptr, c.out.candidates_bytes = 0))
    EXPECT(Place, "candidates before the rest", "candidates buffer too small", (c.out.candidates_bytes = 0, c.out.scores_bytes = 0))
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}

// Host driver of tests/test_kmeans_cpu.py: the argument checks and the grid and scratch sizing of vocabulary training
// (visualslam_amd/csrc/vslam_kmeans_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities,
// vocabulary sizes and set counts whose row ids fit 32 bits up to their extremes and checks every size against its product formed
// in 128 bits and every grid dimension against HIP's limits; then every rejection of the check over pointers it never follows,
// with its message byte for byte, each output one byte short at the largest call, and the order of the checks.
//   driver          "plan checked=N bad=B first=...", "args checked=N bad=B first=...", and one "size ..." line per plan the
//                   test works out by hand
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_kmeans_plan.h"

using namespace vslam;

namespace {
struct Call {  // a valid vslam_vocab_kmeans_dev call: 3 sets of capacity 50, K = 100, 5 rounds, in place
    alignas(16) float desc[8];
    alignas(16) float other[8];
    uint32_t counts[1];
    uint32_t u32[1];
    vslam_kmeans_round rec[1];
    vslam_desc_sets S{desc, nullptr, nullptr, counts, 50};
    const vslam_desc_sets* s = &S;
    int n_sets = 3;
    uint32_t K = 100;
    const float* vocab_in = desc;
    bool device = true;
    vslam_kmeans_params P{5, 0};
    const vslam_kmeans_params* p = &P;
    vslam_kmeans_out out{};
    const vslam_kmeans_out* o = &out;
    Call() {
        out.struct_size = sizeof(out);
        out.vocab = desc, out.vocab_bytes = 100 * 512;
        out.sizes = u32, out.sizes_bytes = 100 * 4;
        out.report = rec, out.report_bytes = 5 * 16;
    }
    const char* why() const { return kmeans_check(s, n_sets, vocab_in, K, p, o, device); }
};

#define EXPECT(what, message, stmt)                                                                   \
    {                                                                                                 \
        Call c;                                                                                       \
        stmt;                                                                                         \
        const char *why = c.why(), *want = message;                                                   \
        args.expect(want ? (why && std::strcmp(why, want) == 0) : why == nullptr, what);               \
    }
}  // namespace

int main() {
    static_assert(sizeof(vslam_kmeans_round) == 16 && sizeof(vslam_kmeans_params) == 8 && sizeof(vslam_kmeans_out) == 7 * sizeof(size_t), "layouts");
    typedef unsigned __int128 u128;
    Tally plan;
    const uint32_t caps[] = {1, 2, 255, 256, 257, 1000, 65535, 65536, 65537, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffffffu};
    const uint32_t Ks[] = {1, 2, 255, 256, 257, 1000, 4096, 65535, 65536};
    const int sets[] = {1, 2, 255, 256, 257, 2048, 65534, 65535};
    for (uint32_t cap : caps)
        for (uint32_t K : Ks)
            for (int n : sets) {
                if ((u128)cap * (unsigned)n > 0xffffffffu) continue;  // refused: row ids past 32 bits
                for (uint32_t rounds : {1u, 64u}) {
                    const KmeansPlan p = kmeans_plan(cap, K, n, rounds);
                    const u128 q = cap, k = K, s = (unsigned)n, rows = s * q;
                    plan.expect((u128)p.rows == rows && rows <= 0xffffffffu, "rows", cap, K, n);
                    plan.expect((u128)p.max_blocks == rows / 256 + k && (u128)p.max_blocks * 256 + 255 * k >= rows && p.max_blocks < (1u << 31), "max_blocks", cap, K, n);
                    plan.expect((u128)p.bsum_elems == (rows / 256 + k) * 128 && (u128)p.bsum_elems * 8 < ((u128)1 << 40), "bsum", cap, K, n);
                    plan.expect((u128)p.init_blocks * 256 >= s && ((u128)p.init_blocks - 1) * 256 < s, "init_blocks", cap, K, n);
                    plan.expect((u128)p.count_blocks * 256 >= q && ((u128)p.count_blocks - 1) * 256 < q && p.count_blocks < (1u << 31), "count_blocks", cap, K, n);
                    plan.expect((u128)p.column_blocks * 256 >= k && ((u128)p.column_blocks - 1) * 256 < k, "column_blocks", cap, K, n);
                    plan.expect((u128)p.sum_blocks * KM_WAVES >= p.max_blocks && ((u128)p.sum_blocks - 1) * KM_WAVES < p.max_blocks && p.sum_blocks < (1u << 31), "sum_blocks",
                                cap, K, n);
                    plan.expect(p.vocab_bytes == (size_t)K * 512 && p.sizes_bytes == (size_t)K * 4 && p.report_bytes == (size_t)rounds * 16, "out bytes", cap, K, n);
                    plan.expect((u128)p.w.hist_elems == s * k && (u128)p.w.row_elems == rows, "words plan", cap, K, n);
                }
            }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);
    const struct {
        uint32_t cap, K;
        int n;
    } shown[] = {{1, 1, 1}, {700, 64, 3}, {2000, 4096, 1}, {65536, 1024, 256}, {65537, 65536, 65535}};
    for (const auto& s : shown) {
        const KmeansPlan p = kmeans_plan(s.cap, s.K, s.n, 8);
        std::printf("size %u %u %d rows=%zu max_blocks=%zu bsum_bytes=%zu init=%u count=%u columns=%u sums=%u\n", s.cap, s.K, s.n, p.rows, p.max_blocks,
                    p.bsum_elems * 8, p.init_blocks, p.count_blocks, p.column_blocks, p.sum_blocks);
    }

    Tally args;
    EXPECT("valid", nullptr, (void)0)
    EXPECT("no sets", nullptr, c.n_sets = 0)
    EXPECT("vocab alone", nullptr, (c.out.sizes = nullptr, c.out.report = nullptr, c.out.sizes_bytes = c.out.report_bytes = 0))
    EXPECT("sizes alone", nullptr, c.out.report = nullptr)
    EXPECT("report alone", nullptr, c.out.sizes = nullptr)
    EXPECT("a separate output", nullptr, c.out.vocab = (float*)((char*)c.desc + (1 << 20)))  // (never followed)
    EXPECT("rounds 1 and 64", nullptr, (c.P.rounds = 64, c.out.report_bytes = 64 * 16))
    EXPECT("largest", nullptr,
           (c.n_sets = 65535, c.S.cap = 65537, c.K = 65536, c.P.rounds = 64, c.out.vocab_bytes = (size_t)65536 * 512, c.out.sizes_bytes = 65536 * 4,
            c.out.report_bytes = 64 * 16))
    EXPECT("largest vocab - 1", "vocab buffer too small", (c.K = 65536, c.out.vocab_bytes = (size_t)65536 * 512 - 1, c.out.sizes_bytes = 65536 * 4))
    EXPECT("largest sizes - 1", "sizes buffer too small", (c.K = 65536, c.out.vocab_bytes = (size_t)65536 * 512, c.out.sizes_bytes = 65536 * 4 - 1))
    EXPECT("largest report - 1", "report buffer too small", (c.P.rounds = 64, c.out.report_bytes = 64 * 16 - 1))
    EXPECT("null sets", "null argument", c.s = nullptr)
    EXPECT("null vocab_in", "null argument", c.vocab_in = nullptr)
    EXPECT("null params", "null argument", c.p = nullptr)
    EXPECT("null out", "null argument", c.o = nullptr)
    EXPECT("struct_size", "out->struct_size is not sizeof(vslam_kmeans_out)", c.out.struct_size -= 8)
    EXPECT("rounds 0", "rounds must be 1 .. 64", c.P.rounds = 0)
    EXPECT("rounds 65", "rounds must be 1 .. 64", (c.P.rounds = 65, c.out.report_bytes = 65 * 16))
    EXPECT("reserved", "params->reserved must be 0", c.P.reserved = 1)
    EXPECT("sets < 0", "0 .. 65535 sets per call", c.n_sets = -1)
    EXPECT("sets 65536", "0 .. 65535 sets per call", c.n_sets = 65536)
    EXPECT("K 0", "1 .. 65536 words", c.K = 0)
    EXPECT("K 65537", "1 .. 65536 words", (c.K = 65537, c.out.vocab_bytes = (size_t)1 << 40, c.out.sizes_bytes = (size_t)1 << 40))
    EXPECT("desc", "a descriptor set needs desc, counts and a capacity", c.S.desc = nullptr)
    EXPECT("counts", "a descriptor set needs desc, counts and a capacity", c.S.counts = nullptr)
    EXPECT("cap", "a descriptor set needs desc, counts and a capacity", c.S.cap = 0)
    EXPECT("a set is asked for without sets too", "a descriptor set needs desc, counts and a capacity", (c.n_sets = 0, c.S.counts = nullptr))
    EXPECT("desc misaligned", "desc must be 16-byte aligned", c.S.desc = c.desc + 1)
    EXPECT("row ids 2^32 - 1", nullptr, (c.n_sets = 65535, c.S.cap = 65537))
    EXPECT("row ids 2^32", "n_sets * cap must fit 32 bits", (c.n_sets = 65536 / 2, c.S.cap = 1u << 17))
    EXPECT("row ids far past", "n_sets * cap must fit 32 bits", (c.n_sets = 65535, c.S.cap = 0xffffffffu))
    EXPECT("vocab_in misaligned", "vocab_in must be 16-byte aligned", (c.vocab_in = c.desc + 1, c.out.vocab = c.desc + 1))
    EXPECT("no vocab", "out->vocab is required", c.out.vocab = nullptr)
    EXPECT("vocab misaligned", "vocab must be 16-byte aligned", c.out.vocab = c.other + 1)
    EXPECT("host arrays need no alignment", nullptr, (c.device = false, c.S.desc = c.desc + 1, c.vocab_in = c.desc + 2, c.out.vocab = c.desc + 2))
    EXPECT("vocab small", "vocab buffer too small", c.out.vocab_bytes -= 1)
    EXPECT("sizes small", "sizes buffer too small", c.out.sizes_bytes -= 1)
    EXPECT("report small", "report buffer too small", c.out.report_bytes -= 1)
    EXPECT("report sized for 5 rounds with 6", "report buffer too small", c.P.rounds = 6)
    EXPECT("overlap from above", "vocab overlaps vocab_in without being vocab_in", c.out.vocab = c.desc + 4)
    EXPECT("overlap from below", "vocab overlaps vocab_in without being vocab_in", (c.vocab_in = c.desc + 4, c.out.vocab = c.desc + 0))
    EXPECT("overlap by the last byte", "vocab overlaps vocab_in without being vocab_in", (c.device = false, c.out.vocab = (float*)((char*)c.desc + 100 * 512 - 1)))
    EXPECT("adjacent", nullptr, (c.device = false, c.out.vocab = (float*)((char*)c.desc + 100 * 512)))
    EXPECT("null before struct_size", "null argument", (c.vocab_in = nullptr, c.out.struct_size = 0))
    EXPECT("struct_size before rounds", "out->struct_size is not sizeof(vslam_kmeans_out)", (c.out.struct_size = 0, c.P.rounds = 0))
    EXPECT("rounds before reserved", "rounds must be 1 .. 64", (c.P.rounds = 0, c.P.reserved = 1))
    EXPECT("reserved before sets", "params->reserved must be 0", (c.P.reserved = 1, c.n_sets = -1))
    EXPECT("sets before K", "0 .. 65535 sets per call", (c.n_sets = -1, c.K = 0))
    EXPECT("K before set", "1 .. 65536 words", (c.K = 0, c.S.desc = nullptr))
    EXPECT("set before row ids", "desc must be 16-byte aligned", (c.S.desc = c.desc + 1, c.n_sets = 65535, c.S.cap = 0xffffffffu))
    EXPECT("row ids before vocab_in", "n_sets * cap must fit 32 bits", (c.n_sets = 65535, c.S.cap = 0xffffffffu, c.vocab_in = c.desc + 1))
    EXPECT("vocab_in before vocab", "vocab_in must be 16-byte aligned", (c.vocab_in = c.desc + 1, c.out.vocab = nullptr))
    EXPECT("vocab before sizes", "vocab must be 16-byte aligned", (c.out.vocab = c.other + 1, c.out.vocab_bytes = 0))
    EXPECT("vocab bytes before sizes", "vocab buffer too small", (c.out.vocab_bytes = 0, c.out.sizes_bytes = 0))
    EXPECT("sizes before report", "sizes buffer too small", (c.out.sizes_bytes = 0, c.out.report_bytes = 0))
    EXPECT("report before overlap", "report buffer too small", (c.out.report_bytes = 0, c.out.vocab = c.desc + 4))
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}

// Host driver of tests/test_resect_refine_cpu.py: the argument checks and the grid and scratch sizing of
// vslam_resect_refine_dev (visualslam_amd/csrc/vslam_resect_refine_plan.h) without a GPU, built with
// -fsanitize=address,undefined.  It sweeps capacities up to 2^32 - 1 and pair counts up to 65535 and checks, per plan: every
// grid dimension within HIP's limits, the blocks cover the capacity, and every scratch size equal to its product computed in
// 128 bits (nothing wrapped).  Then every rejection of the ABI, over pointers it never follows, a buffer one record short for
// each output, the overlap rule, and the order of the checks: of two things wrong, which one is reported.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_resect_refine_plan.h"

using namespace vslam;

namespace {
struct Call {
    alignas(16) vslam_resect_corr rows[2];
    vslam_resect models_in[8];
    vslam_resect models[8];
    vslam_resect_refine info[1];
    uint64_t bits[1];
    vslam_resect_refine_params prm{4, 4.0, {800.0, 800.0, 960.0, 540.0}};
    vslam_resect_refine_out out{};
    uint32_t obs_cap = 70;
    int n_pairs = 3;
    bool aligned = true;
    const vslam_resect* mi = models_in;
    const vslam_resect_corr* cs = rows;
    const vslam_resect_refine_params* p = &prm;
    const vslam_resect_refine_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.models = models;
        out.models_bytes = 3 * sizeof(vslam_resect);
        out.info = info;
        out.info_bytes = 3 * sizeof(vslam_resect_refine);
        out.inlier_bits = bits;
        out.inlier_bits_bytes = 3 * 2 * 8;
    }
    const char* why() const { return resect_refine_check_args(mi, cs, obs_cap, n_pairs, p, o, aligned); }
    bool valid() const { return why() == nullptr; }
    bool says(const char* word) const { return why() && std::strstr(why(), word); }
};
}  // namespace

int main() {
    static_assert(sizeof(vslam_resect_refine) == 32 && sizeof(vslam_resect) == 120 && sizeof(vslam_resect_corr) == 48, "record layouts");
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xfffff000u, 0xfffff001u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    for (uint32_t cap : caps)
        for (int np : pairs) {
            const ResectRefinePlan p = resect_refine_plan(cap, np);
            const unsigned __int128 c = cap, n = (unsigned)np, lim = (unsigned __int128)1 << 63;
            plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np);
            plan.expect((unsigned __int128)p.sum_blocks * REFIT_BLOCK >= c && p.sum_blocks >= 1 && p.sum_blocks <= (1u << 20) &&
                            ((unsigned __int128)p.sum_blocks - 1) * REFIT_BLOCK < c, "sum_blocks", cap, np);
            plan.expect((unsigned __int128)p.row_blocks * REFIT_WG >= c && p.row_blocks >= 1 && p.row_blocks < (1u << 31) &&
                            ((unsigned __int128)p.row_blocks - 1) * REFIT_WG < c, "row_blocks", cap, np);
            const unsigned int word_blocks = (p.fwords + REFIT_WG - 1) / REFIT_WG;  // grid.x of the kernel that clears the words
            plan.expect(word_blocks >= 1 && (unsigned __int128)word_blocks * REFIT_WG >= p.fwords && word_blocks < (1u << 31), "word_blocks", cap, np);
            plan.expect(p.pair_blocks >= 1 && (unsigned __int128)p.pair_blocks * RR_PAIR_WG >= n && ((unsigned __int128)p.pair_blocks - 1) * RR_PAIR_WG < n,
                        "pair_blocks", cap, np);
            plan.expect(np <= 65535, "grid.y", cap, np);
            plan.expect((unsigned __int128)p.partial_elems == n * p.sum_blocks * RR_SUMS && (unsigned __int128)p.partial_elems * 8 < lim, "partial", cap, np);
            plan.expect(p.state_elems == (size_t)np && (unsigned __int128)p.state_elems * sizeof(RrState) < lim, "state", cap, np);
            // the last row a lane of the last block may index, and the last byte of the last pair's list, in 64 bits
            plan.expect(((unsigned __int128)p.sum_blocks * REFIT_BLOCK) < ((unsigned __int128)1 << 33) && n * c * sizeof(vslam_resect_corr) < lim, "row index", cap, np);
        }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no pairs");
        c.n_pairs = 1;
        args.expect(c.valid(), "one pair");
        c.n_pairs = 3;
        c.out.models = c.models_in;
        args.expect(c.valid(), "models aliased onto models_in");
        c.out.models = c.models;
        c.out.info = nullptr, c.out.inlier_bits = nullptr, c.out.info_bytes = c.out.inlier_bits_bytes = 0;
        args.expect(c.valid(), "models alone");
        for (uint32_t r = 1; r <= 8; ++r) {
            c.prm.rounds = r;
            args.expect(c.valid(), "rounds", r);
        }
        c.prm.K.cx = -1e300, c.prm.K.cy = 0.0, c.prm.K.fx = 5e-324;
        args.expect(c.valid(), "extreme intrinsics");
        c.cs = reinterpret_cast<const vslam_resect_corr*>(reinterpret_cast<const char*>(c.rows) + 8);
        args.expect(!c.valid() && c.says("aligned"), "an 8-byte aligned list on the device path");
        c.aligned = false;
        args.expect(c.valid(), "an 8-byte aligned list on the host path");
    }
    {
        Call c;
        c.n_pairs = 65535, c.obs_cap = 0xffffffffu;  // the largest call
        c.mi = reinterpret_cast<const vslam_resect*>((uintptr_t)1 << 40), c.out.models = reinterpret_cast<vslam_resect*>((uintptr_t)1 << 41);
        c.out.models_bytes = 65535 * sizeof(vslam_resect);
        c.out.info_bytes = 65535 * sizeof(vslam_resect_refine);
        c.out.inlier_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        args.expect(c.valid(), "largest");
        c.out.inlier_bits_bytes -= 1;
        args.expect(!c.valid() && c.says("inlier_bits"), "largest bits - 1");
        c.out.inlier_bits_bytes += 1, c.out.info_bytes -= 1;
        args.expect(!c.valid() && c.says("info"), "largest info - 1");
        c.out.info_bytes += 1, c.out.models_bytes -= 1;
        args.expect(!c.valid() && c.says("models buffer"), "largest models - 1");
        c.out.models_bytes += 1;
        args.expect(c.valid(), "largest again");
        // the overlap rule at the largest span: one record short of disjoint, either side
        const uintptr_t span = (uintptr_t)65535 * sizeof(vslam_resect), base = (uintptr_t)1 << 40;
        c.out.models = reinterpret_cast<vslam_resect*>(base + span);
        args.expect(c.valid(), "models right behind models_in");
        c.out.models = reinterpret_cast<vslam_resect*>(base + span - sizeof(vslam_resect));
        args.expect(!c.valid() && c.says("overlaps"), "models one record into models_in's end");
        c.out.models = reinterpret_cast<vslam_resect*>(base - span);
        args.expect(c.valid(), "models right before models_in");
        c.out.models = reinterpret_cast<vslam_resect*>(base - span + 8);
        args.expect(!c.valid() && c.says("overlaps"), "models_in eight bytes into models' end");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null models_in", c.mi = nullptr)
    REJECT("null correspondences", c.cs = nullptr)
    REJECT("null models", c.out.models = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("rounds 0", c.prm.rounds = 0)
    REJECT("rounds 9", c.prm.rounds = 9)
    REJECT("rounds max", c.prm.rounds = 0xffffffffu)
    REJECT("dist 0", c.prm.max_dist2 = 0.0)
    REJECT("dist -0", c.prm.max_dist2 = -0.0)
    REJECT("dist < 0", c.prm.max_dist2 = -4.0)
    REJECT("dist nan", c.prm.max_dist2 = std::nan(""))
    REJECT("dist inf", c.prm.max_dist2 = HUGE_VAL)
    REJECT("fx 0", c.prm.K.fx = 0.0)
    REJECT("fy < 0", c.prm.K.fy = -800.0)
    REJECT("fx nan", c.prm.K.fx = std::nan(""))
    REJECT("fy inf", c.prm.K.fy = HUGE_VAL)
    REJECT("cx nan", c.prm.K.cx = std::nan(""))
    REJECT("cy inf", c.prm.K.cy = -HUGE_VAL)
    REJECT("obs_cap 0", c.obs_cap = 0)
    REJECT("models one short", c.out.models_bytes = 3 * sizeof(vslam_resect) - 1)
    REJECT("info one short", c.out.info_bytes = 3 * sizeof(vslam_resect_refine) - 1)
    REJECT("bits one short", c.out.inlier_bits_bytes = 3 * 2 * 8 - 1)
    REJECT("overlap by one record", c.out.models = c.models_in + 1)
    REJECT("overlap from below", c.mi = c.models + 2)
    {
        // the order: null, struct_size, n_pairs, the parameters, the inputs, the buffers
        Call c;
        c.out.struct_size = 0, c.n_pairs = -1;
        args.expect(c.says("struct_size"), "struct_size before n_pairs");
        c.out.struct_size = sizeof(c.out), c.prm.rounds = 0;
        args.expect(c.says("pairs"), "n_pairs before rounds");
        c.n_pairs = 3, c.prm.max_dist2 = 0.0;
        args.expect(c.says("rounds"), "rounds before max_dist2");
        c.prm.rounds = 4, c.prm.K.fx = -1.0;
        args.expect(c.says("max_dist2"), "max_dist2 before the intrinsics");
        c.prm.max_dist2 = 4.0, c.obs_cap = 0;
        args.expect(c.says("fx and fy"), "the intrinsics before the inputs");
        c.prm.K.fx = 800.0, c.out.models = nullptr;
        args.expect(c.says("capacity"), "the inputs before the buffers");
        c.obs_cap = 70, c.out.info_bytes = 0;
        args.expect(c.says("models is required"), "models before info");
        c.out.models = c.models_in + 1;
        args.expect(c.says("info"), "the sizes before the overlap");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}

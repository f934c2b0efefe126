// Host driver of tests/test_chain_plan_cpu.py: the argument checks and the grid and scratch sizing of vslam_chain_dev
// (visualslam_amd/csrc/vslam_chain_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities and
// pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the record blocks cover the
// capacity, and every scratch size equal to its product computed in 128 bits (nothing wrapped).  Then every rejection of the
// ABI, over pointers it never follows, and the order the checks are made in.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_chain_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_pose poses[1];
    double points[3];
    uint64_t bits[1];
    vslam_chain_params prm{16};
    vslam_chain_out out{};
    uint32_t match_cap = 100, point_cap = 50;
    int n_pairs = 3;
    const vslam_pose* ps = poses;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const double* pt = points;
    const uint64_t* fb = bits;
    const vslam_chain_params* p = &prm;
    const vslam_chain_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.chain = reinterpret_cast<vslam_chain*>(matches);
        out.chain_bytes = 3 * sizeof(vslam_chain);
        out.map = reinterpret_cast<double*>(matches);
        out.map_bytes = 3 * 100 * 3 * sizeof(double);
        out.links = reinterpret_cast<int32_t*>(matches);
        out.links_bytes = 3 * 100 * sizeof(int32_t);
        out.ratios = reinterpret_cast<double*>(matches);
        out.ratios_bytes = 3 * 100 * sizeof(double);
    }
    const char* why() const { return chain_check_args(ps, m, mc, match_cap, pt, fb, point_cap, n_pairs, p, o); }
    bool valid() const { return why() == nullptr; }
};
}  // namespace

int main() {
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const uint32_t pcaps[] = {1, 512, 65536, 1u << 31, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const unsigned __int128 lim = (unsigned __int128)1 << 63;
    for (uint32_t cap : caps)
        for (uint32_t pcap : pcaps)
            for (int np : pairs) {
                const ChainPlan p = chain_plan(cap, pcap, np);
                const unsigned __int128 c = cap, pc = pcap, n = (unsigned)np;
                plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, pcap, np);
                plan.expect((unsigned __int128)p.rec_blocks * CHAIN_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                                ((unsigned __int128)p.rec_blocks - 1) * CHAIN_REC_WG < c, "rec_blocks", cap, pcap, np);
                // grid.y of k_chain_link and grid.x of k_chain_median: n_pairs - 1; grid.y of the other record kernels: n_pairs
                plan.expect(p.link_pairs == (unsigned)np - 1 && p.link_pairs <= 65534 && np <= 65535, "link_pairs", cap, pcap, np);
                plan.expect((unsigned __int128)p.table_elems == (n - 1) * pc && (unsigned __int128)p.table_elems * 4 < lim, "table", cap, pcap, np);
                plan.expect((unsigned __int128)p.key_elems == (n - 1) * c && (unsigned __int128)p.key_elems * 8 < lim, "keys", cap, pcap, np);
                plan.expect((unsigned __int128)p.pair_elems == n, "pair_elems", cap, pcap, np);
                // the four scratch buffers together, each rounded up to 256 bytes, and the largest index k_chain_map forms
                plan.expect((unsigned __int128)p.table_elems * 4 + (unsigned __int128)p.key_elems * 8 + n * 12 + 4 * 256 < lim, "scratch sum", cap, pcap, np);
                plan.expect(n * c * 24 < lim, "map", cap, pcap, np);
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
        c.out.map = nullptr, c.out.links = nullptr, c.out.ratios = nullptr;
        c.out.map_bytes = c.out.links_bytes = c.out.ratios_bytes = 0;
        c.n_pairs = 3;
        args.expect(c.valid(), "chain alone");
        c.prm.min_links = 0xffffffffu;
        args.expect(c.valid(), "largest min_links");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.point_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.chain_bytes = 65535 * sizeof(vslam_chain);
        c.out.map_bytes = (size_t)65535 * 0xffffffffu * 24;
        c.out.links_bytes = (size_t)65535 * 0xffffffffu * 4;
        c.out.ratios_bytes = (size_t)65535 * 0xffffffffu * 8;
        args.expect(c.valid(), "largest");
        // a buffer one record short, for each output
        c.out.map_bytes -= 24;
        args.expect(!c.valid(), "largest map - 1 record");
        c.out.map_bytes += 24, c.out.links_bytes -= 4;
        args.expect(!c.valid(), "largest links - 1 record");
        c.out.links_bytes += 4, c.out.ratios_bytes -= 8;
        args.expect(!c.valid(), "largest ratios - 1 record");
        c.out.ratios_bytes += 8, c.out.chain_bytes -= sizeof(vslam_chain);
        args.expect(!c.valid(), "largest chain - 1 record");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null poses", c.ps = nullptr)
    REJECT("null matches", c.m = nullptr)
    REJECT("null counts", c.mc = nullptr)
    REJECT("null points", c.pt = nullptr)
    REJECT("null bits", c.fb = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("min_links 0", c.prm.min_links = 0)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("point_cap 0", c.point_cap = 0)
    REJECT("no chain", c.out.chain = nullptr)
    REJECT("chain small", c.out.chain_bytes -= 1)
    REJECT("chain one record short", c.out.chain_bytes -= sizeof(vslam_chain))
    REJECT("map small", c.out.map_bytes -= 1)
    REJECT("map one record short", c.out.map_bytes -= 24)
    REJECT("links small", c.out.links_bytes -= 1)
    REJECT("links one record short", c.out.links_bytes -= 4)
    REJECT("ratios small", c.out.ratios_bytes -= 1)
    REJECT("ratios one record short", c.out.ratios_bytes -= 8)
    {
        // the ABI's order: null, struct_size, the pair count, the parameters, the inputs, the buffers - a call that fails every
        // check is repaired one step at a time, and each time the message is the next check's
        Call c;
        c.out.struct_size -= 8, c.n_pairs = -1, c.prm.min_links = 0, c.ps = nullptr, c.match_cap = 0, c.out.chain = nullptr, c.out.map_bytes = 0;
        const auto says = [&](const char* part) { const char* w = c.why(); return w && std::strstr(w, part); };
        args.expect(says("struct_size"), "order: struct_size");
        c.out.struct_size += 8;
        args.expect(says("pairs"), "order: pairs");
        c.n_pairs = 3;
        args.expect(says("min_links"), "order: min_links");
        c.prm.min_links = 1;
        args.expect(says("null input"), "order: null input");
        c.ps = c.poses;
        args.expect(says("capacity"), "order: capacity");
        c.match_cap = 100;
        args.expect(says("chain is required"), "order: chain");
        c.out.chain = reinterpret_cast<vslam_chain*>(c.matches);
        args.expect(says("map buffer"), "order: map");
        c.out.map_bytes = 3 * 100 * 24;
        args.expect(c.valid(), "order: repaired");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}

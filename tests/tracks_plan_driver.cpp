// Host driver of tests/test_tracks_cpu.py: the argument checks and the grid and scratch sizing of vslam_tracks_dev
// (visualslam_amd/csrc/vslam_tracks_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities and
// pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the record blocks cover the
// capacity, and every scratch size equal to its product computed in 128 bits (nothing wrapped).  Then every rejection of the
// ABI, over pointers it never follows, and the order the checks are made in.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cmath>
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_tracks_plan.h"

using namespace vslam;

namespace {
struct Call {
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_pose poses[1];
    uint64_t bits[1];
    vslam_chain chain[1];
    vslam_point frames[1];
    vslam_tracks_params prm{{800.0, 800.0, 960.0, 540.0}, 4.0, 2, 0};
    vslam_tracks_out out{};
    uint32_t match_cap = 100, point_cap = 50;
    int n_pairs = 3;
    const vslam_pose* ps = poses;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const uint64_t* fb = bits;
    const vslam_chain* ch = chain;
    const vslam_point* fp = frames;
    const vslam_tracks_params* p = &prm;
    const vslam_tracks_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.tracks = reinterpret_cast<vslam_track*>(matches);
        out.tracks_bytes = 3 * 100 * sizeof(vslam_track);
        out.refs = reinterpret_cast<vslam_track_ref*>(matches);
        out.refs_bytes = 3 * 100 * sizeof(vslam_track_ref);
        out.good_bits = reinterpret_cast<uint64_t*>(matches);
        out.good_bits_bytes = 3 * 2 * sizeof(uint64_t);
        out.summary = reinterpret_cast<vslam_track_summary*>(matches);
        out.summary_bytes = 3 * sizeof(vslam_track_summary);
    }
    const char* why() const { return tracks_check_args(ps, m, mc, match_cap, fb, point_cap, n_pairs, ch, fp, p, o); }
    bool valid() const { return why() == nullptr; }
};
}  // namespace

int main() {
    static_assert(sizeof(vslam_track) == 48 && sizeof(vslam_track_ref) == 8 && sizeof(vslam_track_summary) == 16, "record layouts");
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const uint32_t pcaps[] = {1, 512, 65536, 1u << 31, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const unsigned __int128 lim = (unsigned __int128)1 << 63;
    for (uint32_t cap : caps)
        for (uint32_t pcap : pcaps)
            for (int np : pairs) {
                const TracksPlan p = tracks_plan(cap, pcap, np);
                const unsigned __int128 c = cap, pc = pcap, n = (unsigned)np;
                plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, pcap, np);
                plan.expect((unsigned __int128)p.rec_blocks * TRK_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                                ((unsigned __int128)p.rec_blocks - 1) * TRK_REC_WG < c, "rec_blocks", cap, pcap, np);
                // grid.y of k_chain_link and k_trk_next: n_pairs - 1; grid.y of k_trk_walk and k_trk_rows: n_pairs
                plan.expect(p.link_pairs == (unsigned)np - 1 && p.link_pairs <= 65534 && np <= 65535, "link_pairs", cap, pcap, np);
                plan.expect((unsigned __int128)p.prev_elems == (n - 1) * pc && (unsigned __int128)p.prev_elems * 4 < lim, "prev", cap, pcap, np);
                plan.expect((unsigned __int128)p.next_elems == (n - 1) * c && (unsigned __int128)p.next_elems * 4 < lim, "next", cap, pcap, np);
                plan.expect((unsigned __int128)p.frame_elems == (n + 1) * pc && (unsigned __int128)p.frame_elems * 24 < lim, "frames", cap, pcap, np);
                // the two tables together are the header's (n_pairs - 1) * (point_cap + match_cap) * 4 bytes, each rounded up to 256
                plan.expect(((unsigned __int128)p.prev_elems + p.next_elems) * 4 == (n - 1) * (pc + c) * 4 && (n - 1) * (pc + c) * 4 + 2 * 256 < lim,
                            "scratch sum", cap, pcap, np);
                // the largest index the kernels form: a track row
                plan.expect(n * c * 48 < lim, "tracks", cap, pcap, np);
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
        c.out.refs = nullptr, c.out.good_bits = nullptr, c.out.summary = nullptr;
        c.out.refs_bytes = c.out.good_bits_bytes = c.out.summary_bytes = 0;
        c.n_pairs = 3;
        args.expect(c.valid(), "tracks alone");
        c.prm.min_views = 0xffffffffu;
        args.expect(c.valid(), "largest min_views");
        c.prm.K.cx = -1e300, c.prm.K.cy = 0.0, c.prm.max_dist2 = 5e-324;
        args.expect(c.valid(), "any finite principal point, the smallest max_dist2");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.point_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.tracks_bytes = (size_t)65535 * 0xffffffffu * 48;
        c.out.refs_bytes = (size_t)65535 * 0xffffffffu * 8;
        c.out.good_bits_bytes = (size_t)65535 * 67108864 * 8;
        c.out.summary_bytes = 65535 * sizeof(vslam_track_summary);
        args.expect(c.valid(), "largest");
        // a buffer one record short, for each output
        c.out.tracks_bytes -= 48;
        args.expect(!c.valid(), "largest tracks - 1 record");
        c.out.tracks_bytes += 48, c.out.refs_bytes -= 8;
        args.expect(!c.valid(), "largest refs - 1 record");
        c.out.refs_bytes += 8, c.out.good_bits_bytes -= 8;
        args.expect(!c.valid(), "largest good_bits - 1 word");
        c.out.good_bits_bytes += 8, c.out.summary_bytes -= sizeof(vslam_track_summary);
        args.expect(!c.valid(), "largest summary - 1 record");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null poses", c.ps = nullptr)
    REJECT("null matches", c.m = nullptr)
    REJECT("null counts", c.mc = nullptr)
    REJECT("null bits", c.fb = nullptr)
    REJECT("null chain", c.ch = nullptr)
    REJECT("null frame_points", c.fp = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("fx nan", c.prm.K.fx = NAN)
    REJECT("fx zero", c.prm.K.fx = 0.0)
    REJECT("fx negative", c.prm.K.fx = -800.0)
    REJECT("fy inf", c.prm.K.fy = INFINITY)
    REJECT("fy zero", c.prm.K.fy = 0.0)
    REJECT("cx nan", c.prm.K.cx = NAN)
    REJECT("cy inf", c.prm.K.cy = -INFINITY)
    REJECT("max_dist2 zero", c.prm.max_dist2 = 0.0)
    REJECT("max_dist2 negative", c.prm.max_dist2 = -1.0)
    REJECT("max_dist2 inf", c.prm.max_dist2 = INFINITY)
    REJECT("max_dist2 nan", c.prm.max_dist2 = NAN)
    REJECT("min_views 0", c.prm.min_views = 0)
    REJECT("min_views 1", c.prm.min_views = 1)
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("point_cap 0", c.point_cap = 0)
    REJECT("no tracks", c.out.tracks = nullptr)
    REJECT("tracks small", c.out.tracks_bytes -= 1)
    REJECT("tracks one record short", c.out.tracks_bytes -= 48)
    REJECT("refs small", c.out.refs_bytes -= 1)
    REJECT("refs one record short", c.out.refs_bytes -= 8)
    REJECT("good_bits small", c.out.good_bits_bytes -= 1)
    REJECT("good_bits one word short", c.out.good_bits_bytes -= 8)
    REJECT("summary small", c.out.summary_bytes -= 1)
    REJECT("summary one record short", c.out.summary_bytes -= 16)
    {
        // the ABI's order: null, struct_size, the pair count, the parameters, the inputs, the buffers - a call that fails every
        // check is repaired one step at a time, and each time the message is the next check's
        Call c;
        c.out.struct_size -= 8, c.n_pairs = -1, c.prm.K.fx = NAN, c.prm.K.fy = -1.0, c.prm.max_dist2 = 0.0, c.prm.min_views = 1, c.ch = nullptr, c.match_cap = 0;
        c.out.tracks = nullptr, c.out.refs_bytes = 0;
        const auto says = [&](const char* part) { const char* w = c.why(); return w && std::strstr(w, part); };
        args.expect(says("struct_size"), "order: struct_size");
        c.out.struct_size += 8;
        args.expect(says("pairs"), "order: pairs");
        c.n_pairs = 3;
        args.expect(says("finite"), "order: finite intrinsics");
        c.prm.K.fx = 800.0;
        args.expect(says("positive"), "order: positive focal lengths");
        c.prm.K.fy = 800.0;
        args.expect(says("max_dist2"), "order: max_dist2");
        c.prm.max_dist2 = 4.0;
        args.expect(says("min_views"), "order: min_views");
        c.prm.min_views = 2;
        args.expect(says("null input"), "order: null input");
        c.ch = c.chain;
        args.expect(says("capacity"), "order: capacity");
        c.match_cap = 100;
        args.expect(says("tracks is required"), "order: tracks");
        c.out.tracks = reinterpret_cast<vslam_track*>(c.matches);
        args.expect(says("refs buffer"), "order: refs");
        c.out.refs_bytes = 3 * 100 * 8;
        args.expect(c.valid(), "order: repaired");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}

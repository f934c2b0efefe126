// Host driver of tests/test_bundle_cpu.py: the argument checks and the grid and scratch sizing of vslam_bundle_dev
// (visualslam_amd/csrc/vslam_bundle_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps capacities and
// pair counts up to their extremes and checks, per plan: every grid dimension within HIP's limits, the blocks of the ordered
// sum cover the 2 * match_cap rows a camera can have, and every scratch size equal to its product computed in 128 bits
// (nothing wrapped).  Then every rejection of the ABI, over pointers it never follows, and the order the checks are made in.
//   driver          one line: "plan checked=N bad=B first=..." and "args checked=N bad=B first=..."
#include <cmath>
#include <cstdio>
#include <cstring>

#include "plan_driver.h"
#include "vslam_bundle_plan.h"

using namespace vslam;

namespace {
// an address `bytes` from p, formed as an integer: the checks compare addresses and never follow them
const vslam_track* apart(const vslam_track* p, long bytes) { return reinterpret_cast<const vslam_track*>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes); }

struct Call {
    vslam_track rows[4];  // tracks_in and tracks point here: equal pointers are allowed
    vslam_match matches[1];
    uint32_t counts[1];
    vslam_pose poses[1];
    uint64_t bits[1];
    vslam_chain chain[1];
    vslam_point frames[1];
    vslam_track_ref refs[1];
    vslam_bundle_params prm{{800.0, 800.0, 960.0, 540.0}, 4.0, 2, 4};
    vslam_bundle_out out{};
    uint32_t match_cap = 100, point_cap = 50;
    int n_pairs = 3;
    const vslam_pose* ps = poses;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const uint64_t* fb = bits;
    const vslam_chain* ch = chain;
    const vslam_point* fp = frames;
    const vslam_track* ti = rows;
    const vslam_track_ref* rf = refs;
    const vslam_bundle_params* p = &prm;
    const vslam_bundle_out* o = &out;
    Call() {
        // sizes of a valid call; the pointers are never followed by the checks
        out.struct_size = sizeof(out);
        out.tracks = rows;
        out.tracks_bytes = 3 * 100 * sizeof(vslam_track);
        out.cams = reinterpret_cast<vslam_bundle_cam*>(matches);
        out.cams_bytes = 3 * sizeof(vslam_bundle_cam);
        out.point_info = reinterpret_cast<vslam_bundle_point*>(matches);
        out.point_info_bytes = 3 * 100 * sizeof(vslam_bundle_point);
        out.member_bits = reinterpret_cast<uint64_t*>(matches);
        out.member_bits_bytes = 3 * 2 * 2 * sizeof(uint64_t);
    }
    const char* why() const { return bundle_check_args(ps, m, mc, match_cap, fb, point_cap, n_pairs, ch, fp, ti, rf, p, o); }
    bool valid() const { return why() == nullptr; }
};
}  // namespace

int main() {
    static_assert(sizeof(vslam_bundle_cam) == 160 && sizeof(vslam_bundle_point) == 40 && sizeof(vslam_bundle_params) == 48 && sizeof(BaCam) == 240,
                  "record layouts");
    Tally plan;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 1000, 2047, 2048, 2049, 4096, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const uint32_t pcaps[] = {1, 512, 65536, 1u << 31, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const unsigned __int128 lim = (unsigned __int128)1 << 63;
    for (uint32_t cap : caps)
        for (uint32_t pcap : pcaps)
            for (int np : pairs) {
                const BundlePlan p = bundle_plan(cap, pcap, np);
                const TracksPlan t = tracks_plan(cap, pcap, np);
                const unsigned __int128 c = cap, n = (unsigned)np, rows = 2 * c;
                // the tables and the record grid are the tracks stage's
                plan.expect(p.trk.fwords == t.fwords && p.trk.rec_blocks == t.rec_blocks && p.trk.link_pairs == t.link_pairs && p.trk.prev_elems == t.prev_elems &&
                                p.trk.next_elems == t.next_elems && p.trk.rec_blocks < (1u << 31) && np <= 65535,
                            "tracks plan", cap, pcap, np);
                // grid.x of k_ba_cam_pass covers the 2 * match_cap rows a camera can have, with no block to spare
                plan.expect((unsigned __int128)p.sum_blocks * REFIT_BLOCK >= rows && ((unsigned __int128)p.sum_blocks - 1) * REFIT_BLOCK < rows &&
                                p.sum_blocks >= 1 && p.sum_blocks < (1u << 31),
                            "sum_blocks", cap, pcap, np);
                plan.expect((unsigned __int128)p.pair_blocks * RR_PAIR_WG >= n && ((unsigned __int128)p.pair_blocks - 1) * RR_PAIR_WG < n, "pair_blocks", cap, pcap, np);
                // the header's n_pairs * ((2 * match_cap + 4095) / 4096) * 232 bytes of block sums and n_pairs * 240 bytes of state
                plan.expect((unsigned __int128)p.partial_elems == n * ((rows + 4095) / 4096) * 29 && (unsigned __int128)p.partial_elems * 8 < lim, "partial", cap, pcap, np);
                plan.expect((unsigned __int128)p.state_elems == n && sizeof(BaCam) == 240, "state", cap, pcap, np);
                plan.expect((unsigned __int128)p.partial_elems * 8 + n * 240 + ((unsigned __int128)p.trk.prev_elems + p.trk.next_elems) * 4 + 4 * 256 < lim, "scratch sum", cap,
                            pcap, np);
                // the largest indices the kernels form: a track row, a point_info row, a member_bits word
                plan.expect(n * c * 48 < lim && n * 2 * p.trk.fwords * 8 < lim, "outputs", cap, pcap, np);
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
        c.out.point_info = nullptr, c.out.member_bits = nullptr;
        c.out.point_info_bytes = c.out.member_bits_bytes = 0;
        c.n_pairs = 3;
        args.expect(c.valid(), "tracks and cams alone");
        c.prm.min_views = 0xffffffffu, c.prm.sweeps = 1;
        args.expect(c.valid(), "largest min_views, one sweep");
        c.prm.sweeps = 64;
        args.expect(c.valid(), "64 sweeps");
        c.prm.K.cx = -1e300, c.prm.K.cy = 0.0, c.prm.max_dist2 = 5e-324;
        args.expect(c.valid(), "any finite principal point, the smallest max_dist2");
        // tracks apart from tracks_in by the whole buffer or more: allowed; by less: refused (below)
        c.ti = apart(c.out.tracks, 3 * 100 * (long)sizeof(vslam_track));
        args.expect(c.valid(), "tracks_in right behind tracks");
        c.ti = apart(c.out.tracks, -3 * 100 * (long)sizeof(vslam_track));
        args.expect(c.valid(), "tracks right behind tracks_in");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.point_cap = 0xffffffffu;  // the largest call: the byte sizes it needs, as size_t
        c.out.tracks_bytes = (size_t)65535 * 0xffffffffu * 48;
        c.out.cams_bytes = (size_t)65535 * 160;
        c.out.point_info_bytes = (size_t)65535 * 0xffffffffu * 40;
        c.out.member_bits_bytes = (size_t)65535 * 2 * 67108864 * 8;
        args.expect(c.valid(), "largest");
        // a buffer one record short, for each output
        c.out.tracks_bytes -= 48;
        args.expect(!c.valid(), "largest tracks - 1 record");
        c.out.tracks_bytes += 48, c.out.cams_bytes -= 160;
        args.expect(!c.valid(), "largest cams - 1 record");
        c.out.cams_bytes += 160, c.out.point_info_bytes -= 40;
        args.expect(!c.valid(), "largest point_info - 1 record");
        c.out.point_info_bytes += 40, c.out.member_bits_bytes -= 8;
        args.expect(!c.valid(), "largest member_bits - 1 word");
        c.out.member_bits_bytes += 8;
        args.expect(c.valid(), "largest again");
    }
    REJECT("null params", c.p = nullptr)
    REJECT("null out", c.o = nullptr)
    REJECT("null poses", c.ps = nullptr)
    REJECT("null matches", c.m = nullptr)
    REJECT("null counts", c.mc = nullptr)
    REJECT("null bits", c.fb = nullptr)
    REJECT("null chain", c.ch = nullptr)
    REJECT("null frame_points", c.fp = nullptr)
    REJECT("null tracks_in", c.ti = nullptr)
    REJECT("null refs", c.rf = nullptr)
    REJECT("null tracks", c.out.tracks = nullptr)
    REJECT("null cams", c.out.cams = nullptr)
    REJECT("struct_size", c.out.struct_size -= 8)
    REJECT("pairs < 0", c.n_pairs = -1)
    REJECT("pairs > 65535", c.n_pairs = 65536)
    REJECT("sweeps 0", c.prm.sweeps = 0)
    REJECT("sweeps 65", c.prm.sweeps = 65)
    REJECT("sweeps max", c.prm.sweeps = 0xffffffffu)
    REJECT("min_views 0", c.prm.min_views = 0)
    REJECT("min_views 1", c.prm.min_views = 1)
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
    REJECT("match_cap 0", c.match_cap = 0)
    REJECT("point_cap 0", c.point_cap = 0)
    REJECT("tracks 1 byte short", c.out.tracks_bytes -= 1)
    REJECT("cams 1 byte short", c.out.cams_bytes -= 1)
    REJECT("point_info 1 byte short", c.out.point_info_bytes -= 1)
    REJECT("member_bits 1 byte short", c.out.member_bits_bytes -= 1)
    REJECT("tracks one row behind tracks_in", c.ti = c.rows + 1)
    REJECT("tracks_in one byte into tracks", c.ti = apart(c.rows, 1))
    REJECT("tracks_in the last row of tracks",
           c.ti = apart(c.out.tracks, -(3 * 100 - 1) * (long)sizeof(vslam_track)))
    // the order of the checks: null, struct_size, n_pairs, the parameters (sweeps, min_views, max_dist2, the intrinsics), the inputs, the buffers
    auto first = [&](const char* want, auto change) {
        Call c;
        change(c);
        const char* why = c.why();
        args.expect(why && std::strstr(why, want), want);
    };
    first("struct_size", [](Call& c) { c.out.struct_size = 0, c.n_pairs = -1; });
    first("pairs", [](Call& c) { c.n_pairs = -1, c.prm.sweeps = 0; });
    first("sweeps", [](Call& c) { c.prm.sweeps = 0, c.prm.min_views = 0; });
    first("min_views", [](Call& c) { c.prm.min_views = 0, c.prm.max_dist2 = NAN; });
    first("max_dist2", [](Call& c) { c.prm.max_dist2 = NAN, c.prm.K.fx = NAN; });
    first("intrinsics", [](Call& c) { c.prm.K.fx = NAN, c.ps = nullptr; });
    first("null input", [](Call& c) { c.ps = nullptr, c.match_cap = 0; });
    first("capacity", [](Call& c) { c.match_cap = 0, c.out.tracks = nullptr; });
    first("tracks is required", [](Call& c) { c.out.tracks = nullptr, c.out.cams = nullptr; });
    first("tracks buffer", [](Call& c) { c.out.tracks_bytes = 0, c.out.cams = nullptr; });
    first("cams is required", [](Call& c) { c.out.cams = nullptr, c.out.point_info_bytes = 0; });
    first("cams buffer", [](Call& c) { c.out.cams_bytes = 0, c.out.point_info_bytes = 0; });
    first("point_info", [](Call& c) { c.out.point_info_bytes = 0, c.out.member_bits_bytes = 0; });
    first("member_bits", [](Call& c) { c.out.member_bits_bytes = 0, c.ti = c.rows + 1; });
    first("overlaps", [](Call& c) { c.ti = c.rows + 1; });
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return plan.bad || args.bad ? 1 : 0;
}

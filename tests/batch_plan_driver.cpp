// Host program of tests/test_batch_plan_cpu.py: the plan of one chunk of a batch call (csrc/vslam_batch_plan.h) for one
// shape, as text, or for the exhaustive sweep, as fixed-size binary records (the sweep has about 1.5 million shapes).
//   driver case nf n_octaves n_tiled lat_variant scan_variant flags   ->  one line of key=value
//   driver sweep                                                       ->  Rec after Rec on stdout
//   driver recsize                                                     ->  sizeof(Rec)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "vslam_batch_plan.h"

using namespace vslam;

enum Flag : unsigned {
    DOG = 1, HARRIS = 2, EXTREMA = 4, LISTS = 8, LOCALIZE = 16, ORIENT = 32, DENSE = 64, WINDOW5 = 128, MX = 256, BASES_SCRATCH = 512,
    SIDE = 1024, CAPTURING = 2048, LATER = 4096, UP2_OK = 8192, ALL_FLAGS = 16383,
};

// The octaves: a tiled prefix of n_tiled (what plan_octave can produce: none, octave 0, octaves 0 and 1); lattice variant
// 0 = every octave has sites, 1 = the last has none; scan variant 0 = every matrix configuration scans, 1 = those of
// octaves 0 and 1 only, 2 = none.
static BatchPlanIn make_in(int nf, int n_oct, int n_tiled, int latv, int scnv, unsigned f) {
    BatchPlanIn in;
    in.nf = nf;
    in.n_octaves = n_oct;
    for (int o = 0; o < n_oct; ++o) {
        in.tiled[o] = o < n_tiled;
        in.lattice[o] = latv == 0 || o != n_oct - 1;
        in.scan_ok[o] = scnv == 0 || (scnv == 1 && o < 2);
    }
    in.up2_ok = f & UP2_OK;
    in.dog = f & DOG, in.harris = f & HARRIS, in.do_extrema = f & EXTREMA, in.lists = f & LISTS;
    in.localize = f & LOCALIZE, in.orient = f & ORIENT, in.extrema_dense = f & DENSE;
    in.extrema_window = (f & WINDOW5) ? 5 : 3;
    in.mx = f & MX, in.bases_are_scratch = f & BASES_SCRATCH, in.side = f & SIDE, in.capturing = f & CAPTURING, in.later_chunk = f & LATER;
    return in;
}

// What the ABI admits (vslam_detect_batch_dev, make_layout): lists come with scans; the dense test needs window 3 and neither
// localize nor orient; orient needs localize, window 3 and the lists; without the DoG path nothing of it is set.
static bool admitted(unsigned f) {
    if (!(f & DOG)) return !(f & (EXTREMA | LISTS | LOCALIZE | ORIENT | DENSE | WINDOW5 | MX | BASES_SCRATCH | UP2_OK));
    if ((f & LISTS) && !(f & EXTREMA)) return false;
    if ((f & DENSE) && (f & (WINDOW5 | LOCALIZE | ORIENT))) return false;
    if ((f & ORIENT) && (!(f & LOCALIZE) || (f & WINDOW5) || !(f & LISTS))) return false;
    return true;
}

struct Rec {
    int16_t nf, n_oct, n_tiled, latv, scnv;
    uint16_t flags;
    int16_t gate, harris_lane, harris_after, scan_lane, ev_oct, up2_fused, nf_a, up_lane, up_waits_chunk, ev_chunk;
    uint16_t fused;  // bit o
    int16_t sitemap, wait_pack, early_edge, early_edge_forked, spread;
    uint32_t after_lo, after_hi;  // after[oo] in 4 bits each, octaves 0..7 and 8..15
};
static_assert(sizeof(Rec) == 52 && VSLAM_MAX_OCTAVES == 16, "the record of tests/test_batch_plan_cpu.py");

static Rec record(int nf, int n_oct, int n_tiled, int latv, int scnv, unsigned f) {
    const BatchPlan p = batch_plan(make_in(nf, n_oct, n_tiled, latv, scnv, f));
    Rec r{};
    r.nf = (int16_t)nf, r.n_oct = (int16_t)n_oct, r.n_tiled = (int16_t)n_tiled, r.latv = (int16_t)latv, r.scnv = (int16_t)scnv, r.flags = (uint16_t)f;
    r.gate = (int16_t)p.gate, r.harris_lane = (int16_t)p.harris_lane, r.harris_after = (int16_t)p.harris_after, r.scan_lane = (int16_t)p.scan_lane;
    r.ev_oct = p.ev_oct, r.up2_fused = p.up2_fused, r.nf_a = (int16_t)p.nf_a, r.up_lane = (int16_t)p.up_lane, r.up_waits_chunk = p.up_waits_chunk;
    r.ev_chunk = p.ev_chunk, r.sitemap = p.sitemap, r.wait_pack = p.wait_pack;
    r.early_edge = p.early_edge, r.early_edge_forked = p.early_edge_forked, r.spread = p.spread;
    for (int o = 0; o < VSLAM_MAX_OCTAVES; ++o) {
        if (p.fused[o]) r.fused |= (uint16_t)(1u << o);
        (o < 8 ? r.after_lo : r.after_hi) |= (uint32_t)(p.after[o] & 15) << (4 * (o & 7));
    }
    return r;
}

int main(int argc, char** argv) {
    const std::string_view mode = argc > 1 ? argv[1] : "";
    if (mode == "recsize") return std::printf("%zu\n", sizeof(Rec)) < 0;
    if (mode == "case" && argc == 8) {
        int a[6];
        for (int i = 0; i < 6; ++i) a[i] = std::atoi(argv[2 + i]);
        if (a[0] < 1 || a[1] < 0 || a[1] > VSLAM_MAX_OCTAVES || a[2] < 0 || a[2] > a[1]) return 2;
        const Rec r = record(a[0], a[1], a[2], a[3], a[4], (unsigned)a[5] & ALL_FLAGS);
        std::printf("gate=%d harris_lane=%d harris_after=%d scan_lane=%d after=", r.gate, r.harris_lane, r.harris_after, r.scan_lane);
        for (int o = 0; o < a[1]; ++o) std::printf("%s%u", o ? "," : "", ((o < 8 ? r.after_lo : r.after_hi) >> (4 * (o & 7))) & 15);
        std::printf(" ev_oct=%d up2_fused=%d nf_a=%d up_lane=%d up_waits_chunk=%d ev_chunk=%d fused=%u sitemap=%d wait_pack=%d early_edge=%d "
                    "early_edge_forked=%d spread=%d\n", r.ev_oct, r.up2_fused, r.nf_a, r.up_lane, r.up_waits_chunk, r.ev_chunk, r.fused, r.sitemap,
                    r.wait_pack, r.early_edge, r.early_edge_forked, r.spread);
        return 0;
    }
    if (mode != "sweep") return 2;
    std::vector<Rec> out;
    for (int nf : {1, 31, 32, 63, 64, 65, 255, 256})
        for (unsigned f = 0; f <= ALL_FLAGS; ++f) {
            if (!admitted(f)) continue;
            // (without the DoG path the layout has no octaves)
            for (int n_oct = (f & DOG) ? 1 : 0; n_oct <= ((f & DOG) ? VSLAM_MAX_OCTAVES : 0); ++n_oct)
                for (int n_tiled = 0; n_tiled <= 2 && n_tiled <= n_oct; ++n_tiled)
                    for (int v = 0; v < ((f & MX) ? 3 : 1); ++v)  // (the lattice and the scan support feed the matrix path's plan only)
                        out.push_back(record(nf, n_oct, n_tiled, v == 1, v, f));
            if (out.size() >= 4096) {
                if (std::fwrite(out.data(), sizeof(Rec), out.size(), stdout) != out.size()) return 1;
                out.clear();
            }
        }
    return std::fwrite(out.data(), sizeof(Rec), out.size(), stdout) != out.size();
}

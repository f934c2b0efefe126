// Host driver of tests/test_hdiff_staging_cpu.py: the per-thread staging bounds of k_gauss_h_diff
// (visualslam_amd/csrc/vslam_octave_launch.h) swept without a GPU.  The kernel holds a level's staging in a fixed
// number of registers per thread - two interior items, one tail item, hd_halo_trips() halo items, LDS indices packed
// in 16 bits - and checks nothing at run time: an item beyond those is silently not staged.
//
//   driver sweep     every width the difference form is used at x every row-pair count up to hd_max_pairs, both
//                    geometries; then strip_launch over rows x batch sizes: it returns nothing above hd_max_pairs
#include <cstdio>
#include <cstring>
#include <set>

#include "diff_taps.gen.h"
#include "vslam_octave_launch.h"

using namespace vslam;

namespace {

struct Hd {
    int nmax, rmax, HL;
};
template <int O>
constexpr Hd hd_geom() {
    return Hd{dtaps::Lvl<O, 5>::n, dtaps::Lvl<O, 5>::n / 2, hd_left_halo(dtaps::Lvl<O, 5>::n / 2)};
}

struct Sweep {
    long checked = 0, launches = 0, bad = 0;
    char first[200] = "";
    int max_interior = 0, max_tail = 0, max_halo[2] = {0, 0};
    std::set<int> npairs;
    void fail(const char* what, int cols, int np, int g) {
        if (!bad++) std::snprintf(first, sizeof first, "%s:cols=%d,npairs=%d,geom=%d", what, cols, np, g);
    }
};

int per_thread(long items) { return (int)((items + 255) / 256); }

int sweep() {
    const Hd hds[2] = {hd_geom<2>(), hd_geom<3>()};
    Sweep sw;
    for (int cols = 1; cols <= 4200; ++cols) {
        if (!hdiff_fits(cols)) {
            if (cols <= 4096) sw.fail("fits_to_4096", cols, 0, 0);
            continue;
        }
        if (cols > 4096) sw.fail("fits_beyond_4096", cols, 0, 0);
        if (!hdiff_stage_fits(cols)) sw.fail("stage_fits", cols, 0, 0);
        const int ncs = (cols + HD_J - 1) / HD_J;
        for (int np = 1; np <= hd_max_pairs(cols); ++np)
            for (int g = 0; g < 2; ++g) {
                ++sw.checked;
                const Hd& hd = hds[g];
                const int nh = hd_halo_cols(cols, hd.HL, hd.rmax), pw = hd_pw(cols, hd.HL, hd.rmax);
                if ((long)np * ncs > 256) sw.fail("items", cols, np, g);
                const int in = per_thread((long)np * (cols >> 3)), tl = per_thread((long)np * (cols & 7)), ha = per_thread((long)np * nh);
                if (in > 2) sw.fail("interior", cols, np, g);
                if (tl > 1) sw.fail("tail", cols, np, g);
                if (ha > hd_halo_trips(hd.HL, hd.rmax)) sw.fail("halo", cols, np, g);
                // every staged column is interior, tail or halo, and the halo is what hd_pw sized the row for
                if (8 * (cols >> 3) + (cols & 7) + nh != hd.HL + HD_J * ncs + hd.rmax || nh < hd.HL + hd.rmax) sw.fail("partition", cols, np, g);
                // LDS indices of the halo copies are packed in 16 bits, 0xffff standing for "no item"
                if ((size_t)np * pw * 8 <= (size_t)kMaxDynLds && (long)np * pw >= 0xffff) sw.fail("index16", cols, np, g);
                sw.max_interior = in > sw.max_interior ? in : sw.max_interior;
                sw.max_tail = tl > sw.max_tail ? tl : sw.max_tail;
                sw.max_halo[g] = ha > sw.max_halo[g] ? ha : sw.max_halo[g];
            }
        // what strip_launch returns lies in the range swept above
        for (int rows : {1, 2, 3, 7, 16, 17, 33, 68, 135, 270, 540, 1080, 2400})
            for (int nf : {1, 2, 3, 8, 31, 64, 255, 256})
                for (int g = 0; g < 2; ++g) {
                    const Hd& hd = hds[g];
                    const int sh = strip_plan_sh(rows, cols, hd.nmax);
                    if (!sh) continue;
                    ++sw.launches;
                    const StripLaunch s = strip_launch(rows, cols, nf, sh, true, hd.nmax, hd.HL, hd.rmax);
                    if (!s.diff || s.npairs < 1 || s.npairs > hd_max_pairs(cols)) sw.fail("launch_npairs", cols, s.npairs, g);
                    if (s.h_lds > (size_t)kMaxDynLds || s.h_lds / 8 >= 0xffff) sw.fail("launch_lds", cols, s.npairs, g);
                    sw.npairs.insert(s.npairs);
                }
    }
    std::printf("sweep checked=%ld launches=%ld bad=%ld first=%s interior=%d tail=%d halo=%d,%d trips=%d,%d npairs=", sw.checked, sw.launches, sw.bad,
                sw.bad ? sw.first : "-", sw.max_interior, sw.max_tail, sw.max_halo[0], sw.max_halo[1], hd_halo_trips(hds[0].HL, hds[0].rmax),
                hd_halo_trips(hds[1].HL, hds[1].rmax));
    for (int n : sw.npairs) std::printf("%d,", n);
    std::printf("\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    std::fprintf(stderr, "usage: %s sweep\n", argv[0]);
    return 2;
}

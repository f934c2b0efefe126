// Host driver of tests/test_octave_launch_cpu.py: the launch choice of the coarse-octave strip kernels
// (visualslam_amd/csrc/vslam_octave_launch.h) swept and queried without a GPU.  Linked with vslam_params.cpp, which gives
// the octave sizes and the trimmed kernel widths of a (frame shape, octaves, sigma0) exactly as the library plans them.
//
//   driver sweep                                   the invariants over the whole sweep, one summary line
//   driver widest                                  widest cols that selects each RI at 16 rows per strip
//   driver plan (NF ROWS COLS N_OCT SIGMA0 HDIFF)...  per batch "case i", then one line per octave (HDIFF 0: the dot2 pass everywhere)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "diff_taps.gen.h"
#include "vslam_internal.h"
#include "vslam_octave_launch.h"

using namespace vslam;

namespace {

// geometry of the two k_gauss_h_diff instantiations (HdGeom<O> of kernels_hdiff.hip.h: level 5 is the widest)
struct Hd {
    int nmax, rmax, HL;
};
template <int O>
constexpr Hd hd_geom() {
    return Hd{dtaps::Lvl<O, 5>::n, dtaps::Lvl<O, 5>::n / 2, hd_left_halo(dtaps::Lvl<O, 5>::n / 2)};
}

template <int O, int L>
bool level_matches(const std::vector<uint16_t>& t) {
    using LV = dtaps::Lvl<O, L>;
    if ((int)t.size() != LV::n) return false;
    for (int k = 0; k < LV::n; ++k)
        if (t[k] != LV::w[k]) return false;
    return true;
}
template <int O>
bool octave_matches(const std::vector<uint16_t> (&t)[6]) {
    return level_matches<O, 0>(t[0]) && level_matches<O, 1>(t[1]) && level_matches<O, 2>(t[2]) && level_matches<O, 3>(t[3]) &&
           level_matches<O, 4>(t[4]) && level_matches<O, 5>(t[5]);
}

bool is_instantiated(int SH, int RI) {
    static const int k[6][2] = {{16, 4}, {16, 2}, {16, 1}, {8, 4}, {4, 4}, {4, 1}};
    for (const auto& p : k)
        if (p[0] == SH && p[1] == RI) return true;
    return false;
}

struct Sweep {
    long checked = 0, plans = 0, bad = 0;
    char first[256] = "";
    std::set<std::pair<int, int>> pairs;
    std::set<int> splits, npairs;
    void fail(const char* what, int rows, int cols, int nf, int nmax, const StripLaunch& s) {
        if (!bad++)
            std::snprintf(first, sizeof first, "%s:rows=%d,cols=%d,nf=%d,nmax=%d,diff=%d,npairs=%d,SH=%d,RI=%d,gy=%d,hlds=%zu,vlds=%zu,split=%d", what, rows,
                          cols, nf, nmax, (int)s.diff, s.npairs, s.SH, s.RI, s.h_grid_y, s.h_lds, s.v_lds, s.lsplit);
    }
    void check(int rows, int cols, int nf, int nmax, const Hd* hd) {
        ++checked;
        const int sh = strip_plan_sh(rows, cols, nmax);
        if (cols > 4096 && sh) {
            StripLaunch none{};
            fail("plan_beyond_4096", rows, cols, nf, nmax, none);
        }
        if (!sh || (hd && !hdiff_fits(cols))) return;
        ++plans;
        const StripLaunch s = hd ? strip_launch(rows, cols, nf, sh, true, nmax, hd->HL, hd->rmax) : strip_launch(rows, cols, nf, sh, false, nmax);
        if (s.lsplit != 1 && s.lsplit != 2 && s.lsplit != 3 && s.lsplit != 6) fail("split", rows, cols, nf, nmax, s);
        if (s.v_lds > (size_t)kMaxDynLds) fail("v_lds", rows, cols, nf, nmax, s);
        if (s.h_lds > (size_t)kMaxDynLds) fail("h_lds", rows, cols, nf, nmax, s);
        splits.insert(s.lsplit);
        if (s.diff != (hd != nullptr)) fail("form", rows, cols, nf, nmax, s);
        if (s.diff) {
            if (s.npairs < 1 || s.npairs > 8) fail("npairs_range", rows, cols, nf, nmax, s);
            if ((long)s.npairs * ((cols + 15) / 16) > 256) fail("diff_items", rows, cols, nf, nmax, s);
            if ((long)s.h_grid_y * 2 * s.npairs < rows) fail("diff_grid", rows, cols, nf, nmax, s);
            if (s.h_lds != (size_t)s.npairs * hd_pw(cols, hd->HL, hd->rmax) * 8) fail("diff_lds_formula", rows, cols, nf, nmax, s);
            npairs.insert(s.npairs);
        } else {
            if (!is_instantiated(s.SH, s.RI)) {
                fail("pair", rows, cols, nf, nmax, s);
                return;
            }
            if ((long)((cols + 7) / 8) * (s.SH / s.RI) > strip_item_capacity(s.RI)) fail("dot2_items", rows, cols, nf, nmax, s);
            if ((long)s.h_grid_y * s.SH < rows) fail("dot2_grid", rows, cols, nf, nmax, s);
            if (s.h_lds != (size_t)s.SH * strip_pw(cols, nmax) * 4) fail("dot2_lds_formula", rows, cols, nf, nmax, s);
            pairs.insert({s.SH, s.RI});
        }
    }
};

int sweep() {
    std::vector<int> rows_list;
    for (int r = 1; r <= 70; ++r) rows_list.push_back(r);
    for (int r : {135, 270, 540, 1080, 2160, 2400}) rows_list.push_back(r);
    const int nfs[] = {1, 2, 3, 8, 28, 29, 31, 32, 63, 64, 128, 255, 256};
    // kernel widths: the narrowest a strip octave can have, the widest of the default pyramid's octaves 3 and 5, and STRIP_MAXN
    const int nmaxs[] = {9, 245, 977, 2047};
    const Hd hds[] = {hd_geom<2>(), hd_geom<3>()};
    Sweep sw;
    for (int cols = 1; cols <= 4200; ++cols)
        for (int rows : rows_list)
            for (int nf : nfs) {
                for (int nmax : nmaxs) sw.check(rows, cols, nf, nmax, nullptr);
                for (const Hd& hd : hds) sw.check(rows, cols, nf, hd.nmax, &hd);
            }
    std::printf("sweep checked=%ld plans=%ld bad=%ld first=%s pairs=", sw.checked, sw.plans, sw.bad, sw.bad ? sw.first : "-");
    for (const auto& p : sw.pairs) std::printf("%d/%d,", p.first, p.second);
    std::printf(" splits=");
    for (int s : sw.splits) std::printf("%d,", s);
    std::printf(" npairs=");
    for (int n : sw.npairs) std::printf("%d,", n);
    std::printf("\n");
    return 0;
}

int widest() {
    int w[5] = {};
    for (int cols = 1; cols <= 1024; ++cols) {
        const StripLaunch s = strip_launch(1080, cols, 256, strip_plan_sh(1080, cols, 9), false, 9);
        if (s.SH != 16) return 1;
        w[s.RI] = cols;
    }
    std::printf("widest ri1=%d ri2=%d ri4=%d\n", w[1], w[2], w[4]);
    return 0;
}

int plan(int nf, int rows, int cols, int n_oct, double sigma0, bool hdiff_on) {
    vslam_params p;
    vslam_params_default(&p, rows, cols);
    p.n_octaves = n_oct;
    p.sigma0 = sigma0;
    vslam_batch_layout L;
    if (vslam_batch_layout_query(&p, &L) != 0) return 1;
    for (int o = 0; o < L.n_octaves; ++o) {
        std::vector<uint16_t> taps[6];
        int ke[6], nmax = 0;
        bool u8 = true;
        for (int l = 0; l < 6; ++l) {
            const double sg = sigma_at(sigma0, o, l);
            if (!gauss_taps_q8_trimmed(gauss_ksize_u8(sg), sg, taps[l])) return 1;
            ke[l] = (int)taps[l].size();
            nmax = ke[l] > nmax ? ke[l] : nmax;
            for (uint16_t v : taps[l]) u8 = u8 && v <= 255;
        }
        const int r = L.rows[o], c = L.cols[o];
        const int sh = u8 && nmax <= 2047 ? strip_plan_sh(r, c, nmax) : 0;
        const int hd = !sh || !hdiff_fits(c) ? 0 : octave_matches<2>(taps) ? 2 : octave_matches<3>(taps) ? 3 : 0;
        std::printf("oct o=%d rows=%d cols=%d ke=%d,%d,%d,%d,%d,%d sh=%d hd=%d wide=%d", o, r, c, ke[0], ke[1], ke[2], ke[3], ke[4], ke[5], sh, hd,
                    (int)pyr_tile_wide(r, c));
        if (sh) {
            const Hd g = hd == 2 ? hd_geom<2>() : hd_geom<3>();
            const StripLaunch s = hd && hdiff_on ? strip_launch(r, c, nf, sh, true, nmax, g.HL, g.rmax) : strip_launch(r, c, nf, sh, false, nmax);
            const long items = s.diff ? (long)s.npairs * ((c + 15) / 16) : (long)((c + 7) / 8) * (s.SH / s.RI);
            std::printf(" diff=%d npairs=%d SH=%d RI=%d split=%d gy=%d hlds=%zu vlds=%zu items=%ld cap=%d", (int)s.diff, s.npairs, s.SH, s.RI, s.lsplit,
                        s.h_grid_y, s.h_lds, s.v_lds, items, s.diff ? 256 : strip_item_capacity(s.RI));
        }
        std::printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 2 && !std::strcmp(argv[1], "widest")) return widest();
    if (argc >= 8 && (argc - 2) % 6 == 0 && !std::strcmp(argv[1], "plan")) {
        for (int i = 2; i < argc; i += 6) {
            std::printf("case %d\n", (i - 2) / 6);
            if (plan(std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]), std::atoi(argv[i + 3]), std::atof(argv[i + 4]), std::atoi(argv[i + 5]) != 0))
                return 1;
        }
        return 0;
    }
    std::fprintf(stderr, "usage: %s sweep | widest | plan (NF ROWS COLS N_OCT SIGMA0 HDIFF)...\n", argv[0]);
    return 2;
}

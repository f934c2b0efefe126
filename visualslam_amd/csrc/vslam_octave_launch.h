// The launch choices of the pyramid's octave kernels, apart from HIP: which coarse-octave ("strip") kernels run an octave
// of `rows` x `cols` for `nf` frames, in which instantiation, on which grid and with how much dynamic LDS, and which tile
// shape k_pyr_octave takes.  No HIP header is included: vslam_hip.hip asks here and launches what comes back, the kernels
// take their geometry constants from here, and tests/test_octave_launch_cpu.py sweeps the same code on the host
// (tests/octave_launch_driver.cpp) - every instantiation that can be chosen has to hold the items it is given, and
// nothing but this arithmetic keeps it so.
#pragma once
#include <algorithm>
#include <cstddef>
#include <initializer_list>

namespace vslam {

constexpr int STRIP_W = 64;  // columns per vertical-pass workgroup (k_gauss_v_strip)
constexpr int HD_J = 16;     // outputs per lane and row of the difference-form horizontal pass (k_gauss_h_diff)
constexpr int HD_PAD = 2;    // ... and its LDS columns of padding after every 16
constexpr int kMaxDynLds = 150 * 1024;  // the most dynamic LDS any launch asks for (raise_dyn_lds)

// ---- vertical pass ---------------------------------------------------------------------------------------------------
// RM: rows of reflect-101 margin staged above and below the image (a multiple of 4, >= nmax / 2); rhq: dword rows staged.
struct StripVGeom {
    int RM, rhq;
    size_t lds;
};
constexpr StripVGeom strip_v_geom(int rows, int nmax) {
    const int RM = (nmax / 2 + 3) & ~3;
    const int rhq = (((rows + 3) & ~3) + 2 * RM + 16) / 4;
    return StripVGeom{RM, rhq, (size_t)rhq * STRIP_W * 4};
}

// ---- horizontal pass, dot2 form (k_gauss_h_strip<SH, RI>) ------------------------------------------------------------
// u16-pair columns of one staged row (left halo + ceil(cols/8) groups + right halo of the widest kernel), a multiple of 4
constexpr int strip_pw(int cols, int nmax) { return ((cols + 7) / 2 + nmax / 2 + 12 + 3) & ~3; }

// Items (8 columns x RI rows) one workgroup of k_gauss_h_strip<SH, RI> computes: NI per thread, NI = 2 for RI == 4 and
// 4 otherwise (the kernel asserts NI * 256 == this).  An item beyond it is not computed.
constexpr int strip_item_capacity(int RI) { return RI == 4 ? 512 : 1024; }

// Rows per horizontal strip workgroup by width (SH rows x ceil(cols/8) column groups in items of 4 rows <= 512); 0: too wide
constexpr int strip_sh(int cols) { return cols <= 1024 ? 16 : cols <= 2048 ? 8 : cols <= 4096 ? 4 : 0; }

// The strip kernels can run the octave at all: the ladder's rows per workgroup, or 0 (the generic kernels run it).
constexpr int strip_plan_sh(int rows, int cols, int nmax) {
    const int sh = strip_sh(cols);
    return sh && strip_v_geom(rows, nmax).lds <= (size_t)kMaxDynLds && (size_t)sh * strip_pw(cols, nmax) * 4 <= (size_t)kMaxDynLds ? sh : 0;
}

// ---- horizontal pass, difference form (k_gauss_h_diff<O>) ------------------------------------------------------------
// left halo of an octave whose widest kernel has radius rmax (>= rmax + 2: the window may start one column early to stay
// 16-byte aligned)
constexpr int hd_left_halo(int rmax) { return (rmax + 2 + 15) & ~15; }
// float2 columns of one staged row pair: left halo + 16 per segment + right halo, padded; a multiple of 16 + HD_PAD
constexpr int hd_pw(int cols, int HL, int rmax) {
    const int ccount = HL + 16 * ((cols + HD_J - 1) / HD_J) + rmax;
    return (ccount + 1 + 15) / 16 * (16 + HD_PAD);  // + 1: the last read of a window may take one column past the staged ones
}
// one item (row pair x 16 columns) per thread: a single row pair must fit the 256 threads
constexpr bool hdiff_fits(int cols) { return (cols + HD_J - 1) / HD_J <= 256; }
// the most row pairs a workgroup takes at this width (strip_launch starts here and only goes down)
constexpr int hd_max_pairs(int cols) { return std::max(1, std::min(8, 256 / ((cols + HD_J - 1) / HD_J))); }
// The kernel keeps the next level's staging loads in registers while it computes this one, a fixed number per thread:
//   - interior items (8 columns of a row pair): at most TWO.  npairs <= 256 / ncs and cols >> 3 <= 2 ncs
//     (ncs = ceil(cols / 16)), so npairs * (cols >> 3) <= 512;
//   - tail items (one of the cols & 7 columns past the last group of 8, of a row pair): at most one, 8 * 7 <= 256;
//   - halo items (one column of a row pair's reflect-101 extension, copied inside LDS): at most hd_halo_trips().
// plan_octave keeps k_gauss_h_strip where this does not hold (nowhere today: tests/test_hdiff_staging_cpu.py sweeps it).
constexpr int hd_halo_cols(int cols, int HL, int rmax) { return HL + HD_J * ((cols + HD_J - 1) / HD_J) - cols + rmax; }
constexpr int hd_halo_trips(int HL, int rmax) { return (8 * (HL + HD_J - 1 + rmax) + 255) / 256; }
constexpr bool hdiff_stage_fits(int cols) { return hd_max_pairs(cols) * (cols >> 3) <= 2 * 256 && hd_max_pairs(cols) * (cols & 7) <= 256; }

// ---- the strip octave's two launches ---------------------------------------------------------------------------------
struct StripLaunch {
    int lsplit;    // vertical pass: workgroups the six levels are split over (1, 2, 3 or 6) = its grid's y extent
    size_t v_lds;  // vertical pass: dynamic LDS
    bool diff;     // horizontal pass: the difference form with `npairs` row pairs per workgroup ...
    int npairs;
    int SH, RI;    // ... or the dot2 form k_gauss_h_strip<SH, RI> (<4, 1>: the small-launch form)
    int h_grid_y;  // horizontal pass: grid y extent
    size_t h_lds;  // horizontal pass: dynamic LDS
    int pw;        // staged row (pair) length the horizontal kernel is given
};

// `sh`: strip_plan_sh() of the octave (> 0); `nmax`: its widest trimmed kernel; `hdiff`: the octave's taps are those of a
// k_gauss_h_diff instantiation whose geometry is (hd_HL, hd_rmax), and hdiff_fits(cols).
inline StripLaunch strip_launch(int rows, int cols, int nf, int sh, bool hdiff, int nmax, int hd_HL = 0, int hd_rmax = 0) {
    StripLaunch s{};
    s.v_lds = strip_v_geom(rows, nmax).lds;
    // small batches: split the six levels over workgroups until the launch has >= 256 of them
    const int strips = (cols + STRIP_W - 1) / STRIP_W;
    const int want = (256 + strips * nf - 1) / (strips * nf);
    s.lsplit = want >= 6 ? 6 : want >= 3 ? 3 : want >= 2 ? 2 : 1;
    if (hdiff) {
        s.pw = hd_pw(cols, hd_HL, hd_rmax);
        // row pairs per workgroup: at most 256 items (one per thread), LDS below the limit, and >= 256 workgroups for small batches
        int npairs = hd_max_pairs(cols);
        while (npairs > 1 && ((size_t)npairs * s.pw * 8 > (size_t)kMaxDynLds || (long)((rows + 2 * npairs - 1) / (2 * npairs)) * nf < 256)) --npairs;
        s.diff = true;
        s.npairs = npairs;
        s.h_grid_y = (rows + 2 * npairs - 1) / (2 * npairs);
        s.h_lds = (size_t)npairs * s.pw * 8;
        return s;
    }
    s.pw = strip_pw(cols, nmax);
    // small batches: shorter row strips, more workgroups
    while (sh > 4 && (long)((rows + sh - 1) / sh) * nf < 256) sh >>= 1;
    int ri = 4;
    // ... and, when even that leaves most threads without an item, one row per item
    if (sh == 4 && (long)((rows + 3) / 4) * nf < 256 && ((cols + 7) / 8) * 4 <= 512) {
        ri = 1;
    } else if (sh == 16) {
        // rows per item (round 5): the items of a workgroup should fill whole waves.  960 columns x 16 rows are 480 items of 8
        // columns x 4 rows = 7.5 waves (every eighth wave-instruction wasted: the kernel runs AT its VALU issue time), but 960
        // items of 2 rows = 15 waves; 480 columns need 1 row per item.  Fewer rows per item amortise the scalar tap loads over
        // fewer dots, so the smaller item must be at least 2 % fuller to be chosen.
        const int ncg = (cols + 7) / 8;
        auto waste = [&](int r) {
            const long items = (long)ncg * (16 / r);
            if (items > strip_item_capacity(r)) return 1e9;
            return (double)((items + 63) / 64 * 64 - items) / (double)items;
        };
        for (int r : {2, 1})
            if (waste(r) + 0.02 < waste(ri)) ri = r;
    }
    s.SH = sh;
    s.RI = ri;
    s.h_grid_y = (rows + sh - 1) / sh;
    s.h_lds = (size_t)sh * s.pw * 4;
    return s;
}

// ---- k_pyr_octave ------------------------------------------------------------------------------------------------------
// tile shape: the wide tile (256 x 32) when it needs no more tile area than the tall one (128 x 64).
// A 384 x 32 tile (1920 = 5 x 384) on 384-thread workgroups was measured in round 3: six waves per
// workgroup sit 2-2-1-1 on the four SIMDs and meet at every barrier: 21.3 vs 18.3 ms per step.
constexpr bool pyr_tile_wide(int rows, int cols) {
    return (long)((cols + 255) / 256) * ((rows + 31) / 32) <= (long)((cols + 127) / 128) * ((rows + 63) / 64);
}

}  // namespace vslam

// The launch geometry of the single-pass Harris kernel (k_harris_strip, kernels_harris_strip.hip.h), apart from HIP: how
// many 240-column wave strips a frame has, into how many row segments each strip is cut, on which grid they run, which
// form of the kernel (aligned / any width) takes the frame, and how many keypoint-flag words the frame needs.  No HIP
// header is included: vslam_hip.hip asks here and launches what comes back, the kernel takes its strip constants from
// here, and tests/test_harris_launch_cpu.py sweeps the same code on the host (tests/harris_launch_driver.cpp).  The
// kernel trusts this arithmetic: a wave beyond nstrips * nseg returns at once, a row beyond the last segment is never
// finalised, and the flag buffer holds exactly the words counted here.
#pragma once
#include <algorithm>
#include <cstddef>

namespace vslam {

constexpr int HS_VALID_LANES = 60;              // lanes 2..61 of a wave store; 0, 1, 62, 63 only feed their neighbours
constexpr int HS_STRIP_W = 4 * HS_VALID_LANES;  // 240 output columns per wave strip
constexpr int HS_WAVES = 4;                     // independent waves (strip x segment items) per 256-thread workgroup
constexpr int HS_MIN_SEG = 16;                  // rows of a segment at least: each pays a 9-row pipeline fill
constexpr long HS_WANT_WAVES = 12288;           // waves a launch aims for: enough to fill the chip several times over

constexpr int harris_nstrips(int cols) { return (cols + HS_STRIP_W - 1) / HS_STRIP_W; }

// Words of keypoint-flag scratch per frame: 4 ballot words (one per pixel slot of a lane) per strip row.
constexpr size_t harris_flag_words(int rows, int cols) { return (size_t)rows * harris_nstrips(cols) * 4; }

struct HarrisLaunch {
    int nstrips;        // wave strips per row
    int seg, nseg;      // rows per segment, segments per strip: nseg * seg >= rows > (nseg - 1) * seg
    unsigned grid_x;    // workgroups of HS_WAVES waves: grid = (grid_x, 1, frames)
    bool aligned;       // k_harris_strip<false>: every row of every frame starts on a dword; else the any-width form
    size_t flag_words;  // harris_flag_words(rows, cols): the per-frame stride of the flag buffer
};

// `fframe`: bytes from one frame to the next (rows are dense: cols bytes each).
inline HarrisLaunch harris_launch(int rows, int cols, int nf, size_t fframe) {
    HarrisLaunch g{};
    g.aligned = cols % 4 == 0 && fframe % 4 == 0;
    g.nstrips = harris_nstrips(cols);
    g.flag_words = harris_flag_words(rows, cols);
    // enough waves to fill the chip several times over, long enough strips to amortise the 9-row pipeline fill
    const long want_seg = std::max<long>(1, HS_WANT_WAVES / ((long)g.nstrips * nf));
    g.seg = (int)std::min<long>(rows, std::max<long>(HS_MIN_SEG, (rows + want_seg - 1) / want_seg));
    g.nseg = (rows + g.seg - 1) / g.seg;
    g.grid_x = (unsigned)((g.nstrips * g.nseg + HS_WAVES - 1) / HS_WAVES);
    return g;
}

}  // namespace vslam

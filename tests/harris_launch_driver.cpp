// Host driver of tests/test_harris_launch_cpu.py: the launch geometry of k_harris_strip (visualslam_amd/csrc/vslam_harris_launch.h)
// swept and queried without a GPU.
//
//   driver sweep                              the invariants over the whole sweep: one summary line, then per image height one line
//                                             "rows R seg S1,S2,..." with every segment length some plan of the sweep gives R rows
//   driver plan (NF ROWS COLS FSTRIDE)...     one line of fields per launch (FSTRIDE: bytes between frames)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "vslam_harris_launch.h"

using namespace vslam;

namespace {

std::vector<int> sweep_cols() {
    std::set<int> s;
    for (int c = 1; c <= 1000; ++c) s.insert(c);
    for (int k = 1; HS_STRIP_W * k - 1 <= 4096; ++k)
        for (int d = -1; d <= 9; ++d)
            if (HS_STRIP_W * k + d <= 4096) s.insert(HS_STRIP_W * k + d);
    return std::vector<int>(s.begin(), s.end());
}

int sweep() {
    const int nfs[] = {1, 2, 3, 31, 32, 64, 255, 256};
    const std::vector<int> cols_list = sweep_cols();
    long checked = 0, bad = 0;
    char first[200] = "-";
    std::vector<std::set<int>> segs(1201);
    auto fail = [&](const char* what, int rows, int cols, int nf, size_t fframe, const HarrisLaunch& g) {
        if (!bad++)
            std::snprintf(first, sizeof first, "%s:rows=%d,cols=%d,nf=%d,fframe=%zu,nstrips=%d,seg=%d,nseg=%d,grid_x=%u,aligned=%d,flag_words=%zu", what, rows,
                          cols, nf, fframe, g.nstrips, g.seg, g.nseg, g.grid_x, (int)g.aligned, g.flag_words);
    };
    for (int rows = 1; rows <= 1200; ++rows)
        for (int cols : cols_list)
            for (int nf : nfs)
                for (int pad = 0; pad <= 4; ++pad) {  // dense frames, and gaps of 1..4 bytes between them
                    const size_t fframe = (size_t)rows * cols + pad;
                    const HarrisLaunch g = harris_launch(rows, cols, nf, fframe);
                    ++checked;
                    if (g.nstrips < 1 || (long)g.nstrips * HS_STRIP_W < cols || (long)(g.nstrips - 1) * HS_STRIP_W >= cols) fail("nstrips", rows, cols, nf, fframe, g);
                    if (g.seg < 1 || g.seg > rows) fail("seg_range", rows, cols, nf, fframe, g);
                    if (g.nseg < 1 || (long)g.nseg * g.seg < rows || (long)(g.nseg - 1) * g.seg >= rows) fail("nseg", rows, cols, nf, fframe, g);
                    if ((long)g.grid_x * HS_WAVES < (long)g.nstrips * g.nseg || g.grid_x < 1) fail("grid", rows, cols, nf, fframe, g);
                    if (((long)g.grid_x - 1) * HS_WAVES >= (long)g.nstrips * g.nseg) fail("grid_idle_workgroup", rows, cols, nf, fframe, g);
                    if (g.flag_words != (size_t)rows * g.nstrips * 4 || g.flag_words != harris_flag_words(rows, cols)) fail("flag_words", rows, cols, nf, fframe, g);
                    if (g.aligned != (cols % 4 == 0 && fframe % 4 == 0)) fail("aligned", rows, cols, nf, fframe, g);
                    if (g.seg >= 1 && g.seg <= rows) segs[rows].insert(g.seg);
                }
    std::printf("sweep checked=%ld bad=%ld ncols=%zu first=%s\n", checked, bad, cols_list.size(), first);
    for (int rows = 1; rows <= 1200; ++rows) {
        std::printf("rows %d seg ", rows);
        for (int s : segs[rows]) std::printf("%d,", s);
        std::printf("\n");
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc >= 6 && (argc - 2) % 4 == 0 && !std::strcmp(argv[1], "plan")) {
        for (int i = 2; i < argc; i += 4) {
            const int nf = std::atoi(argv[i]), rows = std::atoi(argv[i + 1]), cols = std::atoi(argv[i + 2]);
            const HarrisLaunch g = harris_launch(rows, cols, nf, (size_t)std::strtoull(argv[i + 3], nullptr, 10));
            std::printf("plan nf=%d rows=%d cols=%d nstrips=%d seg=%d nseg=%d grid_x=%u aligned=%d flag_words=%zu\n", nf, rows, cols, g.nstrips, g.seg, g.nseg,
                        g.grid_x, (int)g.aligned, g.flag_words);
        }
        return 0;
    }
    std::fprintf(stderr, "usage: %s sweep | plan (NF ROWS COLS FSTRIDE)...\n", argv[0]);
    return 2;
}

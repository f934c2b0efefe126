// What the searches over descriptor rows share (kernels_match.hip.h: the matcher; kernels_match_guided.hip.h and
// kernels_match_guided_hf.hip.h: the guided passes): the tiling constants, the partial result of one workgroup for one query row,
// the exact merge of two such results, and what the guided passes know about a row beyond its descriptor.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"

namespace vslam {

constexpr int MT_Q = 128;  // query rows per workgroup: 32 per wave
constexpr int MT_T = 64;   // train rows per LDS tile: two 32-column MFMA blocks
// floats per LDS row.  128 would put every row on the same banks; + 4 spreads the 16 lanes that one ds_read_b128 cycle
// serves over all 64 banks (lane j starts at bank 4 j mod 64, and no two lanes of a group are 16 apart)
constexpr int MT_LD = 132;
constexpr int MT_MAX_SPLIT = 16;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MatchPart {  // what one workgroup knows about one query row
    float best, second;
    int index;
};

__device__ __forceinline__ float match_inf() { return __int_as_float(0x7f800000); }

// (b, s, i) <- the nearest two of the union of two disjoint sets of train rows
__device__ __forceinline__ void match_merge(float& b, float& s, int& i, float ob, float os, int oi) {
    const bool win = ob < b || (ob == b && (unsigned int)oi < (unsigned int)i);
    const float loser = win ? b : ob;
    float ns = os < s ? os : s;
    ns = loser < ns ? loser : ns;
    b = win ? ob : b;
    i = win ? oi : i;
    s = ns;
}

__device__ __forceinline__ double guided_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// The two-view section's coordinates of a point, exact; false: the point's octave is outside 0 .. 31
__device__ __forceinline__ bool guided_xy(const vslam_point& p, double& x, double& y) {
    if ((unsigned int)p.octave > 31u) return false;
    const double s = p.octave == 0 ? 0.5 : (double)(1u << (p.octave - 1));
    x = (double)((long long)p.col - (long long)p.padding) * s;
    y = (double)((long long)p.row - (long long)p.padding) * s;
    return true;
}

struct GuidedQn {  // the f32 side of a query row in LDS
    float norm;
    int octave;
};

}  // namespace vslam

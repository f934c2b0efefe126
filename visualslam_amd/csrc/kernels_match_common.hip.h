// What the two searches over descriptor rows share (kernels_match.hip.h: the matcher; kernels_match_guided.hip.h: the guided
// pass): the tiling constants, the partial result of one workgroup for one query row, and the exact merge of two such results.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace vslam

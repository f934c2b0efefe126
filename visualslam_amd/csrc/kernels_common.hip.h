// Device primitives shared by the kernel headers: leaf code only (__device__ __forceinline__ / constexpr), no kernels, so
// every translation unit - the matrix-path units too - can include it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vslam {

// cv::borderInterpolate(p, len, BORDER_REFLECT_101), repeated until inside.
__device__ __forceinline__ int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- two u16 in a dword (the v_pk_*_u16 operand shape) and the dot products ------------------------------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t udot4(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_udot4(a, b, c, false);
}
__device__ __forceinline__ uint32_t udot2(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b), c, false);
}
// packed u16 saturating subtract (v_pk_sub_u16 clamp)
__device__ __forceinline__ uint32_t pk_sub_sat_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_sub_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_min_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_lshr_u16(uint32_t a, int sh) {
    return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) >> (unsigned short)sh));
}

// ---- 4x4 byte transpose ----------------------------------------------------------------------------------------------
// r0..r3 = four pixels of four consecutive rows; result .x/.y/.z/.w = column 0..3, each holding its four rows in byte
// order - the operand shape of a vertical dot4.  Eight v_perm.
__device__ __forceinline__ uint4 transpose4x4_u8(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
    const uint32_t p01l = __builtin_amdgcn_perm(r1, r0, 0x05010400), p01h = __builtin_amdgcn_perm(r1, r0, 0x07030602);
    const uint32_t p23l = __builtin_amdgcn_perm(r3, r2, 0x05010400), p23h = __builtin_amdgcn_perm(r3, r2, 0x07030602);
    uint4 t;
    t.x = __builtin_amdgcn_perm(p23l, p01l, 0x05040100);
    t.y = __builtin_amdgcn_perm(p23l, p01l, 0x07060302);
    t.z = __builtin_amdgcn_perm(p23h, p01h, 0x05040100);
    t.w = __builtin_amdgcn_perm(p23h, p01h, 0x07060302);
    return t;
}

// ---- level epilogue ------------------------------------------------------------------------------------------------
// Four horizontal sums s0..s3 of one Gaussian level -> the four pixels G = s >> 16 (byte 2 of each sum) as one dword.
// The even / odd pixels are picked straight into 16-bit lanes (the shape the saturating subtract wants), then
// interleaved.  From level 1 on d = D_{L-1} = saturate_u8(G_L - G_{L-1}), GaussPyramid.cpp:197, against the previous level's lanes
// in prev_e / prev_o, which then take this level's.
__device__ __forceinline__ void level_pack4(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, int level, uint32_t& g, uint32_t& d,
                                            uint32_t& prev_e, uint32_t& prev_o) {
    const uint32_t e = __builtin_amdgcn_perm(s2, s0, 0x0c060c02);  // (G0, G2)
    const uint32_t o = __builtin_amdgcn_perm(s3, s1, 0x0c060c02);  // (G1, G3)
    g = __builtin_amdgcn_perm(o, e, 0x06020400);  // bytes (e0, o0, e1, o1): interleave in one v_perm
    if (level > 0) d = __builtin_amdgcn_perm(pk_sub_sat_u16(o, prev_o), pk_sub_sat_u16(e, prev_e), 0x06020400);
    prev_e = e;
    prev_o = o;
}
// The even bytes of (lo, hi): a 2:1 decimated row piece (the next octave's base from Gaussian[3]).  Eight pixels as two
// dwords or their four even ones as two (G0, G2) lane pairs give the same four bytes.
__device__ __forceinline__ uint32_t even_bytes(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x06040200); }

// ---- XCD-aware tile order ------------------------------------------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (b and b+8 share an L2), so the linear id is remapped to give every
// XCD one contiguous run of tiles - row-major neighbours, which share their halo rows and columns, then meet in the same
// 4 MB L2 instead of each fetching the halo from HBM.  Placement is a speed matter only.
// grid = (tiles x, tiles y, frames) -> frame fz, tile row by, tile column bx of this workgroup.
// (block and grid are the caller's blockIdx and gridDim: read inside this function, the compiler forms the grid-size
// product with its operands the other way round and schedules the calling kernel differently)
__device__ __forceinline__ void xcd_tile_id(const dim3 block, const dim3 grid, unsigned int& fz, unsigned int& by, unsigned int& bx) {
    unsigned int bid = block.x + grid.x * (block.y + grid.y * block.z);
    const unsigned int per_xcd = (grid.x * grid.y * grid.z) >> 3;
    if (bid < (per_xcd << 3)) bid = (bid & 7u) * per_xcd + (bid >> 3);
    const unsigned int tiles_per_frame = grid.x * grid.y;
    fz = bid / tiles_per_frame;
    const unsigned int rem = bid - fz * tiles_per_frame;
    by = rem / grid.x, bx = rem - by * grid.x;
}

// ---- Sobel (ksize 1) differences of a u8 Gaussian level at one pixel, reflect-101 neighbours -----------------------
// (processGradients, GaussPyramid.cpp:65-104: integers, exact in f32)
__device__ __forceinline__ void gradient_at(const uint8_t* __restrict__ G, int gpitch, int rows, int cols, int r, int c, float& x, float& y) {
    x = (float)((int)G[(size_t)r * gpitch + reflect101(c + 1, cols)] - (int)G[(size_t)r * gpitch + reflect101(c - 1, cols)]);
    y = (float)((int)G[(size_t)reflect101(r + 1, rows) * gpitch + c] - (int)G[(size_t)reflect101(r - 1, rows) * gpitch + c]);
}

// ---- tile staging ----------------------------------------------------------------------------------------------------
// Four pixels of one image row at columns x .. x+3 under BORDER_REFLECT_101: one dword load where the four lie inside the
// row, one dword load of the mirrored run with its bytes reversed where they lie wholly in the first reflection on either
// side, byte by byte (repeated reflection) only where they straddle an edge or the row is shorter than the halo.
__device__ __forceinline__ uint32_t load4_reflect101(const uint8_t* __restrict__ row, int x, int cols) {
    if (x >= 0 && x + 3 < cols) return *reinterpret_cast<const uint32_t*>(row + x);
    if (x + 3 < 0 && -x < cols) {  // columns x..x+3 mirror to -x, -x-1, -x-2, -x-3 (all >= 1)
        uint32_t v;
        __builtin_memcpy(&v, row + (-x - 3), 4);
        return __builtin_amdgcn_perm(0u, v, 0x00010203);
    }
    if (x >= cols && 2 * (cols - 1) - x - 3 >= 0) {  // mirror to 2(cols-1)-x, ... - 3 (all <= cols - 2)
        uint32_t v;
        __builtin_memcpy(&v, row + (2 * (cols - 1) - x - 3), 4);
        return __builtin_amdgcn_perm(0u, v, 0x00010203);
    }
    return (uint32_t)row[reflect101(x, cols)] | ((uint32_t)row[reflect101(x + 1, cols)] << 8) | ((uint32_t)row[reflect101(x + 2, cols)] << 16) |
           ((uint32_t)row[reflect101(x + 3, cols)] << 24);
}

// Stages the TW x TH tile at (tile_x0, tile_y0) with halo R into rp[(TH + 2R) / 4][RWP] dwords, BYTE-TRANSPOSED (a dword =
// 4 vertically adjacent pixels of one column), BORDER_REFLECT_101 resolved at fill time (valid for every level because the
// taps are symmetric), every byte ^ bias (0x80808080: pixels - 128 as signed bytes).  NT threads; R a multiple of 16 and
// the tile origin 16-byte aligned.  The 4 pad dwords per row quad are left uninitialised.
// UNROLL: items in flight per thread in the border branch.
template <int TW, int TH, int R, int RWP, int NT, int UNROLL>
__device__ __forceinline__ void stage_tile_transposed(const uint8_t* __restrict__ src, int rows, int cols, int pitch, int tile_x0, int tile_y0,
                                                      uint32_t* __restrict__ rp, uint32_t bias) {
    constexpr int RW = TW + 2 * R, RQ = (TH + 2 * R) / 4;
    const int tid = threadIdx.x;
    auto transposed = [&](uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
        uint4 t = transpose4x4_u8(r0, r1, r2, r3);
        t.x ^= bias, t.y ^= bias, t.z ^= bias, t.w ^= bias;
        return t;
    };
    const bool interior = tile_x0 - R >= 0 && tile_x0 + TW + R <= cols && tile_y0 - R >= 0 && tile_y0 + TH + R <= rows;
    if (interior) {
        // 16 pixels x 4 rows per item: 16-byte coalesced loads, four 4x4 byte transposes, four 16-byte LDS stores
        for (int it = tid; it < RQ * (RW / 16); it += NT) {
            const int yq = it / (RW / 16), xs = it - yq * (RW / 16);
            const uint8_t* p = src + (size_t)(tile_y0 - R + 4 * yq) * pitch + (tile_x0 - R + 16 * xs);
            uint4 a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = *reinterpret_cast<const uint4*>(p + (size_t)k * pitch);
            const uint32_t* aw[4] = {&a[0].x, &a[1].x, &a[2].x, &a[3].x};
#pragma unroll
            for (int q = 0; q < 4; ++q)  // dword q of each row = pixels 4q..4q+3
                *reinterpret_cast<uint4*>(rp + yq * RWP + 16 * xs + 4 * q) = transposed(aw[0][q], aw[1][q], aw[2][q], aw[3][q]);
        }
    } else if (cols >= 4 && R < cols && tile_x0 + TW + R - 1 <= 2 * (cols - 1) && R < rows && tile_y0 + TH + R - 1 <= 2 * (rows - 1)) {
        // Border tiles whose halo reaches at most ONE reflection on either side (16 % of the tiles of a 3840 x 2160 octave,
        // 24 % of a 1920 x 1080 one; every tile of the coarse octaves at camera sizes: 30 of 40 tiles of a 960 x 540 octave,
        // all of a 480 x 270 one).  Round 5: branch-free.  Four pixels at columns x .. x+3 under BORDER_REFLECT_101 always lie
        // within four consecutive bytes of the row - a forward run, a mirrored run, or a run folded around column 0 / cols-1 -
        // so every case is ONE unaligned dword load at `base` and one v_perm whose selector holds the four byte positions
        // relative to base.  No divergent paths: the four row loads of an item issue back to back and UNROLL items are in
        // flight per thread.  The matrix kernels run with one workgroup per CU beside the HBM-bound Harris chain and are
        // bound by the latency of exactly these loads (UNROLL = 4).
        auto f1 = [](int x, int n) { return x < 0 ? -x : (x >= n ? 2 * (n - 1) - x : x); };
#pragma unroll UNROLL
        for (int it = tid; it < RQ * (RW / 4); it += NT) {
            const int yq = it / (RW / 4), xq = it - yq * (RW / 4);
            const int gy = tile_y0 - R + 4 * yq, gx = tile_x0 - R + 4 * xq;
            const int p0 = f1(gx, cols), p1 = f1(gx + 1, cols), p2 = f1(gx + 2, cols), p3 = f1(gx + 3, cols);
            const int base = min(min(min(p0, p1), min(p2, p3)), cols - 4);
            const uint32_t sel = (uint32_t)(p0 - base) | ((uint32_t)(p1 - base) << 8) | ((uint32_t)(p2 - base) << 16) | ((uint32_t)(p3 - base) << 24);
            uint32_t a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                uint32_t v;
                __builtin_memcpy(&v, src + (size_t)f1(gy + k, rows) * pitch + base, 4);
                a[k] = __builtin_amdgcn_perm(0u, v, sel);
            }
            *reinterpret_cast<uint4*>(rp + yq * RWP + 4 * xq) = transposed(a[0], a[1], a[2], a[3]);
        }
    } else {
        // tiny images (a halo wider than the image: repeated reflection): one dword column (4 pixels) x 4 rows per item, rows
        // reflected per row, columns per dword
        for (int it = tid; it < RQ * (RW / 4); it += NT) {
            const int yq = it / (RW / 4), xq = it - yq * (RW / 4);
            const int gy = tile_y0 - R + 4 * yq, gx = tile_x0 - R + 4 * xq;
            uint32_t a[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = load4_reflect101(src + (size_t)reflect101(gy + k, rows) * pitch, gx, cols);
            *reinterpret_cast<uint4*>(rp + yq * RWP + 4 * xq) = transposed(a[0], a[1], a[2], a[3]);
        }
    }
}

}  // namespace vslam

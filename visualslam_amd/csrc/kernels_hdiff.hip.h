// K-D3d: the horizontal pass of the coarse octaves in difference form (default pyramid; k_gauss_h_strip otherwise).
//
// The 16-bit pass of k_gauss_h_strip costs ceil((n+1)/2) v_dot2_u32_u16 per output (2 MACs at 4.27 cycles).  Its
// error-diffused taps are mostly small integers that repeat, so the differences d[e] = w[e+r] - w[e+r+1] are sparse:
// out[j] = out[j-1] + sum_e d[e] h[j+e] needs nnz(d) MACs per output (octave 2: 222 over the six levels against 416
// dense).  The arithmetic is f32 and exact: every operand and partial sum is an integer below 2^24 (vslam::diff_form
// checks the bound per level; prefixes of the differences are differences of two outputs).  v_pk_fma_f32 does one MAC
// for each of two rows at the price of one dot2, so a lane owns HD_J = 16 consecutive outputs of TWO rows:
//   - the row sums are staged once per level as f32 pairs {row 2p, row 2p+1} with the reflect-101 extension;
//   - the lane streams its window of (HD_J + n + 1) columns through ds_read_b128 (two columns per read) and feeds each
//     column to every (output, tap) pair it belongs to: offsets and coefficients are compile-time (diff_taps.gen.h), so
//     the whole level is straight-line v_pk_fma_f32 with constant operands;
//   - a dense sum seeds the lane at out[x0 - 1] (n MACs per 16 outputs); the prefix sum of the 16 differences then
//     gives the outputs, rounded exactly as k_gauss_h_strip does: (acc + 32768) >> 16, the 32768 arriving with the data.
// Levels whose taps do not pay (the cost model of vslam::diff_form) run the dense f32 form in the same code.
// LDS columns are padded by 2 after every 16 so that the 16 lanes of a ds_read_b128 lane group, 144 bytes apart, hit
// distinct banks.
#pragma once
#include <hip/hip_runtime.h>

#include <utility>
#include <vector>

#include "diff_taps.gen.h"
#include "kernels_strip.hip.h"
#include "vslam_internal.h"

namespace vslam {

typedef float hd_f2 __attribute__((ext_vector_type(2)));

template <class F, int... I>
__device__ __forceinline__ void hd_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void hd_for(F&& f) {
    hd_for_impl(f, std::make_integer_sequence<int, N>{});
}

__host__ __device__ constexpr int hd_phys(int c) { return c + (c >> 4) * HD_PAD; }

template <class LV>
__host__ __device__ constexpr int hd_w(int k) { return k >= 0 && k < LV::n ? (int)LV::w[k] : 0; }

// coefficient of input column x0 + e in output x0 (difference form: of out[x0] - out[x0 - 1])
template <class LV>
__host__ __device__ constexpr int hd_coef(int e) {
    if (LV::form == 1) {
        for (int i = 0; i < LV::nd; ++i)
            if (LV::de[i] == e) return LV::dc[i];
        return 0;
    }
    return hd_w<LV>(e + LV::n / 2);
}

// geometry of octave O: widest kernel and left halo (hd_left_halo, vslam_octave_launch.h, with HD_J, HD_PAD and hd_pw)
template <int O>
struct HdGeom {
    static constexpr int nmax = dtaps::Lvl<O, 5>::n;  // widths grow with the level
    static constexpr int rmax = nmax / 2;
    static constexpr int HL = hd_left_halo(rmax);
    static_assert(dtaps::Lvl<O, 0>::n <= nmax && dtaps::Lvl<O, 4>::n <= nmax, "level 5 is the widest");
};

// One level of one lane: acc[j] = {out(row 0), out(row 1)} of output x0 + j, exact integers (bias and rounding constant included).
template <class LV, int HL>
__device__ __forceinline__ void hd_level(const hd_f2* __restrict__ lane, hd_f2 (&acc)[HD_J]) {
    constexpr int n = LV::n, r = n / 2;
    constexpr bool DIFF = LV::form == 1;
    constexpr int lo = DIFF ? -r - 1 : -r, hi = HD_J - 1 + r;  // input columns (relative to x0) the lane reads
    constexpr int t0 = (HL + lo) & ~1, Q = (HL + hi - t0) / 2 + 1;
    hd_f2 seed = {0.f, 0.f};
    hd_for<HD_J>([&](auto j) { acc[decltype(j)::value] = hd_f2{0.f, 0.f}; });
    hd_for<Q>([&](auto q) {
        constexpr int t = t0 + 2 * decltype(q)::value;  // logical LDS column of the read (even: 16-byte aligned, inside one group of 16)
        const float4 v = *reinterpret_cast<const float4*>(lane + hd_phys(t));
        const hd_f2 hv[2] = {hd_f2{v.x, v.y}, hd_f2{v.z, v.w}};
        hd_for<2>([&](auto b) {
            constexpr int x = t + decltype(b)::value - HL;  // input column relative to x0
            if constexpr (DIFF) {  // seed = out[x0 - 1] = sum_k w[k] h[x0 - 1 - r + k]
                constexpr int wk = hd_w<LV>(x + 1 + r);
                if constexpr (wk != 0) seed = __builtin_elementwise_fma(hd_f2((float)wk), hv[decltype(b)::value], seed);
            }
            hd_for<HD_J>([&](auto j) {
                constexpr int c = hd_coef<LV>(x - decltype(j)::value);
                if constexpr (c != 0)
                    acc[decltype(j)::value] = __builtin_elementwise_fma(hd_f2((float)c), hv[decltype(b)::value], acc[decltype(j)::value]);
            });
        });
    });
    if constexpr (DIFF) {
        acc[0] += seed;
        hd_for<HD_J - 1>([&](auto j) { acc[decltype(j)::value + 1] += acc[decltype(j)::value]; });
    }
}

// grid = (1, ceil(rows / (2 npairs)), frames), block 256; dynamic LDS = npairs * pw * 8 bytes (pw = hd_pw); items
// (row pair x 16-column segment) = npairs * ceil(cols/16) <= 256.  Arguments and outputs as k_gauss_h_strip: G planes,
// saturating DoG against the previous level, the next octave's base from G3.
template <int O>
__global__ __launch_bounds__(256) void k_gauss_h_diff(const uint16_t* __restrict__ h, size_t hframe, uint8_t* __restrict__ oct_out,
                                                       size_t pframe, int rows, int cols, int pitch, int npairs, int pw,
                                                       uint8_t* __restrict__ next_base, size_t nframe, int nrows, int ncols, int npitch) {
    using G = HdGeom<O>;
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    hd_f2* hp = reinterpret_cast<hd_f2*>(smem);  // [npairs][pw]: logical column c = image column + HL at hd_phys(c)
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * 2 * npairs;
    const size_t P = (size_t)rows * pitch;
    uint8_t* out = oct_out + blockIdx.z * pframe;
    const int ncs = (cols + HD_J - 1) / HD_J;
    const int n8 = cols >> 3, tl = cols & 7;             // interior groups of 8 columns; tail columns past the last group
    const int nh = hd_halo_cols(cols, G::HL, G::rmax);  // halo columns: left of column 0, and from column `cols` on
    const bool active = tid < npairs * ncs;
    const int ip = tid / ncs, is = tid - ip * ncs;
    const hd_f2* lane = hp + ip * pw + is * (HD_J + HD_PAD);

    // The staging plan of this thread, the same for every level (only the plane differs), made once.  A thread holds at
    // most two interior items, one tail item and HT halo items (hdiff_stage_fits, vslam_octave_launch.h).  An item the
    // thread does not have loads column 0 of the workgroup's first row (always there) and writes nothing.
    constexpr int HT = hd_halo_trips(G::HL, G::rmax);
    const uint16_t* h0 = h + blockIdx.z * hframe;
    auto row_of = [&](int p, int rho) { return h0 + (size_t)min(y0 + 2 * p + rho, rows - 1) * pitch; };
    const uint16_t *ia[2], *ib[2], *ta, *tb;  // level 0's addresses of both rows of the pair
    float4* iq[2];                            // where an interior item goes (HL % 16 == 0: inside one group of 16)
    hd_f2* tq;
    bool iv[2];
    {
        const int n8d = max(n8, 1);  // (no interior group at all below 8 columns)
        int p = tid / n8d, k = tid - p * n8d;
        const int dp = 256 / n8d, dk = 256 - dp * n8d;  // (item -> (pair, column) by increments)
        hd_for<2>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if (k >= n8d) k -= n8d, ++p;
            iv[i] = tid + 256 * i < npairs * n8;
            const int pp = iv[i] ? p : 0, kk = iv[i] ? k : 0;
            ia[i] = row_of(pp, 0) + 8 * kk;
            ib[i] = row_of(pp, 1) + 8 * kk;
            iq[i] = reinterpret_cast<float4*>(hp + pp * pw + hd_phys(G::HL + 8 * kk));
            p += dp, k += dk;
        });
    }
    const bool tv = tid < npairs * tl;
    {
        const int tld = max(tl, 1);
        const int p = tv ? tid / tld : 0, x = tv ? 8 * n8 + tid - p * tld : 0;
        ta = row_of(p, 0) + x;
        tb = row_of(p, 1) + x;
        tq = hp + p * pw + hd_phys(G::HL + x);
    }
    // halo item: copy of the staged column it reflects to (reflect-101, repeated for kernels wider than the row), inside
    // LDS: source index | destination index << 16 in hp (both < 2^16: LDS is below 512 KB); 0xffff: no item
    uint32_t hx[HT];
    {
        int p = tid / nh, i = tid - p * nh;
        const int dp = 256 / nh, di = 256 - dp * nh;
        hd_for<HT>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            if (i >= nh) i -= nh, ++p;
            const int c = i < G::HL ? i : cols + i;  // logical column: image column c - HL
            const int x = reflect101(c - G::HL, cols);
            hx[t] = tid + 256 * t < npairs * nh ? (uint32_t)(p * pw + hd_phys(G::HL + x)) | (uint32_t)(p * pw + hd_phys(c)) << 16 : 0xffff0000u;
            p += dp, i += di;
        });
    }

    // the level's interior and tail, held in registers from the loads (issued under the previous level's arithmetic)
    // to the LDS writes (after the barrier that ends that level's reads)
    uint4 ra[2], rb[2];
    uint16_t rta, rtb;
    auto load_level = [&](auto lc) {
        const size_t lo = (size_t)decltype(lc)::value * P;
        hd_for<2>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            ra[i] = *reinterpret_cast<const uint4*>(ia[i] + lo);
            rb[i] = *reinterpret_cast<const uint4*>(ib[i] + lo);
        });
        rta = ta[lo];
        rtb = tb[lo];
    };
    uint32_t prev_e[2][4], prev_o[2][4];

    load_level(std::integral_constant<int, 0>{});
    hd_for<VSLAM_NUM_LEVELS>([&](auto lc) {
        constexpr int L = decltype(lc)::value;
        if constexpr (L > 0) __syncthreads();  // the previous level's reads are done
        hd_for<2>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            if (iv[i]) {
                const uint32_t av[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w}, bv[4] = {rb[i].x, rb[i].y, rb[i].z, rb[i].w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    iq[i][j] = make_float4((float)(av[j] & 0xffffu), (float)(bv[j] & 0xffffu), (float)(av[j] >> 16), (float)(bv[j] >> 16));
            }
        });
        if (tv) *tq = hd_f2{(float)rta, (float)rtb};
        __syncthreads();  // every image column of the row pairs is in LDS
        {
            hd_f2 hv[HT];
            hd_for<HT>([&](auto tc) { hv[decltype(tc)::value] = hp[hx[decltype(tc)::value] & 0xffffu]; });
            hd_for<HT>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                if ((hx[t] >> 16) != 0xffffu) hp[hx[t] >> 16] = hv[t];
            });
        }
        __syncthreads();
        if constexpr (L + 1 < VSLAM_NUM_LEVELS) load_level(std::integral_constant<int, L + 1>{});
        if (active) {
            hd_f2 acc[HD_J];
            hd_level<dtaps::Lvl<O, L>, G::HL>(lane, acc);
            const int x = HD_J * is;
            hd_for<2>([&](auto rc) {
                constexpr int rho = decltype(rc)::value;
                const int y = y0 + 2 * ip + rho;
                uint32_t u[HD_J], g[4], d[4];
                hd_for<HD_J>([&](auto j) { u[decltype(j)::value] = (uint32_t)acc[decltype(j)::value][rho]; });
#pragma unroll
                for (int hw = 0; hw < 4; ++hw) {
                    const uint32_t e = __builtin_amdgcn_perm(u[4 * hw + 2], u[4 * hw + 0], 0x0c060c02);
                    const uint32_t o = __builtin_amdgcn_perm(u[4 * hw + 3], u[4 * hw + 1], 0x0c060c02);
                    g[hw] = __builtin_amdgcn_perm(o, e, 0x06020400);
                    if constexpr (L > 0)
                        d[hw] = __builtin_amdgcn_perm(pk_sub_sat_u16(o, prev_o[rho][hw]), pk_sub_sat_u16(e, prev_e[rho][hw]), 0x06020400);
                    prev_e[rho][hw] = e;
                    prev_o[rho][hw] = o;
                }
                if (y < rows) {  // 16-byte stores: pitch is a multiple of 16 and x < cols, so the group ends inside the row's pitch
                    const size_t off = (size_t)y * pitch + x;
                    *reinterpret_cast<uint4*>(out + (size_t)L * P + off) = make_uint4(g[0], g[1], g[2], g[3]);
                    if constexpr (L > 0)
                        *reinterpret_cast<uint4*>(out + (size_t)(VSLAM_NUM_LEVELS + L - 1) * P + off) = make_uint4(d[0], d[1], d[2], d[3]);
                    // next octave's base = Gaussian[3] decimated 2:1 (y0 and 2 ip are even: row 0 of the pair is the even row)
                    if constexpr (L == 3 && rho == 0)
                        if (next_base && (y >> 1) < nrows && (x >> 1) < ncols)
                            *reinterpret_cast<uint2*>(next_base + blockIdx.z * nframe + (size_t)(y >> 1) * npitch + (x >> 1)) =
                                make_uint2(even_bytes(g[0], g[1]), even_bytes(g[2], g[3]));
                }
            });
        }
    });
}

// Host side: the octave of diff_taps.gen.h whose six levels equal the plan's trimmed taps (the form and the difference
// pairs re-derived by vslam::diff_form must equal the header's too), or 0.
template <int O, int L>
static bool hd_level_matches(const std::vector<uint16_t>& t) {
    using LV = dtaps::Lvl<O, L>;
    if ((int)t.size() != LV::n) return false;
    for (int k = 0; k < LV::n; ++k)
        if (t[k] != LV::w[k]) return false;
    std::vector<int> off, coef;
    if (diff_form(t.data(), LV::n, off, coef) != LV::form) return false;
    if (LV::form == 1) {
        if ((int)off.size() != LV::nd) return false;
        for (int i = 0; i < LV::nd; ++i)
            if (off[i] != LV::de[i] || coef[i] != LV::dc[i]) return false;
    }
    return true;
}
template <int O>
static bool hd_octave_matches(const std::vector<uint16_t> (&taps)[6]) {
    return hd_level_matches<O, 0>(taps[0]) && hd_level_matches<O, 1>(taps[1]) && hd_level_matches<O, 2>(taps[2]) &&
           hd_level_matches<O, 3>(taps[3]) && hd_level_matches<O, 4>(taps[4]) && hd_level_matches<O, 5>(taps[5]);
}

}  // namespace vslam

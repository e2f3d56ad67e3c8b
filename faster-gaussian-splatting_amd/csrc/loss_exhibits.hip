// The loss kernels' A/B exhibit: the TILED formulation the product shipped until the streaming one of loss.hip replaced it. libfgs_hip_dev.so only
// (-DFGS_DEV_SWITCHES; the Makefile lists this unit in DEVOBJ and not in OBJ, with loss.o's flags); the product library has none of this file.
//   option 16  g_loss_form -- bit 0: the forward kernel below instead of loss.hip's, bit 1: the backward kernel below; 0 = the product's kernels.
//   ssim_forward_tiled_kernel : 32x32 output tile per 256-thread workgroup, x/y tile + 5-pixel halo staged in LDS, separable register-blocked
//                               filtering (11 horizontal taps into LDS, 11 vertical taps); per-workgroup partial sums.
//   ssim_backward_tiled_kernel: 64x32 tiles of the three derivative maps, the same two passes.
// Per pixel both formulations run the same operations in the same order (fgs_loss.h), so the derivative maps and the gradient are equal bit for bit
// (tests/test_loss_stream.py, tests/test_gpu_loss_stream.py); the loss scalars differ by the order of their partial sums. Figures: profiles/loss_streaming.txt.
#ifdef FGS_DEV_SWITCHES   // the whole unit: compiled without the define (the product flavour of the simulation does, it takes every csrc/*.hip) it is empty
#include "fgs_loss.h"

namespace fgs {

#ifndef FGS_LOSS_TILE_W
#define FGS_LOSS_TILE_W 32   // tools/ab_loss_tiles.sh, 1080p, one box, loss stage: unblocked 32x16 (round 1) 0.182 ms; blocked 32x16 0.164,
#define FGS_LOSS_TILE_H 32   // 32x32 0.150 (default), 64x16 0.160, 64x32 0.175 (206 VGPRs + 79 KB LDS: 2 workgroups per CU)
#endif
constexpr int kLossTileW = FGS_LOSS_TILE_W, kLossTileH = FGS_LOSS_TILE_H;
constexpr int kRegionW = kLossTileW + 2 * kHalo, kRegionH = kLossTileH + 2 * kHalo;   // 42 x 42: halo re-reads 1.72x (32x16 tiles: 2.13x;
                                                                                      // rocprofv3 round 2: 239 MB fetched for 50 MB of input)
constexpr int kRowsPerThread = (kLossTileW * kLossTileH) / 256;                       // 4: thread = one output column x 4 consecutive rows
constexpr int kHzGroups = kLossTileW / 4;                                             // horizontal pass: 4 adjacent outputs per work item
static_assert(kLossTileW * (kLossTileH / kRowsPerThread) == 256, "one (column, row strip) per thread");

// Tiles in (channel, row, column) order, dealt to the XCDs in contiguous runs (xcd_region_unit)
__device__ __forceinline__ bool loss_tile_of(const unsigned block, const unsigned tiles_x, const unsigned tiles_y, unsigned& tx, unsigned& ty, unsigned& c,
                                             unsigned& logical) {
    if (!xcd_region_unit(block, tiles_x * tiles_y * 3u, logical)) return false;
    c = logical / (tiles_x * tiles_y);
    const unsigned in_plane = logical - c * tiles_x * tiles_y;
    ty = in_plane / tiles_x; tx = in_plane - ty * tiles_x;
    return true;
}

// Both filter passes are register-blocked: round 2's profile had 417 lane-instructions per output (one LDS read and an index div/mod per
// FMA); the horizontal pass now takes 14 staged values for 4 outputs x 11 taps, the vertical pass kRowsPerThread + 10 for kRowsPerThread
// outputs. Staging keeps a flat index: a row-per-128-threads loop (no div/mod, 42 % idle lanes in the global loads) measured 0.213 ms at 64x32.
template <int MAPS, typename Load>
__device__ __forceinline__ void stage_region(float (*dst)[kRegionH][kRegionW], const int x0, const int y0, const int width, const int height, Load load) {
    for (int idx = threadIdx.x; idx < kRegionH * kRegionW; idx += 256) {            // flat index: every lane loads (division by a constant)
        const int ry = idx / kRegionW, rx = idx - ry * kRegionW;
        const int gy = y0 + ry - kHalo, gx = x0 + rx - kHalo;
        const bool in = gy >= 0 && gy < height && gx >= 0 && gx < width;            // zero padding
#pragma unroll
        for (int k = 0; k < MAPS; ++k) dst[k][ry][rx] = in ? load(k, (size_t)gy * width + gx) : 0.0f;
    }
}

// LDS: the staged x / y region (14.1 KB) is dead once the horizontal pass has read it -- the L1 term of the tile's own pixels is taken there,
// from registers -- so the fifth filtered map lives in ITS memory: 14.1 + 4 x 5.4 = 35.6 KB per workgroup instead of 41.0, i.e. four
// workgroups per CU instead of three (160 KB), and the register budget is capped to match (FGS_LOSS_FWD_WAVES waves per SIMD). Round 2's
// counters had this kernel at 9 resident waves per CU, 45 % of the issue slots, LDS busy a fifth of the time: latency-bound at low occupancy.
#ifndef FGS_LOSS_FWD_WAVES
#define FGS_LOSS_FWD_WAVES 4
#endif
#if FGS_LOSS_FWD_WAVES > 0
#define FGS_LOSS_FWD_BOUNDS __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FGS_LOSS_FWD_WAVES, FGS_LOSS_FWD_WAVES)))
#else
#define FGS_LOSS_FWD_BOUNDS __launch_bounds__(256)
#endif

// WEIGHTED: the weight plane is never staged (a [42][42] copy would be the 7 KB that drop the kernel to three workgroups per CU): staging substitutes
// the target where the weight is not positive, the L1 term and the output stage read the weight of their own pixel from global memory.
template <bool WEIGHTED>
__global__ void FGS_LOSS_FWD_BOUNDS ssim_forward_tiled_kernel(const LossArgs a, const GaussWindow gw) {
    constexpr int kMapFloats = kRegionH * kLossTileW;                                 // one horizontally filtered map
    static_assert(2 * kRegionH * kRegionW >= kMapFloats + 12, "the fifth map and the reduction scratch fit in the staged region");
    __shared__ float sxy[2][kRegionH][kRegionW];
    __shared__ float hz4[4][kRegionH][kLossTileW];
    float (*const hz_last)[kLossTileW] = reinterpret_cast<float (*)[kLossTileW]>(&sxy[0][0][0]);      // map 4, written after the barrier below
    float* const s_red = &sxy[0][0][0] + kMapFloats;                                   // 8 floats behind it
    unsigned tile_x, tile_y, chan, logical;
    if (!loss_tile_of(blockIdx.x, (a.width + kLossTileW - 1) / kLossTileW, (a.height + kLossTileH - 1) / kLossTileH, tile_x, tile_y, chan, logical)) return;   // workgroup-uniform
    const int x0 = tile_x * kLossTileW, y0 = tile_y * kLossTileH, c = chan;
    const size_t plane = (size_t)a.width * a.height;
    const float* __restrict__ X = a.image + c * plane; const float* __restrict__ Y = a.target + c * plane;
    const float* __restrict__ Wt = a.weight;
    if constexpr (WEIGHTED)     // x' = x where the weight is positive, the target elsewhere: a select, whatever x holds there (NaN included) goes nowhere
        stage_region<2>(sxy, x0, y0, a.width, a.height, [&](int k, size_t e) { return k == 0 && Wt[e] > 0.0f ? X[e] : Y[e]; });
    else
        stage_region<2>(sxy, x0, y0, a.width, a.height, [&](int k, size_t e) { return k == 0 ? X[e] : Y[e]; });
    __syncthreads();
    float l1_sum = 0.0f;
    constexpr int kItems = kRegionH * kHzGroups, kItemsPerThread = (kItems + 255) / 256;
    float keep[kItemsPerThread][4];                                                    // map 4 of this thread's items, until sxy may be overwritten
#pragma unroll
    for (int it = 0; it < kItemsPerThread; ++it) {                                     // horizontal taps: 4 outputs from 14 inputs
        const int item = threadIdx.x + it * 256;
        if (item < kItems) {
            const int ry = item / kHzGroups, cx = (item % kHzGroups) * 4;
            float p[14], q[14], p2[14], q2[14], pq[14];
#pragma unroll
            for (int t = 0; t < 14; ++t) { p[t] = sxy[0][ry][cx + t]; q[t] = sxy[1][ry][cx + t]; }
            // the three products once per staged value, not once per (output, tap): 42 multiplications instead of 132 per work item (round 4)
#pragma unroll
            for (int t = 0; t < 14; ++t) { p2[t] = p[t] * p[t]; q2[t] = q[t] * q[t]; pq[t] = p[t] * q[t]; }
            const int gy = y0 + ry - kHalo;
            const bool own_row = ry >= kHalo && ry < kHalo + kLossTileH && gy < a.height;
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float m1 = 0.0f, m2 = 0.0f, m11 = 0.0f, m22 = 0.0f, m12 = 0.0f;
#pragma unroll
                for (int t = 0; t < kTaps; ++t) {
                    const float w = gw.w[t];
                    m1 = tap(w, p[o + t], m1); m2 = tap(w, q[o + t], m2); m11 = tap(w, p2[o + t], m11); m22 = tap(w, q2[o + t], m22); m12 = tap(w, pq[o + t], m12);
                }
                hz4[0][ry][cx + o] = m1; hz4[1][ry][cx + o] = m2; hz4[2][ry][cx + o] = m11; hz4[3][ry][cx + o] = m22;
                keep[it][o] = m12;
                if constexpr (WEIGHTED) {                                                               // |x' - y|: 0 where the weight is not positive
                    if (own_row && x0 + cx + o < a.width) l1_sum += effective_weight(Wt[(size_t)gy * a.width + x0 + cx + o]) * fabsf(p[o + kHalo] - q[o + kHalo]);
                } else {
                    if (own_row && x0 + cx + o < a.width) l1_sum += fabsf(p[o + kHalo] - q[o + kHalo]);     // the tile's own pixel (cx + o, ry - 5)
                }
            }
        }
    }
    __syncthreads();                                                                   // every read of sxy is done
#pragma unroll
    for (int it = 0; it < kItemsPerThread; ++it) {
        const int item = threadIdx.x + it * 256;
        if (item < kItems) {
            const int ry = item / kHzGroups, cx = (item % kHzGroups) * 4;
#pragma unroll
            for (int o = 0; o < 4; ++o) hz_last[ry][cx + o] = keep[it][o];
        }
    }
    __syncthreads();
    float ssim_sum = 0.0f;
    [[maybe_unused]] float w_sum = 0.0f;                                               // WEIGHTED: the effective weights of this thread's output pixels
    const int ox = threadIdx.x % kLossTileW, oy0 = (threadIdx.x / kLossTileW) * kRowsPerThread;   // lanes of a wave: adjacent columns
    const int gx = x0 + ox;
    float v[5][kRowsPerThread];
#pragma unroll
    for (int m = 0; m < 5; ++m) {                                                   // vertical taps: 4 outputs from 14 inputs per map
        float col[kRowsPerThread + kTaps - 1];
#pragma unroll
        for (int t = 0; t < kRowsPerThread + kTaps - 1; ++t) col[t] = m < 4 ? hz4[m][oy0 + t][ox] : hz_last[oy0 + t][ox];
#pragma unroll
        for (int o = 0; o < kRowsPerThread; ++o) {
            float acc = 0.0f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) acc = tap(gw.w[t], col[o + t], acc);
            v[m][o] = acc;
        }
    }
#pragma unroll
    for (int o = 0; o < kRowsPerThread; ++o) {
        const int oy = oy0 + o, gy = y0 + oy;
        if (gy < a.height && gx < a.width) {
            const SsimPoint s = ssim_point(v[0][o], v[1][o], v[2][o], v[3][o], v[4][o]);
            const size_t e = c * plane + (size_t)gy * a.width + gx;
            if constexpr (WEIGHTED) {
                const float wp = effective_weight(Wt[(size_t)gy * a.width + gx]);
                w_sum += wp;
                ssim_sum += wp * s.value;
                a.d_mu[e] = wp * s.d_mu; a.d_m11[e] = wp * s.d_m11; a.d_m12[e] = wp * s.d_m12;
            } else {
                ssim_sum += s.value;
                a.d_mu[e] = s.d_mu; a.d_m11[e] = s.d_m11; a.d_m12[e] = s.d_m12;
            }
        }
    }
    const float bl = block_sum_256(l1_sum, s_red);
    const float bs = block_sum_256(ssim_sum, s_red + 4);
    if constexpr (WEIGHTED) {
        const float bw = block_sum_256(w_sum, s_red + 8);
        if (threadIdx.x == 255) {
            a.partials[2 * logical] = bl; a.partials[2 * logical + 1] = bs;
            if (c == 0) a.wpartials[logical] = bw;                               // once, not once per channel: channel 0's logical index IS the tile's index in the plane
        }
    } else {
        if (threadIdx.x == 255) {
            a.partials[2 * logical] = bl; a.partials[2 * logical + 1] = bs;          // in tile order whatever the mapping: the reduction order is fixed
        }
    }
}

// The backward pass has its own tile (round 4): it stages three maps instead of two and keeps three filtered maps instead of five, so a 64 x 32 tile
// (halo re-reads 1.38x instead of 1.72x: rocprofv3 round 3 had this kernel fetching 3.7x its input) fits in the LDS budget that limits the forward
// kernel to 32 x 32 (FGS_LOSS_BWD_TILE_W / _H: A/B knobs).
#ifndef FGS_LOSS_BWD_TILE_W
#define FGS_LOSS_BWD_TILE_W 64
#define FGS_LOSS_BWD_TILE_H 32
#endif
constexpr int kBwdTileW = FGS_LOSS_BWD_TILE_W, kBwdTileH = FGS_LOSS_BWD_TILE_H;
constexpr int kBwdRegionW = kBwdTileW + 2 * kHalo, kBwdRegionH = kBwdTileH + 2 * kHalo;
constexpr int kBwdRows = (kBwdTileW * kBwdTileH) / 256;                               // thread = one output column x kBwdRows consecutive rows
constexpr int kBwdHzGroups = kBwdTileW / 4;
static_assert(kBwdTileW * (kBwdTileH / kBwdRows) == 256 && kBwdTileW % 4 == 0, "one (column, row strip) per thread");

template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_backward_tiled_kernel(const LossArgs a, const GaussWindow gw, const unsigned n_reduce) {
    // The horizontally filtered maps go back into the memory of the staged region (dead once every thread has read its inputs into registers).
    constexpr int kMapFloats = kBwdRegionH * kBwdTileW;
    static_assert(3 * kBwdRegionH * kBwdRegionW >= 3 * kMapFloats, "the three filtered maps fit in the staged region");
    __shared__ float sd[3][kBwdRegionH][kBwdRegionW];
    float (*const hz)[kBwdRegionH][kBwdTileW] = reinterpret_cast<float (*)[kBwdRegionH][kBwdTileW]>(&sd[0][0][0]);
    const float n_total = backward_head<WEIGHTED>(a, n_reduce, &sd[0][0][0]);
    unsigned tile_x, tile_y, chan, logical;
    if (!loss_tile_of(blockIdx.x, (a.width + kBwdTileW - 1) / kBwdTileW, (a.height + kBwdTileH - 1) / kBwdTileH, tile_x, tile_y, chan, logical)) return;     // workgroup-uniform
    const int x0 = tile_x * kBwdTileW, y0 = tile_y * kBwdTileH, c = chan;
    const size_t plane = (size_t)a.width * a.height;
    const float* __restrict__ m0 = a.d_mu + c * plane; const float* __restrict__ m1 = a.d_m11 + c * plane; const float* __restrict__ m2 = a.d_m12 + c * plane;
    for (int idx = threadIdx.x; idx < kBwdRegionH * kBwdRegionW; idx += 256) {       // flat index: every lane loads (division by a constant)
        const int ry = idx / kBwdRegionW, rx = idx - ry * kBwdRegionW;
        const int gy = y0 + ry - kHalo, gx = x0 + rx - kHalo;
        const bool in = gy >= 0 && gy < a.height && gx >= 0 && gx < a.width;         // zero padding
        const size_t e = (size_t)gy * a.width + gx;
        sd[0][ry][rx] = in ? m0[e] : 0.0f; sd[1][ry][rx] = in ? m1[e] : 0.0f; sd[2][ry][rx] = in ? m2[e] : 0.0f;
    }
    __syncthreads();
    constexpr int kItems = kBwdRegionH * kBwdHzGroups, kItemsPerThread = (kItems + 255) / 256;
    float keep[kItemsPerThread][3][4];
#pragma unroll
    for (int it = 0; it < kItemsPerThread; ++it) {
        const int item = threadIdx.x + it * 256;
        if (item < kItems) {
            const int ry = item / kBwdHzGroups, cx = (item % kBwdHzGroups) * 4;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float p[14];
#pragma unroll
                for (int t = 0; t < 14; ++t) p[t] = sd[k][ry][cx + t];
#pragma unroll
                for (int o = 0; o < 4; ++o) {
                    float f = 0.0f;
#pragma unroll
                    for (int t = 0; t < kTaps; ++t) f = tap(gw.w[t], p[o + t], f);
                    keep[it][k][o] = f;
                }
            }
        }
    }
    __syncthreads();                                                                   // every read of sd is done
#pragma unroll
    for (int it = 0; it < kItemsPerThread; ++it) {
        const int item = threadIdx.x + it * 256;
        if (item < kItems) {
            const int ry = item / kBwdHzGroups, cx = (item % kBwdHzGroups) * 4;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int o = 0; o < 4; ++o) hz[k][ry][cx + o] = keep[it][k][o];
        }
    }
    __syncthreads();
    const float up = a.upstream != nullptr ? *a.upstream : 1.0f;
    const float ks = -a.lambda_dssim / n_total * up, kl = a.lambda_l1 / n_total * up;
    const int ox = threadIdx.x % kBwdTileW, oy0 = (threadIdx.x / kBwdTileW) * kBwdRows;
    const int gx = x0 + ox;
    float v[3][kBwdRows];
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float col[kBwdRows + kTaps - 1];
#pragma unroll
        for (int t = 0; t < kBwdRows + kTaps - 1; ++t) col[t] = hz[m][oy0 + t][ox];
#pragma unroll
        for (int o = 0; o < kBwdRows; ++o) {
            float acc = 0.0f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) acc = tap(gw.w[t], col[o + t], acc);
            v[m][o] = acc;
        }
    }
#pragma unroll
    for (int o = 0; o < kBwdRows; ++o) {
        const int gy = y0 + oy0 + o;
        if (gy >= a.height || gx >= a.width) continue;
        const size_t e = c * plane + (size_t)gy * a.width + gx;
        float wp = 0.0f;
        if constexpr (WEIGHTED) wp = a.weight[(size_t)gy * a.width + gx];
        a.grad[e] = loss_gradient<WEIGHTED>(ks, kl, v[0][o], v[1][o], v[2][o], a.image[e], a.target[e], wp);
    }
}

static unsigned forward_tiles(int width, int height) { return static_cast<unsigned>((width + kLossTileW - 1) / kLossTileW) * static_cast<unsigned>((height + kLossTileH - 1) / kLossTileH) * 3u; }

size_t loss_exhibit_partials(int width, int height) { return 2 * static_cast<size_t>(forward_tiles(width, height)); }

hipError_t launch_loss_forward_exhibit(const LossArgs& a, const GaussWindow& gw, hipStream_t s) {
    const dim3 grid = loss_grid(forward_tiles(a.width, a.height));
    if (a.weight != nullptr) hipLaunchKernelGGL(ssim_forward_tiled_kernel<true>, grid, dim3(256), 0, s, a, gw);
    else hipLaunchKernelGGL(ssim_forward_tiled_kernel<false>, grid, dim3(256), 0, s, a, gw);
    return hipGetLastError();
}

hipError_t launch_loss_backward_exhibit(const LossArgs& a, const GaussWindow& gw, const unsigned n_reduce, hipStream_t s) {
    const unsigned tiles = static_cast<unsigned>((a.width + kBwdTileW - 1) / kBwdTileW) * static_cast<unsigned>((a.height + kBwdTileH - 1) / kBwdTileH) * 3u;
    if (a.weight != nullptr) hipLaunchKernelGGL(ssim_backward_tiled_kernel<true>, loss_grid(tiles), dim3(256), 0, s, a, gw, n_reduce);
    else hipLaunchKernelGGL(ssim_backward_tiled_kernel<false>, loss_grid(tiles), dim3(256), 0, s, a, gw, n_reduce);
    return hipGetLastError();
}

}  // namespace fgs
#endif  // FGS_DEV_SWITCHES

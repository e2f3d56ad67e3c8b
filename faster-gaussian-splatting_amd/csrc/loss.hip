// Fused photometric loss  lambda_l1 * L1 + lambda_dssim * (1 - SSIM)  and its gradient w.r.t. the rendered image, for
// gfx950: the step between the two halves of the hot path in every training iteration (Trainer.py:190-196, Loss.py:15-16;
// SURVEY.md 8f rank 2). The reference calls `fused_dssim` from the un-vendored NeRFICG framework; this implements the
// published SSIM as used by 3D Gaussian Splatting (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2,
// C2 = 0.03^2, mean over channels and pixels); tests/test_loss.py pins it against a torch conv2d + autograd implementation.
//
// Two launches replace the ~30 elementwise/conv kernels of a framework-level SSIM:
//   ssim_forward_kernel : 32x32 output tile per 256-thread workgroup, x/y tile + 5-pixel halo staged in LDS, separable
//                         register-blocked filtering (11 horizontal taps into LDS, 11 vertical taps), SSIM value + the three partial
//                         derivative maps (d/dmu1, d/dE[x^2], d/dE[xy]); per-workgroup sums leave through two atomics.
//   ssim_backward_kernel: filters the three derivative maps with the same (self-adjoint) window and combines them with
//                         x, y and the L1 sign: dloss/dimage, no dependence on the loss value -> no host sync anywhere.
// Each kernel is a template <bool WEIGHTED>: false is the loss above, true the same loss with a per-pixel weight / mask (INTEGRATION.md 'Weighted loss').
#include "fgs_kernels.h"
#include <fgs_wave.h>

namespace fgs {

#ifndef FGS_LOSS_TILE_W
#define FGS_LOSS_TILE_W 32   // tools/ab_loss_tiles.sh, 1080p, one box, loss stage: unblocked 32x16 (round 1) 0.182 ms; blocked 32x16 0.164,
#define FGS_LOSS_TILE_H 32   // 32x32 0.150 (default), 64x16 0.160, 64x32 0.175 (206 VGPRs + 79 KB LDS: 2 workgroups per CU)
#endif
constexpr int kLossTileW = FGS_LOSS_TILE_W, kLossTileH = FGS_LOSS_TILE_H, kHalo = 5, kTaps = 11;
constexpr int kRegionW = kLossTileW + 2 * kHalo, kRegionH = kLossTileH + 2 * kHalo;   // 42 x 42: halo re-reads 1.72x (32x16 tiles: 2.13x;
                                                                                      // rocprofv3 round 2: 239 MB fetched for 50 MB of input)
constexpr int kRowsPerThread = (kLossTileW * kLossTileH) / 256;                       // 4: thread = one output column x 4 consecutive rows
constexpr int kHzGroups = kLossTileW / 4;                                             // horizontal pass: 4 adjacent outputs per work item
static_assert(kLossTileW * (kLossTileH / kRowsPerThread) == 256, "one (column, row strip) per thread");

struct GaussWindow { float w[kTaps]; };

// Which tile does workgroup `block` of a 1-D launch filter? The hardware deals workgroups to the 8 XCDs round-robin (XCD = block % 8) and every tile
// re-reads a 5-pixel halo of its neighbours' pixels: with the natural order the four neighbours of a tile run on four other XCDs, each with an L2 of
// its own, and every one of them fetches the shared 128-byte lines from memory again (round-5 counters: the two kernels fetched 2.4x their
// algorithmic bytes). Here XCD x owns the contiguous band of tiles [x * per_xcd, (x + 1) * per_xcd) in (channel, row, column) order -- a dozen full
// tile rows -- so a tile's neighbours are its own XCD's neighbours in time and space. FGS_LOSS_XCD_BANDS=0: the natural order (A/B).
#ifndef FGS_LOSS_XCD_BANDS
#define FGS_LOSS_XCD_BANDS 1
#endif
#ifndef FGS_LOSS_XCD_BANDS_BWD
#define FGS_LOSS_XCD_BANDS_BWD FGS_LOSS_XCD_BANDS
#endif
template <bool BANDS>
__device__ __forceinline__ bool loss_tile_of(const unsigned block, const unsigned tiles_x, const unsigned tiles_y, unsigned& tx, unsigned& ty, unsigned& c,
                                             unsigned& logical) {
    const unsigned total = tiles_x * tiles_y * 3u;
    const unsigned per_xcd = (total + kXcds - 1u) / kXcds;
    logical = BANDS ? (block % kXcds) * per_xcd + block / kXcds : block;
    if (logical >= total) return false;
    c = logical / (tiles_x * tiles_y);
    const unsigned in_plane = logical - c * tiles_x * tiles_y;
    ty = in_plane / tiles_x; tx = in_plane - ty * tiles_x;
    return true;
}

__device__ __forceinline__ float block_sum_256(float v, float* s_red) {   // sum over the 256-thread workgroup, valid in thread 255
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    v = wave_sum_to_lane63(v);
    if (lane == 63u) s_red[wv] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
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
__device__ __forceinline__ float effective_weight(const float w) { return w > 0.0f ? w : 0.0f; }   // negative and NaN count as 0

// WEIGHTED (a.weight, [H,W]; INTEGRATION.md 'Weighted loss'): the same tiles and the same order of every sum, so all-ones weights reproduce the
// unweighted bits. Three differences, none of which costs LDS (the weight plane is never staged: a [42][42] copy would be the 7 KB that drop the kernel
// to three workgroups per CU): staging substitutes the target where the weight is not positive (one more global read per staged element), the L1 term
// and the output stage read the weight of their own pixel from global memory (lines the staging just brought in) and multiply the SSIM value and
// the three derivative maps by it, and the workgroups of channel 0 leave their tile's sum of weights in a.wpartials.
template <bool WEIGHTED>
__global__ void FGS_LOSS_FWD_BOUNDS ssim_forward_kernel(const LossArgs a, const GaussWindow gw) {
    constexpr int kMapFloats = kRegionH * kLossTileW;                                 // one horizontally filtered map
    static_assert(2 * kRegionH * kRegionW >= kMapFloats + 12, "the fifth map and the reduction scratch fit in the staged region");
    __shared__ float sxy[2][kRegionH][kRegionW];
    __shared__ float hz4[4][kRegionH][kLossTileW];
    float (*const hz_last)[kLossTileW] = reinterpret_cast<float (*)[kLossTileW]>(&sxy[0][0][0]);      // map 4, written after the barrier below
    float* const s_red = &sxy[0][0][0] + kMapFloats;                                   // 8 floats behind it
    unsigned tile_x, tile_y, chan, logical;
    if (!loss_tile_of<FGS_LOSS_XCD_BANDS != 0>(blockIdx.x, (a.width + kLossTileW - 1) / kLossTileW, (a.height + kLossTileH - 1) / kLossTileH, tile_x, tile_y, chan, logical)) return;   // workgroup-uniform
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
                    m1 += w * p[o + t]; m2 += w * q[o + t]; m11 += w * p2[o + t]; m22 += w * q2[o + t]; m12 += w * pq[o + t];
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
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
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
            for (int t = 0; t < kTaps; ++t) acc += gw.w[t] * col[o + t];
            v[m][o] = acc;
        }
    }
#pragma unroll
    for (int o = 0; o < kRowsPerThread; ++o) {
        const int oy = oy0 + o, gy = y0 + oy;
        if (gy < a.height && gx < a.width) {
            const float mu1 = v[0][o], mu2 = v[1][o], m11 = v[2][o], m22 = v[3][o], m12 = v[4][o];
            const float s11 = m11 - mu1 * mu1, s22 = m22 - mu2 * mu2, s12 = m12 - mu1 * mu2;
            const float A1 = 2.0f * mu1 * mu2 + C1, A2 = 2.0f * s12 + C2, B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s11 + s22 + C2;
            const float den = B1 * B2;
            if constexpr (WEIGHTED) {            // the weight of the OUTPUT pixel on the SSIM value and on its three derivatives: the backward filter stays what it is
                const float wp = effective_weight(Wt[(size_t)gy * a.width + gx]);
                w_sum += wp;
                ssim_sum += wp * ((A1 * A2) / den);
                const size_t e = c * plane + (size_t)gy * a.width + gx;
                a.d_mu[e] = wp * (((2.0f * mu2 * A2 - 2.0f * mu2 * A1) * den - A1 * A2 * (2.0f * mu1 * B2 - 2.0f * mu1 * B1)) / (den * den));
                a.d_m11[e] = wp * (-(A1 * A2) / (B1 * B2 * B2));
                a.d_m12[e] = wp * (2.0f * A1 / den);
            } else {
                ssim_sum += (A1 * A2) / den;
                const size_t e = c * plane + (size_t)gy * a.width + gx;
                a.d_mu[e] = ((2.0f * mu2 * A2 - 2.0f * mu2 * A1) * den - A1 * A2 * (2.0f * mu1 * B2 - 2.0f * mu1 * B1)) / (den * den);
                a.d_m11[e] = -(A1 * A2) / (B1 * B2 * B2);
                a.d_m12[e] = 2.0f * A1 / den;
            }
        }
    }
    const float bl = block_sum_256(l1_sum, s_red);
    const float bs = block_sum_256(ssim_sum, s_red + 4);
    // per-workgroup partial sums, reduced by ssim_reduce_kernel: thousands of workgroups adding to two words would serialise on the
    // same-address atomic rate (measured 0.28 ms at 1080p), and a fixed order makes the loss reproducible
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

// The forward kernel's per-workgroup partial sums -> means and the scalar loss, in a fixed order (one 256-thread workgroup; s_red: 8 floats of LDS).
// WEIGHTED: `total_weight` = S (weight_total below, valid in every thread) takes the place of W H; S = 0 (nothing counts) is loss 0, L1 0, SSIM 1.
template <bool WEIGHTED>
__device__ __forceinline__ void reduce_loss_partials(const LossArgs& a, const unsigned n_blocks, float* s_red, const float total_weight = 0.0f) {
    const float2* __restrict__ part = reinterpret_cast<const float2*>(a.partials);
    float l1 = 0.0f, ss = 0.0f;
    for (unsigned b = threadIdx.x; b < n_blocks; b += 256u) { const float2 v = part[b]; l1 += v.x; ss += v.y; }
    const float tl = block_sum_256(l1, s_red);
    const float ts = block_sum_256(ss, s_red + 4);
    if (threadIdx.x == 255) {
        if constexpr (WEIGHTED) {
            const float n_total = 3.0f * total_weight;
            const float l1 = total_weight > 0.0f ? tl / n_total : 0.0f, ssim = total_weight > 0.0f ? ts / n_total : 1.0f;
            a.sums[0] = l1; a.sums[1] = ssim;
            a.sums[2] = a.lambda_l1 * l1 + a.lambda_dssim * (1.0f - ssim);
            a.total_weight[0] = total_weight;                                     // for a backward launch of its own (split and autograd forms)
        } else {
            const float n_total = 3.0f * static_cast<float>(a.width) * static_cast<float>(a.height);
            const float l1 = tl / n_total, ssim = ts / n_total;
            a.sums[0] = l1; a.sums[1] = ssim;                                         // means, and the scalar loss itself:
            a.sums[2] = a.lambda_l1 * l1 + a.lambda_dssim * (1.0f - ssim);           // no framework-side arithmetic kernels
        }
    }
}

// S = the sum of the forward tiles' weight sums (a.wpartials, n_tiles = one channel plane's tiles), in a fixed order by one 256-thread workgroup;
// valid in every thread. s_red: 4 floats of LDS that no other block_sum_256 of the kernel uses. Whoever needs S calls THIS, so every call form
// sees the same bits.
__device__ __forceinline__ float weight_total(const LossArgs& a, const unsigned n_tiles, float* s_red) {
    float w = 0.0f;
    for (unsigned b = threadIdx.x; b < n_tiles; b += 256u) w += a.wpartials[b];
    return block_sum_256(w, s_red);
}

#ifndef FGS_LOSS_SEPARATE_REDUCE
#define FGS_LOSS_SEPARATE_REDUCE 0       // A/B knob: 1 = the reduction as a launch of its own between the two filter kernels (until round 6)
#endif
// Loss value only (no gradient asked for: the autograd form, whose forward call must leave a valid value). With a gradient in the same call, workgroup 0 of
// the backward kernel does this on its way in (round 6: one launch less, -12 us per fused iteration, profiles/r06_ab_loss_reduce.txt).
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_reduce_kernel(const LossArgs a, const unsigned n_blocks) {
    __shared__ float s_red[WEIGHTED ? 12 : 8];
    if constexpr (WEIGHTED) reduce_loss_partials<true>(a, n_blocks, s_red, weight_total(a, n_blocks / 3u, s_red + 8));
    else reduce_loss_partials<false>(a, n_blocks, s_red);
}

// The weighted backward kernel needs S in EVERY workgroup, and S is a reduction over the forward launch: workgroup 0 cannot produce it for the others
// without them waiting on it (no inter-workgroup waits here). One call with a gradient therefore either launches ssim_reduce_kernel between the two
// filter kernels (0) or has every backward workgroup re-sum the tiles' weight sums itself (1: a couple of thousand L2-resident floats at 1080p, the
// same weight_total, so the same bits). Measured by tools/ab_weighted_loss.py (profiles/weighted_loss_ab.json).
#ifndef FGS_LOSS_WEIGHTED_RESUM
#define FGS_LOSS_WEIGHTED_RESUM 1
#endif

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

// WEIGHTED: the maps arrive weighted, so the filter is the unweighted one; the gradient is SELECTED to 0.0f where the weight is not positive (there x'
// is the target, not the image: nothing of the image is read into the result) and the L1 sign carries the pixel's weight elsewhere. 3 S takes the place of
// 3 W H: from a.total_weight, or with n_reduce != 0 re-summed by this workgroup (FGS_LOSS_WEIGHTED_RESUM).
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_backward_kernel(const LossArgs a, const GaussWindow gw, const unsigned n_reduce) {
    // The horizontally filtered maps go back into the memory of the staged region (dead once every thread has read its inputs into registers).
    constexpr int kMapFloats = kBwdRegionH * kBwdTileW;
    static_assert(3 * kBwdRegionH * kBwdRegionW >= 3 * kMapFloats, "the three filtered maps fit in the staged region");
    __shared__ float sd[3][kBwdRegionH][kBwdRegionW];
    float (*const hz)[kBwdRegionH][kBwdTileW] = reinterpret_cast<float (*)[kBwdRegionH][kBwdTileW]>(&sd[0][0][0]);
    [[maybe_unused]] float total_weight = 0.0f;
    if constexpr (WEIGHTED) {
        if (n_reduce != 0u) {                         // workgroup-uniform
            total_weight = weight_total(a, n_reduce / 3u, &sd[0][0][0] + 8);
            if (blockIdx.x == 0u) reduce_loss_partials<true>(a, n_reduce, &sd[0][0][0], total_weight);
            __syncthreads();
        } else total_weight = a.total_weight[0];
    } else {
        if (n_reduce != 0u && blockIdx.x == 0u) {        // the forward kernel's partial sums (complete: it is the launch in front) -> a.sums, by ONE workgroup
            reduce_loss_partials<false>(a, n_reduce, &sd[0][0][0]);
            __syncthreads();                              // the scratch words are staged over below
        }
    }
    unsigned tile_x, tile_y, chan, logical;
    if (!loss_tile_of<FGS_LOSS_XCD_BANDS_BWD != 0>(blockIdx.x, (a.width + kBwdTileW - 1) / kBwdTileW, (a.height + kBwdTileH - 1) / kBwdTileH, tile_x, tile_y, chan, logical)) return;     // workgroup-uniform
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
                    for (int t = 0; t < kTaps; ++t) f += gw.w[t] * p[o + t];
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
    const float n_total = WEIGHTED ? 3.0f * total_weight : 3.0f * static_cast<float>(a.width) * static_cast<float>(a.height);
    // the upstream gradient dL/dloss (a device scalar: no host read) is folded into the two constants -- a framework-level
    // `grad * upstream` is one more pass over the 25 MB gradient image (11 us per iteration at 1080p)
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
            for (int t = 0; t < kTaps; ++t) acc += gw.w[t] * col[o + t];
            v[m][o] = acc;
        }
    }
#pragma unroll
    for (int o = 0; o < kBwdRows; ++o) {
        const int gy = y0 + oy0 + o;
        if (gy >= a.height || gx >= a.width) continue;
        const size_t e = c * plane + (size_t)gy * a.width + gx;
        const float p = a.image[e], q = a.target[e];
        const float diff = p - q;
        const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
        if constexpr (WEIGHTED) {
            const float wp = a.weight[(size_t)gy * a.width + gx];
            const float g = ks * (v[0][o] + 2.0f * p * v[1][o] + q * v[2][o]) + kl * (effective_weight(wp) * sgn);
            a.grad[e] = wp > 0.0f ? g : 0.0f;                        // a select: p may be anything where the weight does not count
        } else {
            a.grad[e] = ks * (v[0][o] + 2.0f * p * v[1][o] + q * v[2][o]) + kl * sgn;
        }
    }
}

size_t l1_dssim_partials(int width, int height) {
    return 2 * static_cast<size_t>((width + kLossTileW - 1) / kLossTileW) * ((height + kLossTileH - 1) / kLossTileH) * 3;
}

static GaussWindow make_window() {
    GaussWindow gw;
    double w[kTaps], sum = 0.0;
    for (int i = 0; i < kTaps; ++i) { w[i] = std::exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += w[i]; }
    for (int i = 0; i < kTaps; ++i) gw.w[i] = static_cast<float>(w[i] / sum);
    return gw;
}

// 1-D launch of one workgroup per tile, rounded up so that every XCD gets the same number of workgroups (loss_tile_of; the spare ones return at once)
static dim3 loss_grid(const unsigned tiles) { return dim3((tiles + kXcds - 1u) / kXcds * kXcds); }

size_t l1_dssim_weight_partials(int width, int height) { return l1_dssim_partials(width, height) / 6; }

template <bool WEIGHTED>
static hipError_t launch_loss(const LossArgs& a, hipStream_t s) {
    constexpr bool kSeparateReduce = WEIGHTED ? !FGS_LOSS_WEIGHTED_RESUM : FGS_LOSS_SEPARATE_REDUCE != 0;
    const GaussWindow gw = make_window();
    const dim3 block(256);
    const unsigned tiles = static_cast<unsigned>((a.width + kLossTileW - 1) / kLossTileW) * static_cast<unsigned>((a.height + kLossTileH - 1) / kLossTileH) * 3u;
    hipLaunchKernelGGL(ssim_forward_kernel<WEIGHTED>, loss_grid(tiles), block, 0, s, a, gw);
    if (a.grad == nullptr || kSeparateReduce) {
        hipLaunchKernelGGL(ssim_reduce_kernel<WEIGHTED>, dim3(1), block, 0, s, a, tiles);
        if (a.grad == nullptr) return hipGetLastError();
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned tiles_b = static_cast<unsigned>((a.width + kBwdTileW - 1) / kBwdTileW) * static_cast<unsigned>((a.height + kBwdTileH - 1) / kBwdTileH) * 3u;
    hipLaunchKernelGGL(ssim_backward_kernel<WEIGHTED>, loss_grid(tiles_b), block, 0, s, a, gw, kSeparateReduce ? 0u : tiles);
    return hipGetLastError();
}

template <bool WEIGHTED>
static hipError_t launch_loss_backward(const LossArgs& a, hipStream_t s) {
    const GaussWindow gw = make_window();
    const unsigned tiles_b = static_cast<unsigned>((a.width + kBwdTileW - 1) / kBwdTileW) * static_cast<unsigned>((a.height + kBwdTileH - 1) / kBwdTileH) * 3u;
    hipLaunchKernelGGL(ssim_backward_kernel<WEIGHTED>, loss_grid(tiles_b), dim3(256), 0, s, a, gw, 0u);
    return hipGetLastError();
}

// a.weight != nullptr: the weighted instantiations (a.wpartials and a.total_weight are then scratch too)
hipError_t launch_l1_dssim(const LossArgs& a, hipStream_t s) { return a.weight != nullptr ? launch_loss<true>(a, s) : launch_loss<false>(a, s); }
hipError_t launch_l1_dssim_backward(const LossArgs& a, hipStream_t s) { return a.weight != nullptr ? launch_loss_backward<true>(a, s) : launch_loss_backward<false>(a, s); }

}  // namespace fgs

// Feature-channel blend of the training render for gfx950: M_c(p) = sum_i w_i f_{i,c} over exactly the (pixel, Gaussian) pairs K10 blended, with
// w_i = T_before_i alpha_i, for F per-Gaussian channels of any sign (fgs_blend_features), and its backward pass (fgs_backward_features).
//
// Both kernels are second walks over the per-tile instance lists K10 built, in the shape of pruning_scores_kernel (blend_forward.hip): one workgroup
// per tile, K10's wave / sub-tile layout (3 wave64, each a 16x4 strip = two 8x4 sub-tiles with the per-sub-tile cull), records staged 192 at a time
// through LDS, the feature rows of the batch staged beside them. alpha is recomputed with K10's expression operation for operation (see the comment
// in blend_backward.hip: the passes must agree on every alpha >= 1/255 decision), and a pixel never walks beyond its n_processed, so the pairs are
// K10's pairs.
//
// Channels: a lane accumulates CW of them per walk (CW = 4, 8 or 16: a row of 16 channels is one 64-byte line) and the list is walked again for the
// next group of a wider F; a ragged last group is padded with zeros in LDS. The walks of the backward pass are independent as well, because
// dL/dalpha is linear in the upstream gradient: with u_i = sum_c f_{i,c} gF_c(p) over the channels of the group and S_i = sum_{j>i} w_j u_j
// = sum_c M_c gF_c - prefix_i, the group's share is dL/dalpha_i = T_i u_i - S_i / (1 - alpha_i) -- K11's expression with cg := u_i and no background
// term -- and the shares of the groups add up in the accumulator records. The forward map takes the place of per-bucket feature checkpoints.
//
// Backward outputs: the pixels of a wave hold the SAME Gaussian, so the CW sums w gF_c and the six geometry sums of K11 (hh, hh dx, hh dy, hh dx^2,
// hh dx dy, hh dy^2 with hh = -alpha/2 dL/dalpha) are reduced over the wave and leave through ONE atomic instruction per (Gaussian, wave): lanes
// 0..CW-1 add into the Gaussian's row of grad_features, the six lanes behind them into words 0..5 of its accumulator record -- its own record for a
// hot Gaussian too (fgs_config.h: correct, only slower). The kernel runs behind K11's fold of the hot replicas and in front of K12.
#include "fgs_kernels.h"
#include <fgs_wave.h>
#include "fgs_k10_mappings.h"   // tile_of_workgroup: the columns mapping of the product's K10

namespace fgs {
namespace {

struct TileWalk {                       // what both kernels know of their pixel and tile
    unsigned tile, tid, wave, lane, half, local;
    bool inside;
    size_t pix;
    float pxf, pyf;
    unsigned sub_y0, sub_y1, subl_x0, subl_x1, subr_x1;
    uint2 range;
};

__device__ __forceinline__ TileWalk tile_walk(const FeatureBlendArgs& a, const unsigned tile) {
    TileWalk w;
    w.tile = tile;
    const unsigned tile_x = tile % a.grid_w, tile_y = tile / a.grid_w;
    w.tid = threadIdx.x; w.wave = w.tid >> 6; w.lane = w.tid & 63u; w.half = w.lane >> 5;
    const unsigned lx = w.half * kSubtileW + (w.lane & 7u), ly = w.wave * kSubtileH + ((w.lane >> 3) & 3u);
    const unsigned px = tile_x * kTileW + lx, py = tile_y * kTileH + ly;
    w.inside = px < a.width && py < a.height;
    w.local = ly * kTileW + lx;
    w.pix = (size_t)a.width * py + px;
    w.pxf = static_cast<float>(px) + 0.5f; w.pyf = static_cast<float>(py) + 0.5f;
    w.sub_y0 = tile_y * kTileH + w.wave * kSubtileH; w.sub_y1 = w.sub_y0 + kSubtileH;
    w.subl_x0 = tile_x * kTileW; w.subl_x1 = w.subl_x0 + kSubtileW; w.subr_x1 = w.subl_x1 + kSubtileW;
    w.range = a.ranges[tile];
    return w;
}

// One batch of up to 192 list entries into LDS: the two record rows the walk reads, the packed bounds, the primitive index, and -- behind a barrier,
// consecutive threads reading consecutive floats of a row -- channels [g0, g0 + CW) of the feature rows, zero beyond F.
template <int CW>
__device__ __forceinline__ void stage_batch(const FeatureBlendArgs& a, const TileWalk& w, const unsigned batch_start, const unsigned batch, const unsigned g0,
                                            float4* s_a, float4* s_b, uint2* s_box, uint32_t* s_prim, float* s_feat) {
    if (w.tid < batch) {
        const uint32_t prim = a.inst_prims[w.range.x + batch_start + w.tid];
        const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
        const float4 r2 = r[2];
        s_a[w.tid] = r[0]; s_b[w.tid] = r[1]; s_box[w.tid] = make_uint2(__float_as_uint(r2.y), __float_as_uint(r2.z)); s_prim[w.tid] = prim;
    }
    __syncthreads();
    for (unsigned e = w.tid; e < batch * CW; e += kBlendBlock) {
        const unsigned row = e / CW, c = g0 + (e % CW);
        s_feat[e] = c < a.n_channels ? a.features[(size_t)s_prim[row] * a.n_channels + c] : 0.0f;
    }
    __syncthreads();
}

// the per-sub-tile cull of K10 (kf:445-451) for entry chunk + lane of the batch
__device__ __forceinline__ void cull_chunk(const TileWalk& w, const uint2* s_box, const unsigned j, const unsigned batch, uint64_t& mine, uint64_t& pending) {
    bool in_l = false, in_r = false;
    if (j < batch) {
        const uint32_t bx = s_box[j].x, by = s_box[j].y;
        const unsigned x_min = bx & 0xffffu, x_max = bx >> 16, y_min = by & 0xffffu, y_max = by >> 16;
        const bool in_y = y_min < w.sub_y1 && w.sub_y0 < y_max;
        in_l = in_y && x_min < w.subl_x1 && w.subl_x0 < x_max;
        in_r = in_y && x_min < w.subr_x1 && w.subl_x1 < x_max;
    }
    const uint64_t mask_l = wave_ballot(in_l), mask_r = wave_ballot(in_r);
    mine = w.half ? mask_r : mask_l;
    pending = mask_l | mask_r;
}

}  // namespace

template <int CW>
__global__ void __launch_bounds__(kBlendBlock) blend_features_kernel(const FeatureBlendArgs a) {
    const unsigned tile = tile_of_workgroup(blockIdx.x, a.grid_w, a.n_tiles, kColumnsTopDown, nullptr, a.grid_h);
    if (tile >= a.n_tiles) return;
    const TileWalk w = tile_walk(a, tile);
    __shared__ float4 s_a[kBlendBlock], s_b[kBlendBlock];
    __shared__ uint2 s_box[kBlendBlock];
    __shared__ uint32_t s_prim[kBlendBlock];
    __shared__ __attribute__((aligned(16))) float s_feat[kBlendBlock * CW];
    // nobody blended behind the tile's max_n_processed, and this pixel nothing at or behind its own n_processed (0 outside the image)
    const unsigned n_walk = min(w.range.y - w.range.x, a.max_n_processed[tile]);
    const unsigned n_proc = w.inside ? a.n_processed[(size_t)tile * kTilePixels + w.local] : 0u;
    const size_t n_pixels = (size_t)a.width * a.height;

    for (unsigned g0 = 0; g0 < a.n_channels; g0 += CW) {
        float m[CW];
#pragma unroll
        for (int c = 0; c < CW; ++c) m[c] = 0.0f;
        float T = 1.0f;
        for (unsigned batch_start = 0; batch_start < n_walk; batch_start += kBlendBlock) {
            if (__syncthreads_and((batch_start >= n_proc || T < kTransmittanceThreshold) ? 1 : 0)) break;
            const unsigned batch = min(static_cast<unsigned>(kBlendBlock), n_walk - batch_start);
            stage_batch<CW>(a, w, batch_start, batch, g0, s_a, s_b, s_box, s_prim, s_feat);
            for (unsigned chunk = 0; chunk < batch; chunk += kWave) {
                uint64_t mine, pending;
                cull_chunk(w, s_box, chunk + w.lane, batch, mine, pending);
                if (wave_ballot(batch_start + chunk < n_proc && T >= kTransmittanceThreshold) == 0) pending = 0;
                while (pending != 0) {
                    const int k = __ffsll(static_cast<unsigned long long>(pending)) - 1;
                    pending &= pending - 1;
                    const unsigned jj = chunk + static_cast<unsigned>(k);
                    const float4 ga = s_a[jj], gb = s_b[jj];
                    const float dx = ga.x - w.pxf, dy = ga.y - w.pyf;
                    const float power = -0.5f * (ga.z * dx * dx + gb.x * dy * dy) - ga.w * dx * dy;
                    const float gauss = __expf(fminf(power, 0.0f));
                    const float alpha = gb.y * gauss;
                    if (((mine >> k) & 1ull) != 0 && batch_start + jj < n_proc && T >= kTransmittanceThreshold && alpha >= kMinAlphaThreshold) {
                        const float wgt = T * alpha;
                        const float4* f = reinterpret_cast<const float4*>(s_feat + jj * CW);
#pragma unroll
                        for (int q = 0; q < CW / 4; ++q) {
                            const float4 v = f[q];
                            m[4 * q] += wgt * v.x; m[4 * q + 1] += wgt * v.y; m[4 * q + 2] += wgt * v.z; m[4 * q + 3] += wgt * v.w;
                        }
                        T *= 1.0f - alpha;
                    }
                }
            }
        }
        if (w.inside) {
#pragma unroll
            for (int c = 0; c < CW; ++c)
                if (g0 + c < a.n_channels) a.feature_map[(size_t)(g0 + c) * n_pixels + w.pix] = m[c];
        }
    }
}

template <int CW, bool GEO>
__global__ void __launch_bounds__(kBlendBlock) blend_features_backward_kernel(const FeatureBlendArgs a) {
    const unsigned tile = tile_of_workgroup(blockIdx.x, a.grid_w, a.n_tiles, kColumnsTopDown, nullptr, a.grid_h);
    if (tile >= a.n_tiles) return;
    const TileWalk w = tile_walk(a, tile);
    __shared__ float4 s_a[kBlendBlock], s_b[kBlendBlock];
    __shared__ uint2 s_box[kBlendBlock];
    __shared__ uint32_t s_prim[kBlendBlock];
    __shared__ __attribute__((aligned(16))) float s_feat[kBlendBlock * CW];
    constexpr unsigned kOut = CW + 6;                               // the sums of one (Gaussian, wave): CW feature words, six record words
    __shared__ float s_out[kBlendBlock / kWave][kOut + 2];
    const unsigned n_walk = min(w.range.y - w.range.x, a.max_n_processed[tile]);
    const unsigned n_proc = w.inside ? a.n_processed[(size_t)tile * kTilePixels + w.local] : 0u;
    const size_t n_pixels = (size_t)a.width * a.height;
    float* const out = s_out[w.wave];

    for (unsigned g0 = 0; g0 < a.n_channels; g0 += CW) {
        // the pixel's upstream gradient of the group and S in front of the first Gaussian: sum_c M_c gF_c
        float g[CW];
        float rem = 0.0f;
        bool any = false;
#pragma unroll
        for (int c = 0; c < CW; ++c) {
            g[c] = 0.0f;
            if (w.inside && n_proc != 0u && g0 + c < a.n_channels) {
                g[c] = a.grad_feature_map[(size_t)(g0 + c) * n_pixels + w.pix];
                rem += a.feature_map_in[(size_t)(g0 + c) * n_pixels + w.pix] * g[c];
                any = any || g[c] != 0.0f;
            }
        }
        // a pixel whose gF is zero in every channel of the group contributes zeros to every sum: it is finished from the start
        const unsigned n_mine = any ? n_proc : 0u;
        float T = 1.0f;
        for (unsigned batch_start = 0; batch_start < n_walk; batch_start += kBlendBlock) {
            if (__syncthreads_and((batch_start >= n_mine || T < kTransmittanceThreshold) ? 1 : 0)) break;
            const unsigned batch = min(static_cast<unsigned>(kBlendBlock), n_walk - batch_start);
            stage_batch<CW>(a, w, batch_start, batch, g0, s_a, s_b, s_box, s_prim, s_feat);
            for (unsigned chunk = 0; chunk < batch; chunk += kWave) {
                uint64_t mine, pending;
                cull_chunk(w, s_box, chunk + w.lane, batch, mine, pending);
                if (wave_ballot(batch_start + chunk < n_mine && T >= kTransmittanceThreshold) == 0) pending = 0;
                while (pending != 0) {
                    const int k = __ffsll(static_cast<unsigned long long>(pending)) - 1;
                    pending &= pending - 1;
                    const unsigned jj = chunk + static_cast<unsigned>(k);
                    const float4 ga = s_a[jj], gb = s_b[jj];
                    const float dx = ga.x - w.pxf, dy = ga.y - w.pyf;
                    const float power = -0.5f * (ga.z * dx * dx + gb.x * dy * dy) - ga.w * dx * dy;
                    const float gauss = __expf(fminf(power, 0.0f));
                    const float alpha = gb.y * gauss;
                    const bool contrib = ((mine >> k) & 1ull) != 0 && batch_start + jj < n_mine && T >= kTransmittanceThreshold && alpha >= kMinAlphaThreshold;
                    if (wave_ballot(contrib) == 0) continue;                        // wave-uniform: nobody in this wave blended the pair
                    float wgt = 0.0f, hh = 0.0f;
                    if (contrib) {
                        wgt = T * alpha;
                        const float4* f = reinterpret_cast<const float4*>(s_feat + jj * CW);
                        float u = 0.0f;
#pragma unroll
                        for (int q = 0; q < CW / 4; ++q) {
                            const float4 v = f[q];
                            u += v.x * g[4 * q] + v.y * g[4 * q + 1] + v.z * g[4 * q + 2] + v.w * g[4 * q + 3];
                        }
                        rem -= wgt * u;                                             // S_i: what is still to come behind this Gaussian
                        const float oma = 1.0f - alpha;
                        const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
                        const float dl_dalpha = T * u - rem * oma_rcp;
                        hh = (-0.5f * alpha) * dl_dalpha;
                        T *= oma;
                    }
                    // convergent from here: every lane of the wave takes part in the reductions, the lanes that did not blend with zeros
#pragma unroll
                    for (int c = 0; c < CW; ++c) {
                        const float total = wave_sum_to_lane63(wgt * g[c]);
                        if (w.lane == 63u) out[c] = total;
                    }
                    if (GEO) {
                        const float t = hh * dx, v = hh * dy;
                        const float a_h = wave_sum_to_lane63(hh), a_x = wave_sum_to_lane63(t), a_y = wave_sum_to_lane63(v);
                        const float a_xx = wave_sum_to_lane63(t * dx), a_xy = wave_sum_to_lane63(t * dy), a_yy = wave_sum_to_lane63(v * dy);
                        if (w.lane == 63u) {                                       // the record words as K11's flush forms them (blend_backward.hip)
                            const float ca = ga.z, cb = ga.w, cc = gb.x, op = gb.y;
                            out[CW] = 2.0f * (ca * a_x + cb * a_y); out[CW + 1] = 2.0f * (cb * a_x + cc * a_y);
                            out[CW + 2] = a_xx; out[CW + 3] = a_xy; out[CW + 4] = a_yy;
                            out[CW + 5] = a.proper_aa ? -2.0f * a_h / op : -2.0f * a_h * (1.0f - op);
                        }
                    }
                    wave_lds_fence();
                    const uint32_t prim = s_prim[jj];
                    if (w.lane < (GEO ? kOut : static_cast<unsigned>(CW))) {
                        const float total = out[w.lane];
                        const bool feature = w.lane < static_cast<unsigned>(CW);
                        if (total != 0.0f && (!feature || g0 + w.lane < a.n_channels))
                            unsafeAtomicAdd(feature ? a.grad_features + ((size_t)prim * a.n_channels + g0 + w.lane)
                                                    : a.acc + ((size_t)prim * kAccRecordWords + (w.lane - CW)), total);
                    }
                    wave_lds_fence();                                              // the next pair overwrites `out`
                }
            }
        }
    }
}

template <int CW>
static void launch_backward_width(const FeatureBlendArgs& a, const dim3 grid, hipStream_t s) {
    if (a.detach_geometry) hipLaunchKernelGGL((blend_features_backward_kernel<CW, false>), grid, dim3(kBlendBlock), 0, s, a);
    else hipLaunchKernelGGL((blend_features_backward_kernel<CW, true>), grid, dim3(kBlendBlock), 0, s, a);
}

// the grid of the columns mapping: its tiles and its padding workgroups
static dim3 feature_grid(const FeatureBlendArgs& a) { return dim3(columns_grid(a.grid_w, a.grid_h)); }

hipError_t launch_blend_features(const FeatureBlendArgs& a, hipStream_t s) {
    const dim3 grid = feature_grid(a), block(kBlendBlock);
    if (a.n_channels <= 4u) hipLaunchKernelGGL(blend_features_kernel<4>, grid, block, 0, s, a);
    else if (a.n_channels <= 8u) hipLaunchKernelGGL(blend_features_kernel<8>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(blend_features_kernel<16>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend_features_backward(const FeatureBlendArgs& a, hipStream_t s) {
    const dim3 grid = feature_grid(a);
    if (a.n_channels <= 4u) launch_backward_width<4>(a, grid, s);
    else if (a.n_channels <= 8u) launch_backward_width<8>(a, grid, s);
    else launch_backward_width<16>(a, grid, s);
    return hipGetLastError();
}

}  // namespace fgs

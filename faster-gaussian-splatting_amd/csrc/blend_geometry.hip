// One render for the 2DGS regularisers of the training pass, for gfx950: per pixel, over exactly the (pixel, Gaussian) pairs K10 blended, in K10's
// order i = 1..n, with w_i = T_before_i alpha_i, a per-Gaussian depth value t_i and five per-Gaussian surface features f_{i,c},
//     X   = sum_a sum_b w_a w_b |t_a - t_b| = 2 sum_i w_i (t_i A_{i-1} - D_{i-1})      the depth-distortion map of blend_distortion.hip
//     M_c = sum_i w_i f_{i,c},  c = 0..4                                              the surface map of blend_features.hip (F = 5)
// in ONE walk (fgs_blend_geometry), and the backward pass of both in one walk (fgs_backward_geometry). Definitions of t (linear / normalized), the
// prefixes A and D, the shift of t by the tile's origin t0 and the closed forms of dX/dw_i and dX/dt_i are blend_distortion.hip's; u_i and the
// feature gradient are blend_features.hip's. Those two units stay what they are: their TileWalk, staging and cull are restated here.
//
// Both kernels are second walks over K10's per-tile instance lists: one workgroup per tile, K10's wave / sub-tile layout and the columns mapping,
// records staged 192 at a time through LDS, alpha recomputed with K10's expression operation for operation, no pixel beyond its n_processed.
// Staged per entry: the two record rows, the packed bounds, the primitive index, (t - t0, dt/dz), and the five features padded to two float4.
//
// A is a register of its own and a plane of its own (fgs_geometry.h): M_4 equals it only when channel 4 holds ones, which the surface features do and
// general channels do not. With it X is blend_distortion's X bit for bit and M is blend_features' M bit for bit whatever the channels hold.
//
// Backward: dL/dalpha is linear in the upstream gradients, so with c_i = gX e_i + u_i, e_i = 2 [t_i (2 A_{i-1} - A_n) - 2 D_{i-1} + D_n],
// u_i = sum_c f_{i,c} gM_c(p) and S_i = sum_{j>i} w_j c_j = gX 2 X + sum_c M_c gM_c - sum_{j<=i} w_j c_j:
//     dL/dalpha_i = T_i c_i - S_i / max(1 - alpha_i, 1e-6)
// -- K11's expression with the per-pair dot replaced by c_i and no background term. Per blended pair the wave reduces twelve sums: the six geometry
// sums of K11 (hh, hh dx, hh dy, hh dx^2, hh dx dy, hh dy^2 with hh = -alpha/2 dL/dalpha), dL/dz = gX dX/dt_i dt_i/dz_i, and the five w_i gM_c. They
// leave through ONE atomic instruction per (Gaussian, wave): lanes 0..5 into words 0..5 of the Gaussian's accumulator record (its own record for a
// hot Gaussian too), lane 6 into acc_z, lanes 7..11 into the Gaussian's row of grad_surface_features. The kernel runs behind K11's folds and in
// front of K12. An absent upstream gradient (WX / WM false) drops its sums and its lanes at compile time.
#include "fgs_geometry.h"
#include <fgs_wave.h>
#include "fgs_k10_mappings.h"   // tile_of_workgroup: the columns mapping of the product's K10

namespace fgs {
namespace {

constexpr unsigned kF = kGeometryChannels;

struct TileWalk {                       // what both kernels know of their pixel and tile
    unsigned tile, tid, wave, lane, half, local;
    bool inside;
    size_t pix;
    float pxf, pyf;
    unsigned sub_y0, sub_y1, subl_x0, subl_x1, subr_x1;
    uint2 range;
};

__device__ __forceinline__ TileWalk tile_walk(const GeometryArgs& a, const unsigned tile) {
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

__device__ __forceinline__ Camera depth_camera(const GeometryArgs& a) {        // the third row of w2c is all view_depth reads
    Camera cam;
    cam.r3[0] = a.w2c[8]; cam.r3[1] = a.w2c[9]; cam.r3[2] = a.w2c[10]; cam.r3[3] = a.w2c[11];
    return cam;
}

// z of the first entry of the tile's list: the tile-uniform origin of t (0 for an empty list, which is never walked)
__device__ __forceinline__ float tile_origin_depth(const GeometryArgs& a, const Camera& cam, const TileWalk& w) {
    if (w.range.y <= w.range.x) return 0.0f;
    const float* m = a.means + 3 * (size_t)a.inst_prims[w.range.x];
    return view_depth(cam, m[0], m[1], m[2]);
}

struct Stage {                          // one batch of up to 192 list entries in LDS
    float4* rec_a; float4* rec_b; uint2* box; uint32_t* prim; float2* t; float4* feat;     // feat: two float4 per entry, (f0 f1 f2 f3) (f4 0 0 0)
};

// The two record rows the walk reads, the packed bounds, the primitive index, (t - t0, dt/dz) of the entry exactly as blend_distortion.hip forms them
// (z >= near > 0 for every listed Gaussian, K1's depth cull), and the entry's five features.
__device__ __forceinline__ void stage_batch(const GeometryArgs& a, const TileWalk& w, const Camera& cam, const float z0, const unsigned batch_start,
                                            const unsigned batch, const Stage& s) {
    if (w.tid < batch) {
        const uint32_t prim = a.inst_prims[w.range.x + batch_start + w.tid];
        const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
        const float4 r2 = r[2];
        s.rec_a[w.tid] = r[0]; s.rec_b[w.tid] = r[1]; s.box[w.tid] = make_uint2(__float_as_uint(r2.y), __float_as_uint(r2.z)); s.prim[w.tid] = prim;
        const float* m = a.means + 3 * (size_t)prim;
        const float z = view_depth(cam, m[0], m[1], m[2]);
        float t = z - z0, dt = 1.0f;
        if (a.normalized) { t = a.depth_scale * t / (z * z0); dt = a.depth_scale / (z * z); }
        s.t[w.tid] = make_float2(t, dt);
        const float* f = a.features + kF * (size_t)prim;
        s.feat[2 * w.tid] = make_float4(f[0], f[1], f[2], f[3]);
        s.feat[2 * w.tid + 1] = make_float4(f[4], 0.0f, 0.0f, 0.0f);
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

__global__ void __launch_bounds__(kBlendBlock) blend_geometry_kernel(const GeometryArgs a) {
    const unsigned tile = tile_of_workgroup(blockIdx.x, a.grid_w, a.n_tiles, kColumnsTopDown, nullptr, a.grid_h);
    if (tile >= a.n_tiles) return;
    const TileWalk w = tile_walk(a, tile);
    __shared__ float4 s_a[kBlendBlock], s_b[kBlendBlock], s_feat[2 * kBlendBlock];
    __shared__ uint2 s_box[kBlendBlock];
    __shared__ uint32_t s_prim[kBlendBlock];
    __shared__ float2 s_t[kBlendBlock];
    const Stage stage{s_a, s_b, s_box, s_prim, s_t, s_feat};
    // nobody blended behind the tile's max_n_processed, and this pixel nothing at or behind its own n_processed (0 outside the image)
    const unsigned n_walk = min(w.range.y - w.range.x, a.max_n_processed[tile]);
    const unsigned n_proc = w.inside ? a.n_processed[(size_t)tile * kTilePixels + w.local] : 0u;
    const Camera cam = depth_camera(a);
    const float z0 = tile_origin_depth(a, cam, w);

    float T = 1.0f, A = 0.0f, D = 0.0f, X = 0.0f;
    float m[kF];
#pragma unroll
    for (unsigned c = 0; c < kF; ++c) m[c] = 0.0f;
    for (unsigned batch_start = 0; batch_start < n_walk; batch_start += kBlendBlock) {
        if (__syncthreads_and((batch_start >= n_proc || T < kTransmittanceThreshold) ? 1 : 0)) break;
        const unsigned batch = min(static_cast<unsigned>(kBlendBlock), n_walk - batch_start);
        stage_batch(a, w, cam, z0, batch_start, batch, stage);
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
                    const float wgt = T * alpha, t = s_t[jj].x;
                    const float4 f0 = s_feat[2 * jj];
                    const float f4 = s_feat[2 * jj + 1].x;
                    X += wgt * (t * A - D);             // exactly 0 for the first Gaussian of the pixel: A = D = 0
                    m[0] += wgt * f0.x; m[1] += wgt * f0.y; m[2] += wgt * f0.z; m[3] += wgt * f0.w; m[4] += wgt * f4;
                    A += wgt; D += wgt * t;
                    T *= 1.0f - alpha;
                }
            }
        }
    }
    if (w.inside) {
        const size_t n_pixels = (size_t)a.width * a.height;
        a.state[w.pix] = 2.0f * X; a.state[kGeometryPlaneD * n_pixels + w.pix] = D; a.state[kGeometryPlaneA * n_pixels + w.pix] = A;
#pragma unroll
        for (unsigned c = 0; c < kF; ++c) a.state[(kGeometryPlaneM + c) * n_pixels + w.pix] = m[c];
    }
}

// WX: there is an upstream gradient of X (a.grad_x); WM: of M (a.grad_m). At least one of them.
template <bool WX, bool WM>
__global__ void __launch_bounds__(kBlendBlock) blend_geometry_backward_kernel(const GeometryArgs a) {
    const unsigned tile = tile_of_workgroup(blockIdx.x, a.grid_w, a.n_tiles, kColumnsTopDown, nullptr, a.grid_h);
    if (tile >= a.n_tiles) return;
    const TileWalk w = tile_walk(a, tile);
    __shared__ float4 s_a[kBlendBlock], s_b[kBlendBlock], s_feat[2 * kBlendBlock];
    __shared__ uint2 s_box[kBlendBlock];
    __shared__ uint32_t s_prim[kBlendBlock];
    __shared__ float2 s_t[kBlendBlock];
    const Stage stage{s_a, s_b, s_box, s_prim, s_t, s_feat};
    constexpr unsigned kOut = 7 + kF;                               // the sums of one (Gaussian, wave): six record words, dL/dz, five feature words
    __shared__ float s_out[kBlendBlock / kWave][16];
    const unsigned n_walk = min(w.range.y - w.range.x, a.max_n_processed[tile]);
    const unsigned n_proc = w.inside ? a.n_processed[(size_t)tile * kTilePixels + w.local] : 0u;
    const size_t n_pixels = (size_t)a.width * a.height;
    const Camera cam = depth_camera(a);
    const float z0 = tile_origin_depth(a, cam, w);
    float* const out = s_out[w.wave];
    // the lanes that carry a sum out: the record words always, dL/dz and the feature words with their term
    const bool carries = w.lane < 6u || (WX && w.lane == 6u) || (WM && w.lane >= 7u && w.lane < kOut);

    // the pixel's upstream gradients, its final sums, and S in front of the first Gaussian: gX 2 X + sum_c M_c gM_c
    float g = 0.0f, a_n = 0.0f, d_n = 0.0f, rem = 0.0f;
    float gm[kF];
#pragma unroll
    for (unsigned c = 0; c < kF; ++c) gm[c] = 0.0f;
    bool any = false;
    if (w.inside && n_proc != 0u) {
        if (WX) {
            g = a.grad_x[w.pix];
            a_n = a.state_in[kGeometryPlaneA * n_pixels + w.pix]; d_n = a.state_in[kGeometryPlaneD * n_pixels + w.pix];
            rem = 2.0f * a.state_in[w.pix] * g;
            any = g != 0.0f;
        }
        if (WM) {
#pragma unroll
            for (unsigned c = 0; c < kF; ++c) {
                gm[c] = a.grad_m[c * n_pixels + w.pix];
                rem += a.state_in[(kGeometryPlaneM + c) * n_pixels + w.pix] * gm[c];
                any = any || gm[c] != 0.0f;
            }
        }
    }
    // a pixel whose gX and gM_c are all zero contributes zeros to every sum: it is finished from the start
    const unsigned n_mine = any ? n_proc : 0u;
    float T = 1.0f, A = 0.0f, D = 0.0f;
    for (unsigned batch_start = 0; batch_start < n_walk; batch_start += kBlendBlock) {
        if (__syncthreads_and((batch_start >= n_mine || T < kTransmittanceThreshold) ? 1 : 0)) break;
        const unsigned batch = min(static_cast<unsigned>(kBlendBlock), n_walk - batch_start);
        stage_batch(a, w, cam, z0, batch_start, batch, stage);
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
                float wgt = 0.0f, hh = 0.0f, dz = 0.0f;
                if (contrib) {
                    wgt = T * alpha;
                    float c_i = 0.0f;
                    if (WX) {
                        const float2 td = s_t[jj];
                        c_i = 2.0f * g * (td.x * (2.0f * A - a_n) - 2.0f * D + d_n);                // gX dX/dw_i
                        dz = 2.0f * g * wgt * (2.0f * A + wgt - a_n) * td.y;                        // gX dX/dt_i dt_i/dz_i
                        A += wgt; D += wgt * td.x;
                    }
                    if (WM) {
                        const float4 f0 = s_feat[2 * jj];
                        const float f4 = s_feat[2 * jj + 1].x;
                        c_i += f0.x * gm[0] + f0.y * gm[1] + f0.z * gm[2] + f0.w * gm[3] + f4 * gm[4];   // u_i
                    }
                    rem -= wgt * c_i;                                               // S_i: what is still to come behind this Gaussian
                    const float oma = 1.0f - alpha;
                    const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
                    const float dl_dalpha = T * c_i - rem * oma_rcp;
                    hh = (-0.5f * alpha) * dl_dalpha;
                    T *= oma;
                }
                // convergent from here: every lane of the wave takes part in the reductions, the lanes that did not blend with zeros
                const float t = hh * dx, v = hh * dy;
                const float a_h = wave_sum_to_lane63(hh), a_x = wave_sum_to_lane63(t), a_y = wave_sum_to_lane63(v);
                const float a_xx = wave_sum_to_lane63(t * dx), a_xy = wave_sum_to_lane63(t * dy), a_yy = wave_sum_to_lane63(v * dy);
                if (WX) {
                    const float a_z = wave_sum_to_lane63(dz);
                    if (w.lane == 63u) out[6] = a_z;
                }
                if (WM) {
#pragma unroll
                    for (unsigned c = 0; c < kF; ++c) {
                        const float total = wave_sum_to_lane63(wgt * gm[c]);
                        if (w.lane == 63u) out[7 + c] = total;
                    }
                }
                if (w.lane == 63u) {                                           // the record words as K11's flush forms them (blend_backward.hip)
                    const float ca = ga.z, cb = ga.w, cc = gb.x, op = gb.y;
                    out[0] = 2.0f * (ca * a_x + cb * a_y); out[1] = 2.0f * (cb * a_x + cc * a_y);
                    out[2] = a_xx; out[3] = a_xy; out[4] = a_yy;
                    out[5] = a.proper_aa ? -2.0f * a_h / op : -2.0f * a_h * (1.0f - op);
                }
                wave_lds_fence();
                const uint32_t prim = s_prim[jj];
                if (carries) {
                    const float total = out[w.lane];
                    if (total != 0.0f) {
                        float* const dst = w.lane < 6u ? a.acc + ((size_t)prim * kAccRecordWords + w.lane)
                                         : w.lane == 6u ? a.acc_z + prim
                                                        : a.grad_features + ((size_t)prim * kF + (w.lane - 7u));
                        unsafeAtomicAdd(dst, total);
                    }
                }
                wave_lds_fence();                                              // the next pair overwrites `out`
            }
        }
    }
}

// the grid of the columns mapping: its tiles and its padding workgroups
static dim3 geometry_grid(const GeometryArgs& a) { return dim3(columns_grid(a.grid_w, a.grid_h)); }

hipError_t launch_blend_geometry(const GeometryArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(blend_geometry_kernel, geometry_grid(a), dim3(kBlendBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend_geometry_backward(const GeometryArgs& a, hipStream_t s) {
    const dim3 grid = geometry_grid(a), block(kBlendBlock);
    if (a.grad_x && a.grad_m) hipLaunchKernelGGL((blend_geometry_backward_kernel<true, true>), grid, block, 0, s, a);
    else if (a.grad_x) hipLaunchKernelGGL((blend_geometry_backward_kernel<true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((blend_geometry_backward_kernel<false, true>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace fgs

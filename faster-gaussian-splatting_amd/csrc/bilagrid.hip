// Per-view bilateral-grid colour correction between the rasterizer and the loss, for gfx950: the affine colour transform of "Bilateral Guided
// Radiance Field Processing" (the `bilagrid` of gsplat's trainer). A grid G [12, L, Hg, Wg] holds a 3 x 4 matrix [A | b] per lattice point (channel
// 4 i + j = entry (i, j)); a pixel reads its matrix by trilinear interpolation at (guide, y, x), guide = clamp(luma(C), 0, 1), and leaves as A C + b.
// The definition is F.grid_sample(G[None], 2 (x, y, g) - 1, bilinear, align_corners=True, padding_mode='border') followed by the matrix product
// (tests/bilagrid_cases.py holds the kernels to that formulation in fp64).
//
//   bilagrid_slice_kernel          : a 64 x 16 pixel tile per 256-thread workgroup, 4 adjacent pixels per thread (one float4 per channel when the rows
//                                    allow it). The lattice points under the tile -- all L planes -- are staged into LDS channel-last (a corner = 12
//                                    consecutive floats = three 16-byte reads) when they fit kBgStageFloats; otherwise every corner is read from
//                                    global memory (the whole grid is ~100 KB: it stays in L2). Which of the two a launch takes is decided on the
//                                    host for the whole launch (bilagrid_staged), so it can be asked for.
//   bilagrid_slice_backward_kernel : the same tiling. dL/dimage is written per pixel (deterministic). dL/dgrid is summed in LDS with float atomics over
//                                    up to kBgMaxReplicas copies of the staged part (lane l adds to copy l % n: neighbouring pixels share their corners)
//                                    and leaves once per workgroup through global float atomics into a
//                                    channel-last scratch grid the entry point has zeroed; without staging the adds go to that scratch grid directly.
//                                    Measured at 1080p, 16 x 16 x 8 (profiles/bilagrid_ab.json): 1.01 ms with the grid gradient, 0.023 ms without -- the 96
//                                    LDS float adds per pixel set the time (~200 cycles per wave instruction; 1.27 ms with one copy; no change from
//                                    giving every lane of a copy another corner order), not the 75 MB of traffic.
//   bilagrid_transpose_kernel      : scratch grid [L, Hg, Wg, 12] -> dL/dgrid [12, L, Hg, Wg], overwriting.
//   bilagrid_tv_kernel             : tv(G) and d tv / dG in one launch of ONE workgroup (a grid is a few tens of thousands of floats): every thread
//                                    gathers its elements' differences, the three sums go through per-wave partials added in a fixed order.
#include "fgs_kernels.h"
#include <fgs_wave.h>

namespace fgs {

constexpr int kBgTileW = 64, kBgTileH = 16, kBgPixels = 4;                 // thread = 4 adjacent pixels of one row: 16 threads per row, 16 rows
static_assert((kBgTileW / kBgPixels) * kBgTileH == 256, "one pixel quad per thread");
// LDS budget. Forward: 15.75 KiB staged -> ten workgroups per CU by LDS (160 KiB), so the 32-wave cap binds, not LDS. Backward: the staged part plus
// 24 KiB of accumulators = 39.75 KiB -> four workgroups (16 waves) per CU.
constexpr int kBgMaxCorners = 336, kBgStageFloats = kBgMaxCorners * 12;
#ifndef FGS_BILAGRID_REPLICAS
#define FGS_BILAGRID_REPLICAS 8      // A/B knob: copies of the LDS accumulators
#endif
constexpr int kBgAccFloats = 6144, kBgMaxReplicas = FGS_BILAGRID_REPLICAS;
static_assert(kBgAccFloats > kBgStageFloats, "one copy of the largest staged part fits the accumulators");

// lattice coordinate of pixel p along an axis of `extent` pixels and `cells` lattice points: lower corner, upper corner (clamped), weight of the upper
struct BgAxis { int i0, i1; float f; };
__host__ __device__ __forceinline__ int bg_min(const int a, const int b) { return a < b ? a : b; }
__host__ __device__ __forceinline__ BgAxis bg_axis(const int p, const int extent, const int cells) {
    const float u = (static_cast<float>(p) + 0.5f) / static_cast<float>(extent) * static_cast<float>(cells - 1);
    BgAxis r;
    r.i0 = bg_min(static_cast<int>(u), cells - 1);            // u >= 0: truncation is floor
    r.i1 = bg_min(r.i0 + 1, cells - 1);
    r.f = u - static_cast<float>(r.i0);
    return r;
}
// the lattice points pixels [p0, p1] touch: bg_axis is monotone in p (every operation rounds monotonically), so the ends bound everything between
struct BgSpan { int first, count; };
__host__ __device__ __forceinline__ BgSpan bg_span(const int p0, const int p1, const int extent, const int cells) {
    const int first = bg_axis(p0, extent, cells).i0;
    return BgSpan{first, bg_axis(p1, extent, cells).i1 - first + 1};
}

// Does the part of the grid under EVERY tile fit the LDS budget? The same arithmetic as the kernels', tile by tile (the two axes are independent).
bool bilagrid_staged(const int gw, const int gh, const int gl, const int width, const int height) {
    int max_x = 1, max_y = 1;
    for (int x0 = 0; x0 < width; x0 += kBgTileW) max_x = -bg_min(-max_x, -bg_span(x0, bg_min(x0 + kBgTileW, width) - 1, width, gw).count);
    for (int y0 = 0; y0 < height; y0 += kBgTileH) max_y = -bg_min(-max_y, -bg_span(y0, bg_min(y0 + kBgTileH, height) - 1, height, gh).count);
    return static_cast<long long>(max_x) * max_y * gl <= kBgMaxCorners;
}

struct BgTile { BgSpan sx, sy; int corners; };          // the staged part: sx.count x sy.count x L lattice points, index (z * sy.count + y) * sx.count + x
__device__ __forceinline__ BgTile bg_tile(const BilagridArgs& a, const int x0, const int y0) {
    BgTile t;
    t.sx = bg_span(x0, min(x0 + kBgTileW, a.width) - 1, a.width, a.gw);
    t.sy = bg_span(y0, min(y0 + kBgTileH, a.height) - 1, a.height, a.gh);
    t.corners = t.sx.count * t.sy.count * a.gl;
    return t;
}

// global [12, L, Hg, Wg] -> LDS [corner][12]; consecutive threads read consecutive x of one channel
__device__ __forceinline__ void bg_stage(const BilagridArgs& a, const BgTile& t, float* s_grid) {
    const int plane = a.gl * a.gh * a.gw;
    for (int idx = threadIdx.x; idx < t.corners * 12; idx += 256) {
        const int c = idx / t.corners, corner = idx - c * t.corners;
        const int lx = corner % t.sx.count, rest = corner / t.sx.count;
        const int ly = rest % t.sy.count, z = rest / t.sy.count;
        s_grid[corner * 12 + c] = a.grid[c * plane + (z * a.gh + t.sy.first + ly) * a.gw + t.sx.first + lx];
    }
}

// Where the eight corners of a pixel are: index of corner (zc, k), k = 2 * (upper y) + (upper x), in the staged part or in the whole grid
template <bool STAGED>
struct BgCorners {
    int at[2][4]; float w[2][4], wz[2];                   // w: the (y, x) weight of corner k; wz: the weight of plane zc
    __device__ __forceinline__ BgCorners(const BilagridArgs& a, const BgTile& t, const BgAxis& ax, const BgAxis& ay, const BgAxis& az) {
        int xs[2] = {ax.i0, ax.i1}, ys[2] = {ay.i0, ay.i1}, zs[2] = {az.i0, az.i1};
        const int nx = STAGED ? t.sx.count : a.gw, ny = STAGED ? t.sy.count : a.gh;
        if (STAGED) {                                     // bg_span bounds every pixel of the tile; the clamps keep a wrong bound inside the array
#pragma unroll
            for (int k = 0; k < 2; ++k) { xs[k] = min(max(xs[k] - t.sx.first, 0), nx - 1); ys[k] = min(max(ys[k] - t.sy.first, 0), ny - 1); }
        }
        const float wx[2] = {1.0f - ax.f, ax.f}, wy[2] = {1.0f - ay.f, ay.f};
        wz[0] = 1.0f - az.f; wz[1] = az.f;
#pragma unroll
        for (int zc = 0; zc < 2; ++zc)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                at[zc][k] = (zs[zc] * ny + ys[k >> 1]) * nx + xs[k & 1];
                w[zc][k] = wy[k >> 1] * wx[k & 1];
            }
    }
};

// the 12 values of one lattice point
template <bool STAGED>
__device__ __forceinline__ void bg_load12(const BilagridArgs& a, const float* s_grid, const int corner, float (&g)[12]) {
    if (STAGED) {
        const float4* q = reinterpret_cast<const float4*>(s_grid + corner * 12);
        const float4 q0 = q[0], q1 = q[1], q2 = q[2];
        g[0] = q0.x; g[1] = q0.y; g[2] = q0.z; g[3] = q0.w; g[4] = q1.x; g[5] = q1.y; g[6] = q1.z; g[7] = q1.w; g[8] = q2.x; g[9] = q2.y; g[10] = q2.z; g[11] = q2.w;
    } else {
        const int plane = a.gl * a.gh * a.gw;
#pragma unroll
        for (int c = 0; c < 12; ++c) g[c] = a.grid[c * plane + corner];
    }
}
// the matrices of the two z planes of a pixel, each interpolated in (y, x)
template <bool STAGED>
__device__ __forceinline__ void bg_planes(const BilagridArgs& a, const float* s_grid, const BgCorners<STAGED>& cn, float (&m0)[12], float (&m1)[12]) {
#pragma unroll
    for (int c = 0; c < 12; ++c) { m0[c] = 0.0f; m1[c] = 0.0f; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float g[12];
        bg_load12<STAGED>(a, s_grid, cn.at[0][k], g);
#pragma unroll
        for (int c = 0; c < 12; ++c) m0[c] += cn.w[0][k] * g[c];
        bg_load12<STAGED>(a, s_grid, cn.at[1][k], g);
#pragma unroll
        for (int c = 0; c < 12; ++c) m1[c] += cn.w[1][k] * g[c];
    }
}

constexpr float kLumaR = 0.299f, kLumaG = 0.587f, kLumaB = 0.114f;
__device__ __forceinline__ float bg_luma(const float r, const float g, const float b) { return kLumaR * r + kLumaG * g + kLumaB * b; }
// z axis from the guide: g (L - 1), lower plane, upper plane (clamped), weight of the upper
__device__ __forceinline__ BgAxis bg_guide_axis(const float luma, const int gl) {
    const float z = fminf(fmaxf(luma, 0.0f), 1.0f) * static_cast<float>(gl - 1);
    BgAxis r;
    r.i0 = min(static_cast<int>(z), gl - 1);
    r.i1 = min(r.i0 + 1, gl - 1);
    r.f = z - static_cast<float>(r.i0);
    return r;
}

// four adjacent pixels of one channel row: one 16-byte access when the launch allows it (width % 4 == 0 and 16-byte aligned tensors), else scalar with a tail
__device__ __forceinline__ void bg_read4(const float* __restrict__ row, const int px, const int width, const bool vec, float (&v)[kBgPixels]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(row + px);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < kBgPixels; ++k) v[k] = px + k < width ? row[px + k] : 0.0f;
    }
}
__device__ __forceinline__ void bg_write4(float* __restrict__ row, const int px, const int width, const bool vec, const float (&v)[kBgPixels]) {
    if (vec) {
        *reinterpret_cast<float4*>(row + px) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kBgPixels; ++k)
            if (px + k < width) row[px + k] = v[k];
    }
}

// A thread walks its four pixels in a loop that is NOT unrolled: unrolled, the compiler hoists the 96 corner reads of all four pixels ahead of their
// use (256 registers, one wave per SIMD; capped at 128 it spills 180 of them), and these kernels stream the image and want the waves. The pixel of
// the turn is picked out of / put into the thread's float4 rows with selects on the (uniform) loop counter, which keeps the rows in registers.
#define FGS_BILAGRID_BOUNDS __launch_bounds__(256)
__device__ __forceinline__ float bg_pick(const float (&v)[kBgPixels], const int k) { return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3]; }
__device__ __forceinline__ void bg_put(float (&v)[kBgPixels], const int k, const float x) {
#pragma unroll
    for (int q = 0; q < kBgPixels; ++q) v[q] = k == q ? x : v[q];
}

template <bool STAGED>
__global__ void FGS_BILAGRID_BOUNDS bilagrid_slice_kernel(const BilagridArgs a) {
    __shared__ __attribute__((aligned(16))) float s_grid[STAGED ? kBgStageFloats : 4];
    const int x0 = blockIdx.x * kBgTileW, y0 = blockIdx.y * kBgTileH;
    const BgTile t = bg_tile(a, x0, y0);
    if (STAGED && t.corners > kBgMaxCorners) return;      // never: bilagrid_staged walked this tile with the same arithmetic (workgroup-uniform)
    if (STAGED) {
        bg_stage(a, t, s_grid);
        __syncthreads();
    }
    const int py = y0 + static_cast<int>(threadIdx.x) / (kBgTileW / kBgPixels), px0 = x0 + (static_cast<int>(threadIdx.x) % (kBgTileW / kBgPixels)) * kBgPixels;
    if (py >= a.height || px0 >= a.width) return;
    const size_t plane = static_cast<size_t>(a.width) * a.height, row = static_cast<size_t>(py) * a.width;
    const bool vec = a.vec4 != 0;
    float C[3][kBgPixels], O[3][kBgPixels];
#pragma unroll
    for (int j = 0; j < 3; ++j) bg_read4(a.image + j * plane + row, px0, a.width, vec, C[j]);
    const BgAxis ay = bg_axis(py, a.height, a.gh);
#pragma unroll 1
    for (int k = 0; k < kBgPixels; ++k) {
        const float c[3] = {bg_pick(C[0], k), bg_pick(C[1], k), bg_pick(C[2], k)};
        const BgAxis ax = bg_axis(min(px0 + k, a.width - 1), a.width, a.gw);
        const BgAxis az = bg_guide_axis(bg_luma(c[0], c[1], c[2]), a.gl);
        const BgCorners<STAGED> cn(a, t, ax, ay, az);
        float m0[12], m1[12];
        bg_planes<STAGED>(a, s_grid, cn, m0, m1);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float m[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) m[j] = cn.wz[0] * m0[4 * i + j] + cn.wz[1] * m1[4 * i + j];
            bg_put(O[i], k, m[0] * c[0] + m[1] * c[1] + m[2] * c[2] + m[3]);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) bg_write4(a.out + i * plane + row, px0, a.width, vec, O[i]);
}

// WITH_GRID: dL/dgrid is wanted (a.scratch); a.grad_image may be NULL then, and is not NULL otherwise
template <bool STAGED, bool WITH_GRID>
__global__ void FGS_BILAGRID_BOUNDS bilagrid_slice_backward_kernel(const BilagridArgs a) {
    __shared__ __attribute__((aligned(16))) float s_grid[STAGED ? kBgStageFloats : 4];
    __shared__ float s_acc[STAGED && WITH_GRID ? kBgAccFloats : 4];
    const int x0 = blockIdx.x * kBgTileW, y0 = blockIdx.y * kBgTileH;
    const BgTile t = bg_tile(a, x0, y0);
    if (STAGED && t.corners > kBgMaxCorners) return;      // never: see the forward kernel
    // copies of the accumulators: as many as fit, on different banks (an odd stride)
    const int staged_floats = t.corners * 12, stride = staged_floats | 1;
    const int replicas = STAGED && WITH_GRID ? max(1, min(kBgMaxReplicas, kBgAccFloats / stride)) : 1;
    if (STAGED) {
        bg_stage(a, t, s_grid);
        if (WITH_GRID)
            for (int idx = threadIdx.x; idx < replicas * stride; idx += 256) s_acc[idx] = 0.0f;
        __syncthreads();
    }
    const int py = y0 + static_cast<int>(threadIdx.x) / (kBgTileW / kBgPixels), px0 = x0 + (static_cast<int>(threadIdx.x) % (kBgTileW / kBgPixels)) * kBgPixels;
    if (py < a.height && px0 < a.width) {
        const size_t plane = static_cast<size_t>(a.width) * a.height, row = static_cast<size_t>(py) * a.width;
        const bool vec = a.vec4 != 0;
        float C[3][kBgPixels], gO[3][kBgPixels], gC[3][kBgPixels];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            bg_read4(a.image + j * plane + row, px0, a.width, vec, C[j]);
            bg_read4(a.grad_out + j * plane + row, px0, a.width, vec, gO[j]);     // a pixel beyond the row reads as zero: it adds nothing below
        }
        const BgAxis ay = bg_axis(py, a.height, a.gh);
        float* const my_acc = s_acc + (static_cast<int>(threadIdx.x) % replicas) * stride;
#pragma unroll 1
        for (int k = 0; k < kBgPixels; ++k) {
            const bool real = px0 + k < a.width;
            const float c[3] = {bg_pick(C[0], k), bg_pick(C[1], k), bg_pick(C[2], k)}, go[3] = {bg_pick(gO[0], k), bg_pick(gO[1], k), bg_pick(gO[2], k)};
            const BgAxis ax = bg_axis(min(px0 + k, a.width - 1), a.width, a.gw);
            const float luma = bg_luma(c[0], c[1], c[2]);
            const BgAxis az = bg_guide_axis(luma, a.gl);
            const BgCorners<STAGED> cn(a, t, ax, ay, az);
            float v[12];                                            // dL/dM: gO_i * (C_j or 1)
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                v[4 * i] = go[i] * c[0]; v[4 * i + 1] = go[i] * c[1]; v[4 * i + 2] = go[i] * c[2]; v[4 * i + 3] = go[i];
            }
            if (a.grad_image != nullptr) {
                float m0[12], m1[12];
                bg_planes<STAGED>(a, s_grid, cn, m0, m1);
                float dz = 0.0f;                                    // dL/dz = sum_c dM_c/dz * dL/dM_c
#pragma unroll
                for (int q = 0; q < 12; ++q) dz += (m1[q] - m0[q]) * v[q];
                // the clamped guide carries no gradient (torch's rule for `border`)
                const float through_guide = luma > 0.0f && luma < 1.0f ? dz * static_cast<float>(a.gl - 1) : 0.0f;
                const float kj[3] = {kLumaR, kLumaG, kLumaB};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    float s = kj[j] * through_guide;
#pragma unroll
                    for (int i = 0; i < 3; ++i) s += (cn.wz[0] * m0[4 * i + j] + cn.wz[1] * m1[4 * i + j]) * go[i];
                    bg_put(gC[j], k, s);
                }
            }
            if (WITH_GRID && real) {
#pragma unroll
                for (int zc = 0; zc < 2; ++zc)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float w = cn.wz[zc] * cn.w[zc][q];
                        if (w == 0.0f) continue;                    // a clamped upper corner, an axis of extent 1
                        if (STAGED) {
                            float* const dst = my_acc + cn.at[zc][q] * 12;
#pragma unroll
                            for (int ch = 0; ch < 12; ++ch) atomicAdd(dst + ch, w * v[ch]);
                        } else {
                            float* const dst = a.scratch + static_cast<size_t>(cn.at[zc][q]) * 12;
#pragma unroll
                            for (int ch = 0; ch < 12; ++ch) unsafeAtomicAdd(dst + ch, w * v[ch]);
                        }
                    }
            }
        }
        if (a.grad_image != nullptr) {
#pragma unroll
            for (int j = 0; j < 3; ++j) bg_write4(a.grad_image + j * plane + row, px0, a.width, vec, gC[j]);
        }
    }
    if (STAGED && WITH_GRID) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < staged_floats; idx += 256) {      // consecutive threads: the 12 channels of consecutive x
            float s = 0.0f;
            for (int r = 0; r < replicas; ++r) s += s_acc[r * stride + idx];
            if (s == 0.0f) continue;
            const int corner = idx / 12, c = idx - corner * 12;
            const int lx = corner % t.sx.count, rest = corner / t.sx.count;
            const int ly = rest % t.sy.count, z = rest / t.sy.count;
            unsafeAtomicAdd(a.scratch + (static_cast<size_t>((z * a.gh + t.sy.first + ly) * a.gw + t.sx.first + lx)) * 12 + c, s);
        }
    }
}

__global__ void __launch_bounds__(256) bilagrid_transpose_kernel(const float* __restrict__ scratch, float* __restrict__ grad_grid, const int corners) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= corners * 12) return;
    const int c = idx / corners, corner = idx - c * corners;
    grad_grid[idx] = scratch[corner * 12 + c];
}

constexpr int kTvThreads = 1024;
__global__ void __launch_bounds__(kTvThreads) bilagrid_tv_kernel(const float* __restrict__ grid, const int gw, const int gh, const int gl, const float inv_x, const float inv_y,
                                                                 const float inv_z, float* __restrict__ loss, float* __restrict__ grad) {
    __shared__ float s_part[3][kTvThreads / 64];
    const int n = 12 * gl * gh * gw, sy = gw, sz = gw * gh;
    float sum_x = 0.0f, sum_y = 0.0f, sum_z = 0.0f;
    for (int e = threadIdx.x; e < n; e += kTvThreads) {
        const int x = e % gw, y = (e / gw) % gh, z = (e / sz) % gl;
        const float g = grid[e];
        float d_tv = 0.0f;
        if (x + 1 < gw) { const float d = grid[e + 1] - g; sum_x += d * d; d_tv -= 2.0f * inv_x * d; }
        if (x > 0) d_tv += 2.0f * inv_x * (g - grid[e - 1]);
        if (y + 1 < gh) { const float d = grid[e + sy] - g; sum_y += d * d; d_tv -= 2.0f * inv_y * d; }
        if (y > 0) d_tv += 2.0f * inv_y * (g - grid[e - sy]);
        if (z + 1 < gl) { const float d = grid[e + sz] - g; sum_z += d * d; d_tv -= 2.0f * inv_z * d; }
        if (z > 0) d_tv += 2.0f * inv_z * (g - grid[e - sz]);
        if (grad != nullptr) grad[e] = d_tv;
    }
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    sum_x = wave_sum_to_lane63(sum_x); sum_y = wave_sum_to_lane63(sum_y); sum_z = wave_sum_to_lane63(sum_z);
    if (lane == 63u) { s_part[0][wave] = sum_x; s_part[1][wave] = sum_y; s_part[2][wave] = sum_z; }
    __syncthreads();
    if (threadIdx.x == 0) {                                       // the wave partials in a fixed order
        float t[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 3; ++k)
            for (int w = 0; w < kTvThreads / 64; ++w) t[k] += s_part[k][w];
        *loss = t[0] * inv_x + t[1] * inv_y + t[2] * inv_z;         // an axis of extent 1 summed nothing
    }
}

static dim3 bg_launch_grid(const BilagridArgs& a) { return dim3((a.width + kBgTileW - 1) / kBgTileW, (a.height + kBgTileH - 1) / kBgTileH); }

hipError_t launch_bilagrid_slice(const BilagridArgs& a, hipStream_t s) {
    if (bilagrid_staged(a.gw, a.gh, a.gl, a.width, a.height)) hipLaunchKernelGGL(bilagrid_slice_kernel<true>, bg_launch_grid(a), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(bilagrid_slice_kernel<false>, bg_launch_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

// a.scratch (when dL/dgrid is wanted) is zero on the stream already; grad_grid receives its transpose
hipError_t launch_bilagrid_slice_backward(const BilagridArgs& a, float* grad_grid, hipStream_t s) {
    const bool staged = bilagrid_staged(a.gw, a.gh, a.gl, a.width, a.height), with_grid = a.scratch != nullptr;
    const dim3 grid = bg_launch_grid(a), block(256);
    if (staged && with_grid) hipLaunchKernelGGL((bilagrid_slice_backward_kernel<true, true>), grid, block, 0, s, a);
    else if (staged) hipLaunchKernelGGL((bilagrid_slice_backward_kernel<true, false>), grid, block, 0, s, a);
    else if (with_grid) hipLaunchKernelGGL((bilagrid_slice_backward_kernel<false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((bilagrid_slice_backward_kernel<false, false>), grid, block, 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !with_grid) return e;
    const int corners = a.gl * a.gh * a.gw;
    hipLaunchKernelGGL(bilagrid_transpose_kernel, dim3((corners * 12 + 255) / 256), block, 0, s, a.scratch, grad_grid, corners);
    return hipGetLastError();
}

hipError_t launch_bilagrid_tv(const float* grid, int gw, int gh, int gl, float* loss, float* grad_grid, hipStream_t s) {
    // mean over the differences of an axis: 12 channels x (extent - 1) x the other two extents; no differences, no term
    const auto inv = [&](int along, int o1, int o2) { return along > 1 ? static_cast<float>(1.0 / (12.0 * (along - 1) * o1 * o2)) : 0.0f; };
    hipLaunchKernelGGL(bilagrid_tv_kernel, dim3(1), dim3(kTvThreads), 0, s, grid, gw, gh, gl, inv(gw, gh, gl), inv(gh, gw, gl), inv(gl, gw, gh), loss, grad_grid);
    return hipGetLastError();
}

}  // namespace fgs

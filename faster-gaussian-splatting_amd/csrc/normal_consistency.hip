// Normal-consistency regulariser of 2DGS, L_n = sum_i w_i (1 - n_i . N), for gfx950: the Gaussians blended into a pixel are asked to face the way the
// surface of the rendered depth map does. The rasterizer supplies the blend (diff_rasterize_features over five channels); this unit supplies the two
// ends (definitions: INTEGRATION.md 'Normal consistency'; tests/normal_cases.py holds the kernels to them in fp64 torch with autograd).
//
//   surface_features_kernel           : a thread per Gaussian -> row (n_cam, z, 1) of the [N,5] feature table. n = the axis of the smallest log-scale
//                                       (lowest index on a tie), turned towards the camera, in camera space; z = the view-space depth of the mean.
//   surface_features_backward_kernel  : the same thread layout; dL/drotations through quat_to_rotation_backward (one column of dL/dR), dL/dmeans from
//                                       the depth channel. Every row is written plainly: nothing is accumulated.
//   normal_consistency_kernel         : a 32 x 8 pixel tile per 256-thread workgroup over the blended map M [5,H,W] = (N_r, D, A). d = D / A and the
//                                       A >= min_alpha flag are staged in LDS at halo 1; a pixel takes its depth normal n_d from the back-projected
//                                       points of its four neighbours and leaves E = A - N_r . n_d (0 where invalid), optionally n_d.
//   normal_consistency_backward_kernel: the same tiling, d and the flag at halo 2, N_r and gE at halo 1. A GATHER: the thread of pixel q recomputes the
//                                       up to four centres q is a neighbour of (and its own, for dL/dN_r) and sums their shares of dL/dd(q) in a fixed
//                                       order -- no float atomics, bit-reproducible run to run. Every element of gM [5,H,W] is written.
//
// Tile shape: 32 x 8. A wave64 covers two rows of 32 pixels = two full 128-byte lines per plane; a row of the staged region is 36 (34) floats, so the
// 32 lanes of an LDS lane group read consecutive banks for every one of the stencil's offsets (no conflicts, no padding needed). The halo-2 region is
// 36 x 12 = 432 cells for 256 pixels (1.69 x; 64 x 4 would be 2.13 x, 16 x 16 1.56 x with 64-byte row segments). LDS: 7.4 KiB backward, 1.7 KiB
// forward -- the 32-wave cap of a CU binds, not LDS. The natural 2-D grid: no tile-to-XCD banding (not measured to help here).
#include "fgs_kernels.h"

namespace fgs {

// ---- per-Gaussian surface features ---------------------------------------------------------------------------------------------------------------------
struct SurfaceAxis { int k; float sign; float a[3]; };      // the normal's column of R, its sign towards the camera, the column itself

// k = index of the smallest log-scale (strict <: the lowest index wins a tie); s = -1 if a . (mean - cam) > 0 else +1 (a . v == 0 does not flip)
__device__ __forceinline__ SurfaceAxis surface_axis(const float (&R)[9], const float* __restrict__ scale, const float* __restrict__ mean, const float* __restrict__ cam) {
    SurfaceAxis s;
    const float s0 = scale[0], s1 = scale[1], s2 = scale[2];
    s.k = 0;
    float smallest = s0;
    if (s1 < smallest) { s.k = 1; smallest = s1; }
    if (s2 < smallest) s.k = 2;
    s.a[0] = R[s.k]; s.a[1] = R[3 + s.k]; s.a[2] = R[6 + s.k];
    const float along = s.a[0] * (mean[0] - cam[0]) + s.a[1] * (mean[1] - cam[1]) + s.a[2] * (mean[2] - cam[2]);
    s.sign = along > 0.0f ? -1.0f : 1.0f;
    return s;
}

__global__ void __launch_bounds__(256) surface_features_kernel(const SurfaceFeatureArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const float4 q = reinterpret_cast<const float4*>(a.rotations)[i];      // 16-byte load: a torch tensor's rows of four floats
    float R[9], norm_sq;
    quat_to_rotation(q.x, q.y, q.z, q.w, R, norm_sq);
    const float* __restrict__ m = a.means + 3 * static_cast<size_t>(i);
    const SurfaceAxis ax = surface_axis(R, a.scales + 3 * static_cast<size_t>(i), m, a.cam_position);
    const float* __restrict__ W = a.w2c;
    float* __restrict__ out = a.features + 5 * static_cast<size_t>(i);
#pragma unroll
    for (int r = 0; r < 3; ++r) out[r] = ax.sign * (W[4 * r] * ax.a[0] + W[4 * r + 1] * ax.a[1] + W[4 * r + 2] * ax.a[2]);
    out[3] = W[8] * m[0] + W[9] * m[1] + W[10] * m[2] + W[11];
    out[4] = 1.0f;
}

__global__ void __launch_bounds__(256) surface_features_backward_kernel(const SurfaceFeatureArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const float* __restrict__ W = a.w2c;
    const float* __restrict__ g = a.grad_features + 5 * static_cast<size_t>(i);
    if (a.grad_rotations != nullptr) {
        const float4 q = reinterpret_cast<const float4*>(a.rotations)[i];
        float R[9], norm_sq;
        quat_to_rotation(q.x, q.y, q.z, q.w, R, norm_sq);
        const SurfaceAxis ax = surface_axis(R, a.scales + 3 * static_cast<size_t>(i), a.means + 3 * static_cast<size_t>(i), a.cam_position);
        float d[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};      // dL/dR: column k only, s (W^T gF[0:3])
        const float g0 = g[0], g1 = g[1], g2 = g[2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float v = ax.sign * (W[r] * g0 + W[4 + r] * g1 + W[8 + r] * g2);
            d[3 * r] = ax.k == 0 ? v : 0.0f; d[3 * r + 1] = ax.k == 1 ? v : 0.0f; d[3 * r + 2] = ax.k == 2 ? v : 0.0f;
        }
        float gq[4];
        quat_to_rotation_backward(q.x, q.y, q.z, q.w, d, gq);               // includes the gradient through the normalisation
        reinterpret_cast<float4*>(a.grad_rotations)[i] = make_float4(gq[0], gq[1], gq[2], gq[3]);
    }
    if (a.grad_means != nullptr) {
        const float gz = g[3];
        float* __restrict__ gm = a.grad_means + 3 * static_cast<size_t>(i);
        gm[0] = gz * W[8]; gm[1] = gz * W[9]; gm[2] = gz * W[10];
    }
}

static dim3 per_gaussian_grid(const int n) { return dim3(static_cast<unsigned>((n + 255) / 256)); }

hipError_t launch_surface_features(const SurfaceFeatureArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(surface_features_kernel, per_gaussian_grid(a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_surface_features_backward(const SurfaceFeatureArgs& a, hipStream_t s) {
    if (a.n <= 0 || (a.grad_rotations == nullptr && a.grad_means == nullptr)) return hipSuccess;
    hipLaunchKernelGGL(surface_features_backward_kernel, per_gaussian_grid(a.n), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---- image space ---------------------------------------------------------------------------------------------------------------------------------------
constexpr int kNcTileW = 32, kNcTileH = 8;
static_assert(kNcTileW * kNcTileH == 256, "one pixel per thread");
constexpr float kNcMinCrossSq = 1e-30f;                                   // |c|^2 at or below it: no normal, the pixel is invalid

// d = D / A and the flag A >= min_alpha of the HALO-wide ring around the tile at (x0, y0). A cell outside the image, or below min_alpha, is flagged 0,
// holds d = 0 and its D / A is never formed; a cell outside the image is never read.
template <int HALO>
__device__ __forceinline__ void nc_stage_depth(const NormalConsistencyArgs& a, const int x0, const int y0, float* __restrict__ s_d, unsigned char* __restrict__ s_ok) {
    constexpr int RW = kNcTileW + 2 * HALO, RH = kNcTileH + 2 * HALO;
    const size_t plane = static_cast<size_t>(a.width) * a.height;
    for (int idx = threadIdx.x; idx < RW * RH; idx += 256) {
        const int ry = idx / RW, rx = idx - ry * RW;
        const int qx = x0 + rx - HALO, qy = y0 + ry - HALO;
        float d = 0.0f;
        bool ok = false;
        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.height) {
            const size_t e = static_cast<size_t>(qy) * a.width + qx;
            const float A = a.map[4 * plane + e];
            ok = A >= a.min_alpha;                                          // false for NaN
            if (ok) d = a.map[3 * plane + e] / A;
        }
        s_d[idx] = d;
        s_ok[idx] = ok ? 1 : 0;
    }
}

// The centre p at cell `at` of a staged region of row stride RW (its four neighbours are staged): is it valid, and if so its depth normal and the two
// tangents. (px, py): p's pixel coordinates.
struct NcCentre { bool valid; float n[3], gx[3], gy[3], inv_len; };
template <int RW>
__device__ __forceinline__ NcCentre nc_centre(const NormalConsistencyArgs& a, const float* __restrict__ s_d, const unsigned char* __restrict__ s_ok, const int at,
                                              const int px, const int py) {
    NcCentre c;
    c.valid = px >= 1 && px <= a.width - 2 && py >= 1 && py <= a.height - 2 &&
              (s_ok[at] & s_ok[at - 1] & s_ok[at + 1] & s_ok[at - RW] & s_ok[at + RW]) != 0;
    if (!c.valid) return c;
    const float fpx = static_cast<float>(px) - a.cx, fpy = static_cast<float>(py) - a.cy;      // ray(q) = ((qx + 0.5 - cx) / fx, (qy + 0.5 - cy) / fy, 1)
    const float rx = (fpx + 0.5f) * a.inv_fx, ry = (fpy + 0.5f) * a.inv_fy;
    const float dl = s_d[at - 1], dr = s_d[at + 1], du = s_d[at - RW], dd = s_d[at + RW];
    // P(q) = ray(q) d(q); the rays of the neighbours differ from p's in one component
    c.gx[0] = (fpx + 1.5f) * a.inv_fx * dr - (fpx - 0.5f) * a.inv_fx * dl; c.gx[1] = ry * dr - ry * dl; c.gx[2] = dr - dl;
    c.gy[0] = rx * dd - rx * du; c.gy[1] = (fpy + 1.5f) * a.inv_fy * dd - (fpy - 0.5f) * a.inv_fy * du; c.gy[2] = dd - du;
    const float cr[3] = {c.gy[1] * c.gx[2] - c.gy[2] * c.gx[1], c.gy[2] * c.gx[0] - c.gy[0] * c.gx[2], c.gy[0] * c.gx[1] - c.gy[1] * c.gx[0]};   // gy x gx: faces the camera
    const float len_sq = cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2];
    c.valid = len_sq > kNcMinCrossSq;
    if (!c.valid) return c;
    c.inv_len = 1.0f / sqrtf(len_sq);
    c.n[0] = cr[0] * c.inv_len; c.n[1] = cr[1] * c.inv_len; c.n[2] = cr[2] * c.inv_len;
    return c;
}

__global__ void __launch_bounds__(256) normal_consistency_kernel(const NormalConsistencyArgs a) {
    constexpr int RW = kNcTileW + 2, RH = kNcTileH + 2;
    __shared__ float s_d[RW * RH];
    __shared__ unsigned char s_ok[RW * RH];
    const int x0 = blockIdx.x * kNcTileW, y0 = blockIdx.y * kNcTileH;
    nc_stage_depth<1>(a, x0, y0, s_d, s_ok);
    __syncthreads();
    const int lx = static_cast<int>(threadIdx.x) % kNcTileW, ly = static_cast<int>(threadIdx.x) / kNcTileW;
    const int px = x0 + lx, py = y0 + ly;
    if (px >= a.width || py >= a.height) return;
    const size_t plane = static_cast<size_t>(a.width) * a.height, e = static_cast<size_t>(py) * a.width + px;
    const NcCentre c = nc_centre<RW>(a, s_d, s_ok, (ly + 1) * RW + lx + 1, px, py);
    float E = 0.0f, n[3] = {0.0f, 0.0f, 0.0f};
    if (c.valid) {
        E = a.map[4 * plane + e] - (a.map[e] * c.n[0] + a.map[plane + e] * c.n[1] + a.map[2 * plane + e] * c.n[2]);
        n[0] = c.n[0]; n[1] = c.n[1]; n[2] = c.n[2];
    }
    a.E[e] = E;
    if (a.normals != nullptr) {
        a.normals[e] = n[0]; a.normals[plane + e] = n[1]; a.normals[2 * plane + e] = n[2];
    }
}

// dL/dgx and dL/dgy of a valid centre whose upstream gradient is gE and whose blended normal is N_r:
// g_n = -gE N_r, g_c = (g_n - n (n . g_n)) / |c|, g_gx = g_c x gy, g_gy = gx x g_c
__device__ __forceinline__ void nc_tangent_gradients(const NcCentre& c, const float gE, const float (&Nr)[3], float (&g_gx)[3], float (&g_gy)[3]) {
    const float gn[3] = {-gE * Nr[0], -gE * Nr[1], -gE * Nr[2]};
    const float along = c.n[0] * gn[0] + c.n[1] * gn[1] + c.n[2] * gn[2];
    const float gc[3] = {(gn[0] - c.n[0] * along) * c.inv_len, (gn[1] - c.n[1] * along) * c.inv_len, (gn[2] - c.n[2] * along) * c.inv_len};
    g_gx[0] = gc[1] * c.gy[2] - gc[2] * c.gy[1]; g_gx[1] = gc[2] * c.gy[0] - gc[0] * c.gy[2]; g_gx[2] = gc[0] * c.gy[1] - gc[1] * c.gy[0];
    g_gy[0] = c.gx[1] * gc[2] - c.gx[2] * gc[1]; g_gy[1] = c.gx[2] * gc[0] - c.gx[0] * gc[2]; g_gy[2] = c.gx[0] * gc[1] - c.gx[1] * gc[0];
}

__global__ void __launch_bounds__(256) normal_consistency_backward_kernel(const NormalConsistencyArgs a) {
    constexpr int RW = kNcTileW + 4, RH = kNcTileH + 4;                   // d and the flag: halo 2
    constexpr int SW = kNcTileW + 2, SH = kNcTileH + 2;                   // N_r and gE: halo 1 (the centres a pixel of the tile gathers from)
    __shared__ float s_d[RW * RH];
    __shared__ unsigned char s_ok[RW * RH];
    __shared__ float s_n[3][SW * SH];
    __shared__ float s_g[SW * SH];
    const int x0 = blockIdx.x * kNcTileW, y0 = blockIdx.y * kNcTileH;
    const size_t plane = static_cast<size_t>(a.width) * a.height;
    nc_stage_depth<2>(a, x0, y0, s_d, s_ok);
    for (int idx = threadIdx.x; idx < SW * SH; idx += 256) {
        const int ry = idx / SW, rx = idx - ry * SW;
        const int qx = x0 + rx - 1, qy = y0 + ry - 1;
        const bool in = qx >= 0 && qx < a.width && qy >= 0 && qy < a.height;      // a cell outside the image is no centre: never read, its zeros never used
        const size_t e = in ? static_cast<size_t>(qy) * a.width + qx : 0;
        s_g[idx] = in ? a.grad_E[e] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) s_n[k][idx] = in ? a.map[k * plane + e] : 0.0f;
    }
    __syncthreads();
    const int lx = static_cast<int>(threadIdx.x) % kNcTileW, ly = static_cast<int>(threadIdx.x) / kNcTileW;
    const int qx = x0 + lx, qy = y0 + ly;
    if (qx >= a.width || qy >= a.height) return;
    const size_t e = static_cast<size_t>(qy) * a.width + qx;
    const int at_d = (ly + 2) * RW + lx + 2, at_s = (ly + 1) * SW + lx + 1;
    const float ray[3] = {(static_cast<float>(qx) - a.cx + 0.5f) * a.inv_fx, (static_cast<float>(qy) - a.cy + 0.5f) * a.inv_fy, 1.0f};

    // the pixel's own centre: dL/dN_r and the E = A - ... part of dL/dA
    float gN[3] = {0.0f, 0.0f, 0.0f}, gA = 0.0f;
    {
        const NcCentre c = nc_centre<RW>(a, s_d, s_ok, at_d, qx, qy);
        if (c.valid) {
            const float gE = s_g[at_s];
            gN[0] = -gE * c.n[0]; gN[1] = -gE * c.n[1]; gN[2] = -gE * c.n[2];
            gA = gE;
        }
    }
    // the four centres q is a neighbour of, in a fixed order: left (q = p + (1, 0): + g_gx), right (-g_gx), up (q = p + (0, 1): + g_gy), down (-g_gy)
    float g_d = 0.0f;
    bool touched = false;
    const int off_x[4] = {-1, 1, 0, 0}, off_y[4] = {0, 0, -1, 1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int cd = at_d + off_y[k] * RW + off_x[k], cs = at_s + off_y[k] * SW + off_x[k];
        const NcCentre c = nc_centre<RW>(a, s_d, s_ok, cd, qx + off_x[k], qy + off_y[k]);
        if (!c.valid) continue;
        touched = true;
        const float Nr[3] = {s_n[0][cs], s_n[1][cs], s_n[2][cs]};
        float g_gx[3], g_gy[3];
        nc_tangent_gradients(c, s_g[cs], Nr, g_gx, g_gy);
        const float* const g = k < 2 ? g_gx : g_gy;
        const float share = ray[0] * g[0] + ray[1] * g[1] + ray[2] * g[2];
        g_d += (k & 1) ? -share : share;
    }
    float gD = 0.0f;
    if (touched) {                                                        // a valid centre beside q: A(q) >= min_alpha > 0 and d(q) = D / A is staged
        const float A = a.map[4 * plane + e];
        gD = g_d / A;
        gA -= gD * s_d[at_d];                                             // g_d D / A^2
    }
    float* __restrict__ gM = a.grad_map;
    gM[e] = gN[0]; gM[plane + e] = gN[1]; gM[2 * plane + e] = gN[2]; gM[3 * plane + e] = gD; gM[4 * plane + e] = gA;
}

static dim3 nc_grid(const NormalConsistencyArgs& a) { return dim3((a.width + kNcTileW - 1) / kNcTileW, (a.height + kNcTileH - 1) / kNcTileH); }

hipError_t launch_normal_consistency(const NormalConsistencyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(normal_consistency_kernel, nc_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_normal_consistency_backward(const NormalConsistencyArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(normal_consistency_backward_kernel, nc_grid(a), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fgs

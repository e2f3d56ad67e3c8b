// K12 (+ optional K13 fusion): per-Gaussian backward of projection / EWA / covariance / quaternion / SH, for gfx950.
// Semantics: reference kernels_backward.cuh:15-257 + sh_utils.cuh:71-155; the fused mode equals
// "backward -> FusedAdam.step()" of the reference (torch_bindings/adam.py:11-36, adam/src/adam.cu:10-34).
//
// CDNA4 shape -- the per-Gaussian payload is 59 floats of which 45 are sh_coefficients_rest, so the work is split by
// access pattern instead of by Gaussian:
//  * geometry kernel: one lane per Gaussian for the 14 "small" floats (means, scales, rotations, opacity, sh0): 12-16 B
//    per lane per tensor, contiguous across the wave. It also leaves the unit view direction of visible Gaussians in a
//    12-byte scratch slot.
//  * SH-rest kernel: the [N,15,3] tensors (parameter, both Adam moments, gradient) are streamed flat in 16-byte pieces by
//    a grid-stride loop; the gradient basis_k(dir) * dL/dcolour is recomputed per (Gaussian, basis) pair from the 12-byte
//    direction + 12-byte colour gradient (L1/L2 hits shared by neighbouring lanes) instead of being gathered with a
//    180-byte per-lane stride as in the reference.
//  * every element of every gradient is written (zeros for invisible Gaussians), which replaces the reference's eight
//    torch::zeros fills (rasterization_api.cu:127-134, 256 B per Gaussian).
//  * fused mode never materialises the 59-float gradient: Adam is applied in registers. Invisible Gaussians still
//    decay their moments and move by momentum (reference: dense zero grads, adam.py:16).
//  * camera-pose gradients (fgs_backward_pose): backward_gradients_kernel<RT, true> also reduces what the per-Gaussian chains say about w2c and
//    cam_position -- 15 sums, per wave and then over the waves in a fixed order, no float atomics. Only that materialised-gradient kernel has the flag:
//    the fused backward + Adam, sharded, record and asynchronous paths take no pose gradients.
// K13 itself, the optimizer over materialised gradients, is adam.hip; the update and its 16-byte piece are shared through fgs_adam.h.
#include "fgs_adam.h"
#include <type_traits>

namespace fgs {

// fused mode: the 14 small floats of a Gaussian (kernel group order means 3, sh0 3, opacity 1, scales 3, rotations 4) and
// their two Adam moments are requested at kernel entry, so the 42 loads are in flight while the gradient is computed.
constexpr int kGroupWidth[5] = {3, 3, 1, 3, 4};
constexpr int kGroupOffset[5] = {0, 3, 6, 7, 10};

// MULTI: the sharded path's owner sums the gradient of its Gaussians over the views of the step in registers (one launch,
// every gradient element written once) instead of one launch and one read-modify-write of the gradients per view.
template <bool MULTI> __device__ __forceinline__ void sum_into(float& dst, const float v) { dst = MULTI ? dst + v : v; }

// Gradient of the 14 small floats of Gaussian i (group order means 3, sh0 3, opacity 1, scales 3, rotations 4), summed over the
// views of the launch; zeros if no view sees it. st_p: the parameters already in registers (fused mode). KEEP_DIR: the unit view
// direction and the colour gradient of the (single) view stay in registers for the caller instead of going through the
// view_dir scratch array.
// Returns "visible" (some view has the Gaussian on screen: n_touched != 0, kb:45); `reached`: K11 added something to its record in some view.
// A visible Gaussian that no pixel's walk got to -- hidden behind opaque ones: both blend kernels stop at a tile's last processed
// Gaussian -- still has the nine zeros K1 cleared its record to, and each of its 59 gradient floats is a product with one of them. Such a
// view counts in densification_info[0] (the count is of VISIBLE Gaussians; += sqrt(0) on the second statistic is exact and omitted) and is
// otherwise skipped: no parameter or coefficient load, no projection, neither backward chain; its contribution is +0.0f.
#ifndef FGS_K12_RECORD_EARLY
#define FGS_K12_RECORD_EARLY 0   // 1 (A/B): single view, the record is requested together with n_touched -- one dependent step less, 36 B more
                                 // per invisible Gaussian (measured: profiles/k12_unreached_skip.txt)
#endif
// POSE (backward_gradients_kernel<RT, true>, fgs_backward_pose; single view): the lane's 15 camera terms go to `pose` -- what dcam, dL/d(J W) and dpos
// say about w2c and cam_position instead of about the mean (layout: PosePart) -- zeros for a Gaussian that is invisible or unreached. Every POSE
// statement is under `if constexpr`: the other instantiations compile to the instructions they had.
template <bool FUSED, bool MULTI, bool KEEP_DIR, bool POSE = false>
__device__ __forceinline__ bool gaussian_backward(const PreprocessBackwardArgs& a, const unsigned i, const float (&st_p)[14],
                                                  float (&grad)[14], float (&dir)[3], float (&gcol_out)[3], bool& reached,
                                                  [[maybe_unused]] float (&pose)[kPoseTerms]) {
    static_assert(!POSE || (!MULTI && !FUSED), "pose gradients: the single-view materialised-gradient kernel only");
    if constexpr (POSE) {
#pragma unroll
        for (int k = 0; k < kPoseTerms; ++k) pose[k] = 0.0f;
    }
    const size_t n = a.n;
    float g_mean[3] = {0.0f, 0.0f, 0.0f}, g_scale[3] = {0.0f, 0.0f, 0.0f}, g_rot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float g_op[1] = {0.0f}, g_sh0[3] = {0.0f, 0.0f, 0.0f};
    bool visible = false;
    reached = false;
    float m[3] = {0.0f, 0.0f, 0.0f}, s[3] = {0.0f, 0.0f, 0.0f}, q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int n_views = MULTI ? a.n_views : 1;
    const Camera cam0 = load_camera(a.view[0].cam);     // single view: requested before the visibility test, as are the moments
    for (int vw = 0; vw < n_views; ++vw) {
        const BackwardView& V = a.view[MULTI ? vw : 0];
        constexpr bool kEarly = !MULTI && FGS_K12_RECORD_EARLY != 0;    // [N][9] records: in bounds for every i (sharded path: slot[] of an invisible one is scratch)
        float rec[kAccRecordWords];
        if (kEarly) {
#pragma unroll
            for (int k = 0; k < kAccRecordWords; ++k) rec[k] = V.acc[(size_t)i * kAccRecordWords + k];
        }
        if (V.n_touched[i] == 0) continue;                                             // kb:45
        visible = true;
        // K11's record of this primitive, 9 contiguous floats: single view [N][9]; sharded path: the record that came back, found through the slot table
        if (!kEarly) {
            const float* const accp = V.acc + (size_t)(MULTI ? V.slot[i] : i) * kAccRecordWords;
#pragma unroll
            for (int k = 0; k < kAccRecordWords; ++k) rec[k] = accp[k];
        }
        // reached: any word that is not +-0 (NaN and Inf count and take the full path). Depth-supervised pass: dL/dz of the Gaussian counts too.
        uint32_t any_bits = 0u;
#pragma unroll
        for (int k = 0; k < kAccRecordWords; ++k) any_bits |= __float_as_uint(rec[k]);
        if (V.acc_z != nullptr) any_bits |= __float_as_uint(V.acc_z[i]);
        if (a.densification_info != nullptr) a.densification_info[i] += 1.0f;         // kb:194-196
        const Camera cam = (MULTI && vw > 0) ? load_camera(V.cam) : cam0;
        if ((any_bits & 0x7fffffffu) == 0u) {
            // the SH-rest pass of the two-kernel forms multiplies basis(view_dir) by this view's zero colour gradient: give it a finite direction
            if (!KEEP_DIR && cam.active_sh_bases > 1) { V.view_dir[3 * (size_t)i] = 0.0f; V.view_dir[3 * (size_t)i + 1] = 0.0f; V.view_dir[3 * (size_t)i + 2] = 0.0f; }
            continue;
        }
        if (!reached) {                                                                // parameters: once, whatever the number of views
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                m[k] = FUSED ? st_p[0 + k] : a.means[3 * (size_t)i + k];
                s[k] = FUSED ? st_p[7 + k] : a.scales[3 * (size_t)i + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = FUSED ? st_p[10 + k] : a.rotations[4 * (size_t)i + k];
        }
        reached = true;
        const float gcol[3] = {rec[6], rec[7], rec[8]};
        if (KEEP_DIR) { gcol_out[0] = gcol[0]; gcol_out[1] = gcol[1]; gcol_out[2] = gcol[2]; }

        // ---- SH backward w.r.t. sh0 and the view direction (sh_utils.cuh:84-153) ----
#pragma unroll
        for (int c = 0; c < 3; ++c) sum_into<MULTI>(g_sh0[c], kC0 * gcol[c]);
        float dpos[3] = {0.0f, 0.0f, 0.0f};
        const unsigned active = static_cast<unsigned>(cam.active_sh_bases);
        if (active > 1) {
            const float xr = m[0] - cam.pos[0], yr = m[1] - cam.pos[1], zr = m[2] - cam.pos[2];
            const float inv = 1.0f / sqrtf(xr * xr + yr * yr + zr * zr);
            const float x = xr * inv, y = yr * inv, z = zr * inv;
            if (KEEP_DIR) { dir[0] = x; dir[1] = y; dir[2] = z; }
            else { V.view_dir[3 * (size_t)i] = x; V.view_dir[3 * (size_t)i + 1] = y; V.view_dir[3 * (size_t)i + 2] = z; }
            // (round 6, measured and withdrawn: the wave's contiguous 11.25 KB coefficient block taken with coalesced 16-byte loads into the LDS slice the
            // products go to afterwards, every lane reading its 45 words from there -- K12 0.282 vs 0.251 ms: the load -> LDS -> read chain in front of
            // the arithmetic costs more at 3 waves per SIMD than the lane-strided loads do, profiles/r06_ab_k12_staged_coeffs.txt)
            const float* k = a.sh_rest + (size_t)i * cam.total_sh_rest * 3;
            float gdx[3], gdy[3], gdz[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { gdx[c] = -kC1 * k[6 + c]; gdy[c] = -kC1 * k[0 + c]; gdz[c] = kC1 * k[3 + c]; }
            if (active > 4) {
                const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, xz = x * z, yz = y * z;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    gdx[c] = gdx[c] + kC2a * y * k[9 + c] - kC2a * z * k[18 + c] + kC2a * x * k[21 + c];
                    gdy[c] = gdy[c] + kC2a * x * k[9 + c] - kC2a * z * k[12 + c] - kC2a * y * k[21 + c];
                    gdz[c] = gdz[c] - kC2a * y * k[12 + c] + kC2e * z * k[15 + c] - kC2a * x * k[18 + c];
                }
                if (active > 9) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        gdx[c] = gdx[c] - kC3i * xy * k[24 + c] + kC3c * yz * k[27 + c] + (kC3d - kC3e * zz) * k[36 + c]
                                 + kC3c * xz * k[39 + c] + kC3b * (yy - xx) * k[42 + c];
                        gdy[c] = gdy[c] + kC3b * (yy - xx) * k[24 + c] + kC3c * xz * k[27 + c] + (kC3d - kC3e * zz) * k[30 + c]
                                 - kC3c * yz * k[39 + c] + kC3i * xy * k[42 + c];
                        gdz[c] = gdz[c] + kC3c * xy * k[27 + c] - kC3j * yz * k[30 + c] + (kC3k * zz - kC3g) * k[33 + c]
                                 - kC3j * xz * k[36 + c] + kC3h * (xx - yy) * k[39 + c];
                    }
                }
            }
            const float gd0 = gdx[0] * gcol[0] + gdx[1] * gcol[1] + gdx[2] * gcol[2];
            const float gd1 = gdy[0] * gcol[0] + gdy[1] * gcol[1] + gdy[2] * gcol[2];
            const float gd2 = gdz[0] * gcol[0] + gdz[1] * gcol[1] + gdz[2] * gcol[2];
            const float xxr = xr * xr, yyr = yr * yr, zzr = zr * zr, xyr = xr * yr, xzr = xr * zr, yzr = yr * zr;
            const float nsq = xxr + yyr + zzr;
            const float sc = 1.0f / sqrtf(nsq * nsq * nsq);
            dpos[0] = ((yyr + zzr) * gd0 - xyr * gd1 - xzr * gd2) * sc;
            dpos[1] = (-xyr * gd0 + (xxr + zzr) * gd1 - yzr * gd2) * sc;
            dpos[2] = (-xzr * gd0 - yzr * gd1 + (xxr + yyr) * gd2) * sc;
        }

        // ---- EWA backward (kb:57-255) ----
        Projection P;
        project_gaussian(cam, m, s, q, P);
        const float ks = cam.proper_aa ? kDilationProperAA : kDilation;
        const float ea = P.a_raw + ks, eb = P.b, ec = P.c_raw + ks;
        const float aa = ea * ea, bb = eb * eb, cc = ec * ec, ac = ea * ec, ab = ea * eb, bc = eb * ec;
        const float det = ac - bb;
        const float det_rcp_sq = 1.0f / (det * det);
        const float gcx = rec[2], gcy = rec[3], gcz = rec[4];
        const float dcov_x = det_rcp_sq * (2.0f * bc * gcy - cc * gcx - bb * gcz);     // kb:130-134
        const float dcov_y = det_rcp_sq * (bc * gcx - (ac + bb) * gcy + ab * gcz);
        const float dcov_z = det_rcp_sq * (2.0f * ab * gcy - bb * gcx - aa * gcz);
        float d_opacity = rec[5];
        if (cam.proper_aa) {                                                           // kb:137-145 (cov2d branch off, cfg:12)
            const float opacity = sigmoid_f(FUSED ? st_p[6] : a.opacities[i]);
            const float det_raw = P.a_raw * P.c_raw - bb;
            d_opacity = d_opacity * sqrtf(fmaxf(det_raw / det, 0.0f)) * opacity * (1.0f - opacity);
        }
        sum_into<MULTI>(g_op[0], d_opacity);
        const float* j1 = P.jw1; const float* j2 = P.jw2;
        float d3[6];                                                                   // kb:163-170
        d3[0] = j1[0] * j1[0] * dcov_x + 2.0f * j1[0] * j2[0] * dcov_y + j2[0] * j2[0] * dcov_z;
        d3[1] = j1[0] * j1[1] * dcov_x + (j1[0] * j2[1] + j1[1] * j2[0]) * dcov_y + j2[0] * j2[1] * dcov_z;
        d3[2] = j1[0] * j1[2] * dcov_x + (j1[0] * j2[2] + j1[2] * j2[0]) * dcov_y + j2[0] * j2[2] * dcov_z;
        d3[3] = j1[1] * j1[1] * dcov_x + 2.0f * j1[1] * j2[1] * dcov_y + j2[1] * j2[1] * dcov_z;
        d3[4] = j1[1] * j1[2] * dcov_x + (j1[1] * j2[2] + j1[2] * j2[1]) * dcov_y + j2[1] * j2[2] * dcov_z;
        d3[5] = j1[2] * j1[2] * dcov_x + 2.0f * j1[2] * j2[2] * dcov_y + j2[2] * j2[2] * dcov_z;
        float djw1[3], djw2[3];                                                        // kb:173-182
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            djw1[k] = 2.0f * (P.jwc1[k] * dcov_x + P.jwc2[k] * dcov_y);
            djw2[k] = 2.0f * (P.jwc1[k] * dcov_y + P.jwc2[k] * dcov_z);
        }
        const float dj11 = cam.r1[0] * djw1[0] + cam.r1[1] * djw1[1] + cam.r1[2] * djw1[2];
        const float dj22 = cam.r2[0] * djw2[0] + cam.r2[1] * djw2[1] + cam.r2[2] * djw2[2];
        const float dj13 = cam.r3[0] * djw1[0] + cam.r3[1] * djw1[1] + cam.r3[2] * djw1[2];
        const float dj23 = cam.r3[0] * djw2[0] + cam.r3[1] * djw2[1] + cam.r3[2] * djw2[2];
        const float gm2x = rec[0], gm2y = rec[1];
        if (a.densification_info != nullptr) {                                         // kb:197-201 (the count of visible views: above)
            const float nx = 0.5f * (gm2x * cam.width), ny = 0.5f * (gm2y * cam.height);
            a.densification_info[n + i] += sqrtf(nx * nx + ny * ny);
        }
        float dcam[3];                                                                 // kb:204-217
        dcam[0] = P.j11 * gm2x;
        dcam[1] = P.j22 * gm2y;
        dcam[2] = -P.j11 * P.x * gm2x - P.j22 * P.y * gm2y;
        const bool valid_x = P.x >= P.clip_l && P.x <= P.clip_r;
        const bool valid_y = P.y >= P.clip_t && P.y <= P.clip_b;
        if (valid_x) dcam[0] -= P.j11 * dj13 / P.depth;
        if (valid_y) dcam[1] -= P.j22 * dj23 / P.depth;
        const float fxm = valid_x ? 2.0f : 1.0f, fym = valid_y ? 2.0f : 1.0f;
        dcam[2] += (P.j11 * (fxm * P.x_clipped * dj13 - dj11) + P.j22 * (fym * P.y_clipped * dj23 - dj22)) / P.depth;
#pragma unroll
        for (int k = 0; k < 3; ++k)                                                    // kb:220-228
            sum_into<MULTI>(g_mean[k], (cam.r1[k] * dcam[0] + cam.r2[k] * dcam[1] + cam.r3[k] * dcam[2]) + dpos[k]);
        if constexpr (POSE) {
            // p = W m + t and J W with W = w2c[:3,:3], t = w2c[:3,3]: dL/dt = dL/dp, dL/dW = dL/dp m^T + J^T dL/d(J W); the colour sees mean - cam_position.
            // dL/dp is dcam plus, on the depth-supervised pass, dL/dz in its third component (z = p.z; launch_depth_mean_gradient is the mean's side of it)
            const float gp[3] = {dcam[0], dcam[1], V.acc_z != nullptr ? dcam[2] + V.acc_z[i] : dcam[2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pose[0 + k] = gp[0] * m[k] + P.j11 * djw1[k];
                pose[4 + k] = gp[1] * m[k] + P.j22 * djw2[k];
                pose[8 + k] = gp[2] * m[k] + (P.j13 * djw1[k] + P.j23 * djw2[k]);      // j13 = -j11 x_clipped, j23 = -j22 y_clipped
                pose[4 * k + 3] = gp[k];
                pose[12 + k] = -dpos[k];
            }
        }
        const float* R = P.R; const float* G = P.RSS;
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                                  // kb:231-240
            const float dvar = R[k] * R[k] * d3[0] + R[3 + k] * R[3 + k] * d3[3] + R[6 + k] * R[6 + k] * d3[5]
                               + 2.0f * (R[k] * R[3 + k] * d3[1] + R[k] * R[6 + k] * d3[2] + R[3 + k] * R[6 + k] * d3[4]);
            sum_into<MULTI>(g_scale[k], 2.0f * P.var[k] * dvar);
        }
        float dR[9];                                                                   // kb:243-253
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dR[0 + k] = 2.0f * (G[0 + k] * d3[0] + G[3 + k] * d3[1] + G[6 + k] * d3[2]);
            dR[3 + k] = 2.0f * (G[0 + k] * d3[1] + G[3 + k] * d3[3] + G[6 + k] * d3[4]);
            dR[6 + k] = 2.0f * (G[0 + k] * d3[2] + G[3 + k] * d3[4] + G[6 + k] * d3[5]);
        }
        float d_rot[4];
        quat_to_rotation_backward(q[0], q[1], q[2], q[3], dR, d_rot);
#pragma unroll
        for (int k = 0; k < 4; ++k) sum_into<MULTI>(g_rot[k], d_rot[k]);
    }
    // group order: 0 means, 1 sh0, 2 opacities, 3 scales, 4 rotations
#pragma unroll
    for (int k = 0; k < 3; ++k) { grad[0 + k] = g_mean[k]; grad[3 + k] = g_sh0[k]; grad[7 + k] = g_scale[k]; }
    grad[6] = g_op[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) grad[10 + k] = g_rot[k];
    return visible;
}
// ... without the camera terms: what every kernel but backward_gradients_kernel<RT, true> calls
template <bool FUSED, bool MULTI, bool KEEP_DIR>
__device__ __forceinline__ bool gaussian_backward(const PreprocessBackwardArgs& a, const unsigned i, const float (&st_p)[14],
                                                  float (&grad)[14], float (&dir)[3], float (&gcol_out)[3], bool& reached) {
    float no_pose[kPoseTerms];            // never touched: every use is under `if constexpr (POSE)`
    return gaussian_backward<FUSED, MULTI, KEEP_DIR, false>(a, i, st_p, grad, dir, gcol_out, reached, no_pose);
}

template <bool FUSED, bool MULTI>
__global__ void __launch_bounds__(kPreprocessBackwardBlock) preprocess_backward_kernel(const PreprocessBackwardArgs a) {
    const unsigned i = blockIdx.x * kPreprocessBackwardBlock + threadIdx.x;
    if (i >= a.n) return;
    float st_p[14], st_m[14], st_v[14];
    if (FUSED) {
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
#pragma unroll
            for (int k = 0; k < kGroupWidth[grp]; ++k) {
                const size_t e = (size_t)i * kGroupWidth[grp] + k;
                st_p[kGroupOffset[grp] + k] = a.p[grp][e]; st_m[kGroupOffset[grp] + k] = a.m[grp][e]; st_v[kGroupOffset[grp] + k] = a.v[grp][e];
            }
    }
    float grad[14], dir[3], gcol[3];
    bool reached;
    gaussian_backward<FUSED, MULTI, false>(a, i, st_p, grad, dir, gcol, reached);

    // Every element is written (zeros if invisible).
    float* const outs[5] = {a.grad_means, a.grad_sh0, a.grad_opacities, a.grad_scales, a.grad_rotations};
#pragma unroll
    for (int grp = 0; grp < 5; ++grp)
#pragma unroll
        for (int k = 0; k < kGroupWidth[grp]; ++k) {
            const size_t e = (size_t)i * kGroupWidth[grp] + k;
            const int o = kGroupOffset[grp] + k;
            if (!FUSED) {
                if (!MULTI || !a.accumulate) outs[grp][e] = grad[o];       // view batches after the first add (sharded path only)
                else if (reached) outs[grp][e] += grad[o];
            } else {
                adam_update(st_p[o], st_m[o], st_v[o], grad[o], a.h[grp]);
                a.p[grp][e] = st_p[o]; a.m[grp][e] = st_m[o]; a.v[grp][e] = st_v[o];
            }
        }
}

// ---- what the wave-per-64-Gaussians kernels share ---------------------------------------------------------------------
// Workgroups of 256. Wave wv of a workgroup owns the Gaussians first .. first + n_here - 1, one per lane, and with them a CONTIGUOUS run of the
// [N, R, 3] tensors: count floats from element base on (64 * R * 12 bytes per wave: 16-byte aligned iff the tensor is). A wave with first >= n
// has nothing to do and returns at once (wave-uniform); n_here and count mean something only for the others.
struct WaveBlock { uint32_t R, lane, wv, first, n_here, count; size_t base; };
template <int RT> __device__ __forceinline__ WaveBlock wave_block(const uint32_t n, const uint32_t total_sh_rest) {
    WaveBlock w;
    w.R = RT > 0 ? static_cast<uint32_t>(RT) : total_sh_rest;
    w.lane = lane_id(); w.wv = threadIdx.x >> 6;
    w.first = blockIdx.x * 256u + w.wv * kWave;
    w.n_here = n - w.first < kWave ? n - w.first : kWave;
    w.count = w.n_here * w.R * 3u;
    w.base = (size_t)w.first * w.R * 3u;
    return w;
}

// The 15 basis values of a view direction: zeros if `on` is false, and for the degrees above the active one (they keep a zero gradient)
__device__ __forceinline__ void lane_sh_basis(float (&B)[15], const bool on, const float x, const float y, const float z, const unsigned active) {
#pragma unroll
    for (int k = 0; k < 15; ++k) B[k] = 0.0f;
    if (on) sh_basis(x, y, z, active, B);
}

// ---- the wave's SH-rest gradient block, kept FACTORED in LDS ---------------------------------------------------------
// The gradient of sh_coefficients_rest[g][k][c] is basis_k(dir_g) * dL/dcolour_c(g) (sh_utils.cuh:90-111): 18 numbers per Gaussian
// (3 colour gradients + 15 basis values) instead of 45 products: 4.5 KB of LDS per wave instead of 11.25 KB, and the product is formed when
// a 16-byte piece of the [N, R, 3] block is assembled -- the same single multiplication, so the result is bit-identical. A float4 piece
// starting at element e0 of the wave's block covers exactly the (Gaussian, basis) pairs e0/3 and e0/3 + 1. Used by the fused kernel, where
// the slice is also the staging area of phase A (one 14 x 64 array at a time); the unfused K12 keeps the block of products (measured: the
// piece assembly costs it 0.003 ms and it gains nothing from the LDS, profiles/archive/r03_ab_fused_factored.txt).
constexpr uint32_t kShFactorStride = 18;                 // floats per Gaussian: colour gradient 3, basis values 15
constexpr uint32_t kShFactorFloats = kWave * kShFactorStride;

__device__ __forceinline__ void put_sh_factors(float* const slice, const uint32_t lane, const bool reached, const float (&dir)[3],
                                               const float (&gcol)[3], const int active_sh_bases) {
    float B[15];
    lane_sh_basis(B, reached && active_sh_bases > 1, dir[0], dir[1], dir[2], active_sh_bases);
    float* const mine = slice + lane * kShFactorStride;
    mine[0] = gcol[0]; mine[1] = gcol[1]; mine[2] = gcol[2];           // zeros for an invisible or unreached Gaussian
#pragma unroll
    for (int k = 0; k < 15; ++k) mine[3 + k] = B[k];
}

template <int RT>
__device__ __forceinline__ float sh_rest_gradient_at(const float* const slice, const uint32_t e, const uint32_t R) {
    const uint32_t pair = e / 3u, c = e - 3u * pair;
    const uint32_t g = RT > 0 ? pair / static_cast<uint32_t>(RT) : pair / R, k = pair - g * R;
    const float* const f = slice + g * kShFactorStride;
    return f[3u + k] * f[c];
}

template <int RT>
__device__ __forceinline__ float4 sh_rest_gradient_piece(const float* const slice, const uint32_t e0, const uint32_t R) {
    const uint32_t p0 = e0 / 3u, r0 = e0 - 3u * p0;                    // first pair of the piece, channel its first element starts at
    const uint32_t g0 = RT > 0 ? p0 / static_cast<uint32_t>(RT) : p0 / R, k0 = p0 - g0 * R;
    const bool wrap = k0 + 1u == R;                                    // the second pair belongs to the next Gaussian
    const float* const f0 = slice + g0 * kShFactorStride;
    const float* const f1 = wrap ? f0 + kShFactorStride : f0;
    const float b0 = f0[3u + k0], b1 = f1[wrap ? 3u : 4u + k0];
    const float v0 = b0 * f0[0], v1 = b0 * f0[1], v2 = b0 * f0[2], v3 = b1 * f1[0], v4 = b1 * f1[1], v5 = b1 * f1[2];
    float4 g;                                                          // elements r0 .. r0 + 3 of (v0 .. v5)
    g.x = r0 == 0u ? v0 : r0 == 1u ? v1 : v2;
    g.y = r0 == 0u ? v1 : r0 == 1u ? v2 : v3;
    g.z = r0 == 0u ? v2 : r0 == 1u ? v3 : v4;
    g.w = r0 == 0u ? v3 : r0 == 1u ? v4 : v5;
    return g;
}

// ---- single-GPU fused backward + Adam (BASELINE.json configs[3]): ONE kernel for all 59 floats of a Gaussian -----------
// A wave owns 64 consecutive Gaussians. Phase A, one lane per Gaussian: the 14 small floats and their moments are requested,
// the gradient of the Gaussian is formed (gaussian_backward, which also gathers the lane's 45 SH-rest coefficients for the
// view-direction term -- the only read of that tensor from HBM), Adam is applied to the 14 floats, and the 45 SH-rest
// gradient floats basis_k(dir) * dL/dcolour (sh_utils.cuh:90-111) go to the wave's private LDS slice, which then holds the
// gradient of the wave's CONTIGUOUS 64 x R x 3 block of the [N, R, 3] tensors. Phase B streams that block of parameter /
// exp_avg / exp_avg_sq as non-temporal 16-byte accesses (the parameter block was just gathered: L2 hits). Compared with the
// two-kernel form of round 1 the SH-rest parameters are read from HBM once instead of twice, the view direction never
// leaves registers, and the 15 basis values are evaluated once per Gaussian instead of once per (Gaussian, basis) pair.
// Bytes per Gaussian: 59 x 24 (state in / out) + 36 + 4 (accumulators, tile count) [+ 16 densification] = 1456.
#ifndef FGS_FUSED_UNROLL
#define FGS_FUSED_UNROLL 3
#endif
constexpr int kFusedUnroll = FGS_FUSED_UNROLL;          // 16-byte pieces of each of the three streams in flight per lane
#ifndef FGS_FUSED_WAVES
#define FGS_FUSED_WAVES 3
#endif
// Phase A moves one array at a time -- the five group tensors of the parameters, of exp_avg or of exp_avg_sq -- between global memory and the 14
// registers of every lane. whole (a full wave of 16-byte aligned tensors): a wave's 64 x w floats of a group are contiguous, so they come in (and go
// out) as ONE coalesced 16-byte access per lane and pass through the wave's LDS slice; otherwise w scalar accesses per lane.
constexpr int kStageLanes[5] = {48, 48, 16, 48, 64};                  // 64 w / 4 float4 pieces
__device__ __forceinline__ void stage_request(float4 (&in)[5], float* const (&src)[5], const bool whole, const WaveBlock& w) {
    if (!whole) return;                                               // stage_in gathers
#pragma unroll
    for (int grp = 0; grp < 5; ++grp)
        if (w.lane < static_cast<uint32_t>(kStageLanes[grp])) in[grp] = load_float4_nt(src[grp] + (size_t)w.first * kGroupWidth[grp] + 4u * w.lane);
}
// ic: the lane's Gaussian; the out-of-range lanes of a partial wave shadow the last one (loads only)
__device__ __forceinline__ void stage_in(float (&st)[14], float* const (&src)[5], const float4 (&in)[5], const bool whole, const uint32_t ic,
                                         const WaveBlock& w, float* const slice) {
    if (whole) {
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
            if (w.lane < static_cast<uint32_t>(kStageLanes[grp])) *reinterpret_cast<float4*>(slice + kGroupOffset[grp] * kWave + 4u * w.lane) = in[grp];
        wave_lds_fence();
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
#pragma unroll
            for (int k = 0; k < kGroupWidth[grp]; ++k) st[kGroupOffset[grp] + k] = slice[kGroupOffset[grp] * kWave + w.lane * kGroupWidth[grp] + k];
        wave_lds_fence();                                             // the next array overwrites the slice
    } else {
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
#pragma unroll
            for (int k = 0; k < kGroupWidth[grp]; ++k) st[kGroupOffset[grp] + k] = src[grp][(size_t)ic * kGroupWidth[grp] + k];
    }
}
__device__ __forceinline__ void stage_out(float* const (&dst)[5], const float (&st)[14], const bool whole, const WaveBlock& w, float* const slice) {
    if (whole) {
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
#pragma unroll
            for (int k = 0; k < kGroupWidth[grp]; ++k) slice[kGroupOffset[grp] * kWave + w.lane * kGroupWidth[grp] + k] = st[kGroupOffset[grp] + k];
        wave_lds_fence();
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
            if (w.lane < static_cast<uint32_t>(kStageLanes[grp]))
                store_float4_nt(dst[grp] + (size_t)w.first * kGroupWidth[grp] + 4u * w.lane, *reinterpret_cast<const float4*>(slice + kGroupOffset[grp] * kWave + 4u * w.lane));
        wave_lds_fence();                                             // the slice is rewritten by the next array, then by the SH-rest factors
    }
}

template <int RT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FGS_FUSED_WAVES, FGS_FUSED_WAVES)))
fused_backward_adam_kernel(const PreprocessBackwardArgs a, const ShRestArgs sh) {
    __shared__ __attribute__((aligned(16))) float s_grad[256 / kWave][kShFactorFloats];   // >= the 14 x 64 floats phase A stages per array
    const WaveBlock w = wave_block<RT>(a.n, sh.total_sh_rest);
    if (w.first >= a.n) return;
    const uint32_t i = w.first + w.lane;
    const bool in_range = i < a.n;
    float* const slice = s_grad[w.wv];                                // the wave's LDS slice: phase A staging now, the SH-rest gradient block later
    const bool whole = a.vector_ok != 0 && w.n_here == kWave;         // 16-byte accesses need 16-byte aligned tensors (checked at launch)

    // ---- phase A: the 14 small floats of parameters and both moments (stage_request / stage_in / stage_out), instead of w scalar accesses per
    // lane at a stride of 4 w bytes -- 42 loads + 42 stores per lane before, more memory instructions than phase B issues for three times the data. ----
    // The parameters come first (the gradient needs them); the moments are requested after the gradient is formed, so 28 registers are not
    // held across gaussian_backward, and every array passes through the same 3.5 KB of the slice. Round 3, one box: 0.850 -> 0.812 ms
    // (profiles/archive/r03_ab_fused_factored.txt; 3 or 4 waves per SIMD measure the same, 5 spills; requesting phase B's first pieces before the
    // gradient, or double-buffering phase B, measured slower at every depth tried).
    float st_p[14], st_m[14], st_v[14];
    float4 in_p[5], in_m[5], in_v[5];
    const uint32_t ic = in_range ? i : a.n - 1u;
    stage_request(in_p, a.p, whole, w);
    stage_in(st_p, a.p, in_p, whole, ic, w, slice);
    float grad[14], dir[3] = {0.0f, 0.0f, 0.0f}, gcol[3] = {0.0f, 0.0f, 0.0f};
    bool reached = false;
#pragma unroll
    for (int k = 0; k < 14; ++k) grad[k] = 0.0f;
    if (in_range) gaussian_backward<true, false, true>(a, i, st_p, grad, dir, gcol, reached);
    stage_request(in_m, a.m, whole, w);                               // both moments are requested before either is consumed
    stage_request(in_v, a.v, whole, w);
    stage_in(st_m, a.m, in_m, whole, ic, w, slice);
    stage_in(st_v, a.v, in_v, whole, ic, w, slice);
    if (in_range) {
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
#pragma unroll
            for (int k = 0; k < kGroupWidth[grp]; ++k) {
                const int o = kGroupOffset[grp] + k;
                adam_update(st_p[o], st_m[o], st_v[o], grad[o], a.h[grp]);
                if (!whole) {                                         // scalar path: stored here, not in stage_out -- 42 values held to the end cost 4 registers
                    const size_t e = (size_t)i * kGroupWidth[grp] + k;
                    a.p[grp][e] = st_p[o]; a.m[grp][e] = st_m[o]; a.v[grp][e] = st_v[o];
                }
            }
    }
    stage_out(a.p, st_p, whole, w, slice);
    stage_out(a.m, st_m, whole, w, slice);
    stage_out(a.v, st_v, whole, w, slice);
    if (w.R == 0) return;

    // ---- the wave's SH-rest gradient factors -> LDS (skipped when K11 reached no Gaussian of the wave: the block is zero) ----
    const bool any_reached = wave_ballot(reached) != 0;
    if (any_reached) {
        put_sh_factors(slice, w.lane, reached, dir, gcol, sh.active_sh_bases);
        wave_lds_fence();
    }

    // ---- phase B: Adam over the wave's contiguous block, 3 streams x kFusedUnroll pieces in flight per lane ----
    float* const P = sh.p + w.base; float* const M = sh.m + w.base; float* const V = sh.v + w.base;
    for (uint32_t e0 = 4u * w.lane; e0 < w.count; e0 += 4u * kWave * kFusedUnroll) {
        AdamPiece piece[kFusedUnroll];
        bool full[kFusedUnroll];
#pragma unroll
        for (int u = 0; u < kFusedUnroll; ++u) {
            const uint32_t e = e0 + 4u * kWave * static_cast<uint32_t>(u);
            full[u] = e + 4u <= w.count && a.vector_ok != 0;                           // 16-byte pieces need 16-byte aligned tensors (checked at launch)
            if (full[u]) piece[u].load(P + e, M + e, V + e);
        }
#pragma unroll
        for (int u = 0; u < kFusedUnroll; ++u) {
            const uint32_t e = e0 + 4u * kWave * static_cast<uint32_t>(u);
            if (full[u])
                piece[u].step(P + e, M + e, V + e, any_reached ? sh_rest_gradient_piece<RT>(slice, e, w.R) : make_float4(0.0f, 0.0f, 0.0f, 0.0f), sh.h);
            else if (e < w.count)                                                      // ragged tail of the last wave (< 4 floats), or unaligned tensors
                adam_scalar_tail(P, M, V, e, w.count < e + 4u ? w.count : e + 4u, sh.h,
                                 [&](const uint32_t j) { return any_reached ? sh_rest_gradient_at<RT>(slice, j, w.R) : 0.0f; });
        }
    }
}

// Unfused single-view K12 as ONE kernel (the form fgs_backward uses): the same wave layout as fused_backward_adam_kernel, with the
// gradients written instead of applied. Against round 1's two kernels it drops the view-direction round trip through HBM and the second
// read of tile counts / colour gradients, and keeps the fully coalesced 16-byte stores of the [N, R, 3] gradient (every element of every
// gradient is written exactly once, zeros for invisible Gaussians: no zero-fill, rasterization_api.cu:127-134).
#ifndef FGS_K12_NT_STORES
#define FGS_K12_NT_STORES 1      // round 6: the 540 MB SH-rest gradient leaves as non-temporal stores (K12 0.248 -> 0.242 ms and the Adam kernel behind it
                                 // 0.771 -> 0.758 in alternating processes, profiles/r06_ab_k12_nt_stores.txt); 2: the 14 small floats as well (A/B)
#endif
// The caller's promise about what the gradient tensors hold NOW (PreprocessBackwardArgs::prior_blocks): block b of all six is zero already. A wave that
// reaches no Gaussian would only write those zeros again -- nine tenths of this kernel's traffic in a dense scene -- so it may leave them alone. Belt and
// braces as in adam_block_gradient_needed (adam.hip): the promise rests on the caller's proof that nobody touched the tensors since the pass that
// published the flag, and a write behind the framework's bookkeeping (`.grad.data.add_(...)`, a raw pointer) is invisible to it. The block's first
// element of every tensor -- six wave-uniform loads, requested at entry for a block flagged 0 -- must compare equal to 0.0f as well; anything else there (a whole-tensor edit such
// as hand-written weight decay, NaN / Inf) and the block is written as before.
__device__ __forceinline__ bool block_promised_zero(const PreprocessBackwardArgs& a, const ShRestArgs& sh, const WaveBlock& w) {
    if (a.prior_blocks == nullptr) return false;
    const size_t first = wave_uniform(w.first);
    if (a.prior_blocks[first >> 6] != 0) return false;
    const float s0 = a.grad_means[3u * first], s1 = a.grad_sh0[3u * first], s2 = a.grad_opacities[first], s3 = a.grad_scales[3u * first],
                s4 = a.grad_rotations[4u * first], s5 = w.R > 0 ? sh.grad_sh_rest[first * w.R * 3u] : 0.0f;
    return s0 == 0.0f && s1 == 0.0f && s2 == 0.0f && s3 == 0.0f && s4 == 0.0f && s5 == 0.0f;
}

// POSE (backward_gradients_kernel<RT, true>, fgs_backward_pose): the arguments are PreprocessBackwardPoseArgs, the lanes' 15 camera terms are summed over the wave (fgs_wave.h: full
// EXEC -- only the wave-uniform exits above and below surround it) and lane 63, which holds the sums, stores the wave's line of PosePart::partials.
// Every wave with first < n stores its line, a wave that reached nothing as zeros, BEFORE the recycled path's early return: the reduction that
// follows reads every line and nothing of what the scratch held before. Every POSE statement is under `if constexpr`:
// backward_gradients_kernel<RT, false> compiles to the instructions the kernel had.
template <bool POSE> using K12ArgsOf = std::conditional_t<POSE, PreprocessBackwardPoseArgs, PreprocessBackwardArgs>;
__device__ __forceinline__ const PreprocessBackwardArgs& k12_part(const PreprocessBackwardArgs& a) { return a; }
__device__ __forceinline__ const PreprocessBackwardArgs& k12_part(const PreprocessBackwardPoseArgs& a) { return a.k12; }
__device__ __forceinline__ float* pose_partials(const PreprocessBackwardArgs&) { return nullptr; }                  // never read: every use is under `if constexpr (POSE)`
__device__ __forceinline__ float* pose_partials(const PreprocessBackwardPoseArgs& a) { return a.pose.partials; }

template <int RT, bool POSE = false>
__global__ void __launch_bounds__(256) backward_gradients_kernel(const K12ArgsOf<POSE> args, const ShRestArgs sh) {
    __shared__ __attribute__((aligned(16))) float s_grad[256 / kWave][kWave * 15 * 3];
    const PreprocessBackwardArgs& a = k12_part(args);
    const WaveBlock w = wave_block<RT>(a.n, sh.total_sh_rest);
    if (w.first >= a.n) return;
    const bool promised_zero = block_promised_zero(a, sh, w);
    const uint32_t i = w.first + w.lane;
    const bool in_range = i < a.n;
    float grad[14], dir[3] = {0.0f, 0.0f, 0.0f}, gcol[3] = {0.0f, 0.0f, 0.0f};
    const float unused[14] = {};
    bool visible = false, reached = false;
    [[maybe_unused]] float pose[kPoseTerms];
    if constexpr (POSE) {
#pragma unroll
        for (int k = 0; k < kPoseTerms; ++k) pose[k] = 0.0f;           // the out-of-range lanes of the last wave
        if (in_range) visible = gaussian_backward<false, false, true, true>(a, i, unused, grad, dir, gcol, reached, pose);
    } else {
        if (in_range) visible = gaussian_backward<false, false, true>(a, i, unused, grad, dir, gcol, reached);
    }
    float* const slice = s_grad[w.wv];
    const bool any_visible = wave_ballot(visible) != 0, any_reached = wave_ballot(reached) != 0;
    if (a.live_blocks != nullptr && w.lane == 0) a.live_blocks[w.first >> 6] = any_visible ? 1 : 0;   // first is a multiple of 64; "visible", not "reached": the flag's contract
    if (a.reached_blocks != nullptr && w.lane == 0) a.reached_blocks[w.first >> 6] = any_reached ? 1 : 0;   // 0: every row of the block is +-0 in all six tensors
    if constexpr (POSE) {
        float* const line = pose_partials(args) + (size_t)(w.first >> 6) * kPoseLineFloats;
        if (any_reached) {                                             // wave-uniform: all 64 lanes take the reductions
#pragma unroll
            for (int k = 0; k < kPoseTerms; ++k) {
                const float total = wave_sum_to_lane63(pose[k]);       // valid in lane 63 only
                if (w.lane == kWave - 1) line[k] = total;
            }
            if (w.lane == kWave - 1) line[kPoseTerms] = 0.0f;
        } else if (w.lane < static_cast<uint32_t>(kPoseLineFloats)) {
            line[w.lane] = 0.0f;                                       // 64 lanes of zeros sum to zero: one coalesced store instead
        }
    }
    if (!any_reached && promised_zero) return;                         // the zeros are there already: none of the block's 59 x 64 floats is stored
    if (in_range) {
        // scalar stores at a stride of 4 w bytes: the write path combines them. Staging the wave's 64 x w block in LDS and storing it as one
        // coalesced 16-byte access per lane -- what pays in the fused kernel, where the same floats are also LOADED three times -- measured
        // 0.261 vs 0.252 ms here (profiles/archive/r02_ab_k12_coalesced_stores.txt)
        float* const outs[5] = {a.grad_means, a.grad_sh0, a.grad_opacities, a.grad_scales, a.grad_rotations};
#pragma unroll
        for (int grp = 0; grp < 5; ++grp)
#pragma unroll
            for (int k = 0; k < kGroupWidth[grp]; ++k) {
#if FGS_K12_NT_STORES >= 2
                __builtin_nontemporal_store(grad[kGroupOffset[grp] + k], outs[grp] + (size_t)i * kGroupWidth[grp] + k);
#else
                outs[grp][(size_t)i * kGroupWidth[grp] + k] = grad[kGroupOffset[grp] + k];
#endif
            }
    }
    if (w.R == 0) return;
    if (any_reached) {                                                 // a wave K11 reached no Gaussian of writes its SH-rest block as zeros
        float B[15];
        lane_sh_basis(B, reached && sh.active_sh_bases > 1, dir[0], dir[1], dir[2], sh.active_sh_bases);
        float* const mine = slice + w.lane * w.R * 3u;
#pragma unroll
        for (int k = 0; k < 15; ++k)
            if (static_cast<uint32_t>(k) < w.R) { mine[3 * k] = B[k] * gcol[0]; mine[3 * k + 1] = B[k] * gcol[1]; mine[3 * k + 2] = B[k] * gcol[2]; }
        wave_lds_fence();
    }
    float* const out = sh.grad_sh_rest + w.base;
    for (uint32_t e = 4u * w.lane; e < w.count; e += 4u * kWave) {
        if (e + 4u <= w.count && a.vector_ok) {                        // 16-byte stores need a 16-byte aligned gradient tensor (checked at launch)
            const float4 g = any_reached ? *reinterpret_cast<const float4*>(slice + e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#if FGS_K12_NT_STORES
            store_float4_nt(out + e, g);
#else
            *reinterpret_cast<float4*>(out + e) = g;
#endif
        } else {
            for (uint32_t j = e; j < w.count && j < e + 4u; ++j) out[j] = any_reached ? slice[j] : 0.0f;
        }
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The SH-rest kernels come in two instantiations: RT = 15 (every degree present: the divisions by R are by a constant) and 0 (R read from the
// arguments). launch(rt) starts the one for decltype(rt)::value; more than 15 coefficients per channel fit none of them.
template <class Launch> static hipError_t dispatch_sh_rest(const uint32_t total_sh_rest, Launch launch) {
    if (total_sh_rest > 15) return hipErrorInvalidValue;
    if (total_sh_rest == 15) launch(std::integral_constant<int, 15>());
    else launch(std::integral_constant<int, 0>());
    return hipGetLastError();
}

hipError_t launch_backward_gradients(const PreprocessBackwardArgs& a_in, const ShRestArgs& sh, hipStream_t s) {
    if (a_in.n == 0) return hipSuccess;
    PreprocessBackwardArgs a = a_in;
    a.vector_ok = aligned16(sh.grad_sh_rest) ? 1 : 0;                  // a wave's block starts 64 * R * 12 bytes into the tensor: aligned iff the tensor is
    const dim3 grid((a.n + 255u) / 256u), block(256);
    return dispatch_sh_rest(sh.total_sh_rest, [&](auto rt) { hipLaunchKernelGGL(backward_gradients_kernel<decltype(rt)::value>, grid, block, 0, s, a, sh); });
}

// ---- the pose partials -> 15 numbers, in a fixed order, accumulated in fp64 ------------------------------------------------------------
// Thread t of a workgroup of 256 owns term t & 15 and every 16th line from line t >> 4 on: a step of the loop reads 16 consecutive lines (1 KB,
// coalesced). The 16 sub-sums of a term are then added in ascending order by one thread. Stage 1: one workgroup per chunk of `lines_per_chunk` lines
// (a multiple of 16) -> chunk_sums[chunk][16] (double). Stage 2: one workgroup adds the chunks the same way and writes the floats. Nothing depends on
// which workgroup runs when; a line or chunk that does not exist contributes nothing.
template <class T>
__device__ __forceinline__ double pose_column_sum(const T* const lines, const uint32_t first, const uint32_t end, double (&s_sub)[16][kPoseLineFloats]) {
    const uint32_t term = threadIdx.x & 15u, sub = threadIdx.x >> 4;
    double acc = 0.0;
    for (uint32_t l = first + sub; l < end; l += 16u) acc += static_cast<double>(lines[(size_t)l * kPoseLineFloats + term]);
    s_sub[sub][term] = acc;
    __syncthreads();
    double total = 0.0;
    if (sub == 0) {
#pragma unroll
        for (int k = 0; k < 16; ++k) total += s_sub[k][term];
    }
    return total;                                                       // valid in threads 0..15
}

__global__ void __launch_bounds__(256) pose_chunk_sums_kernel(const PosePart p, const uint32_t n_lines, const uint32_t lines_per_chunk) {
    __shared__ double s_sub[16][kPoseLineFloats];
    const uint32_t first = blockIdx.x * lines_per_chunk;
    const uint32_t end = first + lines_per_chunk < n_lines ? first + lines_per_chunk : n_lines;
    const double total = pose_column_sum(p.partials, first, end, s_sub);
    if (threadIdx.x < static_cast<uint32_t>(kPoseLineFloats)) p.chunk_sums[(size_t)blockIdx.x * kPoseLineFloats + threadIdx.x] = total;
}

__global__ void __launch_bounds__(256) pose_final_sum_kernel(const PosePart p, const uint32_t n_chunks) {
    __shared__ double s_sub[16][kPoseLineFloats];
    const double total = pose_column_sum(p.chunk_sums, 0u, n_chunks, s_sub);
    const uint32_t term = threadIdx.x;
    if (term < 12u) { if (p.grad_w2c != nullptr) p.grad_w2c[term] = static_cast<float>(total); }
    else if (term < static_cast<uint32_t>(kPoseTerms)) { if (p.grad_cam_position != nullptr) p.grad_cam_position[term - 12u] = static_cast<float>(total); }
}

hipError_t launch_backward_gradients_pose(const PreprocessBackwardArgs& a_in, const ShRestArgs& sh, const PosePart& pose, hipStream_t s) {
    if (a_in.n == 0) return hipSuccess;                                // the caller writes the 15 zeros
    PreprocessBackwardPoseArgs a{a_in, pose};
    a.k12.vector_ok = aligned16(sh.grad_sh_rest) ? 1 : 0;
    const dim3 grid((a.k12.n + 255u) / 256u), block(256);
    const hipError_t e = dispatch_sh_rest(sh.total_sh_rest, [&](auto rt) { hipLaunchKernelGGL((backward_gradients_kernel<decltype(rt)::value, true>), grid, block, 0, s, a, sh); });
    if (e != hipSuccess) return e;
    const uint32_t n_lines = (a.k12.n + kWave - 1u) / kWave;
    const uint32_t per_chunk = ((n_lines + kPoseMaxChunks - 1u) / kPoseMaxChunks + 15u) / 16u * 16u;
    const uint32_t n_chunks = (n_lines + per_chunk - 1u) / per_chunk;   // <= kPoseMaxChunks
    hipLaunchKernelGGL(pose_chunk_sums_kernel, dim3(n_chunks), block, 0, s, pose, n_lines, per_chunk);
    hipLaunchKernelGGL(pose_final_sum_kernel, dim3(1), block, 0, s, pose, n_chunks);
    return hipGetLastError();
}

hipError_t launch_fused_backward_adam(const PreprocessBackwardArgs& a_in, const ShRestArgs& sh, hipStream_t s) {
    if (a_in.n == 0) return hipSuccess;
    PreprocessBackwardArgs a = a_in;
    a.vector_ok = 1;
    for (int g = 0; g < 5; ++g) a.vector_ok = a.vector_ok && aligned16(a.p[g]) && aligned16(a.m[g]) && aligned16(a.v[g]);
    a.vector_ok = a.vector_ok && aligned16(sh.p) && aligned16(sh.m) && aligned16(sh.v);          // phase B: a wave's block starts 64 * R * 12 bytes in
    const dim3 grid((a.n + 255u) / 256u), block(256);
    return dispatch_sh_rest(sh.total_sh_rest, [&](auto rt) { hipLaunchKernelGGL(fused_backward_adam_kernel<decltype(rt)::value>, grid, block, 0, s, a, sh); });
}

hipError_t launch_preprocess_backward(bool fused_adam, const PreprocessBackwardArgs& a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    const dim3 grid((a.n + kPreprocessBackwardBlock - 1) / kPreprocessBackwardBlock), block(kPreprocessBackwardBlock);
    if (fused_adam && a.view[0].slot != nullptr) hipLaunchKernelGGL((preprocess_backward_kernel<true, true>), grid, block, 0, s, a);
    else if (fused_adam) hipLaunchKernelGGL((preprocess_backward_kernel<true, false>), grid, block, 0, s, a);
    else if (a.view[0].slot == nullptr) hipLaunchKernelGGL((preprocess_backward_kernel<false, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((preprocess_backward_kernel<false, true>), grid, block, 0, s, a);
    return hipGetLastError();
}

// ---- SH-rest pass: the [N, R, 3] tensors are streamed FLAT in 16-byte pieces (grid-stride, a few thousand workgroups) ----
// A float4 piece starting at element e0 covers exactly the (Gaussian, basis) pairs p0 = e0/3 and p0+1; for each of the two
// the lane rebuilds basis_k(view_dir) * dL/dcolour (sh_utils.cuh:90-111) from 28 bytes that 15 neighbouring lanes share.
struct PairGrad { float b; float c[3]; };

template <int RT, bool RECORDS>
__device__ __forceinline__ PairGrad pair_gradient(const ShRestArgs& a, const ShRestView& V, const uint32_t pair_in, const uint32_t n_pairs) {
    // All seven loads are issued unconditionally (one memory round trip instead of a dependent chain); the result is
    // SELECTED to zero for invisible Gaussians / inactive degrees because their view_dir slot is uninitialised scratch.
    const uint32_t pair = pair_in < n_pairs ? pair_in : n_pairs - 1u;
    const uint32_t R = RT > 0 ? static_cast<uint32_t>(RT) : a.total_sh_rest;
    const uint32_t gi = pair / R, k = pair - gi * R;
    const uint32_t touched = V.n_touched[gi];
    const float x = V.view_dir[3 * (size_t)gi], y = V.view_dir[3 * (size_t)gi + 1], z = V.view_dir[3 * (size_t)gi + 2];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    if (!RECORDS) {                      // K11's own records [N][9]: always in bounds, requested together with everything else
        const float* const accp = V.acc + (size_t)gi * kAccRecordWords;
        c0 = accp[6]; c1 = accp[7]; c2 = accp[8];
    } else if (touched != 0) {           // sharded path: a record exists only for visible primitives (slot[] of the others is scratch)
        const float* const accp = V.acc + (size_t)V.slot[gi] * kAccRecordWords;
        c0 = accp[6]; c1 = accp[7]; c2 = accp[8];
    }
    // coefficient k belongs to degree 1 (k<3), 2 (k<8), 3 (k<15); it receives a gradient only if that degree is active
    const bool degree_on = (k < 3 && a.active_sh_bases > 1) || (k >= 3 && k < 8 && a.active_sh_bases > 4) ||
                           (k >= 8 && k < 15 && a.active_sh_bases > 9);
    const bool on = pair_in < n_pairs && degree_on && touched != 0;
    float B[15];
    lane_sh_basis(B, true, x, y, z, a.active_sh_bases);
    float bk = 0.0f;
#pragma unroll
    for (int j = 0; j < 15; ++j) bk = (k == static_cast<uint32_t>(j)) ? B[j] : bk;   // select, no dynamic register indexing
    PairGrad r;
    r.b = on ? bk : 0.0f;
    r.c[0] = on ? c0 : 0.0f; r.c[1] = on ? c1 : 0.0f; r.c[2] = on ? c2 : 0.0f;
    return r;
}

// Unfused form (the gradient tensor is materialised). One lane per GAUSSIAN evaluates the 15 basis values once and forms its
// 45 gradient floats; the wave's 64 x 45 block is contiguous in the [N, R, 3] tensor, so it is transposed through the wave's
// private LDS slice and leaves as fully coalesced 16-byte stores. (v1: one lane per (Gaussian, basis) pair evaluated all 15
// basis functions to keep one -- 33 VALU instructions per output float, half VALU-bound at 0.184 ms for a 540 MB write.)
// MULTI (sharded path): the gradient is summed over the views of the launch, colour gradients come from the accumulator records.
// The lane of Gaussian w.first + w.lane: its 3 * R gradient floats, summed over the views of the launch, go to the wave's LDS slice.
template <bool MULTI>
__device__ __forceinline__ void sh_rest_block_to_lds(const ShRestArgs& a, const WaveBlock& w, float* slice) {
    const uint32_t gi = w.first + w.lane;
    const bool in_range = gi < a.n;
    float g[15][3];
#pragma unroll
    for (int k = 0; k < 15; ++k) { g[k][0] = 0.0f; g[k][1] = 0.0f; g[k][2] = 0.0f; }
    const int n_views = MULTI ? a.n_views : 1;
    for (int vw = 0; vw < n_views; ++vw) {
        const ShRestView& V = a.view[MULTI ? vw : 0];
        if (!in_range || V.n_touched[gi] == 0) continue;
        const float x = V.view_dir[3 * (size_t)gi], y = V.view_dir[3 * (size_t)gi + 1], z = V.view_dir[3 * (size_t)gi + 2];
        float c[3];
        const float* const r = V.acc + (size_t)(MULTI ? V.slot[gi] : gi) * kAccRecordWords;       // K11's record (sharded path: through the slot table)
        c[0] = r[6]; c[1] = r[7]; c[2] = r[8];
        float B[15];
        lane_sh_basis(B, a.active_sh_bases > 1, x, y, z, a.active_sh_bases);
#pragma unroll
        for (int k = 0; k < 15; ++k) {
            if (!MULTI) { g[k][0] = B[k] * c[0]; g[k][1] = B[k] * c[1]; g[k][2] = B[k] * c[2]; }
            else { g[k][0] += B[k] * c[0]; g[k][1] += B[k] * c[1]; g[k][2] += B[k] * c[2]; }
        }
    }
    float* mine = slice + w.lane * w.R * 3u;
#pragma unroll
    for (int k = 0; k < 15; ++k)
        if (static_cast<uint32_t>(k) < w.R) { mine[3 * k] = g[k][0]; mine[3 * k + 1] = g[k][1]; mine[3 * k + 2] = g[k][2]; }
    wave_lds_fence();
}

template <int RT, bool MULTI>
__global__ void __launch_bounds__(256) sh_rest_gradient_kernel(const ShRestArgs a) {
    __shared__ __attribute__((aligned(16))) float s_out[256 / kWave][kWave * 15 * 3];
    const WaveBlock w = wave_block<RT>(a.n, a.total_sh_rest);
    if (w.first >= a.n) return;
    sh_rest_block_to_lds<MULTI>(a, w, s_out[w.wv]);
    float* out = a.grad_sh_rest + w.base;
    const bool add = MULTI && a.accumulate;                                            // view batches after the first
    for (uint32_t e = 4u * w.lane; e < w.count; e += 4u * kWave) {
        if (e + 4u <= w.count) {
            float4 v = *reinterpret_cast<const float4*>(&s_out[w.wv][e]);
            if (add) { const float4 o = *reinterpret_cast<const float4*>(out + e); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            *reinterpret_cast<float4*>(out + e) = v;
        } else {
            for (uint32_t j = e; j < w.count; ++j) out[j] = add ? out[j] + s_out[w.wv][j] : s_out[w.wv][j];
        }
    }
}

// Sharded path, fused with Adam: the wave's gradient block (summed over the views) stays in LDS and feeds the update of the
// wave's contiguous 64 x R x 3 slice of parameter / exp_avg / exp_avg_sq, streamed as non-temporal 16-byte accesses.
template <int RT>
__global__ void __launch_bounds__(256) sh_rest_adam_views_kernel(const ShRestArgs a) {
    __shared__ __attribute__((aligned(16))) float s_out[256 / kWave][kWave * 15 * 3];
    const WaveBlock w = wave_block<RT>(a.n, a.total_sh_rest);
    if (w.first >= a.n) return;
    sh_rest_block_to_lds<true>(a, w, s_out[w.wv]);
    float* const P = a.p + w.base; float* const M = a.m + w.base; float* const V = a.v + w.base;
    for (uint32_t e = 4u * w.lane; e < w.count; e += 4u * kWave) {
        if (e + 4u <= w.count) {
            AdamPiece piece;
            piece.load(P + e, M + e, V + e);
            piece.step(P + e, M + e, V + e, *reinterpret_cast<const float4*>(&s_out[w.wv][e]), a.h);
        } else {
            adam_scalar_tail(P, M, V, e, w.count, a.h, [&](const uint32_t j) { return s_out[w.wv][j]; });
        }
    }
}

template <bool FUSED, int RT>
__global__ void __launch_bounds__(256) sh_rest_backward_kernel(const ShRestArgs a) {
    const uint32_t R = RT > 0 ? static_cast<uint32_t>(RT) : a.total_sh_rest;
    const uint32_t n_pairs = a.n * R;
    const uint32_t n_elems = n_pairs * 3u;                 // host guarantees < 2^32
    const uint32_t n_vec = (n_elems + 3u) / 4u;
    for (uint32_t v = blockIdx.x * 256u + threadIdx.x; v < n_vec; v += gridDim.x * 256u) {
        const uint32_t e0 = 4u * v;
        const uint32_t p0 = e0 / 3u, c0 = e0 - 3u * p0;
        const bool full = e0 + 4u <= n_elems;
        float4 p4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m4 = p4, v4 = p4;           // hand-written piece: AdamPiece costs this kernel its register count (profiles/k12_k13_split.txt)
        if (FUSED && full) { p4 = load_float4_nt(a.p + e0); m4 = load_float4_nt(a.m + e0); v4 = load_float4_nt(a.v + e0); }   // the 48 bytes of state are requested before the gradient is rebuilt (streamed once per step: non-temporal like the Adam kernel)
        const PairGrad q0 = pair_gradient<RT, false>(a, a.view[0], p0, n_pairs), q1 = pair_gradient<RT, false>(a, a.view[0], p0 + 1u, n_pairs);
        float g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t cj = c0 + static_cast<uint32_t>(j);               // 0..5: first pair while < 3
            const bool in_first = cj < 3u;                                   // scalar selects only: a pointer/reference select
            const uint32_t c = in_first ? cj : cj - 3u;                      // between q0 and q1 sends both structs to scratch
            const float qb = in_first ? q0.b : q1.b;
            const float qc0 = in_first ? q0.c[0] : q1.c[0], qc1 = in_first ? q0.c[1] : q1.c[1], qc2 = in_first ? q0.c[2] : q1.c[2];
            g[j] = qb * (c == 0u ? qc0 : (c == 1u ? qc1 : qc2));
        }
        if (!FUSED) {
            if (full) *reinterpret_cast<float4*>(a.grad_sh_rest + e0) = make_float4(g[0], g[1], g[2], g[3]);
            else for (uint32_t j = 0; e0 + j < n_elems; ++j) a.grad_sh_rest[e0 + j] = g[j];
        } else if (full) {
            adam_update(p4.x, m4.x, v4.x, g[0], a.h); adam_update(p4.y, m4.y, v4.y, g[1], a.h);
            adam_update(p4.z, m4.z, v4.z, g[2], a.h); adam_update(p4.w, m4.w, v4.w, g[3], a.h);
            store_float4_nt(a.p + e0, p4); store_float4_nt(a.m + e0, m4); store_float4_nt(a.v + e0, v4);
        } else {
            adam_scalar_tail(a.p, a.m, a.v, e0, n_elems, a.h, [&](const uint32_t e) { return g[e - e0]; });
        }
    }
}

hipError_t launch_sh_rest_backward(bool fused_adam, const ShRestArgs& a, hipStream_t s) {
    const uint64_t n_elems = (uint64_t)a.n * a.total_sh_rest * 3u;
    if (n_elems == 0) return hipSuccess;
    if (n_elems >= (1ull << 32)) return hipErrorInvalidValue;        // 32-bit element indices: N * (K-1) * 3 < 2^32
    const uint64_t n_vec = (n_elems + 3) / 4;
    const unsigned blocks = static_cast<unsigned>(n_vec / 256 + 1 < 8192 ? n_vec / 256 + 1 : 8192);   // grid-stride: 32 workgroups per CU
    const dim3 grid(blocks), ggrid((a.n + 255u) / 256u), block(256);       // flat kernel; a wave per 64 Gaussians
    const bool views = a.view[0].slot != nullptr;                          // sharded path: records + sum over views
    return dispatch_sh_rest(a.total_sh_rest, [&](auto rt) {
        constexpr int RT = decltype(rt)::value;
        if (!fused_adam && views) hipLaunchKernelGGL((sh_rest_gradient_kernel<RT, true>), ggrid, block, 0, s, a);
        else if (!fused_adam) hipLaunchKernelGGL((sh_rest_gradient_kernel<RT, false>), ggrid, block, 0, s, a);
        else if (views) hipLaunchKernelGGL(sh_rest_adam_views_kernel<RT>, ggrid, block, 0, s, a);
        else hipLaunchKernelGGL((sh_rest_backward_kernel<true, RT>), grid, block, 0, s, a);
    });
}

}  // namespace fgs

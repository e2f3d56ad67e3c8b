// What the two formulations of the L1 + DSSIM loss kernels share (loss.hip: the product's; loss_exhibits.hip: the dev library's other arm): the
// window, the per-pixel algebra -- one definition, so both forms produce the same bits per pixel -- the XCD mapping and the fixed-order reductions.
#pragma once
#include "fgs_kernels.h"
#include <fgs_wave.h>
#include <cmath>

namespace fgs {

constexpr int kHalo = 5, kTaps = 11;
struct GaussWindow { float w[kTaps]; };

inline GaussWindow make_window() {
    GaussWindow gw;
    double w[kTaps], sum = 0.0;
    for (int i = 0; i < kTaps; ++i) { w[i] = std::exp(-((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += w[i]; }
    for (int i = 0; i < kTaps; ++i) gw.w[i] = static_cast<float>(w[i] / sum);
    return gw;
}

// One tap of either filter pass: every form sums its taps from t = 0 to 10 into 0.0f through THIS, an explicit fused multiply-add, so the device, the
// simulation and both formulations round alike (the filtered maps and the gradient are equal bit for bit between the forms: tests/test_loss_stream.py).
__device__ __forceinline__ float tap(const float w, const float v, const float acc) { return __builtin_fmaf(w, v, acc); }

__device__ __forceinline__ float effective_weight(const float w) { return w > 0.0f ? w : 0.0f; }   // negative and NaN count as 0

// SSIM of one pixel from its five filtered moments, and the three partial derivative maps (d/dmu1, d/dE[x^2], d/dE[xy]) the backward filter takes.
struct SsimPoint { float value, d_mu, d_m11, d_m12; };
__device__ __forceinline__ SsimPoint ssim_point(const float mu1, const float mu2, const float m11, const float m22, const float m12) {
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float s11 = m11 - mu1 * mu1, s22 = m22 - mu2 * mu2, s12 = m12 - mu1 * mu2;
    const float A1 = 2.0f * mu1 * mu2 + C1, A2 = 2.0f * s12 + C2, B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s11 + s22 + C2;
    const float den = B1 * B2;
    SsimPoint r;
    r.value = (A1 * A2) / den;
    r.d_mu = ((2.0f * mu2 * A2 - 2.0f * mu2 * A1) * den - A1 * A2 * (2.0f * mu1 * B2 - 2.0f * mu1 * B1)) / (den * den);
    r.d_m11 = -(A1 * A2) / (B1 * B2 * B2);
    r.d_m12 = 2.0f * A1 / den;
    return r;
}

// dloss/dimage of one pixel from the three filtered derivative maps v0..v2, the pixel p, its target q and (WEIGHTED) its weight wp:
// ks * (v0 + 2 p v1 + q v2) + kl * sign(p - q) [* w^]. ks and kl carry lambda / n and the upstream gradient. The fused multiply-adds are written out, in
// the order the compiler chose for the tiled kernel this expression came from: left to itself it fused ks * (...) into the sum in one kernel and
// kl * sign into it in the other, one float32 step apart (profiles/loss_streaming.txt). WEIGHTED: SELECTED to 0.0f where the weight is not positive --
// p may be anything there.
template <bool WEIGHTED>
__device__ __forceinline__ float loss_gradient(const float ks, const float kl, const float v0, const float v1, const float v2, const float p, const float q,
                                               [[maybe_unused]] const float wp) {
    const float diff = p - q;
    const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
    const float filtered = __builtin_fmaf(q, v2, __builtin_fmaf(p + p, v1, v0));
    if constexpr (WEIGHTED) {
        const float g = __builtin_fmaf(kl, effective_weight(wp) * sgn, ks * filtered);
        return wp > 0.0f ? g : 0.0f;
    } else {
        return __builtin_fmaf(kl, sgn, ks * filtered);
    }
}

// Which unit of work does workgroup `block` of a 1-D launch take? The hardware deals workgroups to the 8 XCDs round-robin (XCD = block % 8) and
// neighbouring units re-read each other's 5-pixel halo: with the natural order the neighbours of a unit run on other XCDs, each with an L2 of its own,
// and every one of them fetches the shared lines from memory again (round-5 counters: the two kernels fetched 2.4x their algorithmic bytes). Here XCD
// x owns the contiguous run [x * per_xcd, (x + 1) * per_xcd) of units, so a unit's neighbours are its own XCD's neighbours in time and space. The grid
// is rounded up to a multiple of 8 (loss_grid); the spare workgroups get `false` and return at once.
__device__ __forceinline__ bool xcd_region_unit(const unsigned block, const unsigned total, unsigned& logical) {
    const unsigned per_xcd = (total + kXcds - 1u) / kXcds;
    logical = (block % kXcds) * per_xcd + block / kXcds;
    return logical < total;
}
inline dim3 loss_grid(const unsigned units) { return dim3((units + kXcds - 1u) / kXcds * kXcds); }

__device__ __forceinline__ float block_sum_256(float v, float* s_red) {   // sum over the 256-thread workgroup, valid in thread 255
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    v = wave_sum_to_lane63(v);
    if (lane == 63u) s_red[wv] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// The forward kernel's partial sums (one float2 per unit of its work) -> means and the scalar loss, in a fixed order (one 256-thread workgroup;
// s_red: 8 floats of LDS). WEIGHTED: `total_weight` = S (weight_total below, valid in every thread) takes the place of W H; S = 0 (nothing counts)
// is loss 0, L1 0, SSIM 1.
template <bool WEIGHTED>
__device__ __forceinline__ void reduce_loss_partials(const LossArgs& a, const unsigned n_partials, float* s_red, const float total_weight = 0.0f) {
    const float2* __restrict__ part = reinterpret_cast<const float2*>(a.partials);
    float l1 = 0.0f, ss = 0.0f;
    for (unsigned b = threadIdx.x; b < n_partials; b += 256u) { const float2 v = part[b]; l1 += v.x; ss += v.y; }
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

// S = the sum of the forward units' weight sums (a.wpartials, n_units = one channel plane's units), in a fixed order by one 256-thread workgroup;
// valid in every thread. s_red: 4 floats of LDS that no other block_sum_256 of the kernel uses. Whoever needs S calls THIS, so every call form
// sees the same bits.
__device__ __forceinline__ float weight_total(const LossArgs& a, const unsigned n_units, float* s_red) {
    float w = 0.0f;
    for (unsigned b = threadIdx.x; b < n_units; b += 256u) w += a.wpartials[b];
    return block_sum_256(w, s_red);
}

// What the head of either backward kernel does before it filters (s: 12 floats of LDS the kernel overwrites afterwards). n_reduce != 0: the forward
// launch in front left n_reduce partial sums; workgroup 0 turns them into a.sums and, WEIGHTED, every workgroup re-sums S (FGS_LOSS_WEIGHTED_RESUM).
// n_reduce == 0: a reduction launch has run and S is in a.total_weight. Returns n = 3 W H or 3 S. Workgroup-uniform: it holds barriers.
template <bool WEIGHTED>
__device__ __forceinline__ float backward_head(const LossArgs& a, const unsigned n_reduce, float* s) {
    if constexpr (WEIGHTED) {
        float total_weight;
        if (n_reduce != 0u) {
            total_weight = weight_total(a, n_reduce / 3u, s + 8);
            if (blockIdx.x == 0u) reduce_loss_partials<true>(a, n_reduce, s, total_weight);
            __syncthreads();                              // the scratch words are overwritten by the caller
        } else total_weight = a.total_weight[0];
        return 3.0f * total_weight;
    } else {
        if (n_reduce != 0u && blockIdx.x == 0u) {        // the forward kernel's partial sums (complete: it is the launch in front) -> a.sums, by ONE workgroup
            reduce_loss_partials<false>(a, n_reduce, s);
            __syncthreads();
        }
        return 3.0f * static_cast<float>(a.width) * static_cast<float>(a.height);
    }
}

#ifdef FGS_DEV_SWITCHES      // loss_exhibits.hip: the other formulation of either kernel, behind option 16 (g_loss_form)
size_t loss_exhibit_partials(int width, int height);                       // floats the exhibit forward kernel leaves in LossArgs::partials
hipError_t launch_loss_forward_exhibit(const LossArgs& a, const GaussWindow& gw, hipStream_t s);
hipError_t launch_loss_backward_exhibit(const LossArgs& a, const GaussWindow& gw, unsigned n_reduce, hipStream_t s);
#endif

}  // namespace fgs

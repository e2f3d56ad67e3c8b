// The Adam update (adam.cu:22-33) and the one way it is applied to a run of three streams parameter / exp_avg / exp_avg_sq: 16-byte pieces, and a
// scalar loop for what is left. Shared by K13 (adam.hip) and the fused forms of K12 (preprocess_backward.hip). Both units are built with
// -ffp-contract=off: sqrtf(m2) * bc2_sqrt_rcp + eps must not contract.
#pragma once
#include "fgs_kernels.h"
#include <fgs_wave.h>

namespace fgs {

__device__ __forceinline__ void adam_update(float& p, float& m, float& v, const float g, const AdamHyper& h) {   // adam.cu:22-33
    const float gsq = g * g;
    const float m1 = fmaf(h.beta1, m - g, g);
    const float m2 = fmaf(h.beta2, v - gsq, gsq);
    const float denom = sqrtf(m2) * h.bc2_sqrt_rcp + h.eps;
    p -= h.step_size * m1 / denom;
    m = m1;
    v = m2;
}

// One 16-byte piece of the three streams (non-temporal), in two halves so that a caller can have the loads of several pieces (and of its gradient) in flight
// before the first update: load() requests the 48 bytes, step() updates the four elements with gradient g and stores them.
struct AdamPiece {
    float4 p, m, v;
    __device__ __forceinline__ void load(const float* P, const float* M, const float* V) { p = load_float4_nt(P); m = load_float4_nt(M); v = load_float4_nt(V); }
    __device__ __forceinline__ void step(float* P, float* M, float* V, const float4 g, const AdamHyper& h) {
        adam_update(p.x, m.x, v.x, g.x, h); adam_update(p.y, m.y, v.y, g.y, h);
        adam_update(p.z, m.z, v.z, g.z, h); adam_update(p.w, m.w, v.w, g.w, h);
        store_float4_nt(P, p); store_float4_nt(M, m); store_float4_nt(V, v);
    }
};

// The elements e .. end - 1 of the three streams, one at a time (fewer than four floats at the end of a run, or a piece of tensors that are not
// 16-byte aligned); grad(e) is the gradient of element e.
template <class Index, class Grad>
__device__ __forceinline__ void adam_scalar_tail(float* P, float* M, float* V, Index e, const Index end, const AdamHyper& h, Grad grad) {
    for (; e < end; ++e) {
        float pp = P[e], mm = M[e], vv = V[e];
        adam_update(pp, mm, vv, grad(e), h);
        P[e] = pp; M[e] = mm; V[e] = vv;
    }
}

}  // namespace fgs

// K13, the optimizer: Adam for all parameter groups in one launch, the block flags that let it skip what the backward pass left zero, and the scan
// that rebuilds the quiet flags. Semantics: reference adam/src/adam.cu:10-34 (torch_bindings/adam.py:11-36). The fused K12+K13 forms are in
// preprocess_backward.hip; both share fgs_adam.h.
#include "fgs_adam.h"

namespace fgs {

// ---- K13: Adam for all parameter groups in one launch (adam.cu:10-34), float4-vectorised, U pieces per thread ----------
// The product runs one form: one 16-byte piece per thread, non-temporal, workgroups in reverse order. The forms it was measured against are the dev
// library's launch_adam_exhibit, in front of the launcher at the end of this file.

// NT: non-temporal access (the state is streamed once per step); only adam_kernel<.., false>, an exhibit, asks for ordinary loads and stores
template <bool NT> __device__ __forceinline__ float4 load4(const float* p) { return NT ? load_float4_nt(p) : *reinterpret_cast<const float4*>(p); }
template <bool NT> __device__ __forceinline__ void store4(float* p, const float4 v) {
    if (NT) store_float4_nt(p, v);
    else *reinterpret_cast<float4*>(p) = v;
}

// Does the optimizer have to READ the gradient of block b (64 Gaussians) of this tensor? Flagged 0: every element is a zero the backward pass wrote --
// skip the read (the kernel is HBM-bound; the index arithmetic is free).
__device__ __forceinline__ bool adam_block_gradient_needed(const AdamArgs& a, const AdamGroup& G, const uint32_t b) {
    if (a.live_blocks[b] != 0) return true;
    // Belt and braces: the promise rests on the caller's proof that nobody touched the gradients since the backward pass,
    // and a write that bypasses the framework's bookkeeping (`.grad.data.add_(...)`, a raw-pointer kernel) cannot be seen by
    // it. One SENTINEL float per flagged-0 block and tensor (the first element of the block: the same cached 4 bytes for every
    // float4 of the block) is read anyway; anything but +-0 there -- a whole-tensor edit such as hand-written weight decay,
    // NaN / Inf -- and the block's gradients are read after all.
    return !(G.grad[(size_t)b * 64u * G.row_len] == 0.0f);
}

// What to do with the elements first .. last (at most four consecutive floats of the [N, L] tensor)? They cover the rows first / L .. last / L, which lie in
// at most two consecutive blocks of 64 Gaussians.
//   kAdamRead : some block's gradient is needed -- the piece is read and stepped in full
//   kAdamZero : no block's gradient is needed -- the piece is stepped with g = 0 without reading it
//   kAdamSkip : as kAdamZero, and both blocks are QUIET (a.quiet_blocks: all moments of the block == 0.0f in every group of the launch). adam_update with
//               g = m = v = 0 leaves m = v = +0 and p -= step_size * 0 / eps = p for eps > 0 and a finite step size (the host hands no quiet flags
//               otherwise): the piece is neither loaded nor stored, and nothing is deferred -- memory is what the full piece would have left (+-0 aside)
// A piece that needs a block's gradient clears that block's quiet byte, with a store only if it read a 1 (steady state: no stores).
// Races between workgroups: skipping needs "gradient not needed", clearing needs "gradient needed", and within one tensor every piece of a block sees the
// same live flag and the same sentinel -- so no piece of a tensor skips a block that another piece of that tensor steps on a gradient. Tensors can differ
// only through their sentinels (one tensor edited behind the flags). A piece of an unedited tensor then reads the quiet byte as 1 or as the 0 another
// tensor's piece just stored: it skips, or it runs kAdamZero on moments that are still all zero (its elements are written by nobody else) -- the identity
// either way, bit for bit. A piece that runs across a block border writes +0 moments and the unchanged parameter into the quiet side: harmless, and the
// reason quiet is defined by == 0.0f and not by the bit pattern.
enum : int { kAdamSkip = 0, kAdamZero = 1, kAdamRead = 2 };
__device__ __forceinline__ int adam_piece_plan(const AdamArgs& a, const AdamGroup& G, const int64_t first, const int64_t last) {
    if (a.live_blocks == nullptr || G.row_len == 0u) return kAdamRead;
    const uint32_t r0 = static_cast<uint32_t>(first) / G.row_len, r1 = static_cast<uint32_t>(last) / G.row_len;
    const uint32_t b0 = r0 >> 6, b1 = r1 >> 6;
    const bool need0 = adam_block_gradient_needed(a, G, b0), need1 = b1 == b0 ? need0 : adam_block_gradient_needed(a, G, b1);
    if (a.quiet_blocks != nullptr) {
        const uint8_t q0 = a.quiet_blocks[b0], q1 = b1 == b0 ? q0 : a.quiet_blocks[b1];
        if (need0 && q0 != 0) a.quiet_blocks[b0] = 0;
        if (b1 != b0 && need1 && q1 != 0) a.quiet_blocks[b1] = 0;
        if (!need0 && !need1 && q0 != 0 && q1 != 0) return kAdamSkip;
    }
    return need0 || need1 ? kAdamRead : kAdamZero;
}

template <int U, bool NT>
__global__ void __launch_bounds__(256) adam_kernel(const AdamArgs a) {
    // a.reverse: workgroups walk the arenas from the end -- the gradient elements the backward pass wrote LAST are the ones most likely to
    // still sit in the 256 MB memory-side cache
    const uint32_t blk = a.reverse ? a.total_blocks - 1u - blockIdx.x : blockIdx.x;
    int gidx = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) if (j < a.n_groups && blk >= a.g[j].first_block) gidx = j;
    const AdamGroup& G = a.g[gidx];
    const int64_t block_base = (int64_t)(blk - G.first_block) * (256 * 4 * U);
    float4 g4[U];
    float4 p4[U], m4[U], v4[U];
    bool full[U], run[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {                       // all loads of the thread are issued before any arithmetic
        const int64_t base = block_base + ((int64_t)u * 256 + threadIdx.x) * 4;
        full[u] = base + 4 <= G.n;
        run[u] = false;
        if (full[u]) {
            const int plan = adam_piece_plan(a, G, base, base + 3);
            run[u] = plan != kAdamSkip;
            if (run[u]) {
                g4[u] = plan == kAdamRead ? load4<NT>(G.grad + base) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                p4[u] = load4<NT>(G.param + base); m4[u] = load4<NT>(G.exp_avg + base); v4[u] = load4<NT>(G.exp_avg_sq + base);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t base = block_base + ((int64_t)u * 256 + threadIdx.x) * 4;
        if (full[u]) {
            if (run[u]) {
                adam_update(p4[u].x, m4[u].x, v4[u].x, g4[u].x, G.h); adam_update(p4[u].y, m4[u].y, v4[u].y, g4[u].y, G.h);
                adam_update(p4[u].z, m4[u].z, v4[u].z, g4[u].z, G.h); adam_update(p4[u].w, m4[u].w, v4[u].w, g4[u].w, G.h);
                store4<NT>(G.param + base, p4[u]); store4<NT>(G.exp_avg + base, m4[u]); store4<NT>(G.exp_avg_sq + base, v4[u]);
            }
        } else if (base < G.n) {
            // the tensor's last (fewer than four) floats: the same plan, or a tensor of 4 k + 1 .. 3 floats would have its tail read and stepped whatever the flags say
            const int plan = adam_piece_plan(a, G, base, G.n - 1);
            if (plan != kAdamSkip)
                adam_scalar_tail(G.param, G.exp_avg, G.exp_avg_sq, base, G.n, G.h, [&](const int64_t e) { return plan == kAdamRead ? G.grad[e] : 0.0f; });
        }
    }
}

// ---- quiet scan: quiet_out[b] = "every moment of block b is zero", for a caller that cannot prove its flags current (once per invalidation, never per step) ----
// One workgroup of 256 per block of 64 Gaussians: per group the block's 64 L floats of exp_avg and of exp_avg_sq are contiguous and start on a multiple of
// 256 bytes behind the tensor's base -- 16-byte loads where the base is 16-byte aligned, scalar loads for the ragged block's tail and unaligned tensors.
__global__ void __launch_bounds__(256) adam_quiet_scan_kernel(const AdamQuietScanArgs a) {
    const uint32_t b = blockIdx.x;
    const uint32_t rows = min(64u, a.rows - b * 64u);
    bool zero = true;
    for (int k = 0; k < a.n_groups; ++k) {
        const size_t first = (size_t)b * 64u * a.row_len[k];
        const uint32_t len = rows * a.row_len[k];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const float* t = (w == 0 ? a.m[k] : a.v[k]) + first;
            const uint32_t vec = (reinterpret_cast<uintptr_t>(t) & 15u) == 0 ? len >> 2 : 0u;
            for (uint32_t i = threadIdx.x; i < vec; i += 256u) {
                const float4 x = load_float4_nt(t + 4u * i);
                zero = zero && x.x == 0.0f && x.y == 0.0f && x.z == 0.0f && x.w == 0.0f;
            }
            for (uint32_t e = 4u * vec + threadIdx.x; e < len; e += 256u) zero = zero && t[e] == 0.0f;
        }
    }
    const int all_zero = __syncthreads_and(zero ? 1 : 0);
    if (threadIdx.x == 0) a.quiet_out[b] = all_zero ? 1 : 0;
}

hipError_t launch_adam_quiet_scan(const AdamQuietScanArgs& a, hipStream_t s) {
    if (a.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(adam_quiet_scan_kernel, dim3((a.rows + 63u) / 64u), dim3(256), 0, s, a);
    return hipGetLastError();
}

// first_block of every group and total_blocks, for workgroups of 256 threads x u 16-byte pieces; returns total_blocks
static uint32_t assign_adam_blocks(AdamArgs& a, const int u) {
    uint32_t blocks = 0;
    for (int k = 0; k < a.n_groups; ++k) { a.g[k].first_block = blocks; blocks += static_cast<uint32_t>((a.g[k].n + 1024 * u - 1) / (1024 * u)); }
    return a.total_blocks = blocks;
}

#ifdef FGS_DEV_SWITCHES
// ---- the dev library's A/B exhibits of K13 (libfgs_hip_dev.so only; the product carries adam_kernel<1, true> and nothing else) ----
// g_adam_unroll = 1: 16-byte pieces per thread (fgs_debug_set_option(1, u)); measured on MI355X: 1, 2 and 4 are within 2 %
// g_adam_reverse = 1 (fgs_debug_set_option(8, 0|1) in the dev build): reversed workgroup order (measured 0.837 vs 0.855 ms at S2, tools/ab_adam_order.py)
// g_adam_nontemporal = 1 (fgs_debug_set_option(2, 0|1) in the dev build): non-temporal loads / stores (state is streamed once per step: +2.3 % measured)
// (round 6, measured and withdrawn: the updated PARAMETERS alone as ordinary stores, on the idea that the next forward pass reads them first -- K1 0.227 vs 0.201 ms,
// Adam 0.797 vs 0.782: dirty lines in eight L2s are the last thing the next kernel's reads want to meet, profiles/r06_ab_adam_param_nt.txt)
// false: the switches select the product's form and nothing was enqueued
static bool launch_adam_exhibit(const AdamArgs& a_in, hipStream_t s) {
    const int unroll_opt = g_adam_unroll, nontemporal = g_adam_nontemporal, reverse = g_adam_reverse;
    if (nontemporal && reverse) return false;
    AdamArgs a = a_in;
    a.reverse = reverse;
    const int u = nontemporal ? 1 : (unroll_opt == 2 || unroll_opt == 4 ? unroll_opt : 1);      // unroll applies to the plain-load kernels only
    const uint32_t blocks = assign_adam_blocks(a, u);
    if (blocks == 0) return true;
    if (nontemporal) hipLaunchKernelGGL((adam_kernel<1, true>), dim3(blocks), dim3(256), 0, s, a);
    else if (u == 1) hipLaunchKernelGGL((adam_kernel<1, false>), dim3(blocks), dim3(256), 0, s, a);
    else if (u == 2) hipLaunchKernelGGL((adam_kernel<2, false>), dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((adam_kernel<4, false>), dim3(blocks), dim3(256), 0, s, a);
    return true;
}
#endif

hipError_t launch_adam(const AdamArgs& a_in, hipStream_t s) {
#ifdef FGS_DEV_SWITCHES
    if (launch_adam_exhibit(a_in, s)) return hipGetLastError();
#endif
    AdamArgs a = a_in;
    a.reverse = 1;
    const uint32_t blocks = assign_adam_blocks(a, 1);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL((adam_kernel<1, true>), dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fgs

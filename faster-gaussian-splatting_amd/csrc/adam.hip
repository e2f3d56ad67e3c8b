// K13, the optimizer: Adam for all parameter groups in one launch, the block flags that let it skip what the backward pass left zero, and the scan
// that rebuilds the quiet flags. Semantics: reference adam/src/adam.cu:10-34 (torch_bindings/adam.py:11-36). The fused K12+K13 forms are in
// preprocess_backward.hip; both share fgs_adam.h.
#include "fgs_adam.h"

namespace fgs {

// ---- K13: Adam for all parameter groups in one launch (adam.cu:10-34), float4-vectorised, U pieces per thread ----------
// The product runs one form: a workgroup per SPAN of g_adam_span (= 1) chunks of 4096 floats, four 16-byte pieces per thread and chunk all in flight at
// once, non-temporal, workgroups and the chunks of a span in reverse order. The forms it was measured against are the dev library's launch_adam_exhibit, in front of the launcher at the
// end of this file, and the other span lengths (fgs_debug_set_option(15, C); C = 1 is a workgroup per chunk).

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
    // it. One SENTINEL float per flagged-0 block and tensor (the first element of the block) is read anyway; anything but +-0
    // there -- a whole-tensor edit such as hand-written weight decay, NaN / Inf -- and the block's gradients are read after all.
    return !(G.grad[(size_t)b * 64u * G.row_len] == 0.0f);
}

// What to do with block b (64 Gaussians) of this tensor?
//   kAdamRead : the block's gradient is needed -- its pieces are read and stepped in full
//   kAdamZero : the gradient is not needed -- its pieces are stepped with g = 0 without reading it
//   kAdamSkip : as kAdamZero, and the block is QUIET (a.quiet_blocks: all moments of the block == 0.0f in every group of the launch). adam_update with
//               g = m = v = 0 leaves m = v = +0 and p -= step_size * 0 / eps = p for eps > 0 and a finite step size (the host hands no quiet flags
//               otherwise): its pieces are neither loaded nor stored, and nothing is deferred -- memory is what the full pieces would have left (+-0 aside)
// A block whose gradient is needed has its quiet byte cleared, with a store only if a 1 was read (steady state: no stores).
// The plans are made ONCE per workgroup, in the kernel's prologue: one thread per block the span touches, into LDS. So every plan of a workgroup comes
// from flag values read before that workgroup clears anything (a thread clears only the byte it has just read, and no two threads of a workgroup take the
// same block). Races between workgroups: skipping needs "gradient not needed", clearing needs "gradient needed", and every span of one tensor that
// touches a block -- two spans share their border block -- sees the same live flag and the same sentinel: they plan alike, clear to the same value, and
// no span of a tensor skips a block that another span of that tensor steps on a gradient. Tensors can differ only through their sentinels (one tensor
// edited behind the flags). A span of an unedited tensor then reads the quiet byte as 1 or as the 0 another tensor's span just stored: it skips, or it
// runs kAdamZero on moments that are still all zero (its elements are written by nobody else) -- the identity either way, bit for bit.
enum : int { kAdamSkip = 0, kAdamZero = 1, kAdamRead = 2 };
__device__ __forceinline__ int adam_block_plan(const AdamArgs& a, const AdamGroup& G, const uint32_t b) {
    const bool need = adam_block_gradient_needed(a, G, b);
    if (a.quiet_blocks != nullptr) {
        const uint8_t q = a.quiet_blocks[b];
        if (need && q != 0) a.quiet_blocks[b] = 0;
        if (!need && q != 0) return kAdamSkip;
    }
    return need ? kAdamRead : kAdamZero;
}

// The plan of the elements first .. last (at most four consecutive floats of the [N, L] tensor), from the block plans of the span (plans[0] is block
// b_first). A block starts on a multiple of 64 L floats, hence of four, and so does every piece: neither a 16-byte piece nor a tensor's scalar tail can
// lie across a block border, and the two-block branch is never taken by any launch the host makes. It is kept as a defence, with the rule it had: read if
// either block is read, skip only if both are skipped, else step on zeros -- the larger of the two plans. Stepping on zeros across a
// border writes +0 moments and the unchanged parameter into the quiet side: harmless, and the reason quiet is defined by == 0.0f and not by the bit pattern.
__device__ __forceinline__ int adam_piece_plan(const uint8_t* plans, const uint32_t b_first, const uint32_t row_len, const int64_t first, const int64_t last) {
    const uint32_t b0 = ((static_cast<uint32_t>(first) / row_len) >> 6) - b_first, b1 = ((static_cast<uint32_t>(last) / row_len) >> 6) - b_first;
    const int p0 = plans[b0];
    return b1 == b0 ? p0 : max(p0, static_cast<int>(plans[b1]));
}

// A span of C chunks covers at most 16 C U blocks, whatever the row length L (floats_per_gaussian: any positive value): with L = 1 it starts on a block
// border and holds exactly that many; with L >= 2 a block is 128 floats or more and the span touches at most 8 C U + 2 <= 16 C U of them.
constexpr uint32_t kAdamMaxSpan = 32;
// The product's form: 4 pieces per thread, all requested before the first update -- a workgroup covers 4096 consecutive floats AT ONCE, not one 1024-float
// chunk after the other. Both quarter the workgroups (43 216 at S2); walking 4 chunks in turn (g_adam_span = 4 at one piece per thread) is the cheaper at
// S2 (0.128 against 0.144 ms per launch, the one-chunk kernel 0.195 .. 0.200) but costs 0.07 ms per launch wherever every span has work, this form 0.006
// (0.587 against 0.581), which is inside the spread of that figure. It takes 97 VGPRs, 4 waves per SIMD: profiles/adam_spans.txt, sections 2 and 3.
constexpr int kAdamPieces = 4;

// The registers of one chunk of a thread: U 16-byte pieces of the four streams and what to do with each (kAdamNotFull: not a whole piece of the tensor)
constexpr int kAdamNotFull = -1;
template <int U> struct AdamChunk { float4 g[U], p[U], m[U], v[U]; int plan[U]; };

template <int U, bool NT>
__global__ void __launch_bounds__(256) adam_kernel(const AdamArgs a) {
    __shared__ uint8_t plans[kAdamMaxSpan * 16 * U];
    // a.reverse: workgroups walk the arenas from the end, and each its span from the end -- the gradient elements the backward pass wrote LAST are the
    // ones most likely to still sit in the 256 MB memory-side cache
    const uint32_t blk = a.reverse ? a.total_blocks - 1u - blockIdx.x : blockIdx.x;
    int gidx = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) if (j < a.n_groups && blk >= a.g[j].first_block) gidx = j;
    const AdamGroup& G = a.g[gidx];
    constexpr int64_t kChunk = 256 * 4 * U;
    const int64_t span_first = (int64_t)(blk - G.first_block) * a.span * kChunk;
    const int64_t span_end = min(G.n, span_first + (int64_t)a.span * kChunk);
    const bool flagged = a.live_blocks != nullptr && G.row_len != 0u;     // the same for the whole workgroup; without flags every piece is read
    uint32_t b_first = 0;
    if (flagged) {
        b_first = (static_cast<uint32_t>(span_first) / G.row_len) >> 6;
        const uint32_t b_last = (static_cast<uint32_t>(span_end - 1) / G.row_len) >> 6;
        bool idle = true;
        for (uint32_t b = b_first + threadIdx.x; b <= b_last; b += 256u) {
            const int plan = adam_block_plan(a, G, b);
            plans[b - b_first] = static_cast<uint8_t>(plan);
            idle = idle && plan == kAdamSkip;
        }
        if (__syncthreads_and(idle ? 1 : 0)) return;       // nothing of the span is loaded or stored; the barrier also publishes the plans
    }
    // The chunks of the span, one after the other: request() issues the loads of a chunk, finish() updates and stores it. Requesting the next chunk BEFORE
    // this one is finished (two chunks' loads in flight, 16 registers more) was measured and bought nothing, and so did a walk that starts at a different chunk
    // in every workgroup: profiles/adam_spans.txt, section 2.
    const int chunks = static_cast<int>((span_end - span_first + kChunk - 1) / kChunk);
    const auto chunk_base = [&](const int c) { return span_first + (int64_t)(a.reverse ? chunks - 1 - c : c) * kChunk; };     // the c-th chunk of the walk
    const auto request = [&](const int64_t chunk, AdamChunk<U>& r) {
#pragma unroll
        for (int u = 0; u < U; ++u) {                       // all loads of the chunk are issued before any arithmetic
            const int64_t base = chunk + ((int64_t)u * 256 + threadIdx.x) * 4;
            r.plan[u] = kAdamNotFull;
            if (base + 4 <= G.n) {
                const int plan = flagged ? adam_piece_plan(plans, b_first, G.row_len, base, base + 3) : kAdamRead;
                r.plan[u] = plan;
                if (plan != kAdamSkip) {
                    r.g[u] = plan == kAdamRead ? load4<NT>(G.grad + base) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    r.p[u] = load4<NT>(G.param + base); r.m[u] = load4<NT>(G.exp_avg + base); r.v[u] = load4<NT>(G.exp_avg_sq + base);
                }
            }
        }
    };
    const auto finish = [&](const int64_t chunk, AdamChunk<U>& r) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t base = chunk + ((int64_t)u * 256 + threadIdx.x) * 4;
            if (r.plan[u] != kAdamNotFull) {
                if (r.plan[u] != kAdamSkip) {
                    adam_update(r.p[u].x, r.m[u].x, r.v[u].x, r.g[u].x, G.h); adam_update(r.p[u].y, r.m[u].y, r.v[u].y, r.g[u].y, G.h);
                    adam_update(r.p[u].z, r.m[u].z, r.v[u].z, r.g[u].z, G.h); adam_update(r.p[u].w, r.m[u].w, r.v[u].w, r.g[u].w, G.h);
                    store4<NT>(G.param + base, r.p[u]); store4<NT>(G.exp_avg + base, r.m[u]); store4<NT>(G.exp_avg_sq + base, r.v[u]);
                }
            } else if (base < G.n) {
                // the tensor's last (fewer than four) floats: the same plan, or a tensor of 4 k + 1 .. 3 floats would have its tail read and stepped whatever the flags say
                const int plan = flagged ? adam_piece_plan(plans, b_first, G.row_len, base, G.n - 1) : kAdamRead;
                if (plan != kAdamSkip)
                    adam_scalar_tail(G.param, G.exp_avg, G.exp_avg_sq, base, G.n, G.h, [&](const int64_t e) { return plan == kAdamRead ? G.grad[e] : 0.0f; });
            }
        }
    };
    AdamChunk<U> cur;
    int64_t chunk = chunk_base(0);
    request(chunk, cur);
    for (int c = 0; c < chunks; ++c) {
        finish(chunk, cur);
        if (c + 1 < chunks) request(chunk = chunk_base(c + 1), cur);
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

// span, first_block of every group and total_blocks, for workgroups of 256 threads that own a span of g_adam_span chunks of u 16-byte pieces per thread
// (the last span of a group is ragged); returns total_blocks. The one place that sizes the grid.
static uint32_t assign_adam_blocks(AdamArgs& a, const int u) {
    a.span = min(max(static_cast<uint32_t>(g_adam_span), 1u), kAdamMaxSpan);
    const int64_t span_floats = (int64_t)a.span * 1024 * u;
    uint32_t blocks = 0;
    for (int k = 0; k < a.n_groups; ++k) { a.g[k].first_block = blocks; blocks += static_cast<uint32_t>((a.g[k].n + span_floats - 1) / span_floats); }
    return a.total_blocks = blocks;
}

#ifdef FGS_DEV_SWITCHES
// ---- the dev library's A/B exhibits of K13 (libfgs_hip_dev.so only; the product carries adam_kernel<4, true> and nothing else) ----
// g_adam_unroll = 1: 16-byte pieces per thread (fgs_debug_set_option(1, u)); measured on MI355X: 1, 2 and 4 are within 2 %
// g_adam_reverse = 1 (fgs_debug_set_option(8, 0|1) in the dev build): reversed workgroup order (measured 0.837 vs 0.855 ms at S2, tools/ab_adam_order.py)
// g_adam_nontemporal = 1 (fgs_debug_set_option(2, 0|1) in the dev build): non-temporal loads / stores (state is streamed once per step: +2.3 % measured)
// (round 6, measured and withdrawn: the updated PARAMETERS alone as ordinary stores, on the idea that the next forward pass reads them first -- K1 0.227 vs 0.201 ms,
// Adam 0.797 vs 0.782: dirty lines in eight L2s are the last thing the next kernel's reads want to meet, profiles/r06_ab_adam_param_nt.txt)
// g_adam_span (fgs_debug_set_option(15, 1..32)) applies to every form, the product's included: profiles/adam_spans.txt
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
    const uint32_t blocks = assign_adam_blocks(a, kAdamPieces);
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL((adam_kernel<kAdamPieces, true>), dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace fgs

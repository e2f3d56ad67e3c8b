// K11's A/B exhibits: the four formulations of the blend backward pass that were built, measured and not adopted. libfgs_hip_dev.so only
// (-DFGS_DEV_SWITCHES; the Makefile lists this unit in DEVOBJ and not in OBJ): tools/ and the variant tests select them with
// fgs_debug_set_backward_variant(); the product library has one formulation, blend_backward_compact_kernel (variant 3, blend_backward.hip), and
// none of this file. History: docs/history.md.
//   variants 0 / 2   blend_backward_kernel<GLOBAL_GRAD>   systolic over all buckets and all 192 pixels (round 1)
//   variant 1        blend_backward_strip_kernel          lane = pixel, DPP reductions
//   variant 5        blend_backward_chained_kernel        the compact kernel's items chained through the lanes without draining (round 6)
//   variant 4        blend_backward_pixel_kernel          lane = pixel, reduction on the matrix cores (round 4)
// The kernels' comments stand as they were written beside the product kernel: "the kernel above" and "the systolic kernel above" in the comments of
// variants 5 and 4 are blend_backward_compact_kernel, and the file header of blend_backward.hip describes the pipeline that variants 0 / 2 introduce.
// The staging and planning passes in front of these kernels and the fold / dirty-mark kernels behind them are blend_backward.hip's
// (launch_stage_pixels, launch_blend_backward): no kernel is launched across translation units.
#ifdef FGS_DEV_SWITCHES   // the whole unit: compiled without the define (the product flavour of the simulation does, it takes every csrc/*.hip) it is empty
#include "fgs_kernels.h"
#include <fgs_wave.h>

#ifndef FGS_CKPT_NT
#define FGS_CKPT_NT 1      // as in blend_backward.hip: the checkpoints are read as non-temporal loads (variant 5); 0: A/B
#endif
namespace fgs {

// ---- variants 0 / 2: the systolic form over all buckets of a tile and all 192 pixels ------------------------------------------------------------
template <bool GLOBAL_GRAD>
__global__ void __launch_bounds__(kBackwardWavesPerBlock * kWave) blend_backward_kernel(const BlendBackwardArgs a) {
    const unsigned lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const unsigned bucket = blockIdx.x * kBackwardWavesPerBlock + wv;
    const unsigned n_buckets = a.bucket_offsets[a.n_tiles - 1];          // device-side count: no host sync for the grid size
    if (bucket >= n_buckets) return;                                       // wave-uniform (no block-level barrier below)
    const unsigned tile = a.bucket_tile[bucket];
    const uint2 range = a.ranges[tile];
    const unsigned tile_n = range.y - range.x;
    const unsigned first = tile == 0 ? 0u : a.bucket_offsets[tile - 1];
    const unsigned tb = bucket - first;
    if (tb * kBucket >= a.max_n_processed[tile]) return;                   // kb:295

    // ---- stage this bucket's 192 pixels in the wave's private LDS slice (kb:349-380): 36 B per pixel ----
    __shared__ float4 s_init[kBackwardWavesPerBlock][kTilePixels];   // C_final - T_final*bg - C_ckpt (rgb), T_ckpt: injected at lane 0
    // dL/dC rgb, T_final * -(dL/dC . bg): read by lane l at pixel i-l. GLOBAL_GRAD reads it from the tile-major staging record
    // (L1/L2-resident, shared by the tile's buckets) instead, which frees 3 KB of LDS per wave -> 32 instead of 21 waves per CU
    __shared__ float4 s_grad[kBackwardWavesPerBlock][GLOBAL_GRAD ? 1 : kTilePixels];
    // last contributor, padded by one wave width on both sides: slots outside the tile read 0, so `tp < last` is the only
    // per-step validity test (no range compare, no index clamp)
    __shared__ uint32_t s_last[kBackwardWavesPerBlock][kWave + kTilePixels + kWave];
    {
        const float4* __restrict__ pix = a.pixrec + (size_t)tile * kTilePixels * 2;
        const float4* __restrict__ ck = a.ckpt + (size_t)bucket * kTilePixels;
#pragma unroll
        for (int c = 0; c < kTilePixels / kWave; ++c) {
            const unsigned p = static_cast<unsigned>(c) * kWave + lane;
            const float4 g = pix[2 * p], cst = pix[2 * p + 1], k = ck[p];
            // A pixel that finished before this bucket never wrote its checkpoint (kf:436): that slot is uninitialised memory.
            // Such pixels are gated out of every update below, but the step body is branch-free (0 * NaN != 0), so they enter
            // the pipeline with a clean zero state instead of whatever the allocator left there.
            const bool live = __float_as_uint(cst.w) > tb * kBucket;
            s_init[wv][p] = live ? make_float4(cst.x - k.x, cst.y - k.y, cst.z - k.z, k.w) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // kb:371-374
            if (!GLOBAL_GRAD) s_grad[wv][p] = g;
            s_last[wv][kWave + p] = __float_as_uint(cst.w);
        }
        s_last[wv][lane] = 0u;
        s_last[wv][kWave + kTilePixels + lane] = 0u;
    }

    const unsigned tp = tb * kBucket + lane;
    const bool valid_prim = tp < tile_n;
    uint32_t prim = 0;
    float mx = 0.0f, my = 0.0f, ca = 0.0f, cb = 0.0f, cc = 0.0f, op = 0.0f;
    float col0 = 0.0f, col1 = 0.0f, col2 = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
    if (valid_prim) {
        prim = a.inst_prims[range.x + tp];
        const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
        const float4 r0 = r[0], r1 = r[1];
        const float raw2 = reinterpret_cast<const float*>(r + 2)[0];
        mx = r0.x; my = r0.y; ca = r0.z; cb = r0.w; cc = r1.x; op = r1.y;
        col0 = fmaxf(r1.z, 0.0f); col1 = fmaxf(r1.w, 0.0f); col2 = fmaxf(raw2, 0.0f);
        f0 = r1.z >= 0.0f ? 1.0f : 0.0f; f1 = r1.w >= 0.0f ? 1.0f : 0.0f; f2 = raw2 >= 0.0f ? 1.0f : 0.0f;   // kb:313-318
    }
    const float x0 = static_cast<float>((tile % a.grid_w) * kTileW) + 0.5f;
    const float y0 = static_cast<float>((tile / a.grid_w) * kTileH) + 0.5f;
    wave_lds_fence();

    float d_mx = 0.0f, d_my = 0.0f, d_ca = 0.0f, d_cb = 0.0f, d_cc = 0.0f, d_op = 0.0f, d_c0 = 0.0f, d_c1 = 0.0f, d_c2 = 0.0f;
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, sT = 0.0f;                      // the pixel state travelling through the lanes
    const bool lane0 = lane == 0;
    uint64_t ever = 0;                   // lanes whose Gaussian passed the alpha test at least once (scalar registers)

    // software-pipelined LDS reads: the values of step i+1 are requested while step i computes. Lanes beyond the bucket's
    // Gaussians carry opacity 0 and fall out at the alpha test, so `tp < last` is the only per-step validity test.
    float4 init_next = s_init[wv][0];
    const uint32_t* my_last = &s_last[wv][kWave - lane];   // slot of pixel (i - lane) at step i is my_last[i]
    uint32_t last_next = my_last[0];
    const float4* __restrict__ gpix = a.pixrec + (size_t)tile * kTilePixels * 2;
    float4 g_next = GLOBAL_GRAD ? gpix[2 * min(max(0 - static_cast<int>(lane), 0), kTilePixels - 1)] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // The step body is branch-free (contributions are gated by selects, not by `continue`) and unrolled (the compiler turns
    // `unroll 2` of the 255 constant-trip steps into 85-step straight-line blocks): the only loop-carried dependence is the
    // 4-value pixel state, so the scheduler overlaps step i+1's exponent / alpha with step i's gradient arithmetic. Measured
    // in-process on MI355X (tools/ab_backward.py, S2): unrolled 0.69 ms, rolled 0.73 ms, dL/dC in LDS 0.73 ms, strip variant 0.85 ms.
#pragma unroll 2
    for (int i = 0; i < kTilePixels + kWave - 1; ++i) {
        // shift the 4 mutable values one lane up (kb:383-393) and inject pixel i at lane 0 (kb:401-410)
        s0 = wave_shift_up1(s0); s1 = wave_shift_up1(s1); s2 = wave_shift_up1(s2); sT = wave_shift_up1(sT);
        const float4 init = init_next;
        const uint32_t last = last_next;
        const float4 g_cur = g_next;
        init_next = s_init[wv][i + 1 < kTilePixels ? i + 1 : kTilePixels - 1];   // wave-uniform address: LDS broadcast
        last_next = my_last[i + 1];
        const int idx = i - static_cast<int>(lane);                        // pixel handled by this lane in this step
        if (GLOBAL_GRAD) g_next = gpix[2 * min(max(idx + 1, 0), kTilePixels - 1)];   // prefetched one step ahead
        s0 = lane0 ? init.x : s0; s1 = lane0 ? init.y : s1; s2 = lane0 ? init.z : s2; sT = lane0 ? init.w : sT;
        const float dx = mx - (x0 + static_cast<float>(idx & (kTileW - 1)));
        const float dy = my - (y0 + static_cast<float>(idx >> 4));
        const float power = -0.5f * (ca * dx * dx + cc * dy * dy) - cb * dx * dy;
        const float gauss_raw = __expf(fminf(power, 0.0f));
        const float alpha_raw = op * gauss_raw;
        const bool contrib = tp < last && alpha_raw >= kMinAlphaThreshold;                     // kb:412,419-421
        const uint64_t contrib_mask = wave_ballot(contrib);
        if (contrib_mask == 0) continue;                                                       // wave-uniform: nothing to do this step
        ever |= contrib_mask;
        const float alpha = contrib ? alpha_raw : 0.0f, gauss = contrib ? gauss_raw : 0.0f;
        const float4 g = GLOBAL_GRAD ? g_cur : s_grad[wv][min(max(idx, 0), kTilePixels - 1)];
        const float T = sT;
        const float w = T * alpha;
        d_c0 += w * g.x * f0; d_c1 += w * g.y * f1; d_c2 += w * g.z * f2;                      // kb:426-427
        s0 -= w * col0; s1 -= w * col1; s2 -= w * col2;                                        // kb:429
        const float oma = 1.0f - alpha;
        const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
        const float dl_dalpha = (T * col0 - s0 * oma_rcp) * g.x + (T * col1 - s1 * oma_rcp) * g.y
                                + (T * col2 - s2 * oma_rcp) * g.z + g.w * oma_rcp;             // kb:434-436
        d_op += gauss * dl_dalpha;
        const float h = -alpha * dl_dalpha;
        const float hh = 0.5f * h;
        d_ca += hh * (dx * dx); d_cb += hh * (dx * dy); d_cc += hh * (dy * dy);                // kb:443-448
        d_mx += h * (ca * dx + cb * dy); d_my += h * (cb * dx + cc * dy);                      // kb:449-453
        sT = T * oma;
    }

    // A Gaussian that never passed the alpha test in this tile has nine zero sums: adding them is a no-op, and the kernel's
    // tail is bound by atomic throughput on contended lines (near-camera Gaussians cover thousands of tiles).
    const bool silent = ((ever >> lane) & 1ull) == 0;
    if (valid_prim && !silent) {                                           // kb:459-470
        float* const rec = a.acc + (size_t)prim * kAccRecordWords;         // the Gaussian's record of nine consecutive floats
        unsafeAtomicAdd(rec, d_mx);
        unsafeAtomicAdd(rec + 1, d_my);
        unsafeAtomicAdd(rec + 2, d_ca);
        unsafeAtomicAdd(rec + 3, d_cb);
        unsafeAtomicAdd(rec + 4, d_cc);
        unsafeAtomicAdd(rec + 5, a.proper_aa ? d_op : op * (1.0f - op) * d_op);
        unsafeAtomicAdd(rec + 6, d_c0);
        unsafeAtomicAdd(rec + 7, d_c1);
        unsafeAtomicAdd(rec + 8, d_c2);
    }
}

// ---- variant 2: pixel-per-lane ("strip") formulation ---------------------------------------------------------------
// One 192-thread workgroup per bucket; wave w owns the 16x4 strip w of the tile, lane = pixel (state in registers, like the
// forward pass). The bucket's 64 Gaussians are staged in LDS; each wave culls them against its strip with one ballot and
// walks the survivors in depth order. Per surviving Gaussian the 9 per-pixel partial gradients are summed across the wave
// with 6 DPP-fused adds each (wave_sum_to_lane63) and lane 63 stores them into the wave's LDS slice; at the end 64 lanes
// add the three slices and issue the 9 global atomics (kb:459-470). Compared with the systolic form it touches only
// (Gaussian, strip) pairs whose bounding boxes overlap -- about 1.4 of 3 strips per Gaussian -- instead of all 192 pixels.
__global__ void __launch_bounds__(kTilePixels) blend_backward_strip_kernel(const BlendBackwardArgs a) {
    const unsigned bucket = blockIdx.x;
    const unsigned n_buckets = a.bucket_offsets[a.n_tiles - 1];
    if (bucket >= n_buckets) return;                                       // workgroup-uniform
    const unsigned tile = a.bucket_tile[bucket];
    const uint2 range = a.ranges[tile];
    const unsigned tile_n = range.y - range.x;
    const unsigned first = tile == 0 ? 0u : a.bucket_offsets[tile - 1];
    const unsigned tb = bucket - first;
    if (tb * kBucket >= a.max_n_processed[tile]) return;                   // kb:295, workgroup-uniform

    __shared__ float4 s_a[kBucket];                  // mean.x mean.y conic.a conic.b
    __shared__ float4 s_b[kBucket];                  // conic.c opacity colour.r colour.g (clamped)
    __shared__ float4 s_c[kBucket];                  // colour.b (clamped), clamp mask bits, bounds x, bounds y
    __shared__ float s_acc[kTilePixels / kWave][kBucket][12];   // per-wave slice: 9 sums per Gaussian (padded to 48 B)
    __shared__ uint32_t s_prim[kBucket];

    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const unsigned n_here = min(static_cast<unsigned>(kBucket), tile_n - tb * kBucket);
    if (tid < kBucket) {
        float4 ga = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gb = ga, gc = ga;
        uint32_t prim = 0;
        if (tid < n_here) {
            prim = a.inst_prims[range.x + tb * kBucket + tid];
            const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            const unsigned fm = (r1.z >= 0.0f ? 1u : 0u) | (r1.w >= 0.0f ? 2u : 0u) | (r2.x >= 0.0f ? 4u : 0u);   // kb:313-318
            ga = r0;
            gb = make_float4(r1.x, r1.y, fmaxf(r1.z, 0.0f), fmaxf(r1.w, 0.0f));
            gc = make_float4(fmaxf(r2.x, 0.0f), __uint_as_float(fm), r2.y, r2.z);
        }
        s_a[tid] = ga; s_b[tid] = gb; s_c[tid] = gc; s_prim[tid] = prim;
    }
    for (unsigned e = tid; e < (kTilePixels / kWave) * kBucket * 12; e += kTilePixels) (&s_acc[0][0][0])[e] = 0.0f;

    // this lane's pixel (same mapping as the forward pass) and its per-pixel constants / checkpointed state
    const unsigned tile_x = tile % a.grid_w, tile_y = tile / a.grid_w;
    const unsigned lx = (lane >> 5) * kSubtileW + (lane & 7u), ly = wave * kSubtileH + ((lane >> 3) & 3u);
    const unsigned local = ly * kTileW + lx;
    const float pxf = static_cast<float>(tile_x * kTileW + lx) + 0.5f, pyf = static_cast<float>(tile_y * kTileH + ly) + 0.5f;
    const float4 g = a.pixrec[((size_t)tile * kTilePixels + local) * 2];
    const float4 cst = a.pixrec[((size_t)tile * kTilePixels + local) * 2 + 1];
    const float4 ck = a.ckpt[(size_t)bucket * kTilePixels + local];
    float s0 = cst.x - ck.x, s1 = cst.y - ck.y, s2 = cst.z - ck.z, sT = ck.w;                  // kb:371-374
    const unsigned last = __float_as_uint(cst.w);                                               // 0 outside the image
    const unsigned strip_y0 = tile_y * kTileH + wave * kSubtileH, strip_y1 = strip_y0 + kSubtileH;
    const unsigned strip_x0 = tile_x * kTileW, strip_x1 = strip_x0 + kTileW;
    __syncthreads();

    bool overlaps = false;
    if (lane < n_here) {
        const uint32_t bx = __float_as_uint(s_c[lane].z), by = __float_as_uint(s_c[lane].w);
        overlaps = (bx & 0xffffu) < strip_x1 && strip_x0 < (bx >> 16) && (by & 0xffffu) < strip_y1 && strip_y0 < (by >> 16);
    }
    uint64_t pending = wave_ballot(overlaps);
    // Gaussians at or beyond every pixel's last contributor cannot contribute (kb:412): trim with the wave maximum
    const unsigned wave_last = wave_max(last);
    while (pending != 0) {                                                 // wave-uniform, depth order
        const int j = __ffsll(static_cast<unsigned long long>(pending)) - 1;
        pending &= pending - 1;
        const unsigned tp = tb * kBucket + static_cast<unsigned>(j);
        if (tp >= wave_last) break;
        const float4 ga = s_a[j], gb = s_b[j], gc = s_c[j];
        const float dx = ga.x - pxf, dy = ga.y - pyf;
        const float power = -0.5f * (ga.z * dx * dx + gb.x * dy * dy) - ga.w * dx * dy;
        const float gauss = __expf(fminf(power, 0.0f));
        const float alpha = gb.y * gauss;
        const bool contrib = tp < last && alpha >= kMinAlphaThreshold;
        if (wave_ballot(contrib) == 0) continue;
        float p_c0 = 0.0f, p_c1 = 0.0f, p_c2 = 0.0f, p_op = 0.0f, p_ca = 0.0f, p_cb = 0.0f, p_cc = 0.0f, p_mx = 0.0f, p_my = 0.0f;
        if (contrib) {
            const unsigned fm = __float_as_uint(gc.y);
            const float T = sT, w = T * alpha;
            p_c0 = (fm & 1u) ? w * g.x : 0.0f; p_c1 = (fm & 2u) ? w * g.y : 0.0f; p_c2 = (fm & 4u) ? w * g.z : 0.0f;   // kb:426-427
            s0 -= w * gb.z; s1 -= w * gb.w; s2 -= w * gc.x;                                                            // kb:429
            const float oma = 1.0f - alpha;
            const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
            const float dl_dalpha = (T * gb.z - s0 * oma_rcp) * g.x + (T * gb.w - s1 * oma_rcp) * g.y
                                    + (T * gc.x - s2 * oma_rcp) * g.z + g.w * oma_rcp;                                 // kb:434-436
            p_op = gauss * dl_dalpha;
            const float h = -alpha * dl_dalpha, hh = 0.5f * h;
            p_ca = hh * (dx * dx); p_cb = hh * (dx * dy); p_cc = hh * (dy * dy);                                      // kb:443-448
            p_mx = h * (ga.z * dx + ga.w * dy); p_my = h * (ga.w * dx + gb.x * dy);                                   // kb:449-453
            sT = T * oma;
        }
        p_mx = wave_sum_to_lane63(p_mx); p_my = wave_sum_to_lane63(p_my);
        p_ca = wave_sum_to_lane63(p_ca); p_cb = wave_sum_to_lane63(p_cb); p_cc = wave_sum_to_lane63(p_cc);
        p_op = wave_sum_to_lane63(p_op);
        p_c0 = wave_sum_to_lane63(p_c0); p_c1 = wave_sum_to_lane63(p_c1); p_c2 = wave_sum_to_lane63(p_c2);
        if (lane == 63u) {
            float4* dst = reinterpret_cast<float4*>(&s_acc[wave][j][0]);
            dst[0] = make_float4(p_mx, p_my, p_ca, p_cb);
            dst[1] = make_float4(p_cc, p_op, p_c0, p_c1);
            s_acc[wave][j][8] = p_c2;
        }
    }
    __syncthreads();

    if (tid < n_here) {                                                    // kb:459-470
        float t[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) t[k] = s_acc[0][tid][k] + s_acc[1][tid][k] + s_acc[2][tid][k];
        const uint32_t prim = s_prim[tid];
        const float op = s_b[tid].y;
        float* const rec = a.acc + (size_t)prim * kAccRecordWords;         // the Gaussian's record of nine consecutive floats
        unsafeAtomicAdd(rec, t[0]);
        unsafeAtomicAdd(rec + 1, t[1]);
        unsafeAtomicAdd(rec + 2, t[2]);
        unsafeAtomicAdd(rec + 3, t[3]);
        unsafeAtomicAdd(rec + 4, t[4]);
        unsafeAtomicAdd(rec + 5, a.proper_aa ? t[5] : op * (1.0f - op) * t[5]);
        unsafeAtomicAdd(rec + 6, t[6]);
        unsafeAtomicAdd(rec + 7, t[7]);
        unsafeAtomicAdd(rec + 8, t[8]);
    }
}

// ---- K11, chained (round 6): the items of a wave follow each other through the lanes without draining ------------------------------------------
// The kernel above runs one item -- (tile, 64-Gaussian bucket) -- at a time: n_px live pixels stream through the 64 lanes in n_px + 63 steps, and
// 63 of the ~240 steps are fill / drain (27 %; removing the drain alone measured -18 % at S2 and -22 % on the layered scene,
// profiles/r06_k11_chain_ceiling.txt). Here a wave owns a CHAIN of items of the live list (every G-th, G = waves launched) and their pixels form ONE stream of positions:
// item i occupies positions [S_i, S_i + n_i), followed by sentinel positions (rel = 0: never contribute) up to S_{i+1} = S_i + L_i with
// L_i = max(round_up_8(n_i + 8), 64). Lane l handles position s - l at step s, so while the tail of item i still travels through the upper lanes the
// lower lanes already work on item i + 1. A lane changes Gaussians when the boundary passes it -- in GROUPS of eight lanes: the >= 8 sentinels in
// front of every boundary mean that at step S_{i+1} + 8 g - 1 all eight lanes of group g look at sentinels, so the group flushes its nine sums of
// item i (72 floats through LDS, two atomic instructions) and takes the parameters of item i + 1 from a shadow register set between two steps;
// L_i >= 64 keeps the eight group switches of one boundary apart from those of the next. Cost per item: n_i + 8..15 steps + eight switches of
// ~60 instructions + the wave's single fill / drain spread over its chain, against n_i + 63.
// LDS must not grow (12.5 KB per wave instead of 7.7 costs this kernel 10 %, same file), so the rings keep their 256 slots = the 64 positions in
// flight + at most 192 staged ahead: the stream is staged in UNITS of one 64-pixel third of an item (its raw records prefetched into registers a
// unit ahead) whenever fewer than 16 positions lie in front of lane 0, into the slots the tail has left.
// MEASURED (profiles/r06_ab_k11_chained.txt, r06_k11_variants_pmc.txt): correct on the simulator and on the MI355X (all parity suites), and never faster than
// the kernel above. A first version defined its prefetch registers inside the loop that runs the steps: the register allocator copies such registers at
// the loop's back edge and the copy waits for ALL outstanding loads (`s_waitcnt vmcnt(0)` in front of every block of eight steps): S2 0.354 vs 0.310 ms,
// layered scene 1.74 vs 1.47. This version issues every load at the outer level of a loop nest (104 registers, no wait left in the step loop): it executes
// 13 % fewer vector instructions than the kernel above and still takes 0.344 / 1.66 ms with 4096 waves -- on average 12 waves per CU are resident instead
// of 19 (16 fit; static chains end at different times), the bookkeeping per block of eight steps adds 60 % scalar instructions, the group switches their
// share. With 16 384 waves (shorter chains) it reaches the kernel above on the layered scene (1.46 ms) and stays behind it at S2 (0.342 vs 0.317).
// Kept as an exhibit of the dev library (variant 5) with its tests; the product's K11 stays the kernel above.
// Which items: wave w chains the items w, w + G, w + 2 G, ... of the live list, G = waves launched = g_k11_chain_waves (fgs_kernels.h: 4096 = 16 resident
// waves x 256 CUs at 110 registers and 8.5 KB of LDS per wave, so every wave of the launch runs from the first cycle): no queue, no atomics, +-1 item of
// imbalance. A first version gave each wave 8 CONSECUTIVE items: 2 770 waves at S2, two thirds of the chip, 0.46 ms instead of 0.32
// (profiles/r06_ab_k11_chained.txt).
constexpr unsigned kChDesc = 32;                            // descriptor window: lane q mod 32 holds item q of the wave's chain, refilled 16 at a time
constexpr unsigned kChRing = 256, kChXyBytes = kChRing * 8u, kChInjBase = kChXyBytes, kChPixBase = 2u * kChXyBytes, kChFlushBase = kChPixBase + kChRing * 16u;
constexpr unsigned kChOffBase = kChFlushBase + 8u * kAccRecordWords * 4u, kChZeroBase = kChOffBase + 8u * 4u, kChBytes = kChZeroBase + 16u;
#ifndef FGS_K11_CHAIN_WAVES_PER_SIMD
#define FGS_K11_CHAIN_WAVES_PER_SIMD 4      // register budget 128: without the cap the compiler takes 143 (3 waves per SIMD, 12 per CU: K11 loses 10 % there)
#endif
__global__ void __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(FGS_K11_CHAIN_WAVES_PER_SIMD, FGS_K11_CHAIN_WAVES_PER_SIMD)))
blend_backward_chained_kernel(const BlendBackwardArgs a) {
    __shared__ __attribute__((aligned(16))) char s_base[kChBytes];
    const unsigned lane = lane_id();
    const float lane_f = static_cast<float>(lane);
    const unsigned n_live = *a.live_count;
    const unsigned first_item = blockIdx.x, stride = gridDim.x;
    if (first_item >= n_live) return;                                                     // wave-uniform
    const unsigned n_items = wave_uniform((n_live - first_item + stride - 1u) / stride);  // this wave's chain: items first_item + q * stride, q < n_items
    float2* const s_xy = reinterpret_cast<float2*>(s_base);
    float2* const s_inj = reinterpret_cast<float2*>(s_base + kChInjBase);
    float4* const s_pix = reinterpret_cast<float4*>(s_base + kChPixBase);
    float* const s_flush = reinterpret_cast<float*>(s_base + kChFlushBase);
    uint32_t* const s_off = reinterpret_cast<uint32_t*>(s_base + kChOffBase);
    if (lane == 0) *reinterpret_cast<float2*>(s_base + kChZeroBase) = make_float2(0.0f, 0.0f);
    // positions -64 .. -1 (what the lanes above lane 0 look at until the stream reaches them): sentinels
    s_pix[kChRing - kWave + lane] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s_xy[kChRing - kWave + lane] = make_float2(0.0f, 0.0f);

    // ---- descriptors: lane j holds item j (tile, bucket in tile, list start, list length, checkpoint row) and, later, its first position ----
    unsigned d_tile = 0, d_tb = 0, d_rx = 0, d_n = 0, d_bucket = 0, d_start = 0;
    auto load_descriptors = [&](const unsigned q0) {                                       // items q0 .. q0 + 15 of the chain (q0 a multiple of 16) -> lanes (q0 & 31) ..
        const unsigned base = q0 & (kChDesc - 1u), q = q0 + (lane - base);
        if (lane >= base && lane < base + 16u && q < n_items) {
            const uint2 work = a.work_list[first_item + q * stride];
            d_tile = work.x; d_tb = work.y;
            const uint2 range = a.ranges[d_tile];
            d_rx = range.x; d_n = range.y - range.x;
            d_bucket = (d_tile == 0 ? 0u : a.bucket_offsets[d_tile - 1]) + d_tb;
        }
    };
    load_descriptors(0u);
    load_descriptors(16u);
    auto slot_of = [&](const unsigned q) { return static_cast<int>(wave_uniform(q & (kChDesc - 1u))); };

    // ---- the lane's Gaussian: ACTIVE set (what the steps use) and SHADOW set (the next item's, requested early) ----
    uint32_t prim = 0, hot_word = 0, rep_tile = 0;
    bool have = false;
    float mx = 0.0f, my = 0.0f, ca = 0.0f, cb = 0.0f, cc = 0.0f, op = 0.0f;           // op = 0: alpha = 0, nothing passes the test (no item yet / after the last)
    float col0 = 0.0f, col1 = 0.0f, col2 = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
    // The SHADOW set: the next item's Gaussian, eleven registers per lane. All loads of this kernel are issued at the OUTER level of the loop nest below:
    // a register that a load defines inside the loop that also runs the steps is copied at that loop's back edge, and the copy makes the compiler
    // wait for every outstanding load in front of every block of steps (the first version of this kernel: profiles/r06_ab_k11_chained.txt).
    struct Shadow { uint32_t prim, tile, hot; bool valid; float mx, my, ca, cb, cc, op, c0, c1, c2; };
    Shadow sh{0u, 0u, 0u, false, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t pf_prim = 0;
    bool pf_valid = false;
    auto prefetch_prim = [&](const unsigned j) {                                         // the primitive index of item j's Gaussian for this lane
        pf_valid = false; pf_prim = 0;
        if (j < n_items) {
            const int jj = slot_of(j);
            const unsigned tp = wave_read(d_tb, jj) * kBucket + lane, list_n = wave_read(d_n, jj), list_first = wave_read(d_rx, jj);   // (convergent: all lanes)
            pf_valid = tp < list_n;
            if (pf_valid) pf_prim = a.inst_prims[list_first + tp];
        }
    };
    auto load_shadow = [&](const unsigned j) {                                           // item j's record (j == n_items: the empty item behind the last)
        sh.valid = pf_valid; sh.prim = pf_prim;
        sh.tile = j < n_items ? wave_read(d_tile, slot_of(j)) : 0u;
        float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
        if (sh.valid) { const float4* r = reinterpret_cast<const float4*>(a.rec + sh.prim); r0 = r[0]; r1 = r[1]; r2 = r[2]; }
        sh.mx = r0.x; sh.my = r0.y; sh.ca = r0.z; sh.cb = r0.w; sh.cc = r1.x; sh.op = r1.y; sh.c0 = r1.z; sh.c1 = r1.w; sh.c2 = r2.x;
        unsigned tx0, tx1, ty0, ty1;
        tile_rect(__float_as_uint(r2.y), __float_as_uint(r2.z), tx0, tx1, ty0, ty1);
        sh.hot = (sh.valid && (tx1 - tx0) * (ty1 - ty0) > kHotFootprint) ? __float_as_uint(r2.w) : 0u;
        prefetch_prim(j + 1u);
    };

    float a_c0 = 0.0f, a_c1 = 0.0f, a_c2 = 0.0f, a_h = 0.0f, a_x = 0.0f, a_y = 0.0f, a_xx = 0.0f, a_xy = 0.0f, a_yy = 0.0f;
    float sT = 0.0f, sS = 0.0f;

    // group g (lanes 8 g .. 8 g + 7) leaves its current item (its nine sums go out, kb:459-470) and takes the shadow set
    constexpr uint32_t kNoRecord = 0xffffffffu;
    auto switch_group = [&](const unsigned g, const bool flush) {
        const bool mine = (lane >> 3) == g;
        if (flush) {
            const bool silent = a_h == 0.0f && a_c0 == 0.0f && a_c1 == 0.0f && a_c2 == 0.0f && a_x == 0.0f && a_y == 0.0f
                                && a_xx == 0.0f && a_xy == 0.0f && a_yy == 0.0f;
            const float v5 = a.proper_aa ? -2.0f * a_h / op : -2.0f * a_h * (1.0f - op);
            const float v0 = 2.0f * (ca * a_x + cb * a_y), v1 = 2.0f * (cb * a_x + cc * a_y);
            const uint32_t rec_off = hot_word != 0u ? static_cast<uint32_t>(a.acc_hot - a.acc) + ((rep_tile % kHotReplicas) * kMaxHot + (hot_word - 1u)) * kAccRecordWords
                                                    : prim * kAccRecordWords;
            if (mine) {
                float* const out = s_flush + (lane & 7u) * kAccRecordWords;
                out[0] = v0; out[1] = v1; out[2] = a_xx; out[3] = a_xy; out[4] = a_yy; out[5] = v5;
                out[6] = a_c0 * f0; out[7] = a_c1 * f1; out[8] = a_c2 * f2;
                s_off[lane & 7u] = (have && !silent) ? rec_off : kNoRecord;
            }
            wave_lds_fence();
            if (lane < 63u) {                                                              // seven records of nine words
                const uint32_t rec = s_off[lane / kAccRecordWords];
                if (rec != kNoRecord) unsafeAtomicAdd(a.acc + (size_t)rec + (lane % kAccRecordWords), s_flush[lane]);
            }
            if (lane < kAccRecordWords) {                                                  // the eighth
                const uint32_t rec = s_off[7];
                if (rec != kNoRecord) unsafeAtomicAdd(a.acc + (size_t)rec + lane, s_flush[63u + lane]);
            }
            wave_lds_fence();
        }
        if (mine) {
            prim = sh.prim; have = sh.valid; rep_tile = sh.tile; hot_word = sh.hot;
            mx = sh.mx; my = sh.my; ca = sh.ca; cb = sh.cb; cc = sh.cc; op = sh.op;
            col0 = fmaxf(sh.c0, 0.0f); col1 = fmaxf(sh.c1, 0.0f); col2 = fmaxf(sh.c2, 0.0f);
            f0 = sh.c0 >= 0.0f ? 1.0f : 0.0f; f1 = sh.c1 >= 0.0f ? 1.0f : 0.0f; f2 = sh.c2 >= 0.0f ? 1.0f : 0.0f;   // kb:313-318
            a_c0 = a_c1 = a_c2 = a_h = a_x = a_y = a_xx = a_xy = a_yy = 0.0f;
        }
    };

    // ---- staging cursor: the next UNIT = third `st_chunk` of item `st_item`, its raw records in (rg, rc, rk) ----
    unsigned st_item = 0, st_chunk = 0, st_pos = 0, st_n = 0;       // uniform; st_pos = first position not staged yet, st_n = live pixels of the item so far
    bool st_done = false;
    float4 rg = make_float4(0.0f, 0.0f, 0.0f, 0.0f), rc = rg, rk = rg;
    auto fetch_unit = [&]() {                                                             // requests the cursor's unit (nothing waits for it here)
        if (st_item >= n_items) return;
        const unsigned tile = wave_read(d_tile, slot_of(st_item)), bucket = wave_read(d_bucket, slot_of(st_item));
        const unsigned p = st_chunk * kWave + lane;
        const float4* __restrict__ pix = a.pixrec + (size_t)tile * kTilePixels * 2;
        rg = pix[2 * p]; rc = pix[2 * p + 1];
#if FGS_CKPT_NT
        rk = load_float4_nt(reinterpret_cast<const float*>(a.ckpt + (size_t)bucket * kTilePixels + p));
#else
        rk = a.ckpt[(size_t)bucket * kTilePixels + p];
#endif
    };
    auto put_sentinels = [&](const unsigned count) {                                      // `count` <= 64 positions from st_pos on that never contribute
        if (lane < count) {
            const unsigned slot = (st_pos + lane) & (kChRing - 1u);
            s_pix[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); s_xy[slot] = make_float2(0.0f, 0.0f); s_inj[slot] = make_float2(0.0f, 0.0f);
        }
        st_pos += count;
    };
    auto stage_unit = [&]() {
        if (st_item >= n_items) { put_sentinels(kWave); st_done = true; return; }         // behind the last item: what the lanes see while it drains
        const unsigned tile = wave_read(d_tile, slot_of(st_item)), first_gaussian = wave_read(d_tb, slot_of(st_item)) * kBucket;
        const float x0 = static_cast<float>((tile % a.grid_w) * kTileW) + 0.5f, y0 = static_cast<float>((tile / a.grid_w) * kTileH) + 0.5f;
        const unsigned p = st_chunk * kWave + lane;
        const unsigned last = __float_as_uint(rc.w);
        const bool live = last > first_gaussian;                                           // kb:349-380, as in the kernel above
        const uint64_t m = wave_ballot(live);
        if (live) {
            const unsigned slot = (st_pos + lanes_below(m)) & (kChRing - 1u);
            const unsigned rel = min(last - first_gaussian, static_cast<unsigned>(kBucket));
            s_pix[slot] = make_float4(rg.x, rg.y, rg.z, static_cast<float>(rel));
            s_xy[slot] = make_float2(x0 + static_cast<float>(p & (kTileW - 1)), y0 + static_cast<float>(p / kTileW));
            const float S = (rc.x - rk.x) * rg.x + (rc.y - rk.y) * rg.y + (rc.z - rk.z) * rg.z;                           // kb:371-374
            s_inj[slot] = make_float2(rk.w, S - rg.w);
        }
        const unsigned added = static_cast<unsigned>(__popcll(m));
        st_pos += added; st_n += added;
        if (++st_chunk == kTilePixels / kWave) {                                           // the item is complete: pad it, the next one starts behind the pads
            const unsigned padded = (st_n + 8u + 7u) & ~7u;
            const unsigned length = padded < static_cast<unsigned>(kWave) ? static_cast<unsigned>(kWave) : padded;
            put_sentinels(length - st_n);                                                  // 8 .. 63 of them
            ++st_item; st_chunk = 0; st_n = 0;
            if (lane == (st_item & (kChDesc - 1u))) d_start = st_pos;                      // (item n_items: where the stream ends)
        }
        fetch_unit();
    };

    // ---- the pipeline ----
    unsigned ring_at = ((0u - lane) & (kChRing - 1u)) * 8u;                                // byte offset of position (step - lane) in the 8-byte rings
    const unsigned inj_mul = lane == 0 ? 1u : 0u, inj_add = lane == 0 ? kChInjBase : kChZeroBase;   // lane 0 injects the position's state, the others add zero
    struct PixRead { float4 g; float2 xy; };
    auto read_inj = [&]() { return *reinterpret_cast<const float2*>(s_base + (ring_at * inj_mul + inj_add)); };
    auto read_pix = [&]() {
        PixRead r;
        r.xy = *reinterpret_cast<const float2*>(s_base + ring_at);
        r.g = *reinterpret_cast<const float4*>(s_base + (2u * ring_at + kChPixBase));
        ring_at = (ring_at + 8u) & (kChXyBytes - 1u);
        return r;
    };
    auto step = [&](const float2 inj, const PixRead pr) {                                 // exactly the step of the kernel above
        sT = wave_shift_up1_zero(sT) + inj.x;                                               // kb:383-410
        sS = wave_shift_up1_zero(sS) + inj.y;
        const float4 px = pr.g;
        const float rel = px.w;
        const float dx = mx - pr.xy.x, dy = my - pr.xy.y;
        const float power = -0.5f * (ca * dx * dx + cc * dy * dy) - cb * dx * dy;
        const float alpha = op * __expf(fminf(power, 0.0f));
        if (lane_f < rel && alpha >= kMinAlphaThreshold) {                                  // kb:412,419-421
            const float T = sT;
            const float w = T * alpha;
            a_c0 += w * px.x; a_c1 += w * px.y; a_c2 += w * px.z;
            const float cg = col0 * px.x + col1 * px.y + col2 * px.z;
            sS -= w * cg;                                                                    // kb:429 projected on dL/dC
            const float oma = 1.0f - alpha;
            const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
            const float dl_dalpha = T * cg - sS * oma_rcp;                                   // kb:434-436
            const float hh = (-0.5f * alpha) * dl_dalpha;
            const float t = hh * dx, u = hh * dy;
            a_h += hh; a_x += t; a_y += u;
            a_xx += t * dx; a_xy += t * dy; a_yy += u * dy;
            sT = T * oma;
        }
    };

    prefetch_prim(0u);
    fetch_unit();
    unsigned next_shadow = 0;                                                              // items < next_shadow have their records in a shadow set
    unsigned sw_item = 0, sw_g = 0;                                                        // the next group switch: group sw_g enters item sw_item
    unsigned s0 = 0;                                                                       // the next step (a multiple of 8)
    unsigned desc_due = 0;                                                                 // first item of the half window to refill (0: none)
    float2 inj_a, inj_b;
    PixRead pix_a, pix_b;
    bool primed = false;
    for (;;) {                                                                             // OUTER level: everything that loads
        while (!st_done && st_pos < s0 + 16u) stage_unit();                                // lane 0 never runs into positions that are not there yet
        wave_lds_fence();
        // the shadow set is free once every group has entered the item it holds: it then takes the next one, a whole item's length before its first use
        if (desc_due != 0u) { load_descriptors(desc_due); desc_due = 0u; }
        if (next_shadow <= n_items && next_shadow <= sw_item) { load_shadow(next_shadow); ++next_shadow; }
        if (!primed) { inj_a = read_inj(); pix_a = read_pix(); primed = true; }            // the reads of step 0
        bool finished = false;
        for (;;) {                                                                         // INNER level: group switches and steps, no load is issued here
            if (sw_item <= st_item) {                                                      // (d_start of item j is written when item j - 1 completes; item 0: 0)
                const unsigned start = wave_read(d_start, slot_of(sw_item));
                if (s0 == start + 8u * sw_g) {
                    if (sw_item >= next_shadow) break;                                     // its record is not requested yet: outer level
                    switch_group(sw_g, sw_item > 0u);
                    if (++sw_g == 8u) {
                        sw_g = 0; ++sw_item;
                        // every group has entered item sw_item - 1, so item sw_item - 2 is staged to its end (an item's start is known only then) and
                        // flushed: nothing refers to the descriptors of items <= sw_item - 2 any more, while staging may still be busy with the tail of
                        // item sw_item - 1 and runs at most three items ahead (256 ring slots, items of >= 64 positions). One item into the other half
                        // of the window, the half the chain has left takes the sixteen items after the next sixteen
                        if (sw_item > n_items) { finished = true; break; }                  // every group has left the last item
                        if ((sw_item & 15u) == 1u && sw_item > 1u) { desc_due = sw_item + 15u; break; }      // (a load: outer level)
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {                                                  // eight steps, the reads of a step issued one step ahead
                inj_b = read_inj(); pix_b = read_pix();
                step(inj_a, pix_a);
                inj_a = read_inj(); pix_a = read_pix();
                step(inj_b, pix_b);
            }
            s0 += 8u;
            if (!st_done && st_pos < s0 + 16u) break;                                      // the stream runs low: outer level
            if (next_shadow <= n_items && next_shadow <= sw_item) break;                   // the shadow set fell free: outer level
        }
        if (finished) break;
    }
}

// ---- variant 4: lane = PIXEL, reduction over the pixels on the matrix cores ----------------------------------------------------------------
// Measured in round 4 (tools/pair_stats.sh, profiles/r04_k11_pair_efficiency.txt): of the (pixel, Gaussian) lane-steps the systolic kernel above
// issues, 33-41 % pass the alpha test (S2, the layered scene, a trained export alike); a quarter of its steps is pipeline fill, and it evaluates
// every Gaussian of a bucket against all 192 pixels of the tile. The forward kernel's formulation -- lane = pixel, each wave walks only the
// Gaussians whose bounding box reaches its 16x4 strip -- visits 0.65-0.72 as many lane-steps, needs no fill, no ring of per-pixel constants (they
// sit in registers) and no shifted state (T and S belong to the lane). What it needs instead is a sum over the 64 pixels of a strip for each of
// the nine per-Gaussian gradients, which as DPP reductions costs 54 cross-lane adds per (Gaussian, strip) pair (the strip variant 1: slower).
// Here that sum is a matrix product. All nine sums are linear in two per-pair values, w = T alpha and hh = -alpha/2 dL/dalpha:
//     dL/dcolour_c = sum_p w g_c(p),      sum_p hh { 1, x', y', x'^2, x'y', y'^2 }   (x', y' = pixel centre relative to the TILE centre: exact
// small half-integers), from which the sums over dx = Dx - x', dy = Dy - y' (Dx, Dy = mean2d relative to the tile centre) follow per Gaussian:
//     sum hh dx = Dx Sh - Sx,  sum hh dx^2 = Dx (Dx Sh - 2 Sx) + Sxx,  sum hh dx dy = Dx Dy Sh - Dx Sy - Dy Sx + Sxy, ...
// So each wave keeps, for up to 8 walked Gaussians, w and hh of its 64 pixels in 16 rows of a private LDS buffer (the transposition: lanes are
// pixels when the rows are written and (k, column) pairs of the matrix instruction when they are read), and one pass of 16
// v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate: bitwise an fmaf chain) multiplies the 9 x 64 feature matrix of the strip
// [g_r, g_g, g_b, 1, x', y', x'^2, x'y', y'^2] with those rows: columns 0..7 = w of the 8 slots, 8..15 = hh. The matrix pipe runs beside the
// vector pipe; the vector instructions per pair are the forward walk's plus the gradient arithmetic. The results of the tile's three strips
// add up in LDS accumulators of the bucket's 64 Gaussians; then lane = Gaussian converts and issues the nine global atomics as the other variants do.
// alpha is the forward kernel's expression operation for operation (same dx, dy: pixel centre = px + 0.5), T and S restart from the bucket's
// checkpoint exactly as in the systolic form.
constexpr unsigned kPixSlots = 8;                        // walked Gaussians per matrix pass
constexpr unsigned kPixRows = 2 * kPixSlots;             // w rows, then hh rows
constexpr unsigned kPixStride = 68;                      // floats per row: 64 pixels + 4, so that the 16-byte reads of 16 columns hit 64 distinct banks
#ifndef FGS_K11M_MAX_BLOCKS
#define FGS_K11M_MAX_BLOCKS 65536
#endif
// Debug-only phase timer (tools/k11m_phases.sh, -DFGS_K11M_PHASES; the product build has none of it): shader cycles per wave summed over the launch --
// [0] items, [1] staging of the records, [2] per strip: pixel loads, feature operand, cull + order table, [3] the walk without its matrix passes,
// [4] the matrix passes, [5] tail (conversion, atomics), [6] pairs walked, [7] matrix passes.
#ifdef FGS_K11M_PHASES
__device__ unsigned long long g_k11m_phases[8];
#define FGS_PH(i) ph_[i] += __builtin_readcyclecounter() - pt_, pt_ = __builtin_readcyclecounter()
#else
#define FGS_PH(i)
#endif
__global__ void __launch_bounds__(kWave) blend_backward_pixel_kernel(const BlendBackwardArgs a) {
    // ONE wave per work item (tile, bucket), as in the systolic form: it walks the tile's three 16x4 strips one after the other, so there is no
    // workgroup barrier (the first version gave each strip its own wave: the two waves with the shorter lists waited at the barrier for the
    // third, and eight 3-wave workgroups per CU did not cover the four dependent loads at the head of every item).
    __shared__ float4 s_rec[3 * kBucket];                                      // mean.xy conic.ab | conic.c opacity r g (clamped) | b (clamped) bounds_x bounds_y flags
    __shared__ float s_acc[9 * kBucket];                                       // planes Sh Sx Sy Sxx Sxy Syy c0 c1 c2 of the bucket's Gaussians
    __shared__ __attribute__((aligned(16))) float s_v[kPixRows * kPixStride];
    __shared__ uint8_t s_order[kBucket + kPixSlots + 4];                       // bucket-relative index of the i-th Gaussian the current strip walks
    const unsigned lane = threadIdx.x, half = lane >> 5;
    float* const v_mine = s_v;
    const unsigned pos = (lane & 3u) * 16u + (lane >> 2);                      // pixel p = 4 s + q of matrix k-step s sits at q * 16 + s of its row
    const unsigned col = lane & 15u, q = lane >> 4;                            // this lane's column / k index in the matrix instruction
    const unsigned lx = half * kSubtileW + (lane & 7u), ly_in_strip = (lane >> 3) & 3u;
    const unsigned n_live = *a.live_count;
#ifdef FGS_K11M_PHASES
    unsigned long long ph_[8] = {0, 0, 0, 0, 0, 0, 0, 0}, pt_ = __builtin_readcyclecounter();
#endif
    // The head of an item is a chain of dependent loads (list entry -> tile range / bucket base -> primitive index -> record), and each strip
    // had two more (pixel record -> checkpoint). With four waves per SIMD that latency was two thirds of a wave's time (tools/k11m_phases.sh). So:
    // the scalar part of the chain is fetched one item AHEAD (the wave keeps the next item's list entry, range and bucket base in scalar
    // registers), and everything per pixel -- the three strips' records and checkpoints -- is requested in one go at the top of the item, next
    // to the primitive indices: two exposed round trips per item instead of ten.
    unsigned item = blockIdx.x;
    uint2 work = make_uint2(0u, 0u), range = make_uint2(0u, 0u);
    unsigned bucket_base = 0;
    if (item < n_live) {
        work = a.work_list[item];
        range = a.ranges[work.x];
        bucket_base = work.x == 0 ? 0u : a.bucket_offsets[work.x - 1];
    }
    for (; item < n_live; item += gridDim.x) {                                 // wave-uniform
#ifdef FGS_K11M_PHASES
        ph_[0] += 1; pt_ = __builtin_readcyclecounter();
#endif
        const unsigned tile = work.x, tb = work.y;
        const unsigned tile_n = range.y - range.x;
        const unsigned bucket = bucket_base + tb;
        const unsigned first_gaussian = tb * kBucket;
        const unsigned n_here = min(static_cast<unsigned>(kBucket), tile_n - first_gaussian);
        const unsigned tile_x = tile % a.grid_w, tile_y = tile / a.grid_w;
        const unsigned range_x = range.x;

        // ---- requests of this item: primitive index, the three strips' pixel records and checkpoints ----
        uint32_t prim = 0, hot_slot_word = 0;
        if (lane < n_here) prim = a.inst_prims[range_x + first_gaussian + lane];
        float4 cst_[3], g_[3], ck_[3];
#pragma unroll
        for (unsigned st = 0; st < 3u; ++st) {
            const unsigned local = (st * kSubtileH + ly_in_strip) * kTileW + lx;
            cst_[st] = a.pixrec[((size_t)tile * kTilePixels + local) * 2 + 1];
            g_[st] = a.pixrec[((size_t)tile * kTilePixels + local) * 2];
            ck_[st] = a.ckpt[(size_t)bucket * kTilePixels + local];
        }
        // ---- the scalar head of the NEXT item ----
        {
            const unsigned next = item + gridDim.x;
            if (next < n_live) {
                work = a.work_list[next];
                range = a.ranges[work.x];
                bucket_base = work.x == 0 ? 0u : a.bucket_offsets[work.x - 1];
            }
        }
        {                                                                      // the bucket's records (kb:297-319), lane = Gaussian
            float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0, r2 = r0;
            uint32_t flags = 0;
            if (lane < n_here) {
                const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
                r0 = r[0]; r1 = r[1]; r2 = r[2];
                flags = (r1.z >= 0.0f ? 1u : 0u) | (r1.w >= 0.0f ? 2u : 0u) | (r2.x >= 0.0f ? 4u : 0u);      // kb:313-318
                hot_slot_word = __float_as_uint(r2.w);
            }
            s_rec[lane] = r0;
            s_rec[kBucket + lane] = make_float4(r1.x, r1.y, fmaxf(r1.z, 0.0f), fmaxf(r1.w, 0.0f));
            s_rec[2 * kBucket + lane] = make_float4(fmaxf(r2.x, 0.0f), r2.y, r2.z, __uint_as_float(flags));
#pragma unroll
            for (unsigned e = 0; e < 9u; ++e) s_acc[e * kBucket + lane] = 0.0f;
        }
        // ---- the pixels' state at the bucket's checkpoint (kb:349-380): six values per strip stay in registers ----
        float gx_[3], gy_[3], gz_[3], T_[3], S_[3];
        unsigned rel_[3];
#pragma unroll
        for (unsigned st = 0; st < 3u; ++st) {
            const unsigned last = __float_as_uint(cst_[st].w);                // 0 outside the image
            // a pixel that finished before this bucket never wrote its checkpoint (kf:436) and receives nothing here
            const bool live = last > first_gaussian;
            rel_[st] = live ? last - first_gaussian : 0u;                      // Gaussians of this bucket in front of the pixel's last contributor
            gx_[st] = g_[st].x; gy_[st] = g_[st].y; gz_[st] = g_[st].z;
            T_[st] = live ? ck_[st].w : 0.0f;
            S_[st] = live ? ((cst_[st].x - ck_[st].x) * g_[st].x + (cst_[st].y - ck_[st].y) * g_[st].y + (cst_[st].z - ck_[st].z) * g_[st].z) - g_[st].w : 0.0f;   // kb:371-377 projected on dL/dC
        }
        wave_lds_fence();
        FGS_PH(1);

#pragma unroll 1
        for (unsigned strip = 0; strip < static_cast<unsigned>(kTilePixels / kWave); ++strip) {
            const unsigned ly = strip * kSubtileH + ly_in_strip;
            const float pxf = static_cast<float>(tile_x * kTileW + lx) + 0.5f, pyf = static_cast<float>(tile_y * kTileH + ly) + 0.5f;
            // (the strip loop stays rolled -- the walk below is long -- so the strip's six values are picked by selects, not by indexing register arrays)
            const unsigned rel = strip == 0u ? rel_[0] : strip == 1u ? rel_[1] : rel_[2];
            // Gaussians at or behind every pixel's last contributor take nothing (kb:412). (The maximum is wave-uniform; the compiler only knows that of
            // a value read through v_readfirstlane, and a list it believes divergent turns the walk below into an EXEC-masked vector loop.)
            const unsigned rel_max = wave_uniform(wave_max(rel));
            if (rel_max == 0u) continue;                                       // no live pixel in this strip
            const float4 g = make_float4(strip == 0u ? gx_[0] : strip == 1u ? gx_[1] : gx_[2], strip == 0u ? gy_[0] : strip == 1u ? gy_[1] : gy_[2],
                                         strip == 0u ? gz_[0] : strip == 1u ? gz_[1] : gz_[2], 0.0f);
            float T = strip == 0u ? T_[0] : strip == 1u ? T_[1] : T_[2], sS = strip == 0u ? S_[0] : strip == 1u ? S_[1] : S_[2];

            // ---- the strip's feature matrix as matrix operand A: row c of [g_r g_g g_b 1 x' y' x'^2 x'y' y'^2], 16 k-steps ----
            float A[16];
            {
                const float xr = static_cast<float>(lx) - 7.5f, yr = static_cast<float>(ly) - 5.5f;
                v_mine[0 * kPixStride + pos] = g.x; v_mine[1 * kPixStride + pos] = g.y; v_mine[2 * kPixStride + pos] = g.z;
                v_mine[3 * kPixStride + pos] = 1.0f; v_mine[4 * kPixStride + pos] = xr; v_mine[5 * kPixStride + pos] = yr;
                v_mine[6 * kPixStride + pos] = xr * xr; v_mine[7 * kPixStride + pos] = xr * yr; v_mine[8 * kPixStride + pos] = yr * yr;
                wave_lds_fence();
                const float4* ap = reinterpret_cast<const float4*>(v_mine + min(col, 8u) * kPixStride + q * 16u);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 t = ap[i];
                    const bool used = col < 9u;
                    A[4 * i] = used ? t.x : 0.0f; A[4 * i + 1] = used ? t.y : 0.0f; A[4 * i + 2] = used ? t.z : 0.0f; A[4 * i + 3] = used ? t.w : 0.0f;
                }
                wave_lds_fence();                                              // the rows are reused for w / hh below
            }

            // ---- cull the bucket against this strip's two 8x4 sub-tiles (kf:445-451) ----
            const unsigned sub_y0 = tile_y * kTileH + strip * kSubtileH, sub_y1 = sub_y0 + kSubtileH;
            const unsigned subl_x0 = tile_x * kTileW, subl_x1 = subl_x0 + kSubtileW, subr_x1 = subl_x1 + kSubtileW;
            bool in_l = false, in_r = false;
            if (lane < n_here) {
                const float4 gc = s_rec[2 * kBucket + lane];
                const uint32_t bx = __float_as_uint(gc.y), by = __float_as_uint(gc.z);
                const unsigned x_min = bx & 0xffffu, x_max = bx >> 16, y_min = by & 0xffffu, y_max = by >> 16;
                const bool in_y = y_min < sub_y1 && sub_y0 < y_max;
                in_l = in_y && x_min < subl_x1 && subl_x0 < x_max;
                in_r = in_y && x_min < subr_x1 && subl_x1 < x_max;
            }
            const uint64_t mask_l = wave_ballot(in_l), mask_r = wave_ballot(in_r);
            const uint64_t pending = (mask_l | mask_r) & (rel_max >= 64u ? ~0ull : ((1ull << rel_max) - 1ull));
            // slot -> Gaussian of the matrix batches: the walk visits the set bits of `pending` in order, so its i-th pair is the i-th set bit
            // (every lane stores -- the lanes outside the list into a spare element -- so that no divergent branch sits between the list and the walk)
            s_order[((pending >> lane) & 1ull) ? lanes_below(pending) : kBucket + kPixSlots] = static_cast<uint8_t>(lane);
            FGS_PH(2);

            // ---- the walk: eight pairs into the rows, then one matrix pass. (Two other schedules were built and measured slower on the layered scene,
            // profiles/r04_k11m_closeout.txt: the matrix instructions of batch n issued between the pairs of batch n + 1 -- 1.69 ms against 1.58 --
            // and groups of four pairs as straight-line code for instruction-level parallelism -- 132 registers, three waves per SIMD, 1.83 ms.)
            unsigned n_slots = 0, n_flushed = 0;                               // filled rows of the current matrix batch, pairs of earlier batches (wave-uniform)
            auto flush = [&](const unsigned n) {
                FGS_PH(3);
                wave_lds_fence();
                const float4* bp = reinterpret_cast<const float4*>(v_mine + col * kPixStride + q * 16u);
                const float4 b0 = bp[0], b1 = bp[1], b2 = bp[2], b3 = bp[3];
                const unsigned slot = col & 7u;
                const unsigned gi = s_order[n_flushed + slot];
                fgs_acc4 d0 = {0.0f, 0.0f, 0.0f, 0.0f}, d1 = {0.0f, 0.0f, 0.0f, 0.0f};      // two chains: a dependent matrix instruction waits 40 cycles, an independent one 32
                if (!(a.ablate & 4)) {
                    wave_mfma_16x16x4(A[0], b0.x, d0); wave_mfma_16x16x4(A[1], b0.y, d1); wave_mfma_16x16x4(A[2], b0.z, d0); wave_mfma_16x16x4(A[3], b0.w, d1);
                    wave_mfma_16x16x4(A[4], b1.x, d0); wave_mfma_16x16x4(A[5], b1.y, d1); wave_mfma_16x16x4(A[6], b1.z, d0); wave_mfma_16x16x4(A[7], b1.w, d1);
                    wave_mfma_16x16x4(A[8], b2.x, d0); wave_mfma_16x16x4(A[9], b2.y, d1); wave_mfma_16x16x4(A[10], b2.z, d0); wave_mfma_16x16x4(A[11], b2.w, d1);
                    wave_mfma_16x16x4(A[12], b3.x, d0); wave_mfma_16x16x4(A[13], b3.y, d1); wave_mfma_16x16x4(A[14], b3.z, d0); wave_mfma_16x16x4(A[15], b3.w, d1);
                }
                // this lane holds D[row 4 q + r][col]: rows 0..2 = colour sums (columns 0..7, the w rows), rows 3..8 = moment sums (columns 8..15, the hh rows).
                // One wave owns the accumulators, and a Gaussian sits in one slot of one pass per strip: plain read-modify-write, in program order.
                const bool is_w = col < 8u;
                if (slot < n && !(a.ablate & 4)) {
                    if (q == 0u) {
                        if (is_w) {
                            s_acc[6 * kBucket + gi] += d0[0] + d1[0]; s_acc[7 * kBucket + gi] += d0[1] + d1[1]; s_acc[8 * kBucket + gi] += d0[2] + d1[2];
                        } else s_acc[gi] += d0[3] + d1[3];
                    } else if (!is_w) {
                        if (q == 1u) {
                            s_acc[1 * kBucket + gi] += d0[0] + d1[0]; s_acc[2 * kBucket + gi] += d0[1] + d1[1];
                            s_acc[3 * kBucket + gi] += d0[2] + d1[2]; s_acc[4 * kBucket + gi] += d0[3] + d1[3];
                        } else if (q == 2u) s_acc[5 * kBucket + gi] += d0[0] + d1[0];
                    }
                }
                n_flushed += n;
                wave_lds_fence();                                              // the next batch overwrites the rows
#ifdef FGS_K11M_PHASES
                ph_[7] += 1; ph_[6] += n;
#endif
                FGS_PH(4);
            };

            float* v_row = v_mine + pos;                                       // this lane's element of the row of the current slot
            uint64_t pend = wave_uniform(pending);                             // (re-stated uniform: see rel_max)
            while (pend != 0ull) {                                             // wave-uniform scalar loop
                const unsigned j = static_cast<unsigned>(__ffsll(static_cast<unsigned long long>(pend))) - 1u;
                pend &= pend - 1ull;
                if (!(a.ablate & 8)) {
                    const float4* const entry = s_rec + j;
                    const float4 ga = entry[0], gb = entry[kBucket];
                    const float colb = entry[2 * kBucket].x;
                    const float dx = ga.x - pxf, dy = ga.y - pyf;
                    const float power = -0.5f * (ga.z * dx * dx + gb.x * dy * dy) - ga.w * dx * dy;
                    const float gauss = __expf(fminf(power, 0.0f));
                    const float alpha_raw = gb.y * gauss;
                    // Contributes (kb:412,419-421; kf:445-467): alpha >= 1/255, the Gaussian in front of this pixel's last contributor, and its box on this
                    // lane's 8x4 sub-tile -- the last one is the same for the 32 lanes of a half, so it is a scalar mask. Branch-free: a pair that does not
                    // contribute runs the same instructions with alpha = 0, which leaves T and S as they are and gives w = hh = 0 -- the contribution block
                    // would run anyway in 92-96 % of the pairs (profiles/r04_k11_pair_efficiency.txt: some lane passes), and there is no EXEC bookkeeping
                    // and no zero-fill of the two values that go to the matrix rows.
                    const uint64_t not_mine = (((mask_l >> j) & 1ull) ? 0ull : 0x00000000ffffffffull) | (((mask_r >> j) & 1ull) ? 0ull : 0xffffffff00000000ull);
                    const uint64_t pass = wave_ballot(alpha_raw >= kMinAlphaThreshold && j < rel) & ~not_mine;
                    const float alpha = lane_select(pass, 0.0f, alpha_raw);
                    const float w = T * alpha;
                    const float cg = gb.z * g.x + gb.w * g.y + colb * g.z;
                    sS -= w * cg;                                               // kb:429 projected on dL/dC
                    const float oma = 1.0f - alpha;
                    const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
                    const float dl_dalpha = T * cg - sS * oma_rcp;              // kb:434-436
                    const float hh = (-0.5f * alpha) * dl_dalpha;
                    T *= oma;
                    v_row[0] = w;
                    v_row[kPixSlots * kPixStride] = hh;
                }
                v_row += kPixStride;
                if (++n_slots == kPixSlots) { flush(kPixSlots); n_slots = 0; v_row = v_mine + pos; }
            }
            if (n_slots != 0) flush(n_slots);
            FGS_PH(3);
        }
        wave_lds_fence();

        // ---- per Gaussian (lane = Gaussian again): moments about the tile centre -> the nine gradients, added to the Gaussian's record (kb:459-470) ----
        if (lane < n_here) {
            const float Sh = s_acc[lane], Sx = s_acc[kBucket + lane], Sy = s_acc[2 * kBucket + lane];
            const float Sxx = s_acc[3 * kBucket + lane], Sxy = s_acc[4 * kBucket + lane], Syy = s_acc[5 * kBucket + lane];
            const float c0 = s_acc[6 * kBucket + lane], c1 = s_acc[7 * kBucket + lane], c2 = s_acc[8 * kBucket + lane];
            const bool silent = Sh == 0.0f && Sx == 0.0f && Sy == 0.0f && Sxx == 0.0f && Sxy == 0.0f && Syy == 0.0f && c0 == 0.0f && c1 == 0.0f && c2 == 0.0f;
            if (!silent && !(a.ablate & 1)) {
                const float4 ga = s_rec[lane], gb = s_rec[kBucket + lane], gc = s_rec[2 * kBucket + lane];
                const float ca = ga.z, cb = ga.w, cc = gb.x, op = gb.y;
                const float Dx = ga.x - (static_cast<float>(tile_x * kTileW) + 8.0f), Dy = ga.y - (static_cast<float>(tile_y * kTileH) + 6.0f);
                const float a_x = Dx * Sh - Sx, a_y = Dy * Sh - Sy;
                const float a_xx = Dx * (Dx * Sh - 2.0f * Sx) + Sxx, a_yy = Dy * (Dy * Sh - 2.0f * Sy) + Syy;
                const float a_xy = Dx * (Dy * Sh - Sy) - Dy * Sx + Sxy;
                const unsigned flags = __float_as_uint(gc.w);
                unsigned tx0, tx1, ty0, ty1;
                tile_rect(__float_as_uint(gc.y), __float_as_uint(gc.z), tx0, tx1, ty0, ty1);
                const unsigned footprint = (tx1 - tx0) * (ty1 - ty0);
                const uint32_t hot_word = footprint > kHotFootprint ? hot_slot_word : 0u;
                // the Gaussian's own record of nine consecutive floats, or (hot) the record of its slot in the tile's replica
                float* dst = hot_word != 0u ? a.acc_hot + ((size_t)(tile % kHotReplicas) * kMaxHot + (hot_word - 1u)) * kAccRecordWords : a.acc + (size_t)prim * kAccRecordWords;
                unsafeAtomicAdd(dst, 2.0f * (ca * a_x + cb * a_y));
                unsafeAtomicAdd(dst + 1, 2.0f * (cb * a_x + cc * a_y));
                unsafeAtomicAdd(dst + 2, a_xx);
                unsafeAtomicAdd(dst + 3, a_xy);
                unsafeAtomicAdd(dst + 4, a_yy);
                unsafeAtomicAdd(dst + 5, a.proper_aa ? -2.0f * Sh / op : -2.0f * Sh * (1.0f - op));
                unsafeAtomicAdd(dst + 6, (flags & 1u) ? c0 : 0.0f);
                unsafeAtomicAdd(dst + 7, (flags & 2u) ? c1 : 0.0f);
                unsafeAtomicAdd(dst + 8, (flags & 4u) ? c2 : 0.0f);
            }
        }
        wave_lds_fence();                                                      // the next item restages the records and clears the accumulators
        FGS_PH(5);
    }
#ifdef FGS_K11M_PHASES
    if (lane == 0) for (int i = 0; i < 8; ++i) if (ph_[i] != 0) atomicAdd(&g_k11m_phases[i], ph_[i]);
#endif
}
#ifdef FGS_K11M_PHASES
}  // namespace fgs
extern "C" __attribute__((visibility("default"))) int fgs_debug_k11m_phases(unsigned long long* out, int reset) {
    if (out != nullptr && hipMemcpyFromSymbol(out, HIP_SYMBOL(fgs::g_k11m_phases), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        void* dev = nullptr;
        if (hipGetSymbolAddress(&dev, HIP_SYMBOL(fgs::g_k11m_phases)) != hipSuccess || hipMemset(dev, 0, sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    }
    return 0;
}
namespace fgs {
#endif

std::atomic<int> g_backward_ablate{0};    // fgs_debug_set_option(7, bits): timing experiments only -- 1: no atomics, 2: no step loop (results are wrong)
std::atomic<int> g_k11m_max_blocks{FGS_K11M_MAX_BLOCKS};   // variant 4: upper bound of its grid (fgs_debug_set_option(13, n)); items beyond it are walked grid-stride

// The exhibit kernel of a.variant (anything but 3), and nothing else: launch_blend_backward (blend_backward.hip) follows it with the kernel that
// ends the pass -- the fold of the hot replicas behind variants 4 / 5, the dirty mark behind variants 0 / 1 / 2 -- and reads the launch error.
void launch_blend_backward_exhibit(const BlendBackwardArgs& a, hipStream_t s) {
    if (a.variant == 4) {
        const unsigned cap_blocks = static_cast<unsigned>(g_k11m_max_blocks.load());
        const unsigned blocks = a.n_buckets_cap < cap_blocks ? a.n_buckets_cap : cap_blocks;
        hipLaunchKernelGGL(blend_backward_pixel_kernel, dim3(blocks), dim3(kWave), 0, s, a);
    } else if (a.variant == 5) {        // chained (round 6): option 14 = its number of waves (tests shorten it so that chains get long)
        const unsigned chain_waves = static_cast<unsigned>(static_cast<int>(g_k11_chain_waves));
        hipLaunchKernelGGL(blend_backward_chained_kernel, dim3(a.n_buckets_cap < chain_waves ? a.n_buckets_cap : chain_waves), dim3(kWave), 0, s, a);
    } else if (a.variant == 1) {
        hipLaunchKernelGGL(blend_backward_strip_kernel, dim3(a.n_buckets_cap), dim3(kTilePixels), 0, s, a);
    } else {
        const dim3 grid((a.n_buckets_cap + kBackwardWavesPerBlock - 1) / kBackwardWavesPerBlock), block(kBackwardWavesPerBlock * kWave);
        if (a.variant == 2) hipLaunchKernelGGL(blend_backward_kernel<true>, grid, block, 0, s, a);
        else hipLaunchKernelGGL(blend_backward_kernel<false>, grid, block, 0, s, a);
    }
}

}  // namespace fgs
#endif  // FGS_DEV_SWITCHES

// K11: blend backward for gfx950 -- one wave64 per bucket of 64 depth-consecutive Gaussians of one tile; the tile's 192
// pixels stream through the wave's lanes as a systolic pipeline (lane l holds Gaussian l, pixel state moves one lane per
// step), gradients accumulate in registers and leave through 9 atomics per lane at the end.
// Semantics: reference kernels_backward.cuh:260-471 (per-32 buckets, 9 shfl_up + an LDS reload per step).
//
// CDNA4 shape:
//  * bucket = wavefront = 64 Gaussians: 255 steps serve 64 lanes (reference: 223 steps serve 32), and the forward
//    pass writes half as many checkpoints.
//  * only the 4 values a Gaussian changes (remaining colour, transmittance) travel through the lanes, one in-place DPP
//    wave_shr:1 each; the next pixel enters at lane 0 from a wave-uniform LDS read, and the 5 per-pixel constants are
//    read by lane l at LDS slot (step - l) -- conflict-free consecutive slots -- instead of being shifted. The wave's
//    6.9 KB LDS slice is private: no workgroup barrier anywhere. (v1 shifted all 9 values through a register ring:
//    ~40 mov/DPP per step; this form needs 8 + 3 LDS reads.)
//  * per-pixel constants (dL/dC, C_final - T_final*bg, T_final*-(dL/dC . bg), last contributor) are staged ONCE per
//    backward pass into a tile-major 32-byte record, so each bucket reads 48 B per pixel with three coalesced 16-byte
//    loads instead of gathering 9 scalars from image-linear arrays per bucket.
#include <type_traits>

#include "fgs_kernels.h"
#include <fgs_wave.h>
#include "fgs_tile_scan.h"
#include "fgs_k11_probes.h"      // FGS_K11_PROBE_*: nothing unless a probe library is being built (-DFGS_PAIR_STATS / -DFGS_K11_TIMELINE)

#ifndef FGS_CKPT_NT
#define FGS_CKPT_NT 1      // round 6: ... and are read as non-temporal loads (training iteration 2.218 -> 2.187 ms, layered scene 3.728 -> 3.706, three alternating pairs: profiles/r06_ab_ckpt_nt.txt); 0: A/B
#endif
namespace fgs {

// staging pass: kb:349-380 hoisted out of the per-bucket loop
// DEPTH (stage_pixels_kernel<true>, fgs_backward_aux): additionally stages (gD, gA, D_final, T_final) per pixel -- the upstream gradients of expected
// depth and accumulated opacity and what K11 needs to enlarge the remaining-colour scalar by gD (D_final - D_ckpt) + gA (T_ckpt - T_final) -- and
// clears acc_z and its hot replicas. Every DEPTH statement is under `if constexpr`: stage_pixels_kernel<false> compiles to the instructions the kernel had.
// ABS (stage_pixels_kernel<*, true>, fgs_backward_absgrad): additionally clears acc_abs and its hot replicas. Every ABS statement is under `if constexpr`
// too, and the ABS = false argument types are the ones above: the two ABS = false instantiations compile to the instructions they had.
template <bool DEPTH, bool ABS = false> using BackwardArgsOf = std::conditional_t<ABS, std::conditional_t<DEPTH, BlendBackwardDepthAbsArgs, BlendBackwardAbsArgs>,
                                                                                   std::conditional_t<DEPTH, BlendBackwardDepthArgs, BlendBackwardArgs>>;
__device__ __forceinline__ const BlendBackwardArgs& blend_part(const BlendBackwardArgs& v) { return v; }
__device__ __forceinline__ const BlendBackwardArgs& blend_part(const BlendBackwardDepthArgs& v) { return v.blend; }
__device__ __forceinline__ const BlendBackwardArgs& blend_part(const BlendBackwardAbsArgs& v) { return v.blend; }
__device__ __forceinline__ const BlendBackwardArgs& blend_part(const BlendBackwardDepthAbsArgs& v) { return v.blend; }
__device__ __forceinline__ BlendDepthPart depth_part(const BlendBackwardArgs&) { return BlendDepthPart{}; }          // never read: every use is under `if constexpr (DEPTH)`
__device__ __forceinline__ const BlendDepthPart& depth_part(const BlendBackwardDepthArgs& v) { return v.d; }
__device__ __forceinline__ BlendDepthPart depth_part(const BlendBackwardAbsArgs&) { return BlendDepthPart{}; }
__device__ __forceinline__ const BlendDepthPart& depth_part(const BlendBackwardDepthAbsArgs& v) { return v.d; }
__device__ __forceinline__ BlendAbsPart abs_part(const BlendBackwardArgs&) { return BlendAbsPart{}; }               // never read: every use is under `if constexpr (ABS)`
__device__ __forceinline__ BlendAbsPart abs_part(const BlendBackwardDepthArgs&) { return BlendAbsPart{}; }
__device__ __forceinline__ const BlendAbsPart& abs_part(const BlendBackwardAbsArgs& v) { return v.abs; }
__device__ __forceinline__ const BlendAbsPart& abs_part(const BlendBackwardDepthAbsArgs& v) { return v.abs; }
template <bool DEPTH, bool ABS>
__global__ void __launch_bounds__(kTilePixels) stage_pixels_kernel(const BackwardArgsOf<DEPTH, ABS> args) {
    const BlendBackwardArgs& a = blend_part(args);
    [[maybe_unused]] const BlendDepthPart& x = depth_part(args);       // DEPTH only
    [[maybe_unused]] const BlendAbsPart& y = abs_part(args);           // ABS only
    // (Round 6, measured and withdrawn: XCD x taking a contiguous band of tiles, so that the two tiles sharing a 128-byte line of the six image planes
    // run under one L2 -- what took 6 % off the loss kernels -- leaves this kernel at 0.040 ms: profiles/r06_ab_stage_pixels_xcd.txt.)
    const unsigned tile = blockIdx.x;
    const unsigned local = threadIdx.x;
    if (tile < a.n_tiles) {
        const unsigned tile_x = tile % a.grid_w, tile_y = tile / a.grid_w;
        const unsigned px = tile_x * kTileW + (local % kTileW), py = tile_y * kTileH + (local / kTileW);
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
        [[maybe_unused]] float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);                       // DEPTH: gD, gA, D_final, T_final
        if (px < a.width && py < a.height) {
            const size_t pix = (size_t)a.width * py + px, n_pixels = (size_t)a.width * a.height;
            const float fT = a.final_T[(size_t)tile * kTilePixels + local];
            const float b0 = a.bg[0], b1 = a.bg[1], b2 = a.bg[2];
            g.x = a.grad_image[pix]; g.y = a.grad_image[n_pixels + pix]; g.z = a.grad_image[2 * n_pixels + pix];
            g.w = fT * -(g.x * b0 + g.y * b1 + g.z * b2);                                  // kb:375-377
            c.x = a.image[pix] - fT * b0; c.y = a.image[n_pixels + pix] - fT * b1; c.z = a.image[2 * n_pixels + pix] - fT * b2;
            c.w = __uint_as_float(a.n_processed[(size_t)tile * kTilePixels + local]);
            if constexpr (DEPTH) {
                e.w = fT;
                if (x.grad_alpha != nullptr) e.y = x.grad_alpha[pix];
                if (x.grad_depth != nullptr) { e.x = x.grad_depth[pix]; e.z = x.depth[pix]; }
            }
        }
        a.pixrec[((size_t)tile * kTilePixels + local) * 2] = g;
        a.pixrec[((size_t)tile * kTilePixels + local) * 2 + 1] = c;
        if constexpr (DEPTH) x.pixaux[(size_t)tile * kTilePixels + local] = e;
        // the tile's entries of the live-bucket list (variant 3): the planning pass has scanned the per-tile counts, the entries are written here,
        // by 12 k workgroups instead of one
        if (a.live_offsets != nullptr) {
            const unsigned nl = (a.max_n_processed[tile] + kBucket - 1) / kBucket;              // kb:295
            const unsigned base = a.live_offsets[tile];
            for (unsigned k = local; k < nl; k += kTilePixels) a.work_list[base + k] = make_uint2(tile, k);
        }
    }
    // K11 adds into records that start at zero (replaces api:127-134). The records of the visible Gaussians were cleared by K1 in the forward pass;
    // left for this kernel are the hot replicas -- or records and replicas alike when no K1 filled the blob or a backward pass already ran over it
    // (BlendBackwardArgs). Every workgroup clears an equal share, 16 bytes per store. (Round 5: a hipMemsetAsync of 117 MB in front of this kernel,
    // 16 us on the critical path of every backward pass; doing all of it here costs the same 16 us -- HBM write rate, profiles/r06_ab_acc_clear.txt.)
    {
        const bool everything = a.clear_everything != 0 || *a.dirty_flag != 0u;
        const unsigned n_f4 = everything ? a.clear_all_f4 : a.clear_hot_f4;
        float4* const z = reinterpret_cast<float4*>(everything ? a.acc : a.acc_hot);
        const unsigned per_group = (n_f4 + gridDim.x - 1u) / gridDim.x;
        const unsigned first = tile * per_group, last = min(first + per_group, n_f4);
        for (unsigned k = first + local; k < last; k += kTilePixels) z[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if constexpr (DEPTH) {       // acc_z and its replicas start every depth pass at zero: K1 does not know of them
        float4* const z = reinterpret_cast<float4*>(x.acc_z);
        const unsigned per_group = (x.clear_z_f4 + gridDim.x - 1u) / gridDim.x;
        const unsigned first = tile * per_group, last = min(first + per_group, x.clear_z_f4);
        for (unsigned k = first + local; k < last; k += kTilePixels) z[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    if constexpr (ABS) {         // acc_abs and its replicas likewise start every pass that sums them at zero
        float4* const z = reinterpret_cast<float4*>(y.acc_abs);
        const unsigned per_group = (y.clear_abs_f4 + gridDim.x - 1u) / gridDim.x;
        const unsigned first = tile * per_group, last = min(first + per_group, y.clear_abs_f4);
        for (unsigned k = first + local; k < last; k += kTilePixels) z[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// ---- variant 3 (default): work list of live buckets + compacted live pixels + two-value pipeline state -----------------
// The formulation this library ships; the four it was measured against -- variants 0 / 2 (the file header's systolic form over ALL buckets and all 192
// pixels), 1, 4 and 5 -- are exhibits of the dev library in a unit of their own, blend_backward_exhibits.hip.
// Three observations about that first systolic form (rocprofv3 PMC, round 1: VALU-issue bound, ~70 instructions per step):
//  (1) 91 % of the launched buckets lie behind their tile's max_n_processed (kb:295) and exit after four dependent loads.
//      A one-workgroup planning pass turns (ranges, max_n_processed) into a dense list of LIVE (tile, bucket) pairs and its
//      length; the blend kernel walks that list (grid-stride), so no wave is ever launched for a dead bucket.
//  (2) inside a live bucket only pixels whose last contributor lies at or behind the bucket's first Gaussian can receive
//      anything (kb:412). The order in which pixels travel through the lanes is irrelevant, so staging COMPACTS the live
//      pixels (ballot + prefix count) and the pipeline runs n_live_pixels + 63 steps instead of 255. Per pixel the LDS holds
//      24 bytes: dL/dC (3 floats) + one packed word (x, y inside the tile and min(last - first Gaussian, 64) as three bytes,
//      each converted by a single v_cvt_f32_ubyteN) read by lane l at slot step - l, and the injected state (8 bytes).
//  (3) dL/dalpha only needs the remaining colour behind a Gaussian projected on the pixel's dL/dC (kb:434-436):
//          dL/dalpha = T (c . g) - (S - g_w) / (1 - alpha),   S = (C_final - T_final bg - C_front) . g
//      so the pixel state that shifts through the lanes is TWO scalars (T, S - g_w) instead of four, S is updated with one
//      FMA, and the per-Gaussian sums that are linear in per-lane constants are factored out of the loop: the colour-clamp
//      gate multiplies sum(w g) once at the end (kb:426-427), dL/dopacity = -2 sum(hh) / opacity because G = alpha / opacity
//      (kb:438), and dL/dmean2d = 2 [a b; b c] (sum(hh dx), sum(hh dy)) (kb:449-453) with hh = -alpha/2 dL/dalpha.
//      About 50 VALU instructions per step remain.
__global__ void __launch_bounds__(kTileScanThreads) plan_blend_backward_kernel(const BlendBackwardArgs a) {
    // One workgroup: exclusive scan of the live-bucket count of every tile (fgs_tile_scan.h: a thread sums 16 consecutive tiles, one DPP wave
    // scan, one barrier per 16 Ki tiles; the first version -- one barrier per 1024-tile chunk -- took 15 us at 1080p, all of it latency). live_offsets[tile] = first list slot of the tile; the entries themselves are written by stage_pixels_kernel
    // (a single workgroup writing 115 k entries took 58 us on the layered scene).
    __shared__ TileScanShared s_scan;
    const unsigned tid = threadIdx.x;
    uint32_t base = 0;                                        // live buckets in front of the current pass (uniform)
    int parity = 0;
    for (unsigned t0 = 0; t0 < a.n_tiles; t0 += kTileScanThreads * kTileScanPerThread, parity ^= 1) {
        uint32_t nl[kTileScanPerThread], ex[kTileScanPerThread];
        const unsigned first = t0 + tid * kTileScanPerThread;
        const bool whole = first + kTileScanPerThread <= a.n_tiles;
        if (whole) {
            const uint4* q = reinterpret_cast<const uint4*>(a.max_n_processed + first);        // 64 contiguous bytes
#pragma unroll
            for (int k = 0; k < kTileScanPerThread / 4; ++k) {
                const uint4 m = q[k];
                nl[4 * k] = (m.x + kBucket - 1) / kBucket; nl[4 * k + 1] = (m.y + kBucket - 1) / kBucket;   // live buckets of the tile (kb:295)
                nl[4 * k + 2] = (m.z + kBucket - 1) / kBucket; nl[4 * k + 3] = (m.w + kBucket - 1) / kBucket;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kTileScanPerThread; ++k) nl[k] = first + k < a.n_tiles ? (a.max_n_processed[first + k] + kBucket - 1) / kBucket : 0u;
        }
        const uint32_t total = tile_scan_pass(nl, ex, s_scan, base, parity);
        if (whole) {
            uint4* o = reinterpret_cast<uint4*>(a.live_offsets + first);
#pragma unroll
            for (int k = 0; k < kTileScanPerThread / 4; ++k) o[k] = make_uint4(ex[4 * k], ex[4 * k + 1], ex[4 * k + 2], ex[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < kTileScanPerThread; ++k) if (first + k < a.n_tiles) a.live_offsets[first + k] = ex[k];
        }
        base += total;
    }
    if (tid == 0) *a.live_count = base;
}

#ifndef FGS_K11_WAVES_PER_GROUP
#define FGS_K11_WAVES_PER_GROUP 1
#endif
constexpr unsigned kCompactWaves = FGS_K11_WAVES_PER_GROUP;      // independent waves (one work item each, no barrier) per workgroup
// DEPTH (blend_backward_compact_kernel<true>, fgs_backward_aux): alpha and expected depth are two more channels of the blend (per-Gaussian value 1
// resp. z, background 0), and the walk is linear in (channel value x upstream gradient): the per-pair dot becomes cg = c . gC + z gD + gA, the
// injected scalar was enlarged by the staging above, and dL/dalpha -- with it the eight geometry sums -- picks both up unchanged. One new sum,
// a_z = sum w gD = dL/dz, leaves through one float atomic per lane into acc_z (hot Gaussians: into the tile's replica, like their records).
// gD and gA ride in the pixel-centre ring, which becomes a 16-byte ring (x, y, gD, gA) read with one ds_read_b128 like the dL/dC ring:
// [xy ring 4 KB | inj 1.5 KB | pix ring 4 KB] = 9 728 bytes per wave = eight allocation granules instead of six. Every DEPTH
// statement is under `if constexpr`, and `a` is the kernel argument itself: blend_backward_compact_kernel<false> compiles to the instructions the kernel had.
// ABS (blend_backward_compact_kernel<*, true>, fgs_backward_absgrad): the pair's share of dL/dmean2d is gx = 2 (ca t + cb u), gy = 2 (cb t + cc u); the record's
// words 0 and 1 are their SIGNED sums, factored out of the loop. Their absolute sums cannot be: two more accumulators per lane, a_ax += |ca t + cb u|,
// a_ay += |cb t + cc u| (the absolute value is a source modifier of the add; no select, no LDS traffic), doubled once at the end. They leave as a [64][2]
// block through the dead 16-byte ring behind the record block, two atomic instructions per item in which lane l adds word l & 1 of Gaussian
// 32 k + (l >> 1): 32 line requests per instruction by the line-request model below. With or without DEPTH; every ABS statement is under `if constexpr`.
template <bool DEPTH, bool ABS>
__global__ void __launch_bounds__(kWave * kCompactWaves) blend_backward_compact_kernel(const BackwardArgsOf<DEPTH, ABS> args) {
    const BlendBackwardArgs& a = blend_part(args);
    [[maybe_unused]] const BlendDepthPart& x = depth_part(args);       // DEPTH only
    [[maybe_unused]] const BlendAbsPart& y = abs_part(args);           // ABS only
    const unsigned lane = threadIdx.x & 63u, wave_in_group = threadIdx.x >> 6;
    // Per live pixel: (dL/dC rgb, rel_last as a float) in s_pix and the pixel centre (x, y) in s_xy; slot n_px = dead sentinel (rel 0).
    // Until here x | y << 8 | rel << 16 were packed in the fourth float: three v_cvt_f32_ubyte (4.3 cycles each, tools/valu_rate.hip) and two
    // adds of the tile origin per (pixel, Gaussian) step -- 14 % of the loop's instructions. The centre is x0 + small integer either way
    // (exact), so dx, dy and every result are bit-identical. TWO dense arrays, not one 32-byte slot: lane l reads slot (step - l), and with a
    // 32-byte lane stride the 16-byte read conflicts every 8 lanes and the 8-byte read four-fold -- SQ_LDS_BANK_CONFLICT 2.3 M -> 42.6 M
    // cycles per launch at S2, LDS busy 34 M -> 86 M, which ate the whole gain (profiles/archive/r02_pmc_k11_lds.txt). 6.7 KB of LDS per wave
    // instead of 5.1: no effect on this kernel up to 8.2 KB (profiles/archive/r02_k11_occupancy.txt).
    // Round 3: the two arrays are RINGS of kRing = 256 slots (live pixels in [0, n_px), sentinels with rel 0 behind them): lane l reads slot
    // (step - l) mod 256, which is a sentinel both before the lane's first pixel arrives (negative -> 193..255) and after its last one has
    // passed (n_px .. n_px + 62 <= 254). The per-step index arithmetic was five vector instructions (step - lane, + look-ahead, unsigned min
    // against n_px, two shifts for the two strides); on the ring it is three: the byte offset into the 8-byte ring walks by 8 and wraps
    // (add, and), the 16-byte ring's offset is one shift-add of it. ONE shared block per wave with the 8-byte ring at offset 0, so that its
    // address IS the ring offset (no base to add): [xy ring 2 KB | inj 1.5 KB | pix ring 4 KB] = 7 680 bytes = six LDS allocation granules
    // (1 280 bytes on this part: with 8 KB the timeline showed 17 waves per CU in flight, with 6.7 KB before the ring 19).
    constexpr unsigned kRing = 256;
    constexpr unsigned kXySlot = DEPTH ? 16u : 8u;
    constexpr unsigned kXyBytes = kRing * kXySlot, kInjBytes = kTilePixels * 8u, kPixBytes = kRing * 16u, kPixBase = kXyBytes + kInjBytes;
    static_assert(kPixBase % 16u == 0, "the 16-byte ring is 16-byte aligned");
    __shared__ __attribute__((aligned(16))) char s_block[kCompactWaves][kXyBytes + kInjBytes + kPixBytes];
    char* const s_base = s_block[wave_in_group];
    float2* const s_xy = reinterpret_cast<float2*>(s_base);
    float4* const s_pix = reinterpret_cast<float4*>(s_base + kPixBase);
    // T_ckpt, S - g_w of the live pixels: enters the pipeline at lane 0, which walks this array one slot per step -- and on into the bytes
    // behind it for the 63 (+ look-ahead) steps after the last pixel: what it reads there is never used, because every lane that the value
    // reaches sees a sentinel pixel (rel 0) in that step and contributes nothing, and the state registers are cleared per work item. Lanes
    // 1..63 read a zero in every step (slot 255 of the xy ring: always a sentinel), which makes "shift up by one lane, inject at lane 0" ONE
    // DPP-fused add per value (shifted-in zero at lane 0 + the lane's own read) instead of a DPP move plus a select.
    float2* const s_inj = reinterpret_cast<float2*>(s_base + kXyBytes);
    const unsigned n_live = *a.live_count;
    const float lane_f = static_cast<float>(lane);
    const bool lane0 = lane == 0;
    [[maybe_unused]] Camera cam;                                   // DEPTH: the depth row of w2c (wave-uniform scalar loads)
    if constexpr (DEPTH) { cam.r3[0] = x.w2c[8]; cam.r3[1] = x.w2c[9]; cam.r3[2] = x.w2c[10]; cam.r3[3] = x.w2c[11]; }
    // (round 6, measured and withdrawn: XCD x walking a contiguous eighth of the live list, so that the buckets of neighbouring tiles share an L2 --
    // K11 0.313 -> 0.319 ms at S2, layered scene 3.73 -> 3.80 ms: the kernel is bound by vector issue, and the bands unbalance the XCDs. profiles/r06_ab_k11_xcd_bands.txt)
    for (unsigned item = blockIdx.x * kCompactWaves + wave_in_group; item < n_live; item += gridDim.x * kCompactWaves) {            // wave-uniform
        FGS_K11_PROBE_ITEM_BEGIN();                         // debug probes (fgs_k11_probes.h): every FGS_K11_PROBE_ line is empty in the product build
        const uint2 work = a.work_list[item];
        const unsigned tile = work.x, tb = work.y;
        const uint2 range = a.ranges[tile];
        const unsigned tile_n = range.y - range.x;
        const unsigned bucket = (tile == 0 ? 0u : a.bucket_offsets[tile - 1]) + tb;
        const unsigned first_gaussian = tb * kBucket;

        const float x0 = static_cast<float>((tile % a.grid_w) * kTileW) + 0.5f;
        const float y0 = static_cast<float>((tile / a.grid_w) * kTileH) + 0.5f;
        // ---- stage the live pixels, compacted (kb:349-380) ----
        unsigned n_px = 0;
        {
            const float4* __restrict__ pix = a.pixrec + (size_t)tile * kTilePixels * 2;
            const float4* __restrict__ ck = a.ckpt + (size_t)bucket * kTilePixels;
            float4 g[kTilePixels / kWave], cst[kTilePixels / kWave], k[kTilePixels / kWave];
            [[maybe_unused]] float4 e[kTilePixels / kWave];                       // DEPTH: gD, gA, D_final, T_final
            [[maybe_unused]] float dk[kTilePixels / kWave];                       // DEPTH: the running depth sum at the checkpoint
#pragma unroll
            for (int c = 0; c < kTilePixels / kWave; ++c) {                        // all nine loads in flight together
                const unsigned p = static_cast<unsigned>(c) * kWave + lane;
                g[c] = pix[2 * p]; cst[c] = pix[2 * p + 1];
                if constexpr (DEPTH) {
                    e[c] = x.pixaux[(size_t)tile * kTilePixels + p];
                    dk[c] = x.ckpt_d != nullptr ? load_float_nt(x.ckpt_d + (size_t)bucket * kTilePixels + p) : 0.0f;   // wave-uniform; without gD the term is 0 anyway
                }
#if FGS_CKPT_NT
                k[c] = load_float4_nt(reinterpret_cast<const float*>(ck + p));
#else
                k[c] = ck[p];
#endif
            }
#pragma unroll
            for (int c = 0; c < kTilePixels / kWave; ++c) {
                const unsigned p = static_cast<unsigned>(c) * kWave + lane;
                const unsigned last = __float_as_uint(cst[c].w);
                // a pixel that finished before this bucket never wrote its checkpoint (kf:436) and receives nothing here
                const bool live = last > first_gaussian;
                const uint64_t m = wave_ballot(live);
                FGS_K11_PROBE_LIVE_PIXELS(c, m);
                if (live) {
                    const unsigned slot = n_px + lanes_below(m);
                    const unsigned rel = min(last - first_gaussian, static_cast<unsigned>(kBucket));
                    s_pix[slot] = make_float4(g[c].x, g[c].y, g[c].z, static_cast<float>(rel));
                    if constexpr (DEPTH) reinterpret_cast<float4*>(s_base)[slot] = make_float4(x0 + static_cast<float>(p & (kTileW - 1)), y0 + static_cast<float>(p / kTileW), e[c].x, e[c].y);
                    else s_xy[slot] = make_float2(x0 + static_cast<float>(p & (kTileW - 1)), y0 + static_cast<float>(p / kTileW));
                    float S = (cst[c].x - k[c].x) * g[c].x + (cst[c].y - k[c].y) * g[c].y + (cst[c].z - k[c].z) * g[c].z;   // kb:371-374
                    if constexpr (DEPTH) S += e[c].x * (e[c].z - dk[c]) + e[c].y * (k[c].w - e[c].w);          // gD (D_final - D_ckpt) + gA (T_ckpt - T_final)
                    s_inj[slot] = make_float2(k[c].w, S - g[c].w);
                }
                n_px += static_cast<unsigned>(__popcll(m));
            }
            for (unsigned sl = n_px + lane; sl < kRing; sl += kWave) {          // sentinels (rel_last 0: never contributes): 1 to 4 rounds
                s_pix[sl] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if constexpr (DEPTH) reinterpret_cast<float4*>(s_base)[sl] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                else s_xy[sl] = make_float2(0.0f, 0.0f);
            }

        }

        const unsigned tp = first_gaussian + lane;
        const bool valid_prim = tp < tile_n;
        uint32_t prim = 0;
        float mx = 0.0f, my = 0.0f, ca = 0.0f, cb = 0.0f, cc = 0.0f, op = 0.0f;
        float col0 = 0.0f, col1 = 0.0f, col2 = 0.0f, f0 = 0.0f, f1 = 0.0f, f2 = 0.0f;
        unsigned footprint = 0;               // candidate tiles of this lane's Gaussian
        uint32_t hot_slot_word = 0;
        [[maybe_unused]] float z = 0.0f;      // DEPTH: view-space depth of this lane's Gaussian
        if (valid_prim) {
            prim = a.inst_prims[range.x + tp];
            if constexpr (DEPTH) { const float* m = x.means + 3 * (size_t)prim; z = view_depth(cam, m[0], m[1], m[2]); }
            const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
            const float4 r0 = r[0], r1 = r[1];
            const float4 r2 = r[2];
            const float raw2 = r2.x;
            mx = r0.x; my = r0.y; ca = r0.z; cb = r0.w; cc = r1.x; op = r1.y;
            col0 = fmaxf(r1.z, 0.0f); col1 = fmaxf(r1.w, 0.0f); col2 = fmaxf(raw2, 0.0f);
            f0 = r1.z >= 0.0f ? 1.0f : 0.0f; f1 = r1.w >= 0.0f ? 1.0f : 0.0f; f2 = raw2 >= 0.0f ? 1.0f : 0.0f;   // kb:313-318
            unsigned tx0, tx1, ty0, ty1;
            tile_rect(__float_as_uint(r2.y), __float_as_uint(r2.z), tx0, tx1, ty0, ty1);
            footprint = (tx1 - tx0) * (ty1 - ty0);
            hot_slot_word = __float_as_uint(r2.w);
        }
        FGS_K11_PROBE_BUCKET_BOUNDS(a, tile, lane, valid_prim, prim);
        wave_lds_fence();
        // alpha is recomputed with the FORWARD kernel's expression, operation for operation (kf:455-466 / kb:415-418; blend_forward.hip): the
        // backward pass replays the forward pass's alpha bit for bit, so both passes agree on every alpha >= 1/255 decision and the
        // transmittance rebuilt here is the one the forward pass used. (Round 3 first folded log2(e) and the -1/2 into per-lane constants --
        // five instructions and a bare v_exp_f32 instead of eight: 1 % of this kernel -- at the price of an alpha that differed from the
        // forward pass's by a rounding; a wide fuzz sweep in the simulator then showed a (pixel, Gaussian) pair blended by one pass and
        // skipped by the other.)
        float a_c0 = 0.0f, a_c1 = 0.0f, a_c2 = 0.0f;                 // sum w g_c               (kb:426-427 without the clamp gate)
        float a_h = 0.0f, a_x = 0.0f, a_y = 0.0f;                     // sum hh, sum hh dx, sum hh dy
        float a_xx = 0.0f, a_xy = 0.0f, a_yy = 0.0f;                  // sum hh dx^2, hh dx dy, hh dy^2   (kb:443-448)
        float sT = 0.0f, sS = 0.0f;                                   // the pixel state travelling through the lanes
        [[maybe_unused]] float a_z = 0.0f;                            // DEPTH: sum w gD = dL/dz
        [[maybe_unused]] float a_ax = 0.0f, a_ay = 0.0f;              // ABS: sum |ca t + cb u|, sum |cb t + cc u|

        // One pipeline step. `inj` / `px`: what this lane read for THIS step (software pipelined: the reads of the following step
        // are issued first). Contributions are made under the lane mask of `contrib` (EXEC), not by selects: a v_cndmask costs
        // several times an FMA on this chip (tools/valu_rate.hip), and the empty-mask branch of the `if` is the wave-uniform skip.
        unsigned inj_at = lane0 ? kXyBytes : (kRing - 1u) * kXySlot;  // byte offsets: lane 0 the slot of the step, other lanes the zero slot
        const unsigned inj_step = lane0 ? 8u : 0u;
        // byte offset into the 8-byte ring of the slot this lane reads for the step whose reads are issued next: (step - lane) mod 256
        unsigned ring_at = ((0u - lane) & (kRing - 1u)) * 8u;
        struct PixRead { float4 g; float2 xy; float gd, ga; };
        auto read_inj = [&]() { const float2 v = *reinterpret_cast<const float2*>(s_base + inj_at); inj_at += inj_step; return v; };
        auto read_pix = [&]() {
            PixRead r;
            if constexpr (DEPTH) {
                const float4 v = *reinterpret_cast<const float4*>(s_base + 2u * ring_at);
                r.xy = make_float2(v.x, v.y); r.gd = v.z; r.ga = v.w;
            } else {
                r.xy = *reinterpret_cast<const float2*>(s_base + ring_at);
                r.gd = 0.0f; r.ga = 0.0f;
            }
            r.g = *reinterpret_cast<const float4*>(s_base + (2u * ring_at + kPixBase));
            ring_at = (ring_at + 8u) & (kRing * 8u - 1u);
            return r;
        };
        auto step = [&](const float2 inj, const PixRead pr) {
            sT = wave_shift_up1_zero(sT) + inj.x;                                               // kb:383-410
            sS = wave_shift_up1_zero(sS) + inj.y;
            const float4 px = pr.g;
            const float rel = px.w;
            const float dx = mx - pr.xy.x, dy = my - pr.xy.y;
            const float power = -0.5f * (ca * dx * dx + cc * dy * dy) - cb * dx * dy;
            const float alpha = op * __expf(fminf(power, 0.0f));
            FGS_K11_PROBE_STEP(lane_f, rel, alpha);
            if (lane_f < rel && alpha >= kMinAlphaThreshold) {                                  // kb:412,419-421
                const float T = sT;
                const float w = T * alpha;
                a_c0 += w * px.x; a_c1 += w * px.y; a_c2 += w * px.z;
                float cg = col0 * px.x + col1 * px.y + col2 * px.z;
                if constexpr (DEPTH) { cg += z * pr.gd + pr.ga; a_z += w * pr.gd; }
                sS -= w * cg;                                                                    // kb:429 projected on dL/dC
                const float oma = 1.0f - alpha;
                const float oma_rcp = fast_rcp(fmaxf(oma, kOneMinusAlphaEps));
                const float dl_dalpha = T * cg - sS * oma_rcp;                                   // kb:434-436
                const float hh = (-0.5f * alpha) * dl_dalpha;
                const float t = hh * dx, u = hh * dy;
                a_h += hh; a_x += t; a_y += u;
                a_xx += t * dx; a_xy += t * dy; a_yy += u * dy;
                if constexpr (ABS) { a_ax += fabsf(ca * t + cb * u); a_ay += fabsf(cb * t + cc * u); }
                sT = T * oma;
            }
        };
        // two steps per trip with the read registers ping-ponged (no copies); an odd step count runs one extra step in which every
        // lane sees the sentinel
        float2 inj_a = read_inj(), inj_b;
        PixRead pix_a = read_pix(), pix_b;
        const int n_steps = (FGS_ABLATE(a) & 2) ? 0 : static_cast<int>(n_px) + kWave - 1;
        for (int i = 0; i < n_steps; i += 2) {
            inj_b = read_inj(); pix_b = read_pix();
            step(inj_a, pix_a);
            inj_a = read_inj(); pix_a = read_pix();
            step(inj_b, pix_b);
        }

        // A Gaussian whose nine sums are all zero has nothing to add (it never passed the alpha test, or only at pixels with a zero
        // image gradient).
        const bool silent = a_h == 0.0f && a_c0 == 0.0f && a_c1 == 0.0f && a_c2 == 0.0f && a_x == 0.0f && a_y == 0.0f
                            && a_xx == 0.0f && a_xy == 0.0f && a_yy == 0.0f && (!DEPTH || a_z == 0.0f);
        if (!(FGS_ABLATE(a) & 1)) {                                                              // kb:459-470
            // The nine sums of a Gaussian leave as its RECORD of nine consecutive floats, SEVEN Gaussians per atomic instruction (lane l of
            // instruction k adds word 63 k + l of the bucket's 64 x 9 block, transposed through the LDS the rings no longer need). Round 4: the
            // memory pipeline merges the lanes of one atomic instruction that fall into one 128-byte line and is bound by LINE requests, about
            // 20 000 per microsecond whatever they carry (tools/atomic_rate.hip: 64 scattered floats 20.8 k atomics / us, 64 consecutive ones 278 k).
            // With one plane per sum (rounds 1-3) an item cost 9 instructions x as many lines as its 64 primitives are scattered over: hidden
            // behind the arithmetic on a Morton-ordered synthetic scene, HALF of this kernel's time on a model trained under the MCMC policy
            // (1.56 -> 0.81 ms, profiles/r04_k11_record_atomics.txt). Now: ~1.3 lines per Gaussian, 10 instructions per item.
            // dL/dopacity = sum G dL/dalpha with G = alpha / opacity; through the sigmoid unless proper antialiasing (kb:462-466)
            const float v5 = a.proper_aa ? -2.0f * a_h / op : -2.0f * a_h * (1.0f - op);
            const float v0 = 2.0f * (ca * a_x + cb * a_y), v1 = 2.0f * (cb * a_x + cc * a_y);
            const uint32_t hot_word = footprint > kHotFootprint ? hot_slot_word : 0u;
            const bool adds = valid_prim && !silent;
            // float offset of the record from a.acc: the Gaussian's own record, or -- a hot Gaussian (fgs_config.h) -- the record of its slot in the
            // tile's replica (acc_hot follows acc in the scratch blob: [kHotReplicas][kMaxHot][9])
            const uint32_t rec_off = hot_word != 0u ? static_cast<uint32_t>(a.acc_hot - a.acc) + ((tile % kHotReplicas) * kMaxHot + (hot_word - 1u)) * kAccRecordWords
                                                    : prim * kAccRecordWords;
            float* const s_t = reinterpret_cast<float*>(s_base + kPixBase);                      // [64][9] in the dead 16-byte ring
            uint32_t* const s_off = reinterpret_cast<uint32_t*>(s_base);                         // record offset of each lane's Gaussian, or "nothing to add"
            constexpr uint32_t kNoRecord = 0xffffffffu;
            wave_lds_fence();                                                                     // the loop's last ring reads are done
            float* const mine = s_t + lane * kAccRecordWords;
            mine[0] = v0; mine[1] = v1; mine[2] = a_xx; mine[3] = a_xy; mine[4] = a_yy; mine[5] = v5;
            mine[6] = a_c0 * f0; mine[7] = a_c1 * f1; mine[8] = a_c2 * f2;
            s_off[lane] = adds ? rec_off : kNoRecord;
            [[maybe_unused]] float* const s_ab = s_t + kBucket * kAccRecordWords;               // ABS: [64][2] behind the record block (2 304 + 512 of the ring's 4 096 bytes)
            [[maybe_unused]] uint32_t* const s_aoff = s_off + kBucket;                           // ABS: float offset of each lane's pair from acc_abs, or "nothing to add"
            if constexpr (ABS) {
                static_assert((kBucket * (kAccRecordWords + 2)) * 4u <= kPixBytes && 2u * kBucket * 4u <= kXyBytes, "both blocks fit the dead rings");
                const float ax = 2.0f * a_ax, ay = 2.0f * a_ay;
                s_ab[2u * lane] = ax; s_ab[2u * lane + 1u] = ay;
                // the Gaussian's own pair, or -- a hot Gaussian -- the pair of its slot in the tile's replica (acc_abs_hot follows acc_abs in the scratch blob)
                const uint32_t abs_off = hot_word != 0u ? static_cast<uint32_t>(y.acc_abs_hot - y.acc_abs) + ((tile % kHotReplicas) * kMaxHot + (hot_word - 1u)) * 2u
                                                        : prim * 2u;
                s_aoff[lane] = (valid_prim && (ax != 0.0f || ay != 0.0f)) ? abs_off : kNoRecord;
            }
            wave_lds_fence();
            const unsigned sub = lane / kAccRecordWords, comp = lane - sub * kAccRecordWords;     // lane 63 idles: 7 records of 9 words per instruction
#pragma unroll
            for (unsigned k = 0; k < (kBucket + 6u) / 7u; ++k) {
                const unsigned gsn = 7u * k + sub;
                if (lane < 63u && gsn < static_cast<unsigned>(kBucket)) {
                    const uint32_t rec = s_off[gsn];
                    if (rec != kNoRecord) unsafeAtomicAdd(a.acc + (size_t)rec + comp, s_t[63u * k + lane]);
                }
            }
            if constexpr (DEPTH) {        // dL/dz leaves on its own: one float per lane that has something to add
                if (valid_prim && a_z != 0.0f)
                    unsafeAtomicAdd(hot_word != 0u ? x.acc_z_hot + ((size_t)(tile % kHotReplicas) * kMaxHot + (hot_word - 1u)) : x.acc_z + prim, a_z);
            }
            if constexpr (ABS) {          // the two absolute sums: 32 Gaussians per instruction, a Gaussian's two words in neighbouring lanes (one line)
#pragma unroll
                for (unsigned k = 0; k < 2u; ++k) {
                    const unsigned gsn = 32u * k + (lane >> 1);
                    const uint32_t off = s_aoff[gsn];
                    if (off != kNoRecord) unsafeAtomicAdd(y.acc_abs + (size_t)off + (lane & 1u), s_ab[2u * gsn + (lane & 1u)]);
                }
            }
        }
        FGS_K11_PROBE_ITEM_END(lane, item, n_steps);
        wave_lds_fence();                                  // the next item restages the LDS slices
    }
}

// after K11: the hot Gaussians' replicas are summed and added to their records (one thread per (slot, sum))
__global__ void __launch_bounds__(256) fold_hot_accumulators_kernel(const BlendBackwardArgs a) {
    const unsigned n_hot = min(*a.hot_count, kMaxHot);
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    // this is K11's last kernel (K12 reads the records after it): the accumulator records now hold sums -- a second backward pass over the same
    // buffers (a retained graph) must clear them itself (stage_pixels_kernel reads the flag)
    if (e == 0u) *a.dirty_flag = 1u;
    const unsigned slot = e / kAccRecordWords, k = e % kAccRecordWords;          // consecutive threads: the nine sums of a slot, then the next slot
    if (slot >= n_hot) return;
    float sum = 0.0f;
#pragma unroll
    for (unsigned r = 0; r < kHotReplicas; ++r) sum += a.acc_hot[((size_t)r * kMaxHot + slot) * kAccRecordWords + k];
    if (sum != 0.0f) a.acc[(size_t)a.hot_list[slot] * kAccRecordWords + k] += sum;      // one slot per primitive: no other writer at this point
}
// the same for dL/dz of a depth backward pass: one thread per hot slot
__global__ void __launch_bounds__(256) fold_hot_depth_kernel(const BlendBackwardDepthArgs a) {
    const unsigned n_hot = min(*a.blend.hot_count, kMaxHot);
    const unsigned slot = blockIdx.x * 256u + threadIdx.x;
    if (slot >= n_hot) return;
    float sum = 0.0f;
#pragma unroll
    for (unsigned r = 0; r < kHotReplicas; ++r) sum += a.d.acc_z_hot[(size_t)r * kMaxHot + slot];
    if (sum != 0.0f) a.d.acc_z[a.blend.hot_list[slot]] += sum;                          // one slot per primitive: no other writer at this point
}
// the same for the absolute sums of an absgrad backward pass: one thread per (hot slot, word)
__global__ void __launch_bounds__(256) fold_hot_abs_kernel(const BlendAbsPart y, const uint32_t* __restrict__ hot_list, const uint32_t* __restrict__ hot_count) {
    const unsigned n_hot = min(*hot_count, kMaxHot);
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    const unsigned slot = e >> 1, k = e & 1u;
    if (slot >= n_hot) return;
    float sum = 0.0f;
#pragma unroll
    for (unsigned r = 0; r < kHotReplicas; ++r) sum += y.acc_abs_hot[((size_t)r * kMaxHot + slot) * 2u + k];
    if (sum != 0.0f) y.acc_abs[(size_t)hot_list[slot] * 2u + k] += sum;                 // one slot per primitive: no other writer at this point
}
// after K12 (which has written every element of grad_means): z_i = w2c[2, 0:3] . mean_i + w2c[2, 3], so dL/dmean_i += dL/dz_i w2c[2, 0:3]
__global__ void __launch_bounds__(256) depth_mean_gradient_kernel(const float* __restrict__ acc_z, const uint32_t* __restrict__ n_touched,
                                                                  const float* __restrict__ w2c, float* __restrict__ grad_means, const uint32_t n) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || n_touched[i] == 0u) return;
    const float g = acc_z[i];
    if (g == 0.0f) return;
    grad_means[3 * (size_t)i] += g * w2c[8]; grad_means[3 * (size_t)i + 1] += g * w2c[9]; grad_means[3 * (size_t)i + 2] += g * w2c[10];
}

// after K12, which is not touched: the absolute-gradient densification statistic of the visible Gaussians, in the arithmetic of the signed one
// (preprocess_backward.hip, kb:194-201). Unreached visible Gaussians count in row 0; += sqrt(0) on row 1 is exact and omitted.
__global__ void __launch_bounds__(256) abs_densification_kernel(const float* __restrict__ acc_abs, const uint32_t* __restrict__ n_touched,
                                                                float* __restrict__ info, const uint32_t n, const float width, const float height) {
#pragma clang fp contract(off)          // nx nx + ny ny rounds as in K12, whose unit is built without contraction
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || n_touched[i] == 0u) return;
    info[i] += 1.0f;
    const float ax = acc_abs[2 * (size_t)i], ay = acc_abs[2 * (size_t)i + 1];
    if (ax == 0.0f && ay == 0.0f) return;
    const float nx = 0.5f * (ax * width), ny = 0.5f * (ay * height);
    info[n + i] += sqrtf(nx * nx + ny * ny);
}

#ifdef FGS_DEV_SWITCHES
__global__ void mark_accumulators_dirty_kernel(uint32_t* flag) { *flag = 1u; }      // the A/B variants that do not end in the fold kernel
std::atomic<int> g_backward_variant{3};   // 3 (default): work list + compacted pixels + two-value state; 2: systolic over all buckets / all 192 pixels, dL/dC from
                              // global memory (round 1: 0.70 ms at S2); 0: same with dL/dC in LDS (0.74); 1: strip (lane = pixel, 0.85 ms);
                              // 4: lane = pixel on the matrix cores; 5: chained -- all but 3 in blend_backward_exhibits.hip; fgs_debug_set_backward_variant()
int blend_backward_variant() { return g_backward_variant.load(); }
#else
int blend_backward_variant() { return 3; }     // the product build has one formulation
#endif

// a.variant: read ONCE per backward pass by the caller (api.hip: run_blend_backward) -- the planning pass and the kernel must agree on it
hipError_t launch_stage_pixels(const BlendBackwardArgs& a_in, hipStream_t s) {
    BlendBackwardArgs a = a_in;
    if (a.variant >= 3 && a.n_buckets_cap != 0) hipLaunchKernelGGL(plan_blend_backward_kernel, dim3(1), dim3(kTileScanThreads), 0, s, a);
    else a.live_offsets = nullptr;                            // the other variants walk all buckets: no list
    hipLaunchKernelGGL((stage_pixels_kernel<false, false>), dim3(a.n_tiles), dim3(kTilePixels), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend_backward(const BlendBackwardArgs& a_in, hipStream_t s) {
    if (a_in.n_buckets_cap == 0) return hipSuccess;
    BlendBackwardArgs a = a_in;
#ifdef FGS_DEV_SWITCHES
    a.ablate = g_backward_ablate;
    if (a.variant != 3) {        // an A/B exhibit (blend_backward_exhibits.hip), then the kernel of this unit that ends its pass
        launch_blend_backward_exhibit(a, s);
        if (a.variant >= 4) hipLaunchKernelGGL(fold_hot_accumulators_kernel, dim3(9u * kMaxHot / 256u), dim3(256), 0, s, a);   // 4 / 5 use the hot replicas
        else hipLaunchKernelGGL(mark_accumulators_dirty_kernel, dim3(1), dim3(1), 0, s, a.dirty_flag);                          // 0 / 1 / 2 do not
        return hipGetLastError();
    }
#endif
    // grid-stride over the live list: at most 64 Ki single-wave workgroups, so a scene with few live buckets does not pay
    // for the launch of a quarter of a million empty ones
    const unsigned blocks = a.n_buckets_cap < kBackwardMaxBlocks ? a.n_buckets_cap : kBackwardMaxBlocks;
    hipLaunchKernelGGL((blend_backward_compact_kernel<false, false>), dim3((blocks + kCompactWaves - 1) / kCompactWaves), dim3(kWave * kCompactWaves), 0, s, a);
    hipLaunchKernelGGL(fold_hot_accumulators_kernel, dim3(9u * kMaxHot / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}

// The depth forms: always the product formulation (the exhibit variants of the dev library have no depth form)
hipError_t launch_stage_pixels_depth(const BlendBackwardDepthArgs& a_in, hipStream_t s) {
    BlendBackwardDepthArgs a = a_in;
    a.blend.variant = 3;
    if (a.blend.n_buckets_cap != 0) hipLaunchKernelGGL(plan_blend_backward_kernel, dim3(1), dim3(kTileScanThreads), 0, s, a.blend);
    else a.blend.live_offsets = nullptr;
    hipLaunchKernelGGL((stage_pixels_kernel<true, false>), dim3(a.blend.n_tiles), dim3(kTilePixels), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend_backward_depth(const BlendBackwardDepthArgs& a_in, hipStream_t s) {
    if (a_in.blend.n_buckets_cap == 0) return hipSuccess;
    BlendBackwardDepthArgs a = a_in;
    a.blend.variant = 3; a.blend.ablate = 0;
    const unsigned blocks = a.blend.n_buckets_cap < kBackwardMaxBlocks ? a.blend.n_buckets_cap : kBackwardMaxBlocks;
    hipLaunchKernelGGL((blend_backward_compact_kernel<true, false>), dim3((blocks + kCompactWaves - 1) / kCompactWaves), dim3(kWave * kCompactWaves), 0, s, a);
    hipLaunchKernelGGL(fold_hot_accumulators_kernel, dim3(9u * kMaxHot / 256u), dim3(256), 0, s, a.blend);
    hipLaunchKernelGGL(fold_hot_depth_kernel, dim3(kMaxHot / 256u), dim3(256), 0, s, a);
    return hipGetLastError();
}

// The absgrad forms, without and with map gradients: the product formulation like the depth forms
template <class Args, bool DEPTH>
static hipError_t stage_pixels_abs(const Args& a_in, hipStream_t s) {
    Args a = a_in;
    a.blend.variant = 3;
    if (a.blend.n_buckets_cap != 0) hipLaunchKernelGGL(plan_blend_backward_kernel, dim3(1), dim3(kTileScanThreads), 0, s, a.blend);
    else a.blend.live_offsets = nullptr;
    hipLaunchKernelGGL((stage_pixels_kernel<DEPTH, true>), dim3(a.blend.n_tiles), dim3(kTilePixels), 0, s, a);
    return hipGetLastError();
}
template <class Args, bool DEPTH>
static hipError_t blend_backward_abs(const Args& a_in, hipStream_t s) {
    if (a_in.blend.n_buckets_cap == 0) return hipSuccess;
    Args a = a_in;
    a.blend.variant = 3; a.blend.ablate = 0;
    const unsigned blocks = a.blend.n_buckets_cap < kBackwardMaxBlocks ? a.blend.n_buckets_cap : kBackwardMaxBlocks;
    hipLaunchKernelGGL((blend_backward_compact_kernel<DEPTH, true>), dim3((blocks + kCompactWaves - 1) / kCompactWaves), dim3(kWave * kCompactWaves), 0, s, a);
    hipLaunchKernelGGL(fold_hot_accumulators_kernel, dim3(9u * kMaxHot / 256u), dim3(256), 0, s, a.blend);
    if constexpr (DEPTH) hipLaunchKernelGGL(fold_hot_depth_kernel, dim3(kMaxHot / 256u), dim3(256), 0, s, BlendBackwardDepthArgs{a.blend, a.d});
    hipLaunchKernelGGL(fold_hot_abs_kernel, dim3(2u * kMaxHot / 256u), dim3(256), 0, s, a.abs, a.blend.hot_list, a.blend.hot_count);
    return hipGetLastError();
}
hipError_t launch_stage_pixels_abs(const BlendBackwardAbsArgs& a, hipStream_t s) { return stage_pixels_abs<BlendBackwardAbsArgs, false>(a, s); }
hipError_t launch_blend_backward_abs(const BlendBackwardAbsArgs& a, hipStream_t s) { return blend_backward_abs<BlendBackwardAbsArgs, false>(a, s); }
hipError_t launch_stage_pixels_depth_abs(const BlendBackwardDepthAbsArgs& a, hipStream_t s) { return stage_pixels_abs<BlendBackwardDepthAbsArgs, true>(a, s); }
hipError_t launch_blend_backward_depth_abs(const BlendBackwardDepthAbsArgs& a, hipStream_t s) { return blend_backward_abs<BlendBackwardDepthAbsArgs, true>(a, s); }

hipError_t launch_abs_densification(const float* acc_abs, const uint32_t* n_touched, float* info, uint32_t n, float width, float height, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(abs_densification_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, acc_abs, n_touched, info, n, width, height);
    return hipGetLastError();
}

hipError_t launch_depth_mean_gradient(const float* acc_z, const uint32_t* n_touched, const float* w2c, float* grad_means, uint32_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(depth_mean_gradient_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, acc_z, n_touched, w2c, grad_means, n);
    return hipGetLastError();
}

}  // namespace fgs

// K10: per-tile front-to-back alpha blending for gfx950 (training variant with per-bucket checkpoints, and the
// forward-only inference variant). Semantics: reference kernels_forward.cuh:362-498 / kernels_inference.cuh:348-463.
//
// CDNA4 shape (not a translation of the 6-warp CUDA block):
//  * a 16x12 tile is 3 wave64; each wave owns a 16x4 strip = the two 8x4 sub-tiles of the reference side by side
//    (lanes 0-31 left, 32-63 right). The reference's per-sub-tile bounding-box cull is kept exactly: each lane tests one
//    of 64 staged Gaussians against BOTH sub-tiles, two 64-bit ballots give the per-half masks, the wave walks the union
//    with scalar bit ops and each half predicates on its own mask.
//  * Gaussians are staged 192 at a time through LDS from ONE 48-byte record per primitive (3 x 16-B loads from one line).
//  * checkpoints are written every kBucket=64 Gaussians (one backward wavefront) -- half the reference's checkpoint
//    traffic -- 1 KiB contiguous per wave; T_final / n_processed are tile-major so backward reads them coalesced.
//  * workgroup -> tile mapping keeps one vertical strip of the image on one XCD (workgroup b runs on XCD b % 8), so the
//    records gathered by neighbouring tiles stay in that XCD's 4 MiB L2 (fgs_k10_mappings.h: tile_of_workgroup).
#include <atomic>

#include "fgs_kernels.h"
#include <fgs_wave.h>
#include "fgs_k10_probes.h"      // FGS_K10_PROBE_*: empty unless a probe library is being built

#ifndef FGS_CKPT_NT
#define FGS_CKPT_NT 1      // round 6: K10's checkpoints -- written once, read once by K11 a millisecond later -- leave as non-temporal stores (training iteration 2.218 -> 2.187 ms, layered scene 3.728 -> 3.706, three alternating pairs: profiles/r06_ab_ckpt_nt.txt); 0: A/B
#endif
#include "fgs_k10_mappings.h"   // tile_of_workgroup, blend_grid: which tile a workgroup blends (BlendArgs::row_group; the product passes kColumnsTopDown)

namespace fgs {

// AUX (inference only, fgs_inference_aux): the same walk also yields per pixel the accumulated opacity 1 - T, the expected depth sum_i w_i z_i and the
// median depth (z of the last blended Gaussian met with T > 0.5), z = view_depth of the Gaussian's mean -- the value behind K1's depth key. z takes the
// seat of the record's hit_mask word in the staged third row, which the blend never reads: it is computed where the record is fetched (the staging and
// the read-ahead of the next batch alike) and rides to the walk with the colours. Every AUX statement is under `if (AUX)`, and the kernels keep their
// names: blend_kernel<true> and blend_kernel<false> compile to the instructions they had (the arguments go to the body BY VALUE: by reference the compiler
// lays the early return out differently), blend_aux_kernel is the third instantiation.
// TRAINING && AUX (fgs_forward_aux, blend_training_aux_kernel: the fourth instantiation) is the training blend that also returns accumulated opacity
// and expected depth for a backward pass: next to every (rgb, T) checkpoint it stores the pixel's running depth sum into the plane ckpt_d [B][192]
// (same condition, same bucket, non-temporal like the checkpoint), which is what K11 needs to start "the depth still to come" at a bucket's first
// Gaussian. No median here: it is piecewise constant and carries no gradient.
template <bool TRAINING, bool AUX>
__device__ __forceinline__ void blend_tile(const BlendArgs a, float* const ckpt_d = nullptr) {
    const unsigned tile = tile_of_workgroup(blockIdx.x, a.grid_w, a.n_tiles, a.row_group, a.tile_plan, a.grid_h);
    if (tile >= a.n_tiles) return;
    FGS_K10_PROBE_TILE_BEGIN()
    const unsigned tile_x = tile % a.grid_w, tile_y = tile / a.grid_w;
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, half = lane >> 5;
    const unsigned lx = half * kSubtileW + (lane & 7u), ly = wave * kSubtileH + ((lane >> 3) & 3u);
    const unsigned px = tile_x * kTileW + lx, py = tile_y * kTileH + ly;
    const bool inside = px < a.width && py < a.height;
    const unsigned local = ly * kTileW + lx;
    const float pxf = static_cast<float>(px) + 0.5f, pyf = static_cast<float>(py) + 0.5f;
    // sub-tile rectangles of this wave (kf:389-398)
    const unsigned sub_y0 = tile_y * kTileH + wave * kSubtileH, sub_y1 = sub_y0 + kSubtileH;
    const unsigned subl_x0 = tile_x * kTileW, subl_x1 = subl_x0 + kSubtileW, subr_x1 = subl_x1 + kSubtileW;

    const uint2 range = a.ranges[tile];
    const unsigned n_total = range.y - range.x;
    unsigned bucket_base = 0;
    if (TRAINING) {
        bucket_base = tile == 0 ? 0u : a.bucket_offsets[tile - 1];
        const unsigned nb = (n_total + kBucket - 1) / kBucket;
        for (unsigned b = tid; b < nb; b += kBlendBlock) a.bucket_tile[bucket_base + b] = tile;   // kf:407-411
    }

    __shared__ float4 s_rec[3 * kBlendBlock];                        // one array: the walk addresses all three rows off one register
    float4* const s_a = s_rec;                                        // mean.x mean.y conic.a conic.b
    float4* const s_b = s_rec + kBlendBlock;                          // conic.c opacity r g
    float4* const s_c = s_rec + 2 * kBlendBlock;                      // b bounds_x bounds_y -
    __shared__ unsigned s_max[kBlendBlock / kWave];

    float cr = 0.0f, cg = 0.0f, cb = 0.0f, T = 1.0f;
    float depth_sum = 0.0f, depth_med = 0.0f;                          // AUX
    Camera cam;                                                        // AUX: the third row of w2c is all view_depth reads (wave-uniform scalar loads)
    if (AUX) { cam.r3[0] = a.w2c[8]; cam.r3[1] = a.w2c[9]; cam.r3[2] = a.w2c[10]; cam.r3[3] = a.w2c[11]; }
    float gate = inside ? kMinAlphaThreshold : __builtin_inff();       // the alpha a pair has to reach to be blended (see the walk below)
    unsigned n_used = 0;
    // "done" (kf:424,477) is not carried as a flag: a pixel is finished exactly when its transmittance has dropped below the threshold
    // (T only ever decreases and the flag is set right after the update that takes it there), or when it lies outside the image. A
    // divergent flag carried through the per-Gaussian loop lives in a scalar register pair that has to be merged after every
    // conditional update (three scalar instructions per merge), and this loop is bound by the ONE scalar unit of the CU.
#define FGS_PIXEL_DONE (!inside || T < kTransmittanceThreshold)

    // Deep tiles fetch ahead: from its second batch on (a tile that needs one has proved to be deep; at S2 a tile walks ~100 of its ~1 500 entries and
    // never gets here) the records of the NEXT batch are loaded into registers while this batch is walked, and the primitive indices of the one after
    // that, so that the two dependent global round trips of the staging (index -> record, ~3 us per batch with the SIMD to itself) leave the serial
    // path of a long list -- the tail of K10 on object-centric / trained scenes (tools/k10_timeline.py).
    float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, n2 = n0;      // records of the next batch (have_next)
    uint32_t prim_ahead = 0;                                           // primitive of the batch after next (have_ahead)
    bool have_next = false, have_ahead = false;                        // workgroup-uniform
    for (unsigned batch_start = 0; batch_start < n_total; batch_start += kBlendBlock) {
        if (__syncthreads_and(FGS_PIXEL_DONE ? 1 : 0)) break;                          // kf:424
        const unsigned batch = min(static_cast<unsigned>(kBlendBlock), n_total - batch_start);
        if (tid < batch) {
            float4 r0, r1, r2;
            if (have_next) { r0 = n0; r1 = n1; r2 = n2; }
            else {
                const uint32_t prim = a.inst_prims[range.x + batch_start + tid];
                const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
                r0 = r[0]; r1 = r[1]; r2 = r[2];
                if (AUX) { const float* m = a.means + 3 * (size_t)prim; r2.w = view_depth(cam, m[0], m[1], m[2]); }
            }
            s_a[tid] = r0;
            if (TRAINING) {                                                            // kf:430 (inference clamps at store, ki:200)
                s_b[tid] = make_float4(r1.x, r1.y, fmaxf(r1.z, 0.0f), fmaxf(r1.w, 0.0f));
                s_c[tid] = make_float4(fmaxf(r2.x, 0.0f), r2.y, r2.z, AUX ? r2.w : 0.0f);
            } else {
                s_b[tid] = r1;
                s_c[tid] = r2;
            }
        }
        __syncthreads();
        {
            const unsigned next_start = batch_start + kBlendBlock, after_start = next_start + kBlendBlock;
            const bool had_ahead = have_ahead;
            have_next = batch_start >= static_cast<unsigned>(kBlendBlock) && next_start < n_total;
            have_ahead = have_next && after_start < n_total;
            if (have_next && next_start + tid < n_total) {
                const uint32_t prim = had_ahead ? prim_ahead : a.inst_prims[range.x + next_start + tid];
                const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
                n0 = r[0]; n1 = r[1]; n2 = r[2];
                if (AUX) { const float* m = a.means + 3 * (size_t)prim; n2.w = view_depth(cam, m[0], m[1], m[2]); }
            }
            if (have_ahead && after_start + tid < n_total) prim_ahead = a.inst_prims[range.x + after_start + tid];
        }
        for (unsigned chunk = 0; chunk < batch; chunk += kBucket) {
            const bool done = FGS_PIXEL_DONE;
            if (TRAINING && !done)                                                     // kf:436-442, every 64 instead of 32
#if FGS_CKPT_NT
                store_float4_nt(reinterpret_cast<float*>(a.ckpt + (size_t)(bucket_base + (batch_start + chunk) / kBucket) * kTilePixels + local), make_float4(cr, cg, cb, T));
#else
                a.ckpt[(size_t)(bucket_base + (batch_start + chunk) / kBucket) * kTilePixels + local] = make_float4(cr, cg, cb, T);
#endif
            if (TRAINING && AUX && !done) store_float_nt(ckpt_d + (size_t)(bucket_base + (batch_start + chunk) / kBucket) * kTilePixels + local, depth_sum);
            bool in_l = false, in_r = false;
            const unsigned j = chunk + lane;
            if (j < batch) {                                                           // kf:445-450
                const uint32_t bx = __float_as_uint(s_c[j].y), by = __float_as_uint(s_c[j].z);
                const unsigned x_min = bx & 0xffffu, x_max = bx >> 16, y_min = by & 0xffffu, y_max = by >> 16;
                const bool in_y = y_min < sub_y1 && sub_y0 < y_max;
                in_l = in_y && x_min < subl_x1 && subl_x0 < x_max;
                in_r = in_y && x_min < subr_x1 && subl_x1 < x_max;
            }
            const uint64_t mask_l = wave_ballot(in_l), mask_r = wave_ballot(in_r);
            const uint64_t mine = inside ? (half ? mask_r : mask_l) : 0ull;            // pixels outside the image never blend
            uint64_t pending = mask_l | mask_r;
            if (wave_ballot(!done) == 0) pending = 0;
            FGS_K10_PROBE_CHUNK(wave, done, batch, chunk)
            // The walk over the set bits saturates the scalar unit (ONE per CU for four SIMDs; rocprofv3 on the layered scene, round 2:
            // SQ_INSTS_SALU = SQ_INSTS_VALU = 457 M per launch), so every test of a (pixel, Gaussian) pair is ONE vector compare:
            //  * the 64-bit list is walked as two bit-reversed 32-bit words from the top (count-leading-zeros / clear on single registers);
            //  * "this Gaussian overlaps my sub-tile" (kf:445-451): the lane's complemented, reversed word shifted left by the same count
            //    has its sign bit set exactly when it does NOT, and that bit is OR-ed into alpha -- a negative alpha fails the alpha test;
            //  * "pixel not finished" (kf:424,477) is folded into the threshold: `gate` is 1/255 (kf:467) while the pixel is alive and
            //    +inf from the update that takes T below the threshold (or outside the image), refreshed where T changes.
            // Three compares, two scalar ANDs and a 64-bit vector shift before; the arithmetic is untouched (bit-identical images).
#pragma unroll
            for (unsigned word = 0; word < 2u; ++word) {
                uint32_t pend = __brev(static_cast<uint32_t>(word ? pending >> 32 : pending));
                const uint32_t not_mine = __brev(~static_cast<uint32_t>(word ? mine >> 32 : mine));
                const unsigned j0 = chunk + 32u * word;
                const unsigned row0 = in_vector_register(j0 * 16u);                     // byte offset of entry j0, kept out of the scalar unit
                // Two list entries per trip, their six LDS reads issued together in front of the first use: left to itself the compiler reads the
                // colours inside the blend branch -- a second LDS round trip per blended entry on the serial path of a long list. The two alphas are
                // independent chains, only the conditional blends are serial. Measured (tools/ab_k10_mapping.py, one box): S2 0.144 -> 0.140 ms,
                // layered 0.600 -> 0.590, bench.py's surface scene (lists of thousands walked by a few tiles at the end of the kernel) 0.387 -> 0.357;
                // three or four entries per trip are slower everywhere (0.156 / 0.162 ms at S2: the control flow, not the LDS, is what a trip pays).
                while (pend != 0) {                                                    // wave-uniform scalar loop
                    const unsigned k = static_cast<unsigned>(__clz(static_cast<int>(pend)));
                    pend &= ~(0x80000000u >> k);
                    const bool second = pend != 0u;                                    // wave-uniform
                    const unsigned k2 = second ? static_cast<unsigned>(__clz(static_cast<int>(pend))) : k;
                    pend &= ~(0x80000000u >> k2);
                    const float4* const entry = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_rec) + (row0 + (k << 4)));
                    const float4* const entry2 = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(s_rec) + (row0 + (k2 << 4)));
                    float4 ga = entry[0], gb = entry[kBlendBlock];
                    float4 ha = entry2[0], hb = entry2[kBlendBlock];
                    float blue = entry[2 * kBlendBlock].x, blue2 = entry2[2 * kBlendBlock].x;
                    asm volatile("" : "+v"(gb.z), "+v"(gb.w), "+v"(blue), "+v"(hb.z), "+v"(hb.w), "+v"(blue2), "+v"(ha.x), "+v"(hb.x));
                    float z = 0.0f, z2 = 0.0f;
                    if (AUX) { z = entry[2 * kBlendBlock].w; z2 = entry2[2 * kBlendBlock].w; asm volatile("" : "+v"(z), "+v"(z2)); }   // read ahead of the branch like the colours
                    const float dx = ga.x - pxf, dy = ga.y - pyf;
                    const float ex = ha.x - pxf, ey = ha.y - pyf;
                    const float power = -0.5f * (ga.z * dx * dx + gb.x * dy * dy) - ga.w * dx * dy;
                    const float power2 = -0.5f * (ha.z * ex * ex + hb.x * ey * ey) - ha.w * ex * ey;
                    const float gauss = __expf(fminf(power, 0.0f));
                    const float gauss2 = __expf(fminf(power2, 0.0f));
                    const float alpha = gb.y * gauss;
                    const float alpha2 = hb.y * gauss2;
                    const float tested = __uint_as_float(((not_mine << k) & 0x80000000u) | __float_as_uint(alpha));
                    const float tested2 = __uint_as_float(((not_mine << k2) & 0x80000000u) | __float_as_uint(alpha2));
                    FGS_K10_PROBE_TRIP(second)
                    FGS_K10_PROBE_ENTRY(not_mine, k, gate, tested)
                    if (tested >= gate) {
                        const float w = T * alpha;
                        cr += w * gb.z; cg += w * gb.w; cb += w * blue;
                        if (AUX) { depth_sum += w * z; if (!TRAINING) depth_med = T > 0.5f ? z : depth_med; }   // T before this Gaussian: a select, no mask merge
                        T *= 1.0f - alpha;
                        gate = T < kTransmittanceThreshold ? __builtin_inff() : gate;
                        n_used = batch_start + j0 + k + 1;                             // kf:474
                    }
                    if (second) {
                        FGS_K10_PROBE_ENTRY(not_mine, k2, gate, tested2)
                        if (tested2 >= gate) {
                            const float w = T * alpha2;
                            cr += w * hb.z; cg += w * hb.w; cb += w * blue2;
                            if (AUX) { depth_sum += w * z2; if (!TRAINING) depth_med = T > 0.5f ? z2 : depth_med; }
                            T *= 1.0f - alpha2;
                            gate = T < kTransmittanceThreshold ? __builtin_inff() : gate;
                            n_used = batch_start + j0 + k2 + 1;
                        }
                    }
                }
            }
        }
    }
#undef FGS_PIXEL_DONE

    if (inside) {
        cr += T * a.bg[0]; cg += T * a.bg[1]; cb += T * a.bg[2];                      // kf:483
        const size_t pix = (size_t)a.width * py + px;
        if (AUX) {                                                                     // image-linear [H,W]; the background is no part of them
            if (a.aux_alpha != nullptr) a.aux_alpha[pix] = 1.0f - T;
            if (a.aux_depth != nullptr) a.aux_depth[pix] = depth_sum;
            if (!TRAINING && a.aux_median != nullptr) a.aux_median[pix] = depth_med;
        }
        const size_t n_pixels = (size_t)a.width * a.height;
        if (TRAINING) {
            a.image[pix] = cr; a.image[n_pixels + pix] = cg; a.image[2 * n_pixels + pix] = cb;
        } else {
            if (a.clamp_output) { cr = saturate_f(cr); cg = saturate_f(cg); cb = saturate_f(cb); }   // ki:445-449
            if (a.to_chw) { a.image[pix] = cr; a.image[n_pixels + pix] = cg; a.image[2 * n_pixels + pix] = cb; }
            else { a.image[3 * pix] = cr; a.image[3 * pix + 1] = cg; a.image[3 * pix + 2] = cb; }
        }
    }
    if (TRAINING) {
        // tile-major (the reference indexes these image-linear, kf:485-491; they are private to the backend)
        a.final_T[(size_t)tile * kTilePixels + local] = T;
        a.n_processed[(size_t)tile * kTilePixels + local] = n_used;                    // 0 for pixels outside the image
        const unsigned wmax = wave_max(n_used);
        if (lane == 0) s_max[wave] = wmax;
        __syncthreads();
        if (tid == 0) a.max_n_processed[tile] = max(s_max[0], max(s_max[1], s_max[2]));   // kf:493-497
    }
    FGS_K10_PROBE_TILE_END(TRAINING, tid, wave, lane, tile, n_total)
}

template <bool TRAINING>
__global__ void __launch_bounds__(kBlendBlock) blend_kernel(const BlendArgs a) { blend_tile<TRAINING, false>(a); }
__global__ void __launch_bounds__(kBlendBlock) blend_aux_kernel(const BlendArgs a) { blend_tile<false, true>(a); }
__global__ void __launch_bounds__(kBlendBlock) blend_training_aux_kernel(const BlendDepthArgs a) { blend_tile<true, true>(a.blend, a.ckpt_d); }

// Speedy-Splat pruning scores (kernels_pruning_scores.cuh:348-505): the tile list is blended twice -- pass 1
// for the final colour / transmittance, pass 2 re-walks it with dL/dC = 1 and adds (opacity * dL/dalpha)^2 of every blended
// (pixel, Gaussian) pair to scores[primitive]. Same wave64 strip / two-sub-tile cull as blend_kernel. The reference issues
// one atomicAdd per (pixel, Gaussian) pair (kp:490); here the 64 lanes of a wave evaluate the SAME Gaussian, so their
// scores are summed with 6 DPP adds and leave through one atomic per (Gaussian, wave).
__global__ void __launch_bounds__(kBlendBlock) pruning_scores_kernel(const BlendArgs a) {
    const unsigned tile = tile_of_workgroup(blockIdx.x, a.grid_w, a.n_tiles, a.row_group, a.tile_plan, a.grid_h);
    if (tile >= a.n_tiles) return;
    const unsigned tile_x = tile % a.grid_w, tile_y = tile / a.grid_w;
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, half = lane >> 5;
    const unsigned lx = half * kSubtileW + (lane & 7u), ly = wave * kSubtileH + ((lane >> 3) & 3u);
    const unsigned px = tile_x * kTileW + lx, py = tile_y * kTileH + ly;
    const bool inside = px < a.width && py < a.height;
    const float pxf = static_cast<float>(px) + 0.5f, pyf = static_cast<float>(py) + 0.5f;
    const unsigned sub_y0 = tile_y * kTileH + wave * kSubtileH, sub_y1 = sub_y0 + kSubtileH;
    const unsigned subl_x0 = tile_x * kTileW, subl_x1 = subl_x0 + kSubtileW, subr_x1 = subl_x1 + kSubtileW;
    const uint2 range = a.ranges[tile];
    const unsigned n_total = range.y - range.x;

    __shared__ float4 s_a[kBlendBlock], s_b[kBlendBlock], s_c[kBlendBlock];
    __shared__ uint32_t s_prim[kBlendBlock];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, T = 1.0f, galpha = 0.0f;

    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) { galpha = T * -(a.bg[0] + a.bg[1] + a.bg[2]); T = 1.0f; }                 // kp:441-444
        // "done" derived from T as in blend_kernel (the loop is bound by the scalar unit; a carried divergent flag costs scalar merges)
#define FGS_PIXEL_DONE (!inside || T < kTransmittanceThreshold)
        for (unsigned batch_start = 0; batch_start < n_total; batch_start += kBlendBlock) {
            if (__syncthreads_and(FGS_PIXEL_DONE ? 1 : 0)) break;
            const unsigned batch = min(static_cast<unsigned>(kBlendBlock), n_total - batch_start);
            if (tid < batch) {
                const uint32_t prim = a.inst_prims[range.x + batch_start + tid];
                const float4* r = reinterpret_cast<const float4*>(a.rec + prim);
                s_a[tid] = r[0]; s_b[tid] = r[1]; s_c[tid] = r[2]; s_prim[tid] = prim;
            }
            __syncthreads();
            for (unsigned chunk = 0; chunk < batch; chunk += kWave) {
                bool in_l = false, in_r = false;
                const unsigned j = chunk + lane;
                if (j < batch) {
                    const uint32_t bx = __float_as_uint(s_c[j].y), by = __float_as_uint(s_c[j].z);
                    const unsigned x_min = bx & 0xffffu, x_max = bx >> 16, y_min = by & 0xffffu, y_max = by >> 16;
                    const bool in_y = y_min < sub_y1 && sub_y0 < y_max;
                    in_l = in_y && x_min < subl_x1 && subl_x0 < x_max;
                    in_r = in_y && x_min < subr_x1 && subl_x1 < x_max;
                }
                const uint64_t mask_l = wave_ballot(in_l), mask_r = wave_ballot(in_r);
                const uint64_t mine = half ? mask_r : mask_l;
                uint64_t pending = mask_l | mask_r;
                if (wave_ballot(!FGS_PIXEL_DONE) == 0) pending = 0;
                while (pending != 0) {
                    const int k = __ffsll(static_cast<unsigned long long>(pending)) - 1;
                    pending &= pending - 1;
                    const unsigned jj = chunk + static_cast<unsigned>(k);
                    const float4 ga = s_a[jj], gb = s_b[jj];
                    const float col2 = s_c[jj].x;
                    const float dx = ga.x - pxf, dy = ga.y - pyf;
                    const float power = -0.5f * (ga.z * dx * dx + gb.x * dy * dy) - ga.w * dx * dy;
                    const float alpha = gb.y * __expf(fminf(power, 0.0f));
                    const bool contrib = inside && ((mine >> k) & 1ull) != 0 && T >= kTransmittanceThreshold && alpha >= kMinAlphaThreshold;
                    float score = 0.0f;
                    if (contrib) {
                        const float w = T * alpha;
                        if (pass == 0) { c0 += w * gb.z; c1 += w * gb.w; c2 += w * col2; }
                        else {
                            c0 -= w * gb.z; c1 -= w * gb.w; c2 -= w * col2;                          // kp:477
                            const float rcp = fast_rcp(fmaxf(1.0f - alpha, kOneMinusAlphaEps));
                            const float dl_dalpha = ((T * gb.z - c0 * rcp) + (T * gb.w - c1 * rcp) + (T * col2 - c2 * rcp)) + galpha * rcp;
                            const float dl_dg = gb.y * dl_dalpha;
                            score = dl_dg * dl_dg;                                                   // kp:487-488
                        }
                        T *= 1.0f - alpha;
                    }
                    if (pass == 1 && wave_ballot(contrib) != 0) {                                   // wave-uniform
                        const float total = wave_sum_to_lane63(score);
                        if (lane == 63u) unsafeAtomicAdd(a.scores + s_prim[jj], total);             // kp:490, one per (Gaussian, wave)
                    }
                }
            }
        }
    }
#undef FGS_PIXEL_DONE
}

// The launchers: one workgroup per tile and the mapping's padding (blend_grid). The mapping itself is the caller's (BlendArgs::row_group).
hipError_t launch_pruning_scores(const BlendArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(pruning_scores_kernel, dim3(blend_grid(a)), dim3(kBlendBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend(bool training, const BlendArgs& a, hipStream_t s) {
    const dim3 grid(blend_grid(a)), block(kBlendBlock);
    if (training) hipLaunchKernelGGL(blend_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(blend_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend_aux(const BlendArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(blend_aux_kernel, dim3(blend_grid(a)), dim3(kBlendBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_blend_training_aux(const BlendDepthArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(blend_training_aux_kernel, dim3(blend_grid(a.blend)), dim3(kBlendBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace fgs

// Launch interface between the C-ABI host layer (api*.hip, fgs_host.h) and the gfx950 kernels. One launcher per pipeline stage;
// stage ids K0..K13 refer to SURVEY.md section 2.1.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "fgs_config.h"
#include "fgs_math.h"

namespace fgs {

struct PreprocessArgs {                 // K1
    const float* means; const float* scales; const float* rotations; const float* opacities;
    const float* sh0; const float* sh_rest;
    PrimRec* rec; uint32_t* n_touched;
    uint32_t* depth_keys; uint32_t* prim_idx;     // compacted (unsorted) visible list
    uint4* foot;                                   // footprint row of every entry of that list (fgs_math.h), or nullptr (sharded owner: no sort behind K1)
    uint32_t* counters;                            // [0] n_visible, [1] n_instances (one packed 64-bit word), [2] K5 work list, [3] huge list, [4] hot slots
    uint32_t* huge_list;                           // indices of footprints > kHugeFootprint candidate tiles (counted by a second kernel)
    uint32_t* hot_list;                            // [kMaxHot] primitive index of hot-accumulator slot s (counters[4] = slots handed out)
    uint2* ranges; uint32_t n_tiles;               // cleared by the kernel (K0)
    float* acc;                                    // training: K11's accumulator records [N][9]; K1 clears those of the Gaussians it finds visible (else nullptr)
    uint32_t n;
    int seq_tiles;                                 // dev library: candidate tiles each lane tests itself before the wave cooperates (1..32, fgs_k1_exhibits.h); 0 = the flattened count
    int count_appended;                            // sharded path: counters[2] counts the huge-footprint entries appended to the list
    CameraArgs cam;
};
hipError_t launch_preprocess(bool inference, const PreprocessArgs& a, hipStream_t s);
// sharded path: the same Gaussians projected for up to kMaxBatchViews cameras in ONE launch (grid.y = view); a shard is too
// small to fill the chip per view (3 M / 8 Gaussians = 733 workgroups) and 8 back-to-back launches measured 2.2x the time
struct PreprocessBatch { int n_views; PreprocessArgs v[kMaxBatchViews]; };
hipError_t launch_preprocess_batch(const PreprocessBatch& b, hipStream_t s);

// K2-K4: depth sort of the visible list + exclusive scan of per-primitive tile counts in depth order
// depth keys lie in [bits(near), bits(far)] (kf:67): the depth sort orders key - base in `bits` bits (radix_sort.hip)
struct DepthKeyRange { uint32_t base; int bits; };
DepthKeyRange depth_key_range(float near_plane, float far_plane);
size_t depth_sort_temp_bytes(uint32_t n);
// `n_visible` = the visible count, or with n_visible_ptr != nullptr a bound of the count stored there on the device (the sort reads it there: it
// can be enqueued before the host knows the count). foot[0] = the footprint rows in compaction order (K1), foot[1] receives them in depth order,
// tile_counts their tile counts in depth order; vals[selector] = the primitives in depth order.
hipError_t run_depth_sort(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n_visible,
                          const uint32_t* n_visible_ptr, DepthKeyRange range, uint4* foot[2], uint32_t* tile_counts,
                          uint32_t* big_list, uint32_t* big_count, hipStream_t s);
// K3 + K4: sums of the depth-ordered tile counts per 64-Gaussian wave segment (wave_sums[ceil(n / 64)]) and per 4096-Gaussian block
// (block_sums[ceil(n / 4096)]). K5 derives every Gaussian's first output slot from them.
// n_visible_ptr != nullptr: n_visible is a bound (the primitive count) and the exact count is read on the device
hipError_t launch_tile_count_sums(const uint32_t* tile_counts, uint32_t* wave_sums, uint32_t* block_sums,
                                  uint32_t n_visible, const uint32_t* n_visible_ptr, hipStream_t s);

// K5-K7: instance creation, tile sort, per-tile ranges. key_bytes is 2 (<= 65536 tiles) or 4.
size_t tile_sort_temp_bytes(uint32_t n_instances, int key_bytes, int end_bit);
// The *_ptr forms serve the host-synchronisation-free forward pass: counts are bounds / capacities, the exact ones are read on the device
// (n_visible from counters[0]; the instance count clamped to `capacity` is written to counters[5], an overflow flag to counters[6]).
hipError_t launch_create_instances(int key_bytes, const uint4* foot_sorted, const uint32_t* wave_sums,
                                   const uint32_t* block_sums, uint32_t* offsets,
                                   const PrimRec* rec, void* inst_keys, uint32_t* inst_prims, uint32_t grid_w, uint32_t n_visible,
                                   const uint32_t* n_visible_ptr, uint32_t capacity, uint32_t* counters,
                                   const uint32_t* big_list, const uint32_t* big_count, hipStream_t s);
hipError_t run_tile_sort(void* temp, size_t temp_bytes, int key_bytes, void* keys[2], uint32_t* vals[2], int& selector,
                         uint32_t n_instances, const uint32_t* n_instances_ptr, int end_bit, hipStream_t s);
hipError_t launch_extract_ranges(int key_bytes, const void* sorted_keys, uint2* ranges, uint32_t n_instances, const uint32_t* n_instances_ptr, hipStream_t s);

// A/B switches. libfgs_hip_dev.so (-DFGS_DEV_SWITCHES) has them as process-wide atomics behind fgs_debug_set_option (api_debug.hip, the one switchboard)
// for the A/B tools; atomics make a concurrent set / launch well defined (a launch sees the old or the new value, never a torn one). The product library
// has none of them -- nothing process-wide can change what a launch does -- but for the one its host code still reads, g_fused_single_kernel, which is a
// compile-time constant there (its adopted value). Each switch names the dev-only file that holds its other arms.
#ifdef FGS_DEV_SWITCHES
#define FGS_SWITCH(name, value) inline std::atomic<int> name{value}
#else
#define FGS_SWITCH(name, value) constexpr int name = (value)
#endif
// K10's tile -> workgroup mappings (fgs_k10_mappings.h), the values of BlendArgs::row_group (0: the round-1 bands, 1..64: row groups, 255: the bands
// bottom first). The product library always runs the first; the dev library selects among all of them (option 10).
constexpr unsigned kColumnsTopDown = 252u, kColumnsBottomUp = 251u;   // one vertical strip of the image per XCD, walked row by row
constexpr unsigned kPlannedBlocks = 254u;            // the device-side block plan (binning_exhibits.hip: plan_tiles_kernel)
constexpr unsigned kBandsThroughPlan = 253u;         // A/B only: the round-1 bands, but with the plan's dependent load on every workgroup's path
#ifdef FGS_DEV_SWITCHES
FGS_SWITCH(g_tile_row_group, static_cast<int>(kColumnsTopDown));   // option 10: the mapping of the next forward pass (api.hip: bucket_scan_and_mapping)
FGS_SWITCH(g_library_bucket_scan, 0);                // option 11: 1 = rocPRIM scan for K8+K9 and no tile plan (round-2 form, A/B)
FGS_SWITCH(g_plan_experiment, 0);                    // binning_exhibits.hip, option 12: 1 = blocks unsorted and dealt statically (A/B of the deal itself)
FGS_SWITCH(g_k11_chain_waves, 4096);                 // blend_backward_exhibits.hip, option 14: waves of the chained K11 exhibit (variant 5); 4096 = 16 resident waves x 256 CUs
FGS_SWITCH(g_seq_tiles, kSeqTiles);                  // fgs_k1_exhibits.h, option 5: PreprocessArgs::seq_tiles of every K1 launch (0: the product's flattened count)
FGS_SWITCH(g_depth_sort_mode, 1);                    // sort_exhibits.hip, option 9 -- bit 0: key range / 9-bit digits, bit 1: 2048-item workgroups; 1 = the product's sort
FGS_SWITCH(g_adam_reverse, 1);                       // adam.hip (launch_adam_exhibit), option 8: reversed workgroup order
FGS_SWITCH(g_adam_nontemporal, 1);                   // same, option 2: non-temporal loads / stores
FGS_SWITCH(g_adam_unroll, 1);                        // same, option 1: 1, 2 or 4 float4 pieces per thread (plain loads / stores only)
FGS_SWITCH(g_loss_form, 0);                          // loss_exhibits.hip, option 16 -- bit 0: the tiled forward loss kernel, bit 1: the tiled backward one; 0 = the product's streaming kernels
#endif
FGS_SWITCH(g_fused_single_kernel, 1);                // option 3: K12 / fused K12+K13 of the single-GPU path as one kernel (1) or as round 1's two (0)
FGS_SWITCH(g_adam_span, 1);                          // adam.hip, option 15: chunks a workgroup of K13 walks one after the other, 1..32 (above 1: costed and not built, profiles/adam_spans.txt)
// radix_sort.hip: stable LSD radix sort of (key, uint32) pairs sized for these two sorts
size_t own_sort_temp_bytes(uint32_t n, int end_bit);
// Side table carried out of the depth sort's LAST scatter pass (radix_sort.hip): the sort's values start as the input positions (the first pass
// makes them up), the last pass gathers rows_in[value] and writes the row, its first word as the sorted value, and the row's tile count in sorted order.
struct SortPayload { const uint4* rows_in; uint4* rows_out; uint32_t* count_out; int iota_values;
                     uint32_t* big_list; uint32_t* big_count; };      // depth-order positions of the rows whose boxes exceed kBigInstanceFootprint candidates
hipError_t own_depth_sort(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n, const uint32_t* n_ptr,
                          DepthKeyRange range, hipStream_t s, const SortPayload* payload = nullptr);
#ifdef FGS_DEV_SWITCHES      // sort_exhibits.hip: the depth sort under option 9 != 1 (true: it ran, `result` is its error code)
bool depth_sort_exhibit(hipError_t& result, void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n,
                        const uint32_t* n_ptr, DepthKeyRange range, hipStream_t s, const SortPayload* payload);
#endif
hipError_t own_sort_pairs_u32(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n, int end_bit, hipStream_t s);
hipError_t own_sort_pairs_u16(void* temp, size_t temp_bytes, uint16_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n, int end_bit, hipStream_t s);
// the item count lives on the device (*n_ptr <= capacity): lets the depth sort start before the host has read the counters back
hipError_t own_sort_pairs_u32_device_count(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t capacity,
                                           const uint32_t* n_ptr, int end_bit, hipStream_t s);
hipError_t own_sort_pairs_u16_device_count(void* temp, size_t temp_bytes, uint16_t* keys[2], uint32_t* vals[2], int& selector, uint32_t capacity,
                                           const uint32_t* n_ptr, int end_bit, hipStream_t s);

// K8+K9: inclusive scan of ceil(len/kBucket) per tile (one single-workgroup kernel). tile_plan: nullptr -- always, in the product library -- or, dev
// library, where the same launch also leaves K10's tile -> workgroup plan [kPlanWords] (binning_exhibits.hip)
hipError_t launch_plan_tiles(const uint2* ranges, uint32_t* bucket_offsets, uint32_t* tile_plan, uint32_t n_tiles, uint32_t grid_w, uint32_t grid_h,
                             hipStream_t s);
#ifdef FGS_DEV_SWITCHES      // binning_exhibits.hip
hipError_t launch_plan_tiles_exhibit(const uint2* ranges, uint32_t* bucket_offsets, uint32_t* tile_plan, uint32_t n_tiles, uint32_t grid_w, uint32_t grid_h,
                                     hipStream_t s);      // the scan, then the plan (tile_plan != nullptr)
size_t bucket_scan_temp_bytes(uint32_t n_tiles);      // the library scan, kept for A/B (fgs_debug_set_option(11, 1))
hipError_t run_bucket_scan(void* temp, size_t temp_bytes, const uint2* ranges, uint32_t* bucket_offsets, uint32_t n_tiles, hipStream_t s);
#endif

struct BlendArgs {                      // K10 / inference blend
    const uint2* ranges; const uint32_t* bucket_offsets; const uint32_t* inst_prims; const PrimRec* rec;
    const float* bg; float* image;
    float* final_T; uint32_t* n_processed; uint32_t* max_n_processed;     // tile-major [T][192]
    uint32_t* bucket_tile; float4* ckpt;                                   // [B], [B][192]
    uint32_t width, height, grid_w, n_tiles;
    // row_group and tile_plan vary in the dev library alone (fgs_k10_mappings.h); the product library always passes kColumnsTopDown and no plan. One
    // kernel-argument layout for both flavours.
    uint32_t row_group;                      // tile -> workgroup mapping, set by the caller (api.hip: once per pass)
    const uint32_t* tile_plan;               // [kPlanWords] written by plan_tiles_kernel; nullptr unless the mapping reads it (kPlannedBlocks, kBandsThroughPlan)
    uint32_t grid_h;
    int to_chw, clamp_output;
    float* scores;                        // pruning-score mode: accumulated per primitive [N]
    // auxiliary maps of the inference blend (launch_blend_aux): image-linear [H,W], each may be nullptr; means [N][3] and w2c (row 2 = the depth row) give z
    const float* means; const float* w2c;
    float* aux_alpha; float* aux_depth; float* aux_median;
};
hipError_t launch_blend(bool training, const BlendArgs& a, hipStream_t s);
hipError_t launch_blend_aux(const BlendArgs& a, hipStream_t s);       // the inference blend + accumulated opacity / expected depth / median depth
hipError_t launch_pruning_scores(const BlendArgs& a, hipStream_t s);   // kernels_pruning_scores.cuh:348-505
// The training blend that also writes accumulated opacity / expected depth (blend.aux_alpha / aux_depth, either may be nullptr; means and w2c give z)
// and, beside every checkpoint, the pixel's running depth sum: ckpt_d [B][192]. A struct of its own: BlendArgs, and with it the kernel-argument
// block of the three other blends, stays what it is.
struct BlendDepthArgs { BlendArgs blend; float* ckpt_d; };
hipError_t launch_blend_training_aux(const BlendDepthArgs& a, hipStream_t s);

struct BlendBackwardArgs {              // K11 (+ per-pixel staging pass)
    const uint2* ranges; const uint32_t* bucket_offsets; const uint32_t* inst_prims; const PrimRec* rec;
    const float* bg; const float* grad_image; const float* image;
    const float* final_T; const uint32_t* n_processed; const uint32_t* max_n_processed;
    const uint32_t* bucket_tile; const float4* ckpt;
    float4* pixrec;                       // [T][192][2] staged per-pixel constants
    float* acc;                           // records [N][9]: d/d(mean2d.x, mean2d.y, conic a,b,c, opacity, colour r,g,b) of each Gaussian, nine consecutive floats
    float* acc_hot;                       // [kHotReplicas][kMaxHot][9]: private records of the hot Gaussians; follows acc in the scratch blob (K11 addresses both as float offsets from acc)
    const uint32_t* hot_list; const uint32_t* hot_count;   // slot -> primitive, number of slots handed out (may exceed kMaxHot)
    uint2* work_list; uint32_t* live_count;   // variant 3: (tile, bucket in tile) of every live bucket and their number
    uint32_t* live_offsets;                   // [T] first list slot of each tile (planning pass -> stage_pixels_kernel)
    uint32_t n, width, height, grid_w, n_tiles, n_buckets_cap;
    // what the staging pass sets to zero: the hot replicas (clear_hot_f4 16-byte pieces from acc_hot), or -- `clear_everything`, or *dirty_flag != 0 --
    // records and replicas (clear_all_f4 pieces from acc). K1 cleared the records of the visible Gaussians during the forward pass (api.hip: run_forward).
    uint32_t clear_all_f4, clear_hot_f4; int clear_everything;
    uint32_t* dirty_flag;                 // counters[7]: set by the last kernel of a backward pass over these buffers
    int proper_aa;
    int ablate;                           // dev build only: timing experiments (fgs_debug_set_option key 7)
    int variant;                          // K11 formulation, read once per backward pass (blend_backward_variant(); 3 in the product build)
};
hipError_t launch_stage_pixels(const BlendBackwardArgs& a, hipStream_t s);      // per-pixel staging pass
hipError_t launch_blend_backward(const BlendBackwardArgs& a, hipStream_t s);    // K11 proper
// K11 with upstream gradients of the accumulated opacity A = 1 - T_final and the expected depth D = sum w z (fgs_backward_aux). Both are two more
// channels of the blend -- value 1 resp. z per Gaussian, background 0 -- so they fold into the per-pair dot and the remaining-colour scalar; the one
// new per-Gaussian sum is dL/dz = sum_pixels w gD. The additions travel in a struct of their own: BlendBackwardArgs stays byte for byte what it is.
struct BlendDepthPart {
    const float* grad_alpha; const float* grad_depth;   // [H,W] image-linear, each may be nullptr (= zero)
    const float* depth;                                  // [H,W] the forward pass's expected depth (D_final); read only with grad_depth
    const float* ckpt_d;                                 // [B][192] running depth sum at every checkpoint (launch_blend_training_aux); read only with grad_depth
    float4* pixaux;                                      // [T][192] staged (gD, gA, D_final, T_final)
    const float* means; const float* w2c;                // z of a Gaussian = view_depth(mean): row 2 of w2c
    float* acc_z;                                        // [N] dL/dz, followed by the hot Gaussians' replicas acc_z_hot [kHotReplicas][kMaxHot]; both cleared by the staging pass
    float* acc_z_hot;
    uint32_t clear_z_f4;                                 // 16-byte pieces from acc_z to the end of acc_z_hot
};
struct BlendBackwardDepthArgs { BlendBackwardArgs blend; BlendDepthPart d; };
hipError_t launch_stage_pixels_depth(const BlendBackwardDepthArgs& a, hipStream_t s);
hipError_t launch_blend_backward_depth(const BlendBackwardDepthArgs& a, hipStream_t s);   // always the product formulation (compact), then both folds
// after K12: grad_means[i] += acc_z[i] * w2c[2, 0:3] for the Gaussians with n_touched != 0 -- all that z_i's own dependence on mean_i contributes
hipError_t launch_depth_mean_gradient(const float* acc_z, const uint32_t* n_touched, const float* w2c, float* grad_means, uint32_t n, hipStream_t s);
// K11 that also sums the ABSOLUTE per-pixel shares of dL/dmean2d (fgs_backward_absgrad): ax_i = sum_p |gx_p|, ay_i = sum_p |gy_p| over the pairs that
// contribute, gx_p = 2 (ca t + cb u), gy_p = 2 (cb t + cc u) -- the terms whose signed sums are words 0 and 1 of the record. Two more per-Gaussian sums
// that ride along like dL/dz; they travel in a struct of their own behind the plain or the depth arguments, which stay byte for byte what they are.
struct BlendAbsPart {
    float* acc_abs;                                      // [N][2] (ax, ay) interleaved, followed by the hot Gaussians' replicas; both cleared by the staging pass
    float* acc_abs_hot;                                  // [kHotReplicas][kMaxHot][2] (K11 addresses both as 32-bit float offsets from acc_abs)
    uint32_t clear_abs_f4;                               // 16-byte pieces from acc_abs to the end of acc_abs_hot
};
struct BlendBackwardAbsArgs { BlendBackwardArgs blend; BlendAbsPart abs; };
struct BlendBackwardDepthAbsArgs { BlendBackwardArgs blend; BlendDepthPart d; BlendAbsPart abs; };
// always the product formulation (compact), then the folds (records, dL/dz with depth arguments, the absolute sums)
hipError_t launch_stage_pixels_abs(const BlendBackwardAbsArgs& a, hipStream_t s);
hipError_t launch_blend_backward_abs(const BlendBackwardAbsArgs& a, hipStream_t s);
hipError_t launch_stage_pixels_depth_abs(const BlendBackwardDepthAbsArgs& a, hipStream_t s);
hipError_t launch_blend_backward_depth_abs(const BlendBackwardDepthAbsArgs& a, hipStream_t s);
// after K12: for the Gaussians with n_touched != 0, info[i] += 1 and info[n + i] += sqrt((0.5 W ax_i)^2 + (0.5 H ay_i)^2) (info: float [2][N])
hipError_t launch_abs_densification(const float* acc_abs, const uint32_t* n_touched, float* info, uint32_t n, float width, float height, hipStream_t s);

// blend_features.hip: F per-Gaussian feature channels blended with the compositing weights of a completed training forward pass (fgs_blend_features),
// and the backward pass of that blend (fgs_backward_features), which runs between K11 and K12. Both walk the tile lists K10 built, bounded per
// pixel by n_processed.
constexpr int kMaxFeatureChannels = 64;
struct FeatureBlendArgs {
    const uint2* ranges; const uint32_t* inst_prims; const PrimRec* rec;
    const uint32_t* n_processed; const uint32_t* max_n_processed;          // tile-major [T][192], [T]: what K10 left
    const float* features;                // [N][F]
    float* feature_map;                   // forward: [F][H][W], every element written
    const float* feature_map_in;          // backward: the forward pass's map
    const float* grad_feature_map;        // backward: [F][H][W]
    float* grad_features;                 // backward: [N][F], zero at launch, added to with float atomics
    float* acc;                           // backward: K11's accumulator records [N][9]; words 0..5 are added to unless detach_geometry
    uint32_t n_channels, width, height, grid_w, grid_h, n_tiles;
    int proper_aa, detach_geometry;
};
hipError_t launch_blend_features(const FeatureBlendArgs& a, hipStream_t s);
hipError_t launch_blend_features_backward(const FeatureBlendArgs& a, hipStream_t s);

struct AdamHyper { float step_size, beta1, beta2, eps, bc2_sqrt_rcp; };

struct BackwardView {                   // what K12 needs per camera view (one on the single-GPU path, up to kMaxBatchViews on the sharded path)
    CameraArgs cam;
    const uint32_t* n_touched;            // [N] tile count of the view, 0 = invisible
    const float* acc;                     // single view: records [N][9] (K11's accumulators). Sharded path (several views per launch):
    const uint32_t* slot;                 //   the returned 9-float accumulator RECORDS, that of visible primitive i being record slot[i]
    float* view_dir;                      // [N][3] scratch: unit view direction of visible primitives, consumed by the SH-rest pass
    const float* acc_z;                   // depth-supervised pass: [N] dL/dz (BlendDepthPart::acc_z), part of K12's "did K11 reach it" test; else nullptr
};
struct PreprocessBackwardArgs {         // K12, optionally fused with K13 for the 14 non-SH-rest floats
    const float* means; const float* scales; const float* rotations; const float* opacities; const float* sh_rest;
    float* grad_means; float* grad_scales; float* grad_rotations; float* grad_opacities; float* grad_sh0;
    float* densification_info;
    uint32_t n;
    int accumulate;                       // unfused only: add into grad_* for visible primitives instead of writing every element
    int n_views; BackwardView view[kMaxBatchViews];   // gradients are summed over the views in registers
    // fused mode (grad_* unused, one view): parameters and moments updated in place, order means, sh0, opacities, scales, rotations
    float* p[5]; float* m[5]; float* v[5]; AdamHyper h[5];
    // single-kernel unfused form only: [ceil(n / 64)] bytes or nullptr -- 1 if any Gaussian of the block 64 b .. 64 b + 63 is visible, 0 if the
    // block's gradients are all zero (they are still written); lets the optimizer skip the read of those zeros (launch_adam)
    uint8_t* live_blocks;
    // same form, same size, or nullptr -- 1 if K11 REACHED some Gaussian of the block (gaussian_backward's test, dL/dz of a depth-supervised pass included),
    // 0 if every row of the block is +-0 in all six gradient tensors: invisible blocks and the visible ones hidden behind opaque Gaussians
    uint8_t* reached_blocks;
    // same form, same size, or nullptr -- the caller's promise going IN: 0 = every element of the block's rows compares equal to 0.0f in all six gradient
    // tensors as they are now (e.g. the reached_blocks of the pass that last wrote these tensors); a wave that reaches no Gaussian then stores nothing,
    // provided the block's first element of each tensor agrees (backward_gradients_kernel: block_promised_zero)
    const uint8_t* prior_blocks;
    int vector_ok;                        // set by the launchers: every per-Gaussian tensor of the call is 16-byte aligned (coalesced 16-byte phase A)
};
hipError_t launch_preprocess_backward(bool fused_adam, const PreprocessBackwardArgs& a, hipStream_t s);

struct ShRestView { const float* view_dir; const uint32_t* n_touched; const float* acc; const uint32_t* slot; };   // acc / slot as in BackwardView
struct ShRestArgs {                     // the 45/59 of the per-Gaussian payload, streamed flat and fully coalesced
    int n_views; ShRestView view[kMaxBatchViews];    // n_views > 1 or a slot table = the sharded path (records found through the slot table), else K11's own records [N][9]
    float* grad_sh_rest;                  // unfused: [N][K-1][3] written for every primitive
    float* p; float* m; float* v; AdamHyper h;   // fused (one view)
    uint32_t n; uint32_t total_sh_rest; uint32_t active_sh_bases;
    int accumulate;                       // unfused only: grad_sh_rest += (sharded path, view batches after the first)
};
hipError_t launch_sh_rest_backward(bool fused_adam, const ShRestArgs& a, hipStream_t s);
// single-view fused backward + Adam over all 59 floats of every Gaussian in one kernel (a: fused-mode arguments, sh: the SH-rest group)
hipError_t launch_fused_backward_adam(const PreprocessBackwardArgs& a, const ShRestArgs& sh, hipStream_t s);
// single-view unfused K12 in one kernel: all six gradients written once (sh: grad_sh_rest + SH layout)
hipError_t launch_backward_gradients(const PreprocessBackwardArgs& a, const ShRestArgs& sh, hipStream_t s);
// Camera-pose gradients (fgs_backward_pose): the same kernel with POSE set also leaves, per wave of 64 Gaussians, the wave's sums of 15 terms -- 12 for
// rows 0..2 of w2c (row-major, column 3 = the translation) and 3 for cam_position -- in one 64-byte line of `partials`; two small kernels then add the
// lines in a fixed order in fp64 (first per chunk of lines into `chunk_sums`, then the chunks) and write grad_w2c [12] / grad_cam_position [3] (either
// may be nullptr). No float atomics: the result is a deterministic function of K11's records. The additions travel in a struct of their own:
// PreprocessBackwardArgs stays byte for byte what it is. Only this materialised-gradient kernel has the flag: the fused backward + Adam, sharded,
// record and asynchronous paths take no pose gradients.
constexpr int kPoseTerms = 15;          // w2c[0..2][0..3], cam_position[0..2]
constexpr int kPoseLineFloats = 16;     // one 64-byte line per wave, the last float is padding (written as 0)
constexpr uint32_t kPoseMaxChunks = 128;
struct PosePart {
    float* partials;                      // [ceil(n / 64)][kPoseLineFloats], every line written by the wave that owns the block
    double* chunk_sums;                   // [kPoseMaxChunks][kPoseLineFloats]
    float* grad_w2c; float* grad_cam_position;
};
struct PreprocessBackwardPoseArgs { PreprocessBackwardArgs k12; PosePart pose; };
hipError_t launch_backward_gradients_pose(const PreprocessBackwardArgs& a, const ShRestArgs& sh, const PosePart& pose, hipStream_t s);

struct AdamGroup { const float* grad; float* param; float* exp_avg; float* exp_avg_sq; int64_t n; AdamHyper h; uint32_t first_block;
                   uint32_t row_len; };      // floats per Gaussian in this tensor (live_blocks only; 0: read every gradient)
// live_blocks: [ceil(N / 64)] bytes or nullptr; 0 = the caller guarantees that the gradient rows of Gaussians 64 b .. 64 b + 63 are zero:
// they are not read (one third of the Gaussians is invisible per view, 85 % of them in such blocks: tools/dead_blocks.py)
// quiet_blocks: [ceil(N / 64)] bytes or nullptr (needs live_blocks and one N for all groups); 1 = every exp_avg / exp_avg_sq element of Gaussians
// 64 b .. 64 b + 63 in every group == 0.0f. With a zero gradient the update is then the identity on parameter and moments: a 16-byte piece whose
// blocks are quiet and not live is neither loaded nor stored. The kernel clears the byte of every block it reads a gradient for (1 -> 0, never back).
// span, first_block and total_blocks are the launcher's: a workgroup owns `span` consecutive chunks (1024 floats per piece a thread holds: 4096 in the product) of one group (launch_adam sets all three)
struct AdamArgs { AdamGroup g[8]; int n_groups; uint32_t total_blocks; int reverse; const uint8_t* live_blocks; uint8_t* quiet_blocks; uint32_t span; };
hipError_t launch_adam(const AdamArgs& a, hipStream_t s);   // K13, all groups in one launch
// quiet_out[b] = 1 iff every moment of block b compares equal to 0.0f in every group (NaN is not zero), else 0: one streaming read of the moments.
// rows = N; group k is [N, row_len[k]]
struct AdamQuietScanArgs { const float* m[8]; const float* v[8]; uint32_t row_len[8]; int n_groups; uint32_t rows; uint8_t* quiet_out; };
hipError_t launch_adam_quiet_scan(const AdamQuietScanArgs& a, hipStream_t s);

struct LossArgs {                       // fused L1 + DSSIM loss and its image gradient (loss.hip)
    const float* image; const float* target;   // [3,H,W]
    float* sums;                                 // [0] sum |x-y|, [1] sum SSIM   (zeroed by the host before the launch)
    float* grad;                                 // [3,H,W] or nullptr
    float* d_mu; float* d_m11; float* d_m12;     // scratch derivative maps, [3,H,W] each
    float* partials;                             // scratch: 2 floats per wave (strip-band) of the forward kernel
    int width, height;
    float lambda_l1, lambda_dssim;
    const float* upstream;                       // device scalar dL/dloss the gradient is multiplied with, or nullptr (= 1)
    // the weighted loss (INTEGRATION.md 'Weighted loss'); all three nullptr for the unweighted one
    const float* weight;                         // [H,W] per-pixel weights shared by the channels: w > 0 counts as w, anything else (0, negative, NaN) as 0
    float* wpartials;                            // scratch: the sum of the effective weights of every strip-band of the forward kernel, one float per strip-band of ONE channel plane
    float* total_weight;                         // scratch: S, their sum in a fixed order (written by the reduction, read by the backward kernel)
};
size_t l1_dssim_partials(int width, int height);   // number of floats in LossArgs::partials
size_t l1_dssim_weight_partials(int width, int height);   // number of floats in LossArgs::wpartials
hipError_t launch_l1_dssim(const LossArgs& a, hipStream_t s);
hipError_t launch_l1_dssim_backward(const LossArgs& a, hipStream_t s);   // gradient only, from the maps a forward launch left in d_mu / d_m11 / d_m12

// bilagrid.hip: per-view bilateral-grid colour correction of the rendered image (slice), its gradients, and the grid's total variation
struct BilagridArgs {
    const float* grid; int gw, gh, gl;           // [12, L, Hg, Wg]
    const float* image; int width, height;       // [3,H,W]
    float* out;                                  // forward: [3,H,W]
    const float* grad_out; float* grad_image;    // backward: upstream [3,H,W]; dL/dimage or nullptr
    float* scratch;                              // backward: dL/dgrid channel-last [L, Hg, Wg, 12], zero on the stream; nullptr = dL/dgrid not wanted
    int vec4;                                    // width % 4 == 0 and every image-shaped tensor 16-byte aligned: rows move as float4
};
bool bilagrid_staged(int gw, int gh, int gl, int width, int height);   // the launches stage the grid under a tile in LDS (else they read it from global memory)
hipError_t launch_bilagrid_slice(const BilagridArgs& a, hipStream_t s);
hipError_t launch_bilagrid_slice_backward(const BilagridArgs& a, float* grad_grid, hipStream_t s);   // grad_grid [12, L, Hg, Wg] is overwritten (with a.scratch)
hipError_t launch_bilagrid_tv(const float* grid, int gw, int gh, int gl, float* loss, float* grad_grid, hipStream_t s);

// normal_consistency.hip: the per-Gaussian surface features (n_cam, z, 1) and the image-space normal-consistency term over their blended map
struct SurfaceFeatureArgs {
    const float* means; const float* scales; const float* rotations;   // [N,3], [N,3] log-scales, [N,4] raw (r, x, y, z)
    const float* w2c; const float* cam_position;                       // device: rows of four floats, rows 0..2 read; [3]
    int n;
    float* features;                                                   // forward: [N,5]
    const float* grad_features; float* grad_rotations; float* grad_means;   // backward: upstream [N,5]; [N,4] / [N,3], each written in full, or nullptr = not wanted
};
struct NormalConsistencyArgs {
    const float* map; int width, height;         // [5,H,W] = (N_r, D, A)
    float inv_fx, inv_fy, cx, cy, min_alpha;
    float* E; float* normals;                    // forward: [H,W]; n_d [3,H,W] or nullptr
    const float* grad_E; float* grad_map;        // backward: upstream [H,W]; [5,H,W], every element written
};
hipError_t launch_surface_features(const SurfaceFeatureArgs& a, hipStream_t s);
hipError_t launch_surface_features_backward(const SurfaceFeatureArgs& a, hipStream_t s);
hipError_t launch_normal_consistency(const NormalConsistencyArgs& a, hipStream_t s);
hipError_t launch_normal_consistency_backward(const NormalConsistencyArgs& a, hipStream_t s);

// tsdf.hip: fused TSDF integration of up to kTsdfMaxViews rendered views into a dense volume, and the marching-tetrahedra mesh of its level set
constexpr int kTsdfMaxViews = 8;
struct TsdfView { const float* w2c; float fx, fy, cx, cy; const float* depth; const float* alpha; const float* color; };   // w2c: device, rows 0..2; alpha / color may be nullptr
struct TsdfIntegrateArgs {
    float2* tsdf_weight; float* color;           // [nz,ny,nx] (tsdf, weight) pairs; planar [3,nz,ny,nx] or nullptr
    int nx, ny, nz; float ox, oy, oz, voxel, trunc, inv_trunc;      // inv_trunc = 1 / trunc, rounded once on the host
    int n_views, width, height;
    float near_plane, depth_max, min_alpha, max_weight;
    TsdfView view[kTsdfMaxViews];
};
hipError_t launch_tsdf_integrate(const TsdfIntegrateArgs& a, hipStream_t s);
struct MeshArgs {
    const float2* tsdf_weight; const float* color; int nx, ny, nz; float ox, oy, oz, voxel, iso, min_weight;
    uint32_t* codes; uint2* block_sums; uint32_t* totals;       // scratch: a code word per lattice point, (vertices, triangles) per workgroup, the two totals
    uint32_t n_vertices; uint64_t n_triangles;                  // emit: the sizes of the caller's buffers (nothing is written past them)
    float* vertices; float* colors; int32_t* faces;             // emit: [Nv,3], [Nv,3] or nullptr, [Nf,3]
};
uint32_t mesh_blocks(uint32_t n_points);                        // workgroups (= block sums) of the two lattice passes
hipError_t launch_tsdf_mesh_count(const MeshArgs& a, hipStream_t s);      // classify + scan: codes, block bases, totals
hipError_t launch_tsdf_mesh_emit(const MeshArgs& a, hipStream_t s);       // from the scratch a count launch over the same volume left

// shard_exchange.hip: record (un)packing either side of the two exchanges of the Gaussian-sharded multi-GPU path
struct PackRecordsView { const PrimRec* rec; const uint32_t* n_touched; const uint32_t* depth_keys; const uint32_t* prim_idx;
                         const uint32_t* counters; uint32_t* slot; uint32_t* out; uint32_t* counts_out; };
struct PackRecordsBatch { int n_views; uint32_t capacity; PackRecordsView v[kMaxBatchViews]; };
hipError_t launch_pack_splat_records(const PackRecordsBatch& b, hipStream_t s);
// how the renderer's record concatenation is made of the shards' segments (n_shards <= 1: the records keep their order)
struct ShardOrder { int n_shards; uint32_t count[kMaxBatchViews]; };
hipError_t launch_unpack_splat_records(const uint32_t* records, uint32_t n, PrimRec* rec, uint32_t* n_touched, uint32_t* depth_keys,
                                       uint32_t* prim_idx, uint4* foot, uint2* ranges, uint32_t n_tiles, uint32_t* hot_list, uint32_t* hot_count, const ShardOrder& order,
                                       hipStream_t s);
hipError_t launch_pack_acc(const float* acc, uint32_t n, float* out, const ShardOrder& order, hipStream_t s);

// aux_ops.hip: the reference's remaining exported operators
hipError_t launch_update_3d_filter(const float* positions, const float* w2c, float* filter_3d, uint8_t* visibility_mask, int n,
                                   float left, float right, float top, float bottom, float near_plane, float distance2filter, hipStream_t s);
void relocation_coefficients(float* out /*[50*50] host*/);
hipError_t launch_relocation(const float* old_opacities, const float* old_scales, const int64_t* n_samples, const float* table_device,
                             float* new_opacities, float* new_scales, unsigned n, hipStream_t s);
hipError_t launch_add_noise(const float* raw_scales, const float* raw_rotations, const float* raw_opacities, const float* random_samples,
                            float* means, unsigned n, float current_lr, hipStream_t s);

// densify.hip: maintenance of the Gaussian set (adaptive density control, prune / sort gathers, Morton order) with the Adam moments
struct AdcPlanArgs {
    const float* densification_info;      // [2, N]
    const float* scales; const float* rotations; const float* opacities;
    uint32_t n;
    float grad_threshold, min_opacity_logit, log_small, log_large; int prune_large;
    uint32_t* plan; uint4* offsets; uint32_t* totals;      // scratch: [N], [N], [4] = survivors, clones, children per copy, split
    void* scan_temp; size_t scan_temp_bytes;
};
size_t adc_scan_temp_bytes(uint32_t n);
hipError_t launch_adc_plan(const AdcPlanArgs& a, hipStream_t s);
struct AdcScatterArgs {
    const float* in_p; const float* in_m; const float* in_v;     // moments may be NULL (no optimizer state yet)
    float* out_p; float* out_m; float* out_v;
    const float* scales; const float* rotations; const float* noise;   // KIND 1 (means) only; noise [2 * n_split, 3]
    const uint32_t* plan; const uint4* offsets; const uint32_t* totals;
    uint32_t n, width;
};
hipError_t launch_adc_scatter(int kind, const AdcScatterArgs& a, hipStream_t s);
constexpr int kGatherTensors = 18;
struct GatherTensor { const float* in; float* out; uint32_t width; uint32_t first_block; };
struct GatherArgs { GatherTensor t[kGatherTensors]; int n_tensors; uint32_t n_rows; const int64_t* index; };
hipError_t launch_gather_rows(const GatherArgs& a, hipStream_t s);
size_t morton_temp_bytes(uint32_t n);
hipError_t run_morton_order(const float* means, const float* lo, const float* hi, int64_t* order_out, uint32_t n, void* temp, size_t temp_bytes, hipStream_t s);

#ifdef FGS_DEV_SWITCHES
extern std::atomic<int> g_backward_ablate;                                   // blend_backward_exhibits.hip, option 7 (FGS_ABLATE: fgs_k11_probes.h)
extern std::atomic<int> g_k11m_max_blocks;                                   // blend_backward_exhibits.hip
extern std::atomic<int> g_backward_variant;                                  // 3 compact (default, blend_backward.hip); 0 / 2 systolic, 1 strip, 4 lane = pixel, 5 chained (blend_backward_exhibits.hip)
// the exhibit kernel of a.variant != 3 alone (blend_backward_exhibits.hip); launch_blend_backward adds the fold / dirty-mark kernel behind it and reads the error
void launch_blend_backward_exhibit(const BlendBackwardArgs& a, hipStream_t s);
#endif
int blend_backward_variant();                                                // the K11 formulation of this pass (always 3 in the product build)
hipError_t launch_wave_selftest(uint32_t* out /*[4*64]*/, hipStream_t s);

}  // namespace fgs

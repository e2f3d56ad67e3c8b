/*
 * fgs_hip.h -- C ABI of libfgs_hip.so, the MI355X (gfx950) implementation of the FasterGS rasterizer hot path.
 *
 * This is the drop-in boundary: each entry point replaces one function of the reference's pybind module
 * `FasterGSCudaBackend._C` (reference: FasterGSCudaBackend/FasterGSCudaBackend/torch_bindings/bindings.cpp:12-21).
 * Plain pointers and sizes only -- no torch types. All pointers are DEVICE pointers unless marked [host].
 * Every function returns FGS_OK (0) or a negative fgs_status and never throws; fgs_last_error() gives the text.
 * All work is enqueued on `stream` (a hipStream_t passed as void*); the reference uses the legacy default stream
 * (rasterization/src/forward.cu:64 etc.), an explicit stream is the MI355X-side change.
 *
 * Tensor layouts are the reference's (torch_bindings/rasterization.py:113-132):
 *   means[N,3] scales[N,3] (log) rotations[N,4] (w first, unnormalised) opacities[N,1] (logit)
 *   sh_coefficients_0[N,1,3] sh_coefficients_rest[N,K-1,3], fp32, contiguous.
 */
#ifndef FGS_HIP_H
#define FGS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 6): the private layout of the primitive blob grew in round 5 (footprint rows, tile counts, wave / block sums, big-footprint list) and the
 * product library stopped exporting fgs_debug_set_option / fgs_debug_set_backward_variant (libfgs_hip_dev.so has them): a caller that sized or
 * decoded blobs by the version-2 layout, or bound the two debug symbols, must notice. Signatures of the version-2 entry points are unchanged. */
#define FGS_ABI_VERSION 3

typedef enum fgs_status {
    FGS_OK = 0,
    FGS_ERR_INVALID_ARGUMENT = -1,
    FGS_ERR_ALLOC = -2,      /* the resize callback returned NULL */
    FGS_ERR_HIP = -3,        /* a HIP runtime call or kernel launch failed */
    FGS_ERR_INTERNAL = -4
} fgs_status;

/* The 13 fields of RasterizerSettings (torch_bindings/rasterization.py:8-38) plus total_sh_bases_rest, which the
 * reference derives from sh_coefficients_rest.size(1) (rasterization/src/rasterization_api.cu:44). */
typedef struct fgs_settings {
    const float* w2c;           /* >= 12 floats: rows 0..2 of the row-major world-to-camera matrix */
    const float* cam_position;  /* 3 floats */
    const float* bg_color;      /* 3 floats */
    int32_t active_sh_bases;
    int32_t total_sh_bases_rest;
    int32_t width;
    int32_t height;
    float focal_x, focal_y, center_x, center_y, near_plane, far_plane;
    int32_t proper_antialiasing;
} fgs_settings;

/* Scratch ownership follows the reference: the caller owns four byte buffers and hands the library a callback that
 * (re)sizes buffer `which` to `bytes` and returns its device pointer -- the C form of resize_function_wrapper
 * (utils/torch_utils.h:6-12) as used at rasterization/src/forward.cu:44,58,179,236. Layout inside is private. */
enum { FGS_BUF_PRIMITIVE = 0, FGS_BUF_TILE = 1, FGS_BUF_INSTANCE = 2, FGS_BUF_BUCKET = 3, FGS_BUF_COUNT = 4 };
typedef void* (*fgs_resize_fn)(void* user, int32_t which, size_t bytes);

/* What _C.forward returns next to the image and what _C.backward takes back (rasterization_api.h:8-59):
 * (n_instances, n_buckets, selector). Opaque to callers; n_visible is extra (reported by bench.py). */
typedef struct fgs_forward_state {
    int32_t n_visible;
    int32_t n_instances;
    int32_t n_buckets;   /* capacity of the bucket buffer (upper bound of the device-side count) */
    int32_t selector;    /* bit 0: which half of the instance double buffer holds the tile-sorted list; bit 1: fgs_forward_aux left depth checkpoints;
                            bit 2: the counts are bounds (fgs_forward_async); bit 3: the buffers were filled from splat records */
} fgs_forward_state;

int32_t fgs_abi_version(void);
const char* fgs_last_error(void);   /* [host] thread-local, valid until the next call on this thread */
const char* fgs_build_info(void);   /* [host] e.g. "gfx950 wave64 tile16x12 bucket64" */

/* replaces _C.forward  (rasterization_api.cu:13-91 -> rasterization/src/forward.cu:11-259). image: [3,H,W]. */
int32_t fgs_forward(const float* means, const float* scales, const float* rotations, const float* opacities,
                    const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                    const fgs_settings* settings, float* image,
                    fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream);

/* Bytes of zero-initialisable scratch fgs_backward needs (replaces the two helper tensors grad_mean2d_helper /
 * grad_conic_helper of rasterization_api.cu:133-134 plus per-pixel staging). */
size_t fgs_backward_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height);

/* replaces _C.backward (rasterization_api.cu:94-178 -> rasterization/src/backward.cu:8-125).
 * The six grad_* outputs need NOT be zero-filled by the caller: every element is written (zeros for primitives
 * that were not visible), which replaces the reference's 8 torch::zeros fills (rasterization_api.cu:127-134).
 * densification_info: [2,N] accumulated in place (kernels_backward.cuh:194-201) or NULL. */
int32_t fgs_backward(const float* grad_image, const float* image,
                     const float* means, const float* scales, const float* rotations, const float* opacities,
                     const float* sh_coefficients_rest,
                     void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                     float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                     float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                     float* densification_info, void* scratch,
                     int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, void* stream);
/* fgs_backward plus one byte per block of 64 consecutive Gaussians: live_blocks[b] = 1 if any Gaussian 64 b .. 64 b + 63 was visible, 0 if
 * all gradients of the block are zero (they are written all the same: the gradient tensors are dense and valid). [ceil(n_primitives / 64)]
 * bytes, or NULL (= fgs_backward). One third of the Gaussians is invisible in a view and 85 % of them sit in such blocks (Morton order):
 * fgs_adam_step_multi_live does not read the zeros back. */
int32_t fgs_backward_live(const float* grad_image, const float* image,
                          const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_rest,
                          void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                          float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                          float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                          float* densification_info, void* scratch,
                          int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks, void* stream);

/* fgs_forward that also returns, from the same walk, the accumulated opacity alpha = 1 - T_final and the expected depth sum_i w_i z_i (definitions:
 * fgs_inference_aux below; fp32 [H,W] image-linear, 0 where nothing was blended, the background is no part of them) -- and keeps what a backward pass
 * needs to differentiate them (the running depth sum beside every checkpoint, at the tail of the bucket buffer: the buffers stay valid input to
 * fgs_backward / fgs_backward_live / fgs_backward_adam_fused). Either map pointer may be NULL, both NULL is FGS_ERR_INVALID_ARGUMENT. `image` is
 * fgs_forward's. n_primitives == 0: image = background, maps 0. There is no asynchronous, sharded or record form of it. */
int32_t fgs_forward_aux(const float* means, const float* scales, const float* rotations, const float* opacities,
                        const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                        const fgs_settings* settings, float* image, float* alpha, float* depth_expected,
                        fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream);
/* fgs_backward_live with upstream gradients of those two maps: grad_alpha, grad_depth [H,W] (NULL = zero; both NULL is exactly fgs_backward_live and
 * takes the plain scratch size), depth_expected = the map fgs_forward_aux returned (read with grad_depth only). The expected depth is NOT normalised:
 * a mean depth depth / alpha is the caller's division, and its chain rule hands both gradients here. A non-NULL grad_depth on buffers that were not
 * filled by fgs_forward_aux is FGS_ERR_INVALID_ARGUMENT (no depth checkpoints). scratch: fgs_backward_aux_scratch_bytes(). The median depth carries no
 * gradient; the fused backward + Adam, asynchronous, sharded and record paths take no map gradients. */
size_t fgs_backward_aux_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height);
int32_t fgs_backward_aux(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                         const float* means, const float* scales, const float* rotations, const float* opacities,
                         const float* sh_coefficients_rest,
                         void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                         float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                         float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                         float* densification_info, void* scratch,
                         int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks, void* stream);
/* fgs_backward_aux plus a second byte per block of 64 consecutive Gaussians: reached_blocks[b] = 1 if the backward blend pass REACHED some Gaussian
 * 64 b .. 64 b + 63 -- added anything that is not +-0 to its nine per-Gaussian sums or, with grad_depth, to its dL/dz; a Gaussian of more than 256 tiles
 * counts through its folded record. 0 is a PROMISE: every row of the block is +-0 in all six gradient tensors (written all the same), also after the
 * depth term has been added to grad_means -- the per-Gaussian test that feeds the flag includes dL/dz, so the flag is exact on the map-gradient path
 * too, not a copy of live_blocks. That covers the invisible blocks and the visible ones hidden behind opaque Gaussians (two thirds of all blocks of a
 * dense scene). reached_blocks[b] <= live_blocks[b]; live_blocks keeps its meaning ("any visible"). [ceil(n_primitives / 64)] bytes each, either may be
 * NULL (both NULL, no map gradients = fgs_backward); the last block may be partial; n_primitives == 0 writes nothing. Either array is a valid
 * `live_blocks` argument of fgs_adam_step_multi_live for exactly these gradient tensors; reached_blocks spares it more reads. */
int32_t fgs_backward_reached(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                             const float* means, const float* scales, const float* rotations, const float* opacities,
                             const float* sh_coefficients_rest,
                             void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                             float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                             float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                             float* densification_info, void* scratch,
                             int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                             uint8_t* reached_blocks, void* stream);
/* fgs_backward_reached for gradient tensors whose content the caller knows -- the tensors of an earlier pass used again instead of new memory.
 * prior_blocks: [ceil(n_primitives / 64)] device bytes, read only. prior_blocks[b] == 0 is the CALLER'S PROMISE that every element of rows
 * 64 b .. 64 b + 63 of all six gradient tensors compares equal to 0.0f now, when the pass starts (+0 or -0) -- e.g. the reached_blocks output of the pass
 * that last wrote these very tensors, if nothing has written to them since. 1 promises nothing. A block with prior_blocks[b] == 0 that this pass
 * reaches no Gaussian of is then NOT WRITTEN: its zeros are there already (the 236 bytes per Gaussian of such blocks are nine tenths of the traffic
 * of this stage in a dense scene). The result is what fgs_backward_reached leaves, bit for bit except that a -0 of such a block stays -0. As a guard
 * the kernel also looks at the block's FIRST element in each of the six tensors and writes the block after all unless all six compare equal to 0.0f:
 * a whole-tensor edit the caller's bookkeeping missed (hand-written weight decay, NaN) is caught; a foreign write that leaves those six elements zero
 * is not -- then the promise was false and the stale values stay. Every other block is written in full as before (a reached block including the
 * zeros of its unreached rows); live_blocks, reached_blocks and densification_info are written as before in every case.
 * NULL prior_blocks is fgs_backward_reached exactly. FGS_ERR_INVALID_ARGUMENT, before anything is launched: prior_blocks without reached_blocks (the
 * caller could not continue the chain), prior_blocks aliasing reached_blocks or live_blocks (ping-pong between two arrays). Map gradients are accepted:
 * the depth term is added to reached Gaussians only. */
int32_t fgs_backward_recycled(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                              const float* means, const float* scales, const float* rotations, const float* opacities,
                              const float* sh_coefficients_rest,
                              void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                              float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                              float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                              float* densification_info, void* scratch,
                              int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                              uint8_t* reached_blocks, const uint8_t* prior_blocks, void* stream);
/* fgs_backward_recycled that also returns the gradient of the CAMERA: grad_w2c (12 device floats, rows 0..2 of settings->w2c row-major) and
 * grad_cam_position (3 device floats). With W = w2c[:3,:3], t = w2c[:3,3], c = cam_position and, per Gaussian i that the pass reached, p_i = W m_i + t,
 * J_i = [[j11, 0, -j11 xc], [0, j22, -j22 yc]] (xc, yc the clipped x/z, y/z), the colour a function of m_i - c:
 *   grad_w2c[:,3]  = sum_i g_i,                       g_i = dL/dp_i (clip cases as in the mean gradient) + e_2 dL/dz_i (with grad_depth),
 *   grad_w2c[:,:3] = sum_i (g_i m_i^T + J_i^T dL/d(J_i W)),
 *   grad_cam_position = - sum_i dL/d(m_i - c)         (exactly 0 when active_sh_bases == 1).
 * w2c and cam_position are INDEPENDENT inputs, as in fgs_settings: the relation c = -W^T t is the caller's chain rule. The proper-antialiasing opacity
 * factor is a constant here as everywhere. The sums are formed inside K12 -- per wave of 64 Gaussians, then over the waves in a fixed order in fp64, no
 * float atomics: a deterministic function of the per-Gaussian sums of the backward blend pass -- and do not depend on what `scratch` held.
 * Either output may be NULL; both NULL is fgs_backward_recycled exactly and takes its scratch size, otherwise scratch:
 * fgs_backward_pose_scratch_bytes(), with or without map gradients. grad_alpha / grad_depth are accepted as by fgs_backward_aux. n_primitives == 0
 * writes 15 zeros. The six parameter gradients, both flag arrays and densification_info are what fgs_backward_recycled leaves. Only this
 * materialised-gradient pass has camera gradients: the fused backward + Adam, sharded, record and asynchronous paths take none, and there is none
 * for the intrinsics. */
size_t fgs_backward_pose_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height);
int32_t fgs_backward_pose(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                          const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_rest,
                          void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                          float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                          float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                          float* densification_info, void* scratch,
                          int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                          uint8_t* reached_blocks, const uint8_t* prior_blocks, float* grad_w2c, float* grad_cam_position, void* stream);
/* fgs_backward_recycled that also accumulates the ABSOLUTE-gradient densification statistic (AbsGS; gsplat's absgrad). For every (pixel p, Gaussian i)
 * pair the backward blend lets contribute, with hh = -1/2 alpha dL/dalpha, t = hh dx, u = hh dy and the conic (ca, cb, cc), the pair's share of
 * dL/dmean2d is gx_p = 2 (ca t + cb u), gy_p = 2 (cb t + cc u); densification_info[1] accumulates the norm of their SIGNED sums, which cancel for a
 * Gaussian that covers many pixels. With ax_i = sum_p |gx_p|, ay_i = sum_p |gy_p| (dL/dalpha includes the alpha and depth terms of map gradients):
 *     abs_densification_info: fp32 [2, n_primitives], accumulated (+=), never cleared here
 *       row 0 += 1 for every visible Gaussian (n_touched != 0), exactly as densification_info[0]
 *       row 1 += sqrt((0.5 W ax_i)^2 + (0.5 H ay_i)^2)
 * -- a drop-in first argument of fgs_adc_plan; the threshold is the caller's. The two sums are formed inside the backward blend kernel (two more
 * accumulators per lane; no second walk) and turned into the statistic by one small kernel behind K12. abs_densification_info == NULL IS
 * fgs_backward_recycled: the same kernels, its scratch size. Otherwise scratch: fgs_backward_absgrad_scratch_bytes(), with or without map gradients
 * (the plain and the aux layout are prefixes of it). densification_info may be given as well, or NULL. The six gradients, both flag arrays and
 * densification_info are what fgs_backward_recycled leaves. FGS_ERR_INVALID_ARGUMENT, never ignored: buffers of fgs_forward_async or of the record /
 * sharded forward passes, abs_densification_info overlapping densification_info. n_primitives == 0 writes nothing. Only this materialised-gradient
 * pass has the statistic: fgs_backward_adam_fused, the sharded and record paths take none; pose and feature gradients have entry points of their own. */
size_t fgs_backward_absgrad_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height);
int32_t fgs_backward_absgrad(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                             const float* means, const float* scales, const float* rotations, const float* opacities,
                             const float* sh_coefficients_rest,
                             void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                             float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                             float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                             float* densification_info, void* scratch,
                             int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                             uint8_t* reached_blocks, const uint8_t* prior_blocks, float* abs_densification_info, void* stream);

/* Feature-channel render of the training pass. features: fp32 [n_primitives, n_channels] contiguous, any sign, 1 <= n_channels <= 64. Over exactly the
 * (pixel, Gaussian) pairs the training blend of the forward pass blended, in its order -- the same sub-tile cull, alpha >= 1/255, T_before >= 1e-4, never
 * beyond the pixel's last contributor -- with w_i = T_before_i alpha_i:
 *     feature_map[c][p] = sum_i w_i features[i][c]            fp32 [n_channels, H, W], every element written
 * No background term, no normalisation; 0 where nothing was blended. A channel of ones is 1 - T_final, a channel holding the view-space depth z_i is
 * fgs_forward_aux's depth_expected. The buffers and `state` are those of a completed SYNCHRONOUS fgs_forward or fgs_forward_aux over the same Gaussians
 * and settings; they are read only, and stay valid input to every backward pass. One walk per 16 channels (4 or 8 for a narrower F).
 * FGS_ERR_INVALID_ARGUMENT, never ignored: n_channels outside 1..64, NULL features (n_primitives > 0) or feature_map, buffers of fgs_forward_async or of
 * the record / sharded forward passes. n_primitives == 0: a zero map, nothing else is written. */
int32_t fgs_blend_features(const float* features, int32_t n_channels, const void* primitive_buffers, const void* tile_buffers, const void* instance_buffers,
                           int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, float* feature_map, void* stream);
/* fgs_backward_reached for a loss that also depends on such a map: feature_map = what fgs_blend_features returned, grad_feature_map = its upstream
 * gradient [n_channels, H, W]. With u_i(p) = sum_c features[i][c] grad_feature_map[c][p] and S_i(p) = sum_{j>i} w_j u_j = sum_c feature_map[c][p]
 * grad_feature_map[c][p] - sum_{j<=i} w_j u_j (the forward map takes the place of per-bucket checkpoints):
 *     grad_features[i][c] = sum_p w_i grad_feature_map[c][p]                       fp32 [n_primitives, n_channels], need not be initialised
 *     dL/dalpha_i(p)     += T_i u_i - S_i / max(1 - alpha_i, 1e-6)                  added to the colour term's per-Gaussian sums, then K12 as always
 * The kernels run K11, the feature backward blend, K12. detach_geometry != 0: grad_features only, the six parameter gradients are fgs_backward_reached's.
 * grad_feature_map == NULL IS fgs_backward_reached: the feature arguments are not looked at. scratch: as for the pass without features
 * (fgs_backward_scratch_bytes, or fgs_backward_aux_scratch_bytes with map gradients). Refused like fgs_blend_features; the fused backward + Adam,
 * asynchronous, sharded and record paths and the pose gradients take no feature gradient. n_primitives == 0 writes nothing. */
int32_t fgs_backward_features(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                              const float* means, const float* scales, const float* rotations, const float* opacities,
                              const float* sh_coefficients_rest,
                              void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                              float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                              float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                              float* densification_info, void* scratch,
                              int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                              uint8_t* reached_blocks, const float* features, int32_t n_channels, const float* feature_map,
                              const float* grad_feature_map, float* grad_features, int32_t detach_geometry, void* stream);

/* Depth-distortion regulariser of the training pass (Mip-NeRF 360's distortion loss; the `distloss` of 2DGS). Over exactly the (pixel, Gaussian) pairs
 * the training blend of the forward pass blended, in its order i = 1..n -- the same sub-tile cull, alpha >= 1/255, T_before >= 1e-4, never beyond the
 * pixel's last contributor -- with w_i = T_before_i alpha_i and a depth value t_i per Gaussian:
 *     X(p) = sum_a sum_b w_a w_b |t_a - t_b| = 2 sum_i w_i (t_i A_{i-1} - D_{i-1}),    A_i = sum_{j<=i} w_j,  D_i = sum_{j<=i} w_j t_j
 * (the lists are in depth order, so t does not decrease along the walk). mode FGS_DISTORTION_LINEAR: t_i = z_i, row 2 of w2c applied to the mean, as in
 * fgs_forward_aux. FGS_DISTORTION_NORMALIZED: t_i = far (z_i - near) / ((far - near) z_i), onto [0, 1) with the settings' near_plane and far_plane.
 * distortion_state: fp32 [3, H, W], every element written. Plane 0 is X, exactly 0 where fewer than two Gaussians were blended; planes 1 and 2 are what
 * fgs_backward_distortion needs and are the library's private format (the walk shifts t by a tile-uniform origin, under which X does not change).
 * `means` are the Gaussians' of the forward pass; the buffers and `state` are those of a completed SYNCHRONOUS fgs_forward or fgs_forward_aux over them
 * with the same settings; they are read only, and stay valid input to every backward pass.
 * FGS_ERR_INVALID_ARGUMENT, never ignored: a mode other than the two, near_plane <= 0 or far_plane <= near_plane in normalized mode, NULL
 * distortion_state, NULL means (n_primitives > 0), buffers of fgs_forward_async or of the record / sharded forward passes. n_primitives == 0: a zero
 * state, nothing else is written. */
enum { FGS_DISTORTION_LINEAR = 0, FGS_DISTORTION_NORMALIZED = 1 };
int32_t fgs_blend_distortion(const float* means, const void* primitive_buffers, const void* tile_buffers, const void* instance_buffers,
                             int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, int32_t mode, float* distortion_state,
                             void* stream);
/* fgs_backward_reached for a loss that also depends on X: distortion_state = what fgs_blend_distortion wrote (same mode), grad_distortion = the
 * upstream gradient of plane 0, [H, W]. With e_i = dX/dw_i = 2 [t_i (2 A_{i-1} - A_n) - 2 D_{i-1} + D_n] and S_i = sum_{j>i} w_j e_j = 2 X - sum_{j<=i} w_j e_j
 * (the forward state takes the place of per-bucket checkpoints):
 *     dL/dalpha_i(p) += gX [T_i e_i - S_i / max(1 - alpha_i, 1e-6)]              added to the colour term's per-Gaussian sums, then K12 as always
 *     dL/dz_i         = sum_p gX 2 w_i (2 A_{i-1} + w_i - A_n) dt_i/dz_i          grad_means[i] += dL/dz_i w2c[2, 0:3] behind K12
 * The kernels run K11, the distortion backward blend, K12, the depth term of the means. dL/dz takes part in K12's "did the blend pass reach it" test,
 * so live_blocks / reached_blocks mean what they mean in fgs_backward_reached. scratch: fgs_backward_aux_scratch_bytes (the plain layout is its prefix),
 * with or without map gradients. grad_distortion == NULL IS fgs_backward_reached: the distortion arguments are not looked at and the scratch is that
 * pass's. Refused like fgs_blend_distortion, and a NULL distortion_state; the fused backward + Adam, asynchronous, sharded and record paths and the
 * pose, feature and absgrad entry points take no distortion gradient. No gradient for near_plane / far_plane. n_primitives == 0 writes nothing. */
int32_t fgs_backward_distortion(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                                const float* means, const float* scales, const float* rotations, const float* opacities,
                                const float* sh_coefficients_rest,
                                void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                                float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                                float* densification_info, void* scratch,
                                int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                                uint8_t* reached_blocks, const float* distortion_state, const float* grad_distortion, int32_t mode, void* stream);

/* One render for the 2DGS regularisers of the training pass: the depth-distortion map X of fgs_blend_distortion (same `mode`, same t) and the blend
 * M_c = sum_i w_i surface_features[i][c] of fgs_blend_features for FIVE channels, over the same pairs in ONE walk. surface_features: fp32
 * [n_primitives, 5] contiguous, any sign -- for the normal-consistency term what fgs_surface_features wrote: the view-space normal, the depth z and a
 * one, so that M[3] is the expected depth and M[4] the accumulated opacity.
 * geometry_state: fp32 [8, H, W], every element written. Plane 0 is X, exactly 0 where fewer than two Gaussians were blended; planes 2..6 are M, a
 * contiguous [5, H, W] that fgs_normal_consistency takes as its surface_map as it is; planes 1 (sum w (t - t0 of the tile)) and 7 (sum w) are what
 * fgs_backward_geometry needs and are the library's private format. X does not read channel 4: it equals fgs_blend_distortion's whatever the channels hold.
 * Buffers and `state`: as for fgs_blend_distortion. FGS_ERR_INVALID_ARGUMENT, never ignored: a mode other than the two, near_plane <= 0 or far_plane <=
 * near_plane in normalized mode, NULL geometry_state, NULL means or surface_features (n_primitives > 0), buffers of fgs_forward_async or of the record /
 * sharded forward passes. n_primitives == 0: a zero state, nothing else is written. */
int32_t fgs_blend_geometry(const float* means, const float* surface_features, const void* primitive_buffers, const void* tile_buffers,
                           const void* instance_buffers, int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, int32_t mode,
                           float* geometry_state, void* stream);
/* fgs_backward_reached for a loss that also depends on X and / or M: geometry_state = what fgs_blend_geometry wrote (same mode and features),
 * grad_distortion = the upstream gradient of plane 0 [H, W], grad_surface_map = that of planes 2..6 [5, H, W]; either may be NULL (= zero, and its sums
 * are not formed). dL/dalpha is linear in them, so one walk serves both: with e_i of fgs_backward_distortion, u_i of fgs_backward_features,
 * c_i = gX e_i + u_i and S_i = gX 2 X + sum_c M_c gM_c - sum_{j<=i} w_j c_j,
 *     dL/dalpha_i(p)           += T_i c_i - S_i / max(1 - alpha_i, 1e-6)               added to the colour term's per-Gaussian sums, then K12 as always
 *     dL/dz_i                   = sum_p gX 2 w_i (2 A_{i-1} + w_i - A_n) dt_i/dz_i      grad_means[i] += dL/dz_i w2c[2, 0:3] behind K12
 *     grad_surface_features[i][c] = sum_p w_i gM_c(p)                                  fp32 [n_primitives, 5], zeroed by the call
 * The kernels run K11, the geometry backward blend, K12, the depth term of the means. scratch: fgs_backward_aux_scratch_bytes, with or without map
 * gradients. Both upstream gradients NULL IS fgs_backward_reached: the geometry arguments are not looked at and the scratch is that pass's. Refused like
 * fgs_blend_geometry, and NULL geometry_state / surface_features / grad_surface_features; the fused backward + Adam, asynchronous, sharded and record
 * paths and the pose and absgrad entry points take no geometry gradient. No gradient for near_plane / far_plane. n_primitives == 0 writes nothing. */
int32_t fgs_backward_geometry(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                              const float* means, const float* scales, const float* rotations, const float* opacities,
                              const float* sh_coefficients_rest,
                              void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                              float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                              float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                              float* densification_info, void* scratch,
                              int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                              uint8_t* reached_blocks, const float* surface_features, const float* geometry_state, const float* grad_distortion,
                              const float* grad_surface_map, float* grad_surface_features, int32_t mode, void* stream);

/* fgs_forward WITHOUT its host synchronisation (the reference blocks three times per forward pass, forward.cu:100,102,234; fgs_forward
 * once): nothing is read back. The instance-stage buffers and launches are sized by `instance_capacity` -- the caller's bound, e.g. 1.25 x
 * the largest count fgs_forward_counts() has reported, scaled with the primitive count -- and every kernel reads the exact counts on the
 * device. state_out: n_visible = n_primitives and n_instances = instance_capacity (bounds; pass them back to fgs_backward unchanged).
 * If the real instance count exceeds the capacity the excess instances are DROPPED (incomplete image) and a flag is raised that
 * fgs_forward_counts() reports: the caller repeats the pass with fgs_forward or a larger capacity. All work is enqueued on `stream`;
 * together with fgs_backward / fgs_adam_step_multi a whole iteration is free of host waits (and capturable, resize callback aside). */
int32_t fgs_forward_async(const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                          const fgs_settings* settings, float* image, int32_t instance_capacity, fgs_resize_fn resize, void* resize_user,
                          fgs_forward_state* state_out, void* stream);
/* Enqueues the copy of (n_visible, n_instances, capacity_exceeded) of the forward pass that filled `primitive_buffers` into
 * host_out[3] (pinned memory recommended); valid once `stream` has reached this point. No synchronisation. */
int32_t fgs_forward_counts(const void* primitive_buffers, int32_t n_primitives, int32_t* host_out, void* stream);

/* replaces _C.inference (rasterization_api.cu:181-247 -> rasterization/src/inference.cu:11-226).
 * image: [3,H,W] if to_chw else [H,W,3]. Only FGS_BUF_PRIMITIVE/TILE/INSTANCE are requested. */
int32_t fgs_inference(const float* means, const float* scales, const float* rotations, const float* opacities,
                      const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                      const fgs_settings* settings, float* image, int32_t to_chw, int32_t clamp_output,
                      fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream);

/* fgs_inference that also returns per-pixel maps of the same walk, fp32 [H,W] image-linear, each optional (NULL = not wanted; all three NULL is
 * FGS_ERR_INVALID_ARGUMENT). They come from exactly the (pixel, Gaussian) pairs the colour blends -- same sub-tile cull, alpha >= 1/255, stop once
 * T < 1e-4 -- with w_i = T_before_i * alpha_i and z_i the view-space depth of Gaussian i's mean (row 2 of w2c applied to it: the depth key's value):
 *   alpha          = 1 - T_final                  (the background is not part of it)
 *   depth_expected = sum_i w_i z_i                (not normalised; divide by alpha for a mean depth; 0 where nothing was blended)
 *   depth_median   = z of the last blended Gaussian whose T_before_i > 0.5: the one that carries T across 0.5 where the pixel becomes more than
 *                    half opaque, otherwise the last one blended; 0 where nothing was blended.
 * `image` is bit-identical to fgs_inference's. These maps carry no gradient (differentiable alpha and expected depth: fgs_forward_aux). Same buffers, same single host read, everything on `stream`.
 * n_primitives == 0: image = background, all maps 0. */
int32_t fgs_inference_aux(const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                          const fgs_settings* settings, float* image, int32_t to_chw, int32_t clamp_output,
                          float* alpha, float* depth_expected, float* depth_median,
                          fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream);

/* replaces _C.pruning_scores (rasterization_api.cu:250-309 -> rasterization/src/pruning_scores.cu):
 * accumulates the Speedy-Splat importance score of every primitive for one view into scores[N]. */
int32_t fgs_pruning_scores(float* scores, const float* means, const float* scales, const float* rotations, const float* opacities,
                           const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                           const fgs_settings* settings, fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream);

/* replaces _C.adam_step (adam/src/adam.cu:36-71): in-place Adam on one tensor, bias corrections in double on the host. */
int32_t fgs_adam_step(const float* grad, float* param, float* exp_avg, float* exp_avg_sq, int64_t n_elements,
                      int32_t step, double lr, double beta1, double beta2, double eps, void* stream);

/* All parameter groups of FusedAdam.step() (torch_bindings/adam.py:11-36) in ONE launch. Arrays are [host], length n_groups <= 8. */
int32_t fgs_adam_step_multi(int32_t n_groups, const float* const* grads, float* const* params, float* const* exp_avgs,
                            float* const* exp_avg_sqs, const int64_t* n_elements, const int32_t* steps, const double* lrs,
                            double beta1, double beta2, double eps, void* stream);
/* The same with the caller's PROMISE that gradient rows of dead blocks are zero: live_blocks as written by fgs_backward_live (or, sparing more reads,
 * reached_blocks as written by fgs_backward_reached) for exactly these gradient tensors (device, [ceil(N / 64)] bytes), floats_per_gaussian[k] = row length of group k ([host]). Gradients of dead blocks are not
 * read -- except one sentinel float per dead block and tensor (the block's first element): if it is not +-0 the block is read after all, so a
 * whole-tensor edit behind the caller's back does not go unnoticed; parameters and moments of every Gaussian are updated as always (the result
 * is bit-identical to fgs_adam_step_multi). NULL = no promise. */
int32_t fgs_adam_step_multi_live(int32_t n_groups, const float* const* grads, float* const* params, float* const* exp_avgs,
                                 float* const* exp_avg_sqs, const int64_t* n_elements, const int32_t* steps, const double* lrs,
                                 double beta1, double beta2, double eps, const uint8_t* live_blocks, const int32_t* floats_per_gaussian,
                                 void* stream);
/* The same with the caller's per-block QUIET flags (device, [ceil(N / 64)] bytes, owned by the optimizer; all groups [N, ...] with ONE N, else
 * FGS_ERR_INVALID_ARGUMENT). quiet_blocks[b] = 1 promises that every exp_avg / exp_avg_sq element of Gaussians 64 b .. 64 b + 63 compares equal to 0.0f
 * in every group of the call; 0 promises nothing. A block that is quiet and whose gradient is not needed (live_blocks 0, sentinel +-0) is neither read
 * nor written: with g = m = v = 0 the update is the identity, so memory is bit for bit what fgs_adam_step_multi_live leaves (+-0 aside). The call
 * clears the byte of every block it reads a gradient for and never sets one; fgs_adam_quiet_scan (re)creates the flags. The flags are not used, and all
 * of them are CLEARED (a memset in front of the launch), when the identity cannot be relied on or nothing says which blocks get a gradient: live_blocks
 * NULL, eps <= 0 (as a float) or not finite, a step size or beta that is not finite, a tensor of 2^32 elements or more. NULL = fgs_adam_step_multi_live. */
int32_t fgs_adam_step_multi_quiet(int32_t n_groups, const float* const* grads, float* const* params, float* const* exp_avgs,
                                  float* const* exp_avg_sqs, const int64_t* n_elements, const int32_t* steps, const double* lrs,
                                  double beta1, double beta2, double eps, const uint8_t* live_blocks, const int32_t* floats_per_gaussian,
                                  uint8_t* quiet_blocks, void* stream);
/* quiet_out[b] = 1 exactly when every element of rows 64 b .. 64 b + 63 of every exp_avgs[k] and exp_avg_sqs[k] compares equal to 0.0f (-0 is zero,
 * NaN is not), else 0: one streaming read of the moments, for a caller whose flags may be stale (moments replaced or edited by someone else). Arrays
 * are [host], length n_groups <= 8; all groups must have the same N = n_elements[k] / floats_per_gaussian[k], else FGS_ERR_INVALID_ARGUMENT. */
int32_t fgs_adam_quiet_scan(int32_t n_groups, const float* const* exp_avgs, const float* const* exp_avg_sqs, const int64_t* n_elements,
                            const int32_t* floats_per_gaussian, uint8_t* quiet_out, void* stream);

/* Fused backward + Adam (the reference's FasterGSFused branch, README.md:37; not in /root/reference -- defined here as
 * "equal to fgs_backward followed by FusedAdam.step() on all six groups"). Gradients are never
 * materialised. params/exp_avg/exp_avg_sq are arrays [host] of 6 device pointers in the order
 * means, sh_coefficients_0, sh_coefficients_rest, opacities, scales, rotations (Model.py:238-245); lrs likewise. */
int32_t fgs_backward_adam_fused(const float* grad_image, const float* image,
                                float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                                void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                float* densification_info, void* scratch,
                                int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state,
                                int32_t step, const double* lrs, double beta1, double beta2, double eps, void* stream);

/* ---- Gaussian-sharded multi-GPU path ------------------------------------------------------------------------------
 * The reference is single-GPU (Renderer.py:58-61, no collective anywhere: SURVEY.md D4 / 8e); these four entry points
 * are the MI355X-side addition that lets G ranks each OWN N/G Gaussians and still render whole views: the pipeline of
 * fgs_forward / fgs_backward cut at the two places where per-Gaussian data is small.
 *
 *   owner of a shard, all views of the step at once: fgs_shard_preprocess    K1 -> 56-byte projected records of the visible
 *   -- all-to-all (records of view v go to the rank rendering v) --
 *   renderer of a view:                            fgs_forward_from_records  K2..K10 over the concatenated records
 *                                                  fgs_backward_to_records   K11 -> 36-byte accumulator record per record
 *   -- all-to-all back (segment s returns to the owner of shard s) --
 *   owner, all views at once:                      fgs_shard_backward        K12 on the shard, summing over views
 *
 * A splat record is the private 48-byte projected primitive + its depth key + its tile count; opaque to callers, only
 * its size is ABI. Records of a (shard, view) keep the order K1 compacted them in; accumulator records come back in
 * the same order. */
#define FGS_SPLAT_RECORD_BYTES 56
#define FGS_ACC_RECORD_BYTES 36

/* K1 over the shard for the n_views cameras of the step in one launch per 8 views. settings: [host] array of n_views
 * (same image size and SH layout). records_out: n_views x n_primitives records, view-major (view v starts at record
 * v * n_primitives; its first n_visible[v] are filled). counts_out: n_views x 2 uint32 device words, (n_visible,
 * n_instances) per view -- read them back for all views at once. Requests FGS_BUF_PRIMITIVE only; keep that buffer until
 * fgs_shard_backward of the same step. No host synchronisation. */
int32_t fgs_shard_preprocess(const float* means, const float* scales, const float* rotations, const float* opacities,
                             const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                             int32_t n_views, const fgs_settings* settings, void* records_out, uint32_t* counts_out,
                             fgs_resize_fn resize, void* resize_user, void* stream);

/* fgs_forward with K1 replaced by n_records received records (any concatenation order). n_instances MUST be the sum of
 * the producers' instance counts (their counts_out[1]); it sizes the instance buffer. No host synchronisation. */
int32_t fgs_forward_from_records(const void* records, int32_t n_records, int32_t n_instances, const fgs_settings* settings,
                                 float* image, fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream);

/* The same for records that are the concatenation of n_shards segments (shard_counts[s] records of shard 0, 1, ...: [host] array): the renderer
 * places them interleaved -- rank r of shard s becomes primitive sum_s' min(count[s'], r + [s' < s]) -- which restores the Morton neighbourhood of
 * owners that hold every n_shards-th Gaussian (K11: 0.51 -> 0.43 ms at 3 M Gaussians, 8 shards). Results are those of fgs_forward_from_records up to
 * the summation order of K11's atomics. More than 8 segments, or NULL: as received. Pair with fgs_backward_to_shard_records and the SAME counts. */
int32_t fgs_forward_from_shard_records(const void* records, int32_t n_records, int32_t n_instances, const int32_t* shard_counts, int32_t n_shards,
                                       const fgs_settings* settings, float* image, fgs_resize_fn resize, void* resize_user,
                                       fgs_forward_state* state_out, void* stream);

/* K11 over the buffers of fgs_forward_from_records; acc_records_out[n_records] (36 bytes each, record order).
 * scratch: fgs_backward_scratch_bytes(n_records, width, height). */
int32_t fgs_backward_to_records(const float* grad_image, const float* image,
                                void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                void* scratch, float* acc_records_out, int32_t n_records,
                                const fgs_settings* settings, const fgs_forward_state* state, void* stream);

/* ... over the buffers of fgs_forward_from_shard_records (same shard_counts): the accumulator records come out in the order the records came in. */
int32_t fgs_backward_to_shard_records(const float* grad_image, const float* image,
                                      void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                      void* scratch, float* acc_records_out, int32_t n_records, const int32_t* shard_counts, int32_t n_shards,
                                      const fgs_settings* settings, const fgs_forward_state* state, void* stream);

/* K12 on the shard for all views of the step: acc_records = the accumulator records returned for the records of
 * fgs_shard_preprocess, concatenated in view order (n_visible[v] records for view v, [host] array; same order as they
 * were sent), primitive_buffers = that call's FGS_BUF_PRIMITIVE, settings = the same array. The gradients of each
 * Gaussian are summed over the views and every gradient element is written once (zeros where no view sees it);
 * densification_info [2,N] or NULL is accumulated per visible view as in fgs_backward.
 * scratch: fgs_shard_backward_scratch_bytes(n_primitives, n_views). */
size_t fgs_shard_backward_scratch_bytes(int32_t n_primitives, int32_t n_views);
int32_t fgs_shard_backward(const float* acc_records, const int32_t* n_visible, const void* primitive_buffers,
                           const float* means, const float* scales, const float* rotations, const float* opacities,
                           const float* sh_coefficients_rest,
                           float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                           float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                           float* densification_info, void* scratch, int32_t n_primitives, int32_t n_views,
                           const fgs_settings* settings, void* stream);

/* fgs_shard_backward fused with Adam on the shard (as fgs_backward_adam_fused is for the single-GPU path): the gradients,
 * summed over the n_views <= 8 views in registers / LDS, are never materialised. params / exp_avgs / exp_avg_sqs / lrs:
 * [host] arrays of 6 in optimizer-group order (means, sh_coefficients_0, sh_coefficients_rest, opacities, scales, rotations). */
int32_t fgs_shard_backward_adam_fused(const float* acc_records, const int32_t* n_visible, const void* primitive_buffers,
                                      float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                                      float* densification_info, void* scratch, int32_t n_primitives, int32_t n_views,
                                      const fgs_settings* settings, int32_t step, const double* lrs, double beta1, double beta2, double eps,
                                      void* stream);

/* Test/bench introspection: byte offsets of the named sub-arrays inside a scratch buffer, so tests can compare every
 * intermediate with the oracle. Returns the number of entries written (<= max_entries); names are static strings. */
typedef struct fgs_blob_entry { const char* name; size_t offset; size_t bytes; } fgs_blob_entry;
int32_t fgs_blob_layout(int32_t which, int32_t n_primitives, int32_t width, int32_t height, int32_t n_instances,
                        int32_t n_buckets, fgs_blob_entry* entries, int32_t max_entries);

/* replaces _C.update_3d_filter (filter3d/src/filter3d.cu:40-83). visibility_mask: one byte per point (torch.bool). */
int32_t fgs_update_3d_filter(const float* positions, const float* w2c, float* filter_3d, uint8_t* visibility_mask, int32_t n_points,
                             int32_t width, int32_t height, float focal_x, float focal_y, float center_x, float center_y,
                             float near_plane, float clipping_tolerance, float distance2filter, void* stream);
/* replaces _C.relocation_adjustment (densification/src/densification_api.cu:9-31, kernels_mcmc.cuh:28-59). The binomial table of
 * Eq. (9) (the reference's __constant__ array, kernels_mcmc.cuh:10-26) is produced on the host by fgs_relocation_table
 * (2500 floats) and passed in as a device buffer. */
int32_t fgs_relocation_table(float* table_host_2500);
int32_t fgs_relocation_adjustment(const float* old_opacities, const float* old_scales, const int64_t* n_samples_per_primitive,
                                  const float* table_device, float* new_opacities, float* new_scales, int32_t n_primitives, void* stream);
/* replaces _C.add_noise (densification_api.cu:33-58, kernels_mcmc.cuh:69-127); random_samples ~ N(0,1) [N,3] from the caller. */
int32_t fgs_add_noise(const float* raw_scales, const float* raw_rotations, const float* raw_opacities, const float* random_samples,
                      float* means, int32_t n_primitives, float current_lr, void* stream);

/* "Next" row: maintenance of the Gaussian set between iterations, on the device and INCLUDING the Adam moments
 * (the reference runs Model.py:275-366, 459-463 as torch mask / index / cat chains plus NeRFICG's extend / prune / sort_param_groups).
 *
 * Adaptive density control (Model.py:312-366) in two calls, because the caller owns the new tensors and must size them:
 *   fgs_adc_plan   classifies every Gaussian (clone if small, split if large, above the mean-gradient threshold; prune by opacity,
 *                  degenerate rotation and -- optionally -- size; the verdict for new Gaussians is taken on the values they will have)
 *                  and scans the plan. counts_out [host, 4]: surviving old Gaussians, surviving clones, surviving children PER COPY
 *                  (two copies), Gaussians that are split. New size = counts[0] + counts[1] + 2 * counts[2]. Synchronises the stream.
 *   fgs_adc_apply  writes the new parameter tensors and Adam moments (arrays of 6 in optimizer-group order means, sh_coefficients_0,
 *                  sh_coefficients_rest, opacities, scales, rotations; exp_avgs / exp_avg_sqs and their outputs may all be NULL): survivors
 *                  in their order with their moments, then clones, then first children, then second children, all with zero moments.
 *                  Children: means + R(q) (exp(s) * noise) with noise [2 * counts[3], 3] ~ N(0,1) from the caller (row = copy * counts[3]
 *                  + rank among the split Gaussians, the layout of the reference's randn_like), scales log(0.625 exp(s)).
 *                  When the new size is 0 there is nothing to apply and no tensor to pass: do not call it (NULL tensors are refused).
 * scratch: fgs_adc_scratch_bytes(n) bytes, the same buffer for both calls.
 * Thresholds. The reference compares float32 tensors with Python doubles, which torch rounds to float32 ONCE: log(percent_dense * extent),
 * log(0.1 * extent) and log(min_opacity / (1 - min_opacity)) evaluated in double. fgs_adc_plan_thresholds takes those three values as the caller
 * rounded them (log_small, log_large, min_opacity_logit; NaN is refused) and is what reproduces the reference bit for bit; fgs_adc_plan forms them
 * from its float arguments, i.e. from float(percent_dense) and float(extent), which is one ulp away for about one extent in seven (log_small)
 * and one in two (log_large). Non-finite inputs are not sanitised: the comparisons are the reference's, a NaN scale component makes the largest scale NaN
 * (not small, not too large), a NaN opacity or rotation is not dead, a NaN gradient sum does not densify. */
size_t fgs_adc_scratch_bytes(int32_t n_primitives);
int32_t fgs_adc_plan(const float* densification_info, const float* scales, const float* rotations, const float* opacities, int32_t n_primitives,
                     float grad_threshold, float min_opacity, int32_t prune_large_gaussians, float percent_dense, float extent,
                     void* scratch, int32_t* counts_out, void* stream);
int32_t fgs_adc_plan_thresholds(const float* densification_info, const float* scales, const float* rotations, const float* opacities, int32_t n_primitives,
                                float grad_threshold, float min_opacity_logit, int32_t prune_large_gaussians, float log_small, float log_large,
                                void* scratch, int32_t* counts_out, void* stream);
int32_t fgs_adc_apply(const float* const* params, const float* const* exp_avgs, const float* const* exp_avg_sqs,
                      float* const* out_params, float* const* out_exp_avgs, float* const* out_exp_avg_sqs,
                      const float* noise, const void* scratch, int32_t n_primitives, int32_t total_sh_bases_rest, void* stream);
/* out[k][r, :] = in[k][index[r], :] for k < n_tensors <= 18 float tensors of row widths widths[k] in ONE launch: prune (index = the
 * survivors, Model.py:275-291) and sort (index = the ordering, :293-306) of the six parameters and their twelve moment tensors. */
int32_t fgs_gather_rows(int32_t n_tensors, const float* const* in, float* const* out, const int32_t* widths, const int64_t* index,
                        int32_t n_rows, void* stream);
/* Morton order of the means (Model.py:459-463): order_out[r] = index of the r-th point along a 30-bit Z-curve over the box lo..hi
 * ([device] 3 floats each; 10 bits per axis, x most significant), equal keys in index order (stable). */
size_t fgs_morton_order_temp_bytes(int32_t n_points);
int32_t fgs_morton_order(const float* means, const float* lo, const float* hi, int64_t* order_out, int32_t n_points, void* temp, size_t temp_bytes,
                         void* stream);

/* "Next" row: the loss between forward and backward of every iteration,
 *   loss = lambda_l1 * mean|image - target| + lambda_dssim * (1 - SSIM(image, target))        (Loss.py:15-16, Trainer.py:52-53)
 * replacing torch.nn.functional.l1_loss + NeRFICG's fused_dssim (Optim/Losses/DSSIM.py, not vendored). Writes three device
 * floats out[0] = mean|x-y|, out[1] = mean SSIM, out[2] = the loss (no host sync) and, if grad_image != NULL,
 * dloss/dimage [3,H,W]. scratch: fgs_l1_dssim_scratch_bytes(width, height) bytes, 8-byte aligned (it holds float2 partial sums; a
 * misaligned pointer is refused with FGS_ERR_INVALID_ARGUMENT). */
size_t fgs_l1_dssim_scratch_bytes(int32_t width, int32_t height);
int32_t fgs_l1_dssim_loss(const float* image, const float* target, int32_t width, int32_t height, float lambda_l1, float lambda_dssim,
                          float* out3, float* grad_image, void* scratch, void* stream);
/* The gradient alone, later: dloss/dimage * upstream from the derivative maps that fgs_l1_dssim_loss (with grad_image == NULL or not) left in
 * `scratch` for the same image / target. `upstream` is a DEVICE float (the dL/dloss an autograd engine hands to the loss node) or NULL for 1:
 * the scalar is folded into the kernel, so a framework does not spend a pass over the image on `grad * upstream`. This is the shape of the
 * reference's loss node (fused_dssim: forward saves maps, backward launches one kernel). */
int32_t fgs_l1_dssim_backward(const float* image, const float* target, int32_t width, int32_t height, float lambda_l1, float lambda_dssim,
                              const float* upstream, float* grad_image, const void* scratch, void* stream);
/* The same loss with a per-pixel weight (masks, confidences; INTEGRATION.md "Weighted loss"). weight: fp32 [H,W], shared by the three channels;
 * w^ = w where w > 0, else 0 (negative and NaN count as 0; infinite weights are the caller's error); S = sum w^. Pixels with w^ = 0 are REPLACED BY THE
 * TARGET before the SSIM windows are formed (x'), so a mask boundary plants no edge:
 *   out3[0] = sum w^ |x' - y| / (3 S),  out3[1] = sum w^ SSIM(x', y) / (3 S),  out3[2] = lambda_l1 * out3[0] + lambda_dssim * (1 - out3[1]);
 * S = 0: (0, 1, 0) and a gradient of zeros. dloss/dimage is exactly 0.0f where w^ = 0, and nothing of `image` there is used (NaN included). The weight
 * gets no gradient. All-ones weights give the bits of the unweighted functions. Same conventions as those: device `upstream` or NULL, no host
 * synchronisation, no allocation; scratch of fgs_l1_dssim_weighted_scratch_bytes(width, height) bytes, 8-byte aligned, shared by the two calls. A NULL
 * weight, a NULL required pointer, a non-positive size or a misaligned scratch is refused with FGS_ERR_INVALID_ARGUMENT. */
size_t fgs_l1_dssim_weighted_scratch_bytes(int32_t width, int32_t height);
int32_t fgs_l1_dssim_weighted_loss(const float* image, const float* target, const float* weight, int32_t width, int32_t height, float lambda_l1,
                                   float lambda_dssim, float* out3, float* grad_image, void* scratch, void* stream);
int32_t fgs_l1_dssim_weighted_backward(const float* image, const float* target, const float* weight, int32_t width, int32_t height, float lambda_l1,
                                       float lambda_dssim, const float* upstream, float* grad_image, const void* scratch, void* stream);

/* ---- Per-view bilateral-grid colour correction between the rasterizer and the loss (csrc/bilagrid.hip; INTEGRATION.md "Bilateral grids") ----
 * grid: fp32 [12, grid_l, grid_h, grid_w], contiguous, every extent >= 1; channel 4 i + j is entry (i, j) of a 3 x 4 matrix [A | b]. For pixel (px, py)
 * of image [3, height, width] (any range):  u = (px + 0.5) / width * (grid_w - 1), v = (py + 0.5) / height * (grid_h - 1),
 * g = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1), z = g * (grid_l - 1), M = trilinear interpolation of grid at (z, v, u) (corner indices clamped to
 * the grid), out_i = sum_j M[4 i + j] * C_j + M[4 i + 3]  ==  F.grid_sample(grid[None], 2 (x, y, g) - 1, bilinear, align_corners=True, border) followed
 * by the matrix product. Every call refuses (FGS_ERR_INVALID_ARGUMENT, text in fgs_last_error) a NULL required pointer, a non-positive extent or image
 * size, a grid of more than 2^31 - 1 floats, and `out` overlapping `image`. No host synchronisation, no allocation; all work on `stream`. */
int32_t fgs_bilagrid_slice(const float* grid, int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* image, int32_t width, int32_t height,
                           float* out, void* stream);
/* Gradients for an upstream grad_out [3,H,W]: grad_grid [12, L, Hg, Wg] (OVERWRITTEN; summed with float atomics: the last bits depend on their order)
 * and grad_image [3,H,W] (written per pixel: deterministic). The guide carries no gradient where it is clamped. Either may be NULL (it then costs
 * nothing); both NULL is refused. scratch: fgs_bilagrid_scratch_bytes bytes, 4-byte aligned, required with grad_grid; the call clears it itself. */
size_t fgs_bilagrid_scratch_bytes(int32_t grid_w, int32_t grid_h, int32_t grid_l);
int32_t fgs_bilagrid_slice_backward(const float* grid, int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* image, const float* grad_out,
                                    int32_t width, int32_t height, float* grad_grid, float* grad_image, void* scratch, void* stream);
/* 1: the two calls above stage the lattice points under each 64 x 16 pixel tile in LDS for this grid and image size; 0: that part exceeds the
 * kernels' LDS budget somewhere and they read the grid from global memory; negative: fgs_status (non-positive argument). */
int32_t fgs_bilagrid_staged(int32_t grid_w, int32_t grid_h, int32_t grid_l, int32_t width, int32_t height);
/* Total variation of one grid, tv = sum over the axes z, y, x of mean((G[next along the axis] - G)^2) over all 12 channels (an axis of extent 1
 * contributes 0): loss = one DEVICE float, grad_grid [12, L, Hg, Wg] = d tv / dG (overwritten) or NULL. One launch, sums in a fixed order. */
int32_t fgs_bilagrid_tv(const float* grid, int32_t grid_w, int32_t grid_h, int32_t grid_l, float* loss, float* grad_grid, void* stream);

/* ---- Normal-consistency regulariser of 2DGS, L_n = sum_i w_i (1 - n_i . N) (csrc/normal_consistency.hip; INTEGRATION.md "Normal consistency") ----
 * Two pairs of calls either side of fgs_blend_features / fgs_backward_features over five channels. All tensors fp32, contiguous, on the current device;
 * outputs caller-allocated; no host synchronisation, no allocation; all work on `stream`. Refused with FGS_ERR_INVALID_ARGUMENT and a text in
 * fgs_last_error, before anything is written: a NULL required pointer, a negative n_primitives, a non-positive width / height / focal length, min_alpha
 * outside (0, 1], rotations / grad_rotations that are not 16-byte aligned.
 *
 * Surface features: features [n_primitives, 5], row i = (n_cam, z_i, 1). k = index of the smallest of the three log-scales (the lowest index on an exact
 * tie), a = column k of quat_to_rotation(rotations[i]) (raw (r, x, y, z), normalised inside), s = -1 if a . (means[i] - cam_position) > 0 else +1,
 * n_cam = w2c[0:3,0:3] (s a), z_i = w2c[2,0:3] . means[i] + w2c[2,3]. w2c: rows of four floats, rows 0..2 read. n_primitives == 0 is valid (nothing is
 * written; the per-Gaussian pointers may then be NULL). */
int32_t fgs_surface_features(const float* means, const float* scales, const float* rotations, int32_t n_primitives, const float* w2c,
                             const float* cam_position, float* features, void* stream);
/* Gradients for an upstream grad_features [n_primitives, 5]: grad_rotations [n_primitives, 4] (through the rotation's normalisation) and grad_means
 * [n_primitives, 3] (= grad_features[:, 3] w2c[2,0:3]), each written plainly in every row when its need_* flag is set and left alone (it may be NULL,
 * it costs nothing) otherwise. No gradient for the scales (the choice of k and the sign are piecewise constant), none from channel 4. */
int32_t fgs_surface_features_backward(const float* means, const float* scales, const float* rotations, int32_t n_primitives, const float* w2c,
                                      const float* cam_position, const float* grad_features, int32_t need_rotations, int32_t need_means,
                                      float* grad_rotations, float* grad_means, void* stream);
/* Normal consistency of a blended map surface_map [5, height, width] = (N_r, D, A): with d = D / A, ray(q) = ((qx + 0.5 - center_x) / focal_x,
 * (qy + 0.5 - center_y) / focal_y, 1), P = ray d, gx = P(p + (1,0)) - P(p - (1,0)), gy = P(p + (0,1)) - P(p - (0,1)), c = gy x gx, n_d = c / |c|:
 * consistency[p] = A(p) - N_r(p) . n_d(p) where p is valid -- not on the image border, A >= min_alpha at p and at its four neighbours, |c|^2 > 1e-30 --
 * and exactly 0 elsewhere (D / A is not formed there). normals [3, height, width]: n_d, zeros where invalid; NULL = not wanted. An image without an
 * interior pixel (width or height < 3) is valid: the outputs are zero. */
int32_t fgs_normal_consistency(const float* surface_map, int32_t width, int32_t height, float focal_x, float focal_y, float center_x, float center_y,
                               float min_alpha, float* consistency, float* normals, void* stream);
/* grad_map [5, height, width] for an upstream grad_consistency [height, width]; every element is written (zero where no valid pixel reaches it). The
 * depth gradient is a gather -- the thread of a pixel recomputes the up to four valid centres it is a neighbour of -- without float atomics: two calls
 * on the same inputs return the same bits. */
int32_t fgs_normal_consistency_backward(const float* surface_map, const float* grad_consistency, int32_t width, int32_t height, float focal_x, float focal_y,
                                        float center_x, float center_y, float min_alpha, float* grad_map, void* stream);

/* ---- TSDF fusion and mesh extraction (csrc/tsdf.hip; INTEGRATION.md "Surface extraction") ----
 * Volume: a dense lattice of nx x ny x nz points, x fastest; point (i,j,k) lies at origin + voxel_size (i,j,k) in world space.
 *   tsdf_weight  fp32 [nz,ny,nx,2]: tsdf in [-1,1] and the accumulated weight, 8-byte aligned;
 *   color        fp32 PLANAR [3,nz,ny,nx] (a wave's 64 points are contiguous in every channel), or NULL.
 * Zeroed buffers are an empty volume. Every call below refuses (FGS_ERR_INVALID_ARGUMENT, text in fgs_last_error, before anything touches the GPU)
 * an extent < 2, nx ny nz > 2^28, voxel_size <= 0, a NULL required pointer and a misaligned tsdf_weight.
 *
 * fgs_tsdf_integrate folds n_views views (1..FGS_TSDF_MAX_VIEWS, all width x height) into the volume in ONE launch, in argument order. For a lattice
 * point p and a view:  c = R p + t (w2c rows 0..2), z = c.z, skip if z <= near_plane;  u = focal_x c.x / z + center_x, v = focal_y c.y / z + center_y
 * (the meaning of fgs_settings; pixel px covers [px, px + 1), the blend evaluates it at px + 0.5), px = floor(u), py = floor(v), skip outside the image;
 * d = depth[py,px] (view-space z: fgs_inference_aux's median depth, or its expected depth divided by alpha), skip if d <= 0, d > depth_max, or
 * alpha[py,px] < min_alpha where an opacity map is given;  sdf = d - z, skip if sdf < -trunc, f = min(1, sdf / trunc);  w' = w + 1,
 * tsdf = (tsdf w + f) / w', colour likewise, w = min(w', max_weight). Nearest pixel, no interpolation. A point that no view of the call updates is
 * not written. The kernel multiplies by fp32 reciprocals (1/z, 1/trunc, 1/w') where the formulas divide: a last-bit difference. One call with V views equals V single-view calls in the same order bit for bit. With a colour volume every view needs a colour map;
 * without one the maps are ignored. Also refused: trunc <= 0, max_weight < 1, a non-positive image size, n_views outside 1..8, a view without w2c / depth. */
#define FGS_TSDF_MAX_VIEWS 8
typedef struct fgs_tsdf_view {
    const float* w2c;                                /* DEVICE: row-major world-to-camera, rows 0..2 (12 floats) */
    float focal_x, focal_y, center_x, center_y;
    const float* depth;                              /* DEVICE [height, width] */
    const float* alpha;                              /* DEVICE [height, width] or NULL */
    const float* color;                              /* DEVICE [3, height, width] or NULL */
} fgs_tsdf_view;
int32_t fgs_tsdf_integrate(float* tsdf_weight, float* color, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z,
                           float voxel_size, float trunc, const fgs_tsdf_view* views, int32_t n_views, int32_t width, int32_t height, float near_plane,
                           float depth_max, float min_alpha, float max_weight, void* stream);
/* Mesh of the level set {tsdf = iso}: marching tetrahedra on the Kuhn split, no case table. A cube (i,j,k) is valid when its eight corners have
 * weight >= min_weight; it is cut into six tetrahedra, one per permutation (p1,p2,p3) of the axes in lexicographic order: v0 = (0,0,0), v1 = v0 + e_p1,
 * v2 = v1 + e_p2, v3 = (1,1,1). An edge runs from a lattice point a to b = a + d, d in {0,1}^3 \ {0} (type 1..7 = d.x + 2 d.y + 4 d.z) and is owned by
 * a; it carries a vertex when both ends are valid and (f_a < iso) != (f_b < iso), at a + d voxel_size (iso - f_a) / (f_b - f_a), colour interpolated
 * alike. Vertices are ordered by owner (linear lattice index), then type; triangles by cube, then tetrahedron (1 for a 1|3 split, 2 for 2|2); normals
 * point from f < iso towards f >= iso. A corner with f == iso counts as outside, which yields zero-area triangles: they are KEPT, the index topology
 * is closed because of them. Both orders are deterministic: two runs give the same bytes.
 *   fgs_tsdf_mesh_count: classifies and scans into `scratch` (fgs_tsdf_mesh_scratch_bytes; 0 for a refused size; 8-byte aligned), then waits for
 *     `stream` and returns the two sizes in HOST counts[2] = (n_vertices, n_triangles). (0, 0) is a normal result.
 *   fgs_tsdf_mesh_emit: fills vertices [Nv,3], colors [Nv,3] (NULL = none; needs `color`) and faces [Nf,3] from the SAME volume, parameters and scratch
 *     the count call saw; nothing is written past the given sizes. Sizes (0, 0) launch nothing; a NULL output with a non-zero size is refused. */
size_t fgs_tsdf_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int32_t fgs_tsdf_mesh_count(const float* tsdf_weight, int32_t nx, int32_t ny, int32_t nz, float iso, float min_weight, void* scratch, int64_t* counts,
                            void* stream);
int32_t fgs_tsdf_mesh_emit(const float* tsdf_weight, const float* color, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y,
                           float origin_z, float voxel_size, float iso, float min_weight, const void* scratch, int64_t n_vertices, int64_t n_triangles,
                           float* vertices, float* colors, int32_t* faces, void* stream);

/* Optional per-stage timing. While enabled (1), every pipeline stage is bracketed by hipEvents recorded on the caller's stream
 * (each event costs a few microseconds of GPU idle time: ~0.2 ms per training iteration with all stages on); enable = 2 + k brackets
 * only stage k (its index in the table fgs_profile_read returns), which leaves a timed loop practically undisturbed;
 * fgs_profile_read() waits for them, returns accumulated milliseconds + launch counts per stage since the last read and
 * clears the records. Not thread-safe; intended for bench.py (roofline) and tests. */
typedef struct fgs_stage_time { const char* name; double total_ms; int64_t calls; } fgs_stage_time;
int32_t fgs_profile_enable(int32_t enable);
int32_t fgs_profile_read(fgs_stage_time* out, int32_t max_entries);

/* Device self-test of the wave64 primitives (DPP shift/rotate direction, ballot prefix, readlane); writes 256 words that
 * tests/test_gpu_parity.py checks against the expected pattern. which == FGS_BUF_COUNT in fgs_blob_layout describes the
 * backward scratch buffer. */
int32_t fgs_debug_wave_selftest(uint32_t* out_device_256, void* stream);

/* Test hook for the binning stage's radix sort (csrc/radix_sort.hip): stable sort of n (key, uint32 value) pairs on key bits
 * [0, end_bit); key_bytes 2 or 4. Returns 0 / 1 = the buffer pair that holds the result, or a negative fgs_status. */
size_t fgs_debug_radix_sort_temp_bytes(int32_t n, int32_t end_bit);
int32_t fgs_debug_radix_sort(void* keys0, void* keys1, uint32_t* vals0, uint32_t* vals1, int32_t n, int32_t key_bytes, int32_t end_bit,
                             void* temp, size_t temp_bytes, void* stream);
/* The same hook for the depth sort as the forward pass runs it (K2): keys are the bit patterns of float depths in [near_plane, far_plane]
 * (everything else is culled in preprocess, kernels_forward.cuh:67), sorted as key - bits(near_plane) in as few 9-bit passes as the range
 * needs (fgs_debug_set_option(9, m) selects the variants). temp as for fgs_debug_radix_sort with end_bit 32. */
int32_t fgs_debug_depth_sort(uint32_t* keys0, uint32_t* keys1, uint32_t* vals0, uint32_t* vals1, int32_t n, float near_plane, float far_plane,
                             void* temp, size_t temp_bytes, void* stream);
/* ---- libfgs_hip_dev.so only (built with -DFGS_DEV_SWITCHES: `make -C faster-gaussian-splatting_amd/csrc dev`). The product library has ONE formulation
 * of every kernel and no process-wide switches (every switch below is a compile-time constant there, csrc/fgs_kernels.h: FGS_SWITCH); the A/B tools
 * under tools/ and the variant tests load the dev library. The K11 formulations other than 3 are kernels of csrc/blend_backward_exhibits.hip,
 * a unit that only the dev library is built from. ---- */
#ifdef FGS_DEV_SWITCHES
/* Selects the blend-backward formulation: 3 (default) = live-bucket list + compacted pixels + two-value pipeline state, 2 / 0 =
 * round-1 systolic form (dL/dC from global memory / LDS), 1 = strip (lane = pixel, DPP reductions), 4 = lane = pixel walk with the
 * per-Gaussian sums reduced on the matrix cores (round 4; measured against 3 in profiles/r04_k11m_closeout.txt). A/B switch for tests and
 * bench: process-wide, unsynchronised; all variants must give the same gradients. */
int32_t fgs_debug_set_backward_variant(int32_t variant);
/* Tuning switches for A/B measurements inside one process (process-wide, unsynchronised: bench / test processes only):
 * key 0 = blend-backward variant, 1 = Adam float4 pieces per thread (1, 2, 4), 2 = Adam non-temporal accesses, 3 = fused
 * backward+Adam as one kernel (1, default) or round 1's two (0), 5 = K1 tile counting: 0 flattened (default) or n sequential
 * candidates per lane, 7 = K11 timing experiments (results WRONG: 1 no atomics, 2 no step loop; variant 4: 4 no
 * matrix instructions / write-out, 8 no pair arithmetic),
 * 8 = Adam walks the arenas from the end (1, default) or the start (0), 9 = depth sort: bit 0 key - bits(near) in 9-bit passes, bit 1
 * 2048-item workgroups (1 default; 0 = round 1: 4 x 8 bits, 4096 items; bit 1 measured slower), 10 = forward-blend tile -> workgroup
 * mapping: 252 (default) = one vertical strip of tile columns per XCD, walked row by row from the top (251: from the bottom), 0 = one
 * contiguous band of tile rows per XCD (rounds 1-2), g = 1..64 = groups of g rows dealt to the XCDs in turn, 255 = the bands walked
 * bottom-up, 254 = blocks of tiles weighed and dealt to the XCDs on the device (plan_tiles_kernel), 253 = the bands read through the plan
 * table (csrc/fgs_k10_mappings.h has the measurements; the product library always runs 252), 11 = 1: rocPRIM scan for the per-tile bucket offsets (and no block plan), 12 = 1: the
 * block plan without sorting (XCD x = block column x), 13 = upper bound of the grid of blend-backward variant 4, 16 = loss kernels: bit 0 the tiled
 * forward kernel, bit 1 the tiled backward kernel of csrc/loss_exhibits.hip (0 default: the streaming kernels of csrc/loss.hip).
 * Apart from key 7, results never depend on them (key 16: derivative maps and gradient bit for bit; the loss scalars and the weighted loss's S are
 * sums over the forward kernel's units and differ in their last bits). */
int32_t fgs_debug_set_option(int32_t key, int32_t value);

#endif /* FGS_DEV_SWITCHES */

#ifdef __cplusplus
}
#endif
#endif /* FGS_HIP_H */

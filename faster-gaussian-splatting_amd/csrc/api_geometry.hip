// C-ABI entry points of the one render of the 2DGS regularisers (blend_geometry.hip): argument checks, the carve of the forward pass's blobs, the
// launches. The backward entry point is fgs_backward_reached's pass with one more blend kernel between K11 and K12, dL/dz on the way that
// fgs_backward_aux's takes, and grad_surface_features cleared in front of it -- the shape of fgs_backward_distortion.
#include "fgs_host.h"
#include "fgs_geometry.h"

using namespace fgs;
namespace {
// 0, or the refusal: the mode, its planes, and buffers this render can walk
int check_geometry(const fgs_settings* settings, const fgs_forward_state* state, int32_t mode) {
    if (mode != FGS_DISTORTION_LINEAR && mode != FGS_DISTORTION_NORMALIZED)
        return fail(FGS_ERR_INVALID_ARGUMENT, "distortion mode %d: FGS_DISTORTION_LINEAR (0) or FGS_DISTORTION_NORMALIZED (1)", mode);
    if (mode == FGS_DISTORTION_NORMALIZED && !(settings->near_plane > 0.0f && settings->far_plane > settings->near_plane))
        return fail(FGS_ERR_INVALID_ARGUMENT, "the normalized distortion needs 0 < near_plane < far_plane, not near %g far %g", settings->near_plane, settings->far_plane);
    if (state->selector & kStateAsyncCounts)
        return fail(FGS_ERR_INVALID_ARGUMENT, "the geometry render needs the buffers of a synchronous forward pass (fgs_forward / fgs_forward_aux), these are fgs_forward_async's");
    if (state->selector & kStateFromRecords)
        return fail(FGS_ERR_INVALID_ARGUMENT, "the geometry render does not take the sharded / record paths: these buffers were filled from splat records");
    return FGS_OK;
}

GeometryArgs geometry_args(const PrimitiveBuffers& pb, const TileBuffers& tb, const InstanceBuffers& ib, const Geometry& geo, const fgs_settings& settings,
                           const fgs_forward_state& state, const float* means, const float* surface_features, int32_t mode) {
    GeometryArgs a{};
    a.ranges = tb.ranges; a.inst_prims = ib.prims[state.selector & 1]; a.rec = pb.rec;
    a.n_processed = tb.n_processed; a.max_n_processed = tb.max_n_processed;
    a.means = means; a.w2c = settings.w2c; a.features = surface_features;
    a.width = settings.width; a.height = settings.height; a.grid_w = geo.grid_w; a.grid_h = geo.grid_h; a.n_tiles = geo.n_tiles;
    a.normalized = mode == FGS_DISTORTION_NORMALIZED ? 1 : 0;
    a.depth_scale = a.normalized ? settings.far_plane * settings.near_plane / (settings.far_plane - settings.near_plane) : 1.0f;
    a.proper_aa = settings.proper_antialiasing ? 1 : 0;
    return a;
}
}  // namespace

extern "C" {
#pragma GCC visibility push(default)
int32_t fgs_blend_geometry(const float* means, const float* surface_features, const void* primitive_buffers, const void* tile_buffers,
                           const void* instance_buffers, int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, int32_t mode,
                           float* geometry_state, void* stream_) {
    if (int rc = check_settings(settings)) return rc;
    if (!state || n_primitives < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad state / n_primitives");
    if (int rc = check_geometry(settings, state, mode)) return rc;
    if (!geometry_state) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL geometry_state");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Geometry geo = geometry_of(settings->width, settings->height);
    if (n_primitives == 0) {               // nothing was blended: a zero state, nothing else is touched
        FGS_HIP(hipMemsetAsync(geometry_state, 0, sizeof(float) * kGeometryPlanes * static_cast<size_t>(settings->width) * settings->height, stream));
        return FGS_OK;
    }
    if (!means) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL means");
    if (!surface_features) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL surface_features");
    if (!primitive_buffers || !tile_buffers || (state->n_instances > 0 && !instance_buffers)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL scratch buffer");
    Carver pc(const_cast<void*>(primitive_buffers)), tc(const_cast<void*>(tile_buffers)), ic(const_cast<void*>(instance_buffers));
    const PrimitiveBuffers pb = PrimitiveBuffers::carve(pc, static_cast<uint32_t>(n_primitives));
    const TileBuffers tb = TileBuffers::carve(tc, geo.n_tiles, true);
    const InstanceBuffers ib = InstanceBuffers::carve(ic, static_cast<uint32_t>(state->n_instances), geo.key_bytes, geo.end_bit);
    GeometryArgs a = geometry_args(pb, tb, ib, geo, *settings, *state, means, surface_features, mode);
    a.state = geometry_state;
    StageScope t(ST_BLEND_FORWARD, stream);
    FGS_HIP(launch_blend_geometry(a, stream));
    return FGS_OK;
}

int32_t fgs_backward_geometry(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                              const float* means, const float* scales, const float* rotations, const float* opacities,
                              const float* sh_coefficients_rest,
                              void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                              float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                              float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                              float* densification_info, void* scratch,
                              int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                              uint8_t* reached_blocks, const float* surface_features, const float* geometry_state, const float* grad_distortion,
                              const float* grad_surface_map, float* grad_surface_features, int32_t mode, void* stream_) {
    if (!grad_distortion && !grad_surface_map)     // neither map in the loss: the pass, its scratch layout and its refusals are fgs_backward_reached's
        return fgs_backward_reached(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                                    primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                                    grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                                    reached_blocks, stream_);
    const bool with_maps = grad_alpha != nullptr || grad_depth != nullptr;
    BackwardPlan P;                        // the aux scratch layout: dL/dz of the distortion term lives in its acc_z
    if (int rc = plan_backward(P, {primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, scratch}, n_primitives, settings, state, true)) return rc;
    if (!grad_image || !image) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL image / grad_image");
    if (int rc = check_geometry(settings, state, mode)) return rc;
    if (!geometry_state) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL geometry_state");
    if (grad_depth && !(state->selector & kStateDepthCheckpoints))
        return fail(FGS_ERR_INVALID_ARGUMENT, "grad_depth needs the depth checkpoints that fgs_forward_aux writes: these buffers were filled by a forward pass without them");
    if (grad_depth && !depth_expected) return fail(FGS_ERR_INVALID_ARGUMENT, "grad_depth without depth_expected (the map fgs_forward_aux returned)");
    if (n_primitives == 0) return FGS_OK;
    if (!means || !scales || !rotations || !opacities || !grad_means || !grad_scales || !grad_rotations || !grad_opacities || !grad_sh_coefficients_0)
        return fail(FGS_ERR_INVALID_ARGUMENT, "NULL parameter / gradient tensor");
    if (!surface_features || !grad_surface_features) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL surface_features / grad_surface_features");
    if (settings->total_sh_bases_rest > 0 && !grad_sh_coefficients_rest) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL grad_sh_coefficients_rest");
    if (!g_fused_single_kernel) return fail(FGS_ERR_INVALID_ARGUMENT, "the geometry gradient goes through the one-kernel K12 only (dev option: the two-kernel form is selected)");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t n = static_cast<uint32_t>(n_primitives);

    // K11: with map gradients its staging pass clears acc_z and its last kernels fold the hot replicas of it; without them acc_z is cleared here
    if (with_maps) { if (int rc = run_blend_backward_aux(P, grad_image, image, grad_alpha, grad_depth, depth_expected, means, stream)) return rc; }
    else {
        if (int rc = run_blend_backward(P, grad_image, image, stream)) return rc;
        FGS_HIP(hipMemsetAsync(P.sc.acc_z, 0, sizeof(float) * n, stream));
    }
    // behind K11's last kernel (the hot replicas are folded, the records are marked dirty), in front of K12: both terms add into the same records
    {
        GeometryArgs g = geometry_args(P.pb, P.tb, P.ib, P.geo, *settings, *state, means, surface_features, mode);
        g.state_in = geometry_state; g.grad_x = grad_distortion; g.grad_m = grad_surface_map;
        g.acc = P.pb.acc; g.acc_z = P.sc.acc_z; g.grad_features = grad_surface_features;
        StageScope t(ST_BLEND_BACKWARD, stream);
        FGS_HIP(hipMemsetAsync(grad_surface_features, 0, sizeof(float) * static_cast<size_t>(n) * kGeometryChannels, stream));
        FGS_HIP(launch_blend_geometry_backward(g, stream));
    }
    PreprocessBackwardArgs a{};
    ShRestArgs sh{};
    fill_backward_args(a, sh, {means, scales, rotations, opacities, nullptr, sh_coefficients_rest}, n, 1, *settings);
    set_backward_view(a, sh, 0, backward_view(*settings, P.geo, P.pb.n_touched, nullptr, P.pb.acc, P.sc.view_dir));
    a.view[0].acc_z = P.sc.acc_z;          // dL/dz is part of K12's "did the blend pass reach it" test, flags included
    a.grad_means = grad_means; a.grad_scales = grad_scales; a.grad_rotations = grad_rotations; a.grad_opacities = grad_opacities;
    a.grad_sh0 = grad_sh_coefficients_0; a.densification_info = densification_info;
    sh.grad_sh_rest = grad_sh_coefficients_rest;
    a.live_blocks = live_blocks; a.reached_blocks = reached_blocks;
    StageScope t(ST_PREPROCESS_BACKWARD, stream);
    FGS_HIP(launch_backward_gradients(a, sh, stream));                                  // K12
    // z_i's own dependence on mean_i: grad_means += dL/dz w2c[2, 0:3], after K12 has written every element
    FGS_HIP(launch_depth_mean_gradient(P.sc.acc_z, P.pb.n_touched, settings->w2c, grad_means, n, stream));
    return FGS_OK;
}
#pragma GCC visibility pop
}  // extern "C"

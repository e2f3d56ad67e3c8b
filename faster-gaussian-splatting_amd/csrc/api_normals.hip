// C-ABI entry points of the normal-consistency regulariser (normal_consistency.hip): argument checks, the degenerate shapes, the launches.
#include "fgs_host.h"

using namespace fgs;
namespace {
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// 0, or the refusal: the Gaussian count, the camera, the three parameter tensors (which may be NULL only when there is no Gaussian)
int check_surface_inputs(const char* who, const float* means, const float* scales, const float* rotations, int32_t n, const float* w2c, const float* cam_position) {
    if (n < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: n_primitives %d is negative", who, n);
    if (!w2c || !cam_position) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: NULL w2c / cam_position", who);
    if (n > 0 && (!means || !scales || !rotations)) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: NULL means / scales / rotations", who);
    if (!aligned16(rotations)) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: rotations must be 16-byte aligned", who);
    return FGS_OK;
}

// 0, or the refusal: image size, intrinsics and threshold of the image-space pair
int check_consistency_inputs(const char* who, int32_t width, int32_t height, float fx, float fy, float min_alpha) {
    if (width <= 0 || height <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: image size %dx%d must be positive", who, width, height);
    if (!(fx > 0.0f) || !(fy > 0.0f)) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: focal lengths %g, %g must be positive", who, fx, fy);
    if (!(min_alpha > 0.0f && min_alpha <= 1.0f)) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: min_alpha %g outside (0, 1]", who, min_alpha);
    return FGS_OK;
}

NormalConsistencyArgs consistency_args(const float* surface_map, int32_t width, int32_t height, float fx, float fy, float cx, float cy, float min_alpha) {
    NormalConsistencyArgs a{};
    a.map = surface_map; a.width = width; a.height = height;
    a.inv_fx = 1.0f / fx; a.inv_fy = 1.0f / fy; a.cx = cx; a.cy = cy; a.min_alpha = min_alpha;
    return a;
}
}  // namespace

extern "C" {
#pragma GCC visibility push(default)
int32_t fgs_surface_features(const float* means, const float* scales, const float* rotations, int32_t n_primitives, const float* w2c,
                             const float* cam_position, float* features, void* stream) {
    if (int st = check_surface_inputs("surface_features", means, scales, rotations, n_primitives, w2c, cam_position)) return st;
    if (n_primitives == 0) return FGS_OK;
    if (!features) return fail(FGS_ERR_INVALID_ARGUMENT, "surface_features: NULL features");
    SurfaceFeatureArgs a{};
    a.means = means; a.scales = scales; a.rotations = rotations; a.w2c = w2c; a.cam_position = cam_position; a.n = n_primitives; a.features = features;
    FGS_HIP(launch_surface_features(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

int32_t fgs_surface_features_backward(const float* means, const float* scales, const float* rotations, int32_t n_primitives, const float* w2c,
                                      const float* cam_position, const float* grad_features, int32_t need_rotations, int32_t need_means,
                                      float* grad_rotations, float* grad_means, void* stream) {
    if (int st = check_surface_inputs("surface_features_backward", means, scales, rotations, n_primitives, w2c, cam_position)) return st;
    if (n_primitives == 0) return FGS_OK;
    if (!grad_features) return fail(FGS_ERR_INVALID_ARGUMENT, "surface_features_backward: NULL grad_features");
    if (need_rotations && !grad_rotations) return fail(FGS_ERR_INVALID_ARGUMENT, "surface_features_backward: need_rotations with a NULL grad_rotations");
    if (need_means && !grad_means) return fail(FGS_ERR_INVALID_ARGUMENT, "surface_features_backward: need_means with a NULL grad_means");
    if (need_rotations && !aligned16(grad_rotations)) return fail(FGS_ERR_INVALID_ARGUMENT, "surface_features_backward: grad_rotations must be 16-byte aligned");
    SurfaceFeatureArgs a{};
    a.means = means; a.scales = scales; a.rotations = rotations; a.w2c = w2c; a.cam_position = cam_position; a.n = n_primitives;
    a.grad_features = grad_features;
    a.grad_rotations = need_rotations ? grad_rotations : nullptr;
    a.grad_means = need_means ? grad_means : nullptr;
    FGS_HIP(launch_surface_features_backward(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

int32_t fgs_normal_consistency(const float* surface_map, int32_t width, int32_t height, float focal_x, float focal_y, float center_x, float center_y,
                               float min_alpha, float* consistency, float* normals, void* stream_) {
    if (!surface_map || !consistency) return fail(FGS_ERR_INVALID_ARGUMENT, "normal_consistency: NULL surface_map / consistency");
    if (int st = check_consistency_inputs("normal_consistency", width, height, focal_x, focal_y, min_alpha)) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const size_t plane = static_cast<size_t>(width) * height;
    if (width < 3 || height < 3) {                                        // no interior pixel: the maps are zero
        FGS_HIP(hipMemsetAsync(consistency, 0, sizeof(float) * plane, stream));
        if (normals) FGS_HIP(hipMemsetAsync(normals, 0, sizeof(float) * 3 * plane, stream));
        return FGS_OK;
    }
    NormalConsistencyArgs a = consistency_args(surface_map, width, height, focal_x, focal_y, center_x, center_y, min_alpha);
    a.E = consistency; a.normals = normals;
    FGS_HIP(launch_normal_consistency(a, stream));
    return FGS_OK;
}

int32_t fgs_normal_consistency_backward(const float* surface_map, const float* grad_consistency, int32_t width, int32_t height, float focal_x, float focal_y,
                                        float center_x, float center_y, float min_alpha, float* grad_map, void* stream_) {
    if (!surface_map || !grad_consistency || !grad_map) return fail(FGS_ERR_INVALID_ARGUMENT, "normal_consistency_backward: NULL surface_map / grad_consistency / grad_map");
    if (int st = check_consistency_inputs("normal_consistency_backward", width, height, focal_x, focal_y, min_alpha)) return st;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (width < 3 || height < 3) {                                        // no interior pixel: the gradient is zero
        FGS_HIP(hipMemsetAsync(grad_map, 0, sizeof(float) * 5 * static_cast<size_t>(width) * height, stream));
        return FGS_OK;
    }
    NormalConsistencyArgs a = consistency_args(surface_map, width, height, focal_x, focal_y, center_x, center_y, min_alpha);
    a.grad_E = grad_consistency; a.grad_map = grad_map;
    FGS_HIP(launch_normal_consistency_backward(a, stream));
    return FGS_OK;
}
#pragma GCC visibility pop
}  // extern "C"

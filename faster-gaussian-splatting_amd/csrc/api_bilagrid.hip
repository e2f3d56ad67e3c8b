// C-ABI entry points of the bilateral-grid colour correction (bilagrid.hip): argument checks, the scratch grid's clear, the launches.
#include "fgs_host.h"

using namespace fgs;
namespace {
// 0, or the refusal: extents and image size positive, the grid addressable with 32-bit indices
int check_bilagrid_extents(int32_t gw, int32_t gh, int32_t gl) {
    if (gw <= 0 || gh <= 0 || gl <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid: grid extents %d x %d x %d must be positive", gw, gh, gl);
    if (static_cast<int64_t>(gw) * gh * gl * 12 > 0x7fffffff) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid: a grid of %d x %d x %d has more than 2^31 - 1 floats", gw, gh, gl);
    return FGS_OK;
}
int check_bilagrid_image(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid: image size %dx%d must be positive", width, height);
    return FGS_OK;
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
}  // namespace

extern "C" {
#pragma GCC visibility push(default)
size_t fgs_bilagrid_scratch_bytes(int32_t grid_w, int32_t grid_h, int32_t grid_l) {
    if (grid_w <= 0 || grid_h <= 0 || grid_l <= 0 || static_cast<int64_t>(grid_w) * grid_h * grid_l * 12 > 0x7fffffff) return 0;
    return sizeof(float) * 12 * static_cast<size_t>(grid_w) * grid_h * grid_l;
}

int32_t fgs_bilagrid_staged(int32_t grid_w, int32_t grid_h, int32_t grid_l, int32_t width, int32_t height) {
    if (int st = check_bilagrid_extents(grid_w, grid_h, grid_l)) return st;
    if (int st = check_bilagrid_image(width, height)) return st;
    return bilagrid_staged(grid_w, grid_h, grid_l, width, height) ? 1 : 0;
}

int32_t fgs_bilagrid_slice(const float* grid, int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* image, int32_t width, int32_t height,
                           float* out, void* stream) {
    if (!grid || !image || !out) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_slice: NULL grid / image / out");
    if (int st = check_bilagrid_extents(grid_w, grid_h, grid_l)) return st;
    if (int st = check_bilagrid_image(width, height)) return st;
    const size_t n = 3 * static_cast<size_t>(width) * height;
    if (out < image + n && image < out + n) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_slice: out aliases image");
    BilagridArgs a{};
    a.grid = grid; a.gw = grid_w; a.gh = grid_h; a.gl = grid_l; a.image = image; a.width = width; a.height = height; a.out = out;
    a.vec4 = width % 4 == 0 && aligned16(image) && aligned16(out);
    FGS_HIP(launch_bilagrid_slice(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

int32_t fgs_bilagrid_slice_backward(const float* grid, int32_t grid_w, int32_t grid_h, int32_t grid_l, const float* image, const float* grad_out,
                                    int32_t width, int32_t height, float* grad_grid, float* grad_image, void* scratch, void* stream_) {
    if (!grid || !image || !grad_out) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_slice_backward: NULL grid / image / grad_out");
    if (!grad_grid && !grad_image) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_slice_backward: grad_grid and grad_image are both NULL");
    if (grad_grid && !scratch) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_slice_backward: grad_grid needs scratch");
    if (int st = check_bilagrid_extents(grid_w, grid_h, grid_l)) return st;
    if (int st = check_bilagrid_image(width, height)) return st;
    if (grad_grid && (reinterpret_cast<uintptr_t>(scratch) & 3u) != 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_slice_backward: scratch must be 4-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    BilagridArgs a{};
    a.grid = grid; a.gw = grid_w; a.gh = grid_h; a.gl = grid_l; a.image = image; a.width = width; a.height = height;
    a.grad_out = grad_out; a.grad_image = grad_image;
    a.vec4 = width % 4 == 0 && aligned16(image) && aligned16(grad_out) && aligned16(grad_image);      // NULL counts as aligned
    if (grad_grid) {
        a.scratch = static_cast<float*>(scratch);
        FGS_HIP(hipMemsetAsync(scratch, 0, fgs_bilagrid_scratch_bytes(grid_w, grid_h, grid_l), stream));
    }
    FGS_HIP(launch_bilagrid_slice_backward(a, grad_grid, stream));
    return FGS_OK;
}

int32_t fgs_bilagrid_tv(const float* grid, int32_t grid_w, int32_t grid_h, int32_t grid_l, float* loss, float* grad_grid, void* stream) {
    if (!grid || !loss) return fail(FGS_ERR_INVALID_ARGUMENT, "bilagrid_tv: NULL grid / loss");
    if (int st = check_bilagrid_extents(grid_w, grid_h, grid_l)) return st;
    FGS_HIP(launch_bilagrid_tv(grid, grid_w, grid_h, grid_l, loss, grad_grid, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}
#pragma GCC visibility pop
}  // extern "C"

// C-ABI entry points of the TSDF fusion and the mesh extraction (tsdf.hip): argument checks, the scratch layout, the launches, the one read-back of sizes.
#include "fgs_host.h"

using namespace fgs;
namespace {
constexpr int64_t kTsdfMaxPoints = int64_t{1} << 28;
// 0, or the refusal: extents >= 2 and the lattice addressable by the kernels' 32-bit indices
int check_tsdf_volume(const char* who, int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: volume extents %d x %d x %d must be at least 2", who, nx, ny, nz);
    if (static_cast<int64_t>(nx) * ny * nz > kTsdfMaxPoints) return fail(FGS_ERR_INVALID_ARGUMENT, "%s: a volume of %d x %d x %d has more than 2^28 points", who, nx, ny, nz);
    return FGS_OK;
}
struct MeshScratch {
    uint32_t* codes; uint2* block_sums; uint32_t* totals;
    static MeshScratch carve(Carver& c, uint32_t n) {
        MeshScratch b;
        b.codes = c.take<uint32_t>("codes", n);
        b.block_sums = c.take<uint2>("block_sums", mesh_blocks(n));
        b.totals = c.take<uint32_t>("totals", 2);
        return b;
    }
};
}  // namespace

extern "C" {
#pragma GCC visibility push(default)
int32_t fgs_tsdf_integrate(float* tsdf_weight, float* color, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z,
                           float voxel_size, float trunc, const fgs_tsdf_view* views, int32_t n_views, int32_t width, int32_t height, float near_plane,
                           float depth_max, float min_alpha, float max_weight, void* stream) {
    if (int st = check_tsdf_volume("tsdf_integrate", nx, ny, nz)) return st;
    if (!(voxel_size > 0.0f) || !(trunc > 0.0f)) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: voxel_size %g and trunc %g must be positive", voxel_size, trunc);
    if (!(max_weight >= 1.0f)) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: max_weight %g must be at least 1", max_weight);
    if (n_views < 1 || n_views > FGS_TSDF_MAX_VIEWS) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: %d views (1..%d per call)", n_views, FGS_TSDF_MAX_VIEWS);
    if (width <= 0 || height <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: image size %dx%d must be positive", width, height);
    if (!tsdf_weight || !views) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: NULL tsdf_weight / views");
    if (reinterpret_cast<uintptr_t>(tsdf_weight) & 7u) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: tsdf_weight must be 8-byte aligned");
    TsdfIntegrateArgs a{};
    a.tsdf_weight = reinterpret_cast<float2*>(tsdf_weight); a.color = color;
    a.nx = nx; a.ny = ny; a.nz = nz; a.ox = origin_x; a.oy = origin_y; a.oz = origin_z; a.voxel = voxel_size; a.trunc = trunc; a.inv_trunc = 1.0f / trunc;
    a.n_views = n_views; a.width = width; a.height = height;
    a.near_plane = near_plane; a.depth_max = depth_max; a.min_alpha = min_alpha; a.max_weight = max_weight;
    for (int v = 0; v < n_views; ++v) {
        const fgs_tsdf_view& in = views[v];
        if (!in.w2c || !in.depth) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: view %d has no w2c / depth", v);
        if (color && !in.color) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_integrate: the volume has colour, view %d has no colour map", v);
        a.view[v] = TsdfView{in.w2c, in.focal_x, in.focal_y, in.center_x, in.center_y, in.depth, in.alpha, color ? in.color : nullptr};
    }
    FGS_HIP(launch_tsdf_integrate(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

size_t fgs_tsdf_mesh_scratch_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || static_cast<int64_t>(nx) * ny * nz > kTsdfMaxPoints) return 0;
    Carver c(nullptr);
    MeshScratch::carve(c, static_cast<uint32_t>(nx) * ny * nz);
    return c.total();
}

int32_t fgs_tsdf_mesh_count(const float* tsdf_weight, int32_t nx, int32_t ny, int32_t nz, float iso, float min_weight, void* scratch, int64_t* counts,
                            void* stream_) {
    if (int st = check_tsdf_volume("tsdf_mesh_count", nx, ny, nz)) return st;
    if (!tsdf_weight || !scratch || !counts) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_count: NULL tsdf_weight / scratch / counts");
    if ((reinterpret_cast<uintptr_t>(tsdf_weight) & 7u) || (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_count: tsdf_weight and scratch must be 8-byte aligned");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Carver c(scratch);
    const MeshScratch sc = MeshScratch::carve(c, static_cast<uint32_t>(nx) * ny * nz);
    MeshArgs a{};
    a.tsdf_weight = reinterpret_cast<const float2*>(tsdf_weight); a.nx = nx; a.ny = ny; a.nz = nz; a.iso = iso; a.min_weight = min_weight;
    a.codes = sc.codes; a.block_sums = sc.block_sums; a.totals = sc.totals;
    FGS_HIP(launch_tsdf_mesh_count(a, stream));
    uint32_t host[2] = {0u, 0u};
    FGS_HIP(hipMemcpyAsync(host, sc.totals, sizeof(host), hipMemcpyDeviceToHost, stream));      // the caller sizes the mesh from these
    FGS_HIP(hipStreamSynchronize(stream));
    counts[0] = host[0]; counts[1] = host[1];
    return FGS_OK;
}

int32_t fgs_tsdf_mesh_emit(const float* tsdf_weight, const float* color, int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y,
                           float origin_z, float voxel_size, float iso, float min_weight, const void* scratch, int64_t n_vertices, int64_t n_triangles,
                           float* vertices, float* colors, int32_t* faces, void* stream) {
    if (int st = check_tsdf_volume("tsdf_mesh_emit", nx, ny, nz)) return st;
    if (!(voxel_size > 0.0f)) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_emit: voxel_size %g must be positive", voxel_size);
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > 0x7fffffffLL || n_triangles > 0xffffffffLL)
        return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_emit: sizes %lld / %lld", static_cast<long long>(n_vertices), static_cast<long long>(n_triangles));
    if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !faces)) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_emit: NULL vertices / faces with non-zero sizes");
    if (colors && !color) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_emit: vertex colours need the colour volume");
    if (n_vertices == 0 && n_triangles == 0) return FGS_OK;          // an empty mesh: nothing to launch
    if (!tsdf_weight || !scratch) return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_emit: NULL tsdf_weight / scratch");
    if ((reinterpret_cast<uintptr_t>(tsdf_weight) & 7u) || (reinterpret_cast<uintptr_t>(scratch) & 7u))
        return fail(FGS_ERR_INVALID_ARGUMENT, "tsdf_mesh_emit: tsdf_weight and scratch must be 8-byte aligned");
    Carver c(const_cast<void*>(scratch));
    const MeshScratch sc = MeshScratch::carve(c, static_cast<uint32_t>(nx) * ny * nz);
    MeshArgs a{};
    a.tsdf_weight = reinterpret_cast<const float2*>(tsdf_weight); a.color = color; a.nx = nx; a.ny = ny; a.nz = nz;
    a.ox = origin_x; a.oy = origin_y; a.oz = origin_z; a.voxel = voxel_size; a.iso = iso; a.min_weight = min_weight;
    a.codes = sc.codes; a.block_sums = sc.block_sums; a.totals = sc.totals;
    a.n_vertices = static_cast<uint32_t>(n_vertices); a.n_triangles = static_cast<uint64_t>(n_triangles);
    a.vertices = vertices; a.colors = colors; a.faces = faces;
    FGS_HIP(launch_tsdf_mesh_emit(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}
#pragma GCC visibility pop
}  // extern "C"

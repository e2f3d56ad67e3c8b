// Surface extraction: fused TSDF integration of rendered depth maps into a dense volume, and a table-free marching-tetrahedra mesh of its level set.
// Definitions: include/fgs_hip.h ("TSDF fusion and mesh extraction") and INTEGRATION.md. Built with -ffp-contract=off: the discrete decisions (pixel of a
// lattice point, the truncation test, the side of the level set a corner lies on) round the same way here, in the CPU simulation and in a restatement.
//
// Integration is a streaming kernel: one thread per lattice point, x fastest, so a wave's 64 points are 512 contiguous bytes of state and project to
// neighbouring pixels. The point's (tsdf, weight) pair is one 8-byte load, lives in registers across the V views of the call, and is stored back only
// if a view updated it. Algorithmic bytes per point: 8 read + (8 written + 4 depth) where touched; the maps (V x H x W x 4..20 bytes) are small beside
// the volume and are served by the caches. No atomics, no LDS.
//
// Extraction is three launches over the same lattice (kMeshBlock points per workgroup, in linear order):
//   mesh_classify_kernel   per lattice point: the 7-bit mask of its owned edges that carry a vertex, the triangle count of the cube rooted there, and the
//                          point's vertex rank inside its workgroup -> one 32-bit code word; per workgroup: (vertices, triangles) -> block_sums
//   mesh_scan_blocks_kernel ONE 1024-thread workgroup: exclusive scan of the block sums in place (fgs_tile_scan.h, as the density-control scan), totals
//   mesh_emit_kernel       vertices by their owners, triangles by their cubes; a triangle finds a vertex as block base + rank of the owner + popcount
//                          of the owner's lower mask bits
#include <fgs_wave.h>
#include "fgs_kernels.h"
#include "fgs_tile_scan.h"

namespace fgs {

// ---------------------------------------------------------------- integration ----------------------------------------------------------------
template <bool COLOR>
__global__ void __launch_bounds__(256) tsdf_integrate_kernel(const TsdfIntegrateArgs a) {
    const uint32_t n = static_cast<uint32_t>(a.nx) * a.ny * a.nz;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = i / a.nx, x = i - row * a.nx, z = row / a.ny, y = row - z * a.ny;
    // the lattice point itself, never a running increment along x
    const float px = a.ox + a.voxel * static_cast<float>(x), py = a.oy + a.voxel * static_cast<float>(y), pz = a.oz + a.voxel * static_cast<float>(z);
    float2 s = a.tsdf_weight[i];
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    bool touched = false;
    const size_t plane = static_cast<size_t>(n);
    for (int v = 0; v < a.n_views; ++v) {
        const TsdfView& V = a.view[v];
        const float* m = V.w2c;
        const float cz = ((m[8] * px + m[9] * py) + m[10] * pz) + m[11];
        if (!(cz > a.near_plane)) continue;
        const float cx = ((m[0] * px + m[1] * py) + m[2] * pz) + m[3];
        const float cy = ((m[4] * px + m[5] * py) + m[6] * pz) + m[7];
        const float rz = 1.0f / cz;                                      // one reciprocal per view for both coordinates
        const float u = V.fx * cx * rz + V.cx, w = V.fy * cy * rz + V.cy;
        const float fu = floorf(u), fw = floorf(w);
        if (!(fu >= 0.0f && fw >= 0.0f && fu < static_cast<float>(a.width) && fw < static_cast<float>(a.height))) continue;      // NaN fails
        const uint32_t pix = static_cast<uint32_t>(fw) * a.width + static_cast<uint32_t>(fu);
        const float d = V.depth[pix];
        if (!(d > 0.0f) || d > a.depth_max) continue;
        if (V.alpha && V.alpha[pix] < a.min_alpha) continue;
        const float sdf = d - cz;
        if (sdf < -a.trunc) continue;
        const float f = fminf(1.0f, sdf * a.inv_trunc);
        const float w1 = s.y + 1.0f, rw = 1.0f / w1;
        if (COLOR) {
            if (!touched) { c0 = a.color[i]; c1 = a.color[plane + i]; c2 = a.color[2 * plane + i]; }
            const size_t hw = static_cast<size_t>(a.width) * a.height;
            c0 = (c0 * s.y + V.color[pix]) * rw;
            c1 = (c1 * s.y + V.color[hw + pix]) * rw;
            c2 = (c2 * s.y + V.color[2 * hw + pix]) * rw;
        }
        s.x = (s.x * s.y + f) * rw;
        s.y = fminf(w1, a.max_weight);
        touched = true;
    }
    if (!touched) return;
    a.tsdf_weight[i] = s;
    if (COLOR) { a.color[i] = c0; a.color[plane + i] = c1; a.color[2 * plane + i] = c2; }
}

hipError_t launch_tsdf_integrate(const TsdfIntegrateArgs& a, hipStream_t s) {
    const uint32_t n = static_cast<uint32_t>(a.nx) * a.ny * a.nz;
    if (n == 0 || a.n_views == 0) return hipSuccess;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (a.color) hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------- extraction -----------------------------------------------------------------
// Corner c of a cube is the bit set (x = 1, y = 2, z = 4). The six tetrahedra are the Kuhn split: for each permutation (p1, p2, p3) of the axes
// v0 = 0, v1 = bit p1, v2 = v1 | bit p2, v3 = 7. An edge runs from corner a to corner b with a a subset of b; it is owned by the lattice point of a
// and has type d = b ^ a in 1..7 (mask bit d - 1).
constexpr uint32_t kMeshBlock = 256;
// code word of a lattice point: bits 0..6 edge mask, 8..11 triangle count of the cube rooted here (<= 12), 16..27 vertex rank inside the workgroup (<= 1785)

__device__ __forceinline__ uint32_t popcount32(uint32_t v) {           // portable spelling (the mask has 7 bits)
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    return (((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24;
}
__device__ __forceinline__ void tet_corners(const int t, int (&v)[4]) {      // permutations in lexicographic order: t / 2 = first axis
    const int p1 = t >> 1;
    const int lo = p1 == 0 ? 1 : 0, hi = p1 == 2 ? 1 : 2;                    // the other two axes, ascending
    const int p2 = (t & 1) ? hi : lo;
    v[0] = 0; v[1] = 1 << p1; v[2] = v[1] | (1 << p2); v[3] = 7;
}
// sign of det(q - p, r - p, s - p) for four cube corners (integer, exact)
__device__ __forceinline__ int corner_det(const int p, const int q, const int r, const int s) {
    const int a0 = (q & 1) - (p & 1), a1 = ((q >> 1) & 1) - ((p >> 1) & 1), a2 = (q >> 2) - (p >> 2);
    const int b0 = (r & 1) - (p & 1), b1 = ((r >> 1) & 1) - ((p >> 1) & 1), b2 = (r >> 2) - (p >> 2);
    const int c0 = (s & 1) - (p & 1), c1 = ((s >> 1) & 1) - ((p >> 1) & 1), c2 = (s >> 2) - (p >> 2);
    return a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
}

struct MeshPoint { uint32_t x, y, z; };
__device__ __forceinline__ MeshPoint mesh_point(const uint32_t i, const int nx, const int ny) {
    const uint32_t row = i / nx, z = row / ny;
    return MeshPoint{i - row * nx, row - z * ny, z};
}
__device__ __forceinline__ uint32_t corner_index(const uint32_t i, const int c, const int nx, const int ny) {
    return i + (c & 1) + ((c >> 1) & 1) * static_cast<uint32_t>(nx) + (c >> 2) * static_cast<uint32_t>(nx) * ny;
}

// (vertices | triangles << 16) of this thread -> its exclusive prefix inside the workgroup and the workgroup's total (both packed; <= 1792 | 3072 << 16)
__device__ __forceinline__ void mesh_block_scan(const uint32_t mine, uint32_t& before, uint32_t& total, uint32_t (&s_tot)[kMeshBlock / 64]) {
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t incl = wave_inclusive_sum(mine);
    if (lane == 63u) s_tot[wv] = incl;
    __syncthreads();
    before = incl - mine; total = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kMeshBlock / 64; ++k) { const uint32_t t = s_tot[k]; before += k < wv ? t : 0u; total += t; }
}

__global__ void __launch_bounds__(kMeshBlock) mesh_classify_kernel(const MeshArgs a) {
    __shared__ uint32_t s_tot[kMeshBlock / 64];
    const uint32_t n = static_cast<uint32_t>(a.nx) * a.ny * a.nz;
    const uint32_t i = blockIdx.x * kMeshBlock + threadIdx.x;
    uint32_t mask = 0u, tris = 0u;
    if (i < n) {
        const MeshPoint p = mesh_point(i, a.nx, a.ny);
        const bool hx = p.x + 1u < static_cast<uint32_t>(a.nx), hy = p.y + 1u < static_cast<uint32_t>(a.ny), hz = p.z + 1u < static_cast<uint32_t>(a.nz);
        bool valid[8], in[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool there = ((c & 1) == 0 || hx) && ((c & 2) == 0 || hy) && ((c & 4) == 0 || hz);
            float2 s = make_float2(0.0f, 0.0f);
            if (there) s = a.tsdf_weight[corner_index(i, c, a.nx, a.ny)];
            valid[c] = there && s.y >= a.min_weight;
            in[c] = s.x < a.iso;
        }
#pragma unroll
        for (int d = 1; d < 8; ++d)
            if (valid[0] && valid[d] && in[0] != in[d]) mask |= 1u << (d - 1);
        bool cube = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) cube = cube && valid[c];
        if (cube) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                int v[4];
                tet_corners(t, v);
                const int k = (in[v[0]] ? 1 : 0) + (in[v[1]] ? 1 : 0) + (in[v[2]] ? 1 : 0) + (in[v[3]] ? 1 : 0);
                tris += k == 2 ? 2u : (k == 1 || k == 3) ? 1u : 0u;
            }
        }
    }
    uint32_t before, total;
    mesh_block_scan(popcount32(mask) | (tris << 16), before, total, s_tot);
    if (i < n) a.codes[i] = mask | (tris << 8) | ((before & 0xffffu) << 16);
    if (threadIdx.x == 0) a.block_sums[blockIdx.x] = make_uint2(total & 0xffffu, total >> 16);
}

__global__ void __launch_bounds__(kTileScanThreads) mesh_scan_blocks_kernel(uint2* __restrict__ block_sums, uint32_t* __restrict__ totals, const uint32_t n_blocks) {
    __shared__ TileScanShared s;
    uint32_t base[2] = {0u, 0u};
    int parity = 0;
    for (uint32_t first = 0; first < n_blocks; first += kTileScanThreads * kTileScanPerThread) {
        const uint32_t mine = first + threadIdx.x * kTileScanPerThread;
        uint32_t v[2][kTileScanPerThread], ex[2][kTileScanPerThread];
#pragma unroll
        for (int k = 0; k < kTileScanPerThread; ++k) {
            const uint2 b = mine + k < n_blocks ? block_sums[mine + k] : make_uint2(0u, 0u);
            v[0][k] = b.x; v[1][k] = b.y;
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) { base[c] += tile_scan_pass(v[c], ex[c], s, base[c], parity); parity ^= 1; }
#pragma unroll
        for (int k = 0; k < kTileScanPerThread; ++k)
            if (mine + k < n_blocks) block_sums[mine + k] = make_uint2(ex[0][k], ex[1][k]);
    }
    if (threadIdx.x == 0) { totals[0] = base[0]; totals[1] = base[1]; }
}

// id of the vertex on the edge between cube corners ca and cb (ca a subset of cb) of the cube rooted at lattice point i
__device__ __forceinline__ uint32_t mesh_vertex_id(const MeshArgs& a, const uint32_t i, const int ca, const int cb) {
    const uint32_t owner = corner_index(i, ca, a.nx, a.ny);
    const uint32_t code = a.codes[owner];
    const int d = ca ^ cb;
    return a.block_sums[owner / kMeshBlock].x + (code >> 16) + popcount32(code & ((1u << (d - 1)) - 1u));
}
__device__ __forceinline__ uint32_t mesh_edge_id(const MeshArgs& a, const uint32_t i, const int c0, const int c1) {
    return c0 < c1 ? mesh_vertex_id(a, i, c0, c1) : mesh_vertex_id(a, i, c1, c0);      // along a Kuhn tetrahedron the smaller corner is the subset
}
__device__ __forceinline__ void mesh_put_triangle(const MeshArgs& a, const uint64_t t, const uint32_t v0, const uint32_t v1, const uint32_t v2, const bool keep) {
    if (t >= a.n_triangles) return;                           // counts that do not belong to this scratch: never past the caller's buffers
    int32_t* f = a.faces + 3u * t;
    f[0] = static_cast<int32_t>(v0); f[1] = static_cast<int32_t>(keep ? v1 : v2); f[2] = static_cast<int32_t>(keep ? v2 : v1);
}

__global__ void __launch_bounds__(kMeshBlock) mesh_emit_kernel(const MeshArgs a) {
    __shared__ uint32_t s_tot[kMeshBlock / 64];
    const uint32_t n = static_cast<uint32_t>(a.nx) * a.ny * a.nz;
    const uint32_t i = blockIdx.x * kMeshBlock + threadIdx.x;
    const uint32_t code = i < n ? a.codes[i] : 0u;
    const uint32_t mask = code & 0x7fu, tris = (code >> 8) & 0xfu;
    uint32_t before, total;
    mesh_block_scan(tris, before, total, s_tot);
    if (i >= n || (mask == 0u && tris == 0u)) return;
    const uint2 base = a.block_sums[blockIdx.x];
    const size_t plane = static_cast<size_t>(n);
    if (mask) {
        const MeshPoint p = mesh_point(i, a.nx, a.ny);
        const float fa = a.tsdf_weight[i].x;
        uint32_t id = base.x + (code >> 16);
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            if (!((mask >> (d - 1)) & 1u)) continue;
            const uint32_t j = corner_index(i, d, a.nx, a.ny);
            const float fb = a.tsdf_weight[j].x;
            const float t = (a.iso - fa) / (fb - fa);
            if (id < a.n_vertices) {
                float* o = a.vertices + 3u * static_cast<size_t>(id);
                const float step = a.voxel * t;
                o[0] = (a.ox + a.voxel * static_cast<float>(p.x)) + ((d & 1) ? step : 0.0f);
                o[1] = (a.oy + a.voxel * static_cast<float>(p.y)) + ((d & 2) ? step : 0.0f);
                o[2] = (a.oz + a.voxel * static_cast<float>(p.z)) + ((d & 4) ? step : 0.0f);
                if (a.colors) {
                    float* c = a.colors + 3u * static_cast<size_t>(id);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float ca = a.color[ch * plane + i], cb = a.color[ch * plane + j];
                        c[ch] = ca + (cb - ca) * t;
                    }
                }
            }
            ++id;
        }
    }
    if (tris) {
        bool in[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = a.tsdf_weight[corner_index(i, c, a.nx, a.ny)].x < a.iso;
        uint64_t t_out = static_cast<uint64_t>(base.y) + before;
        for (int t = 0; t < 6; ++t) {
            int v[4];
            tet_corners(t, v);
            int ins[4], outs[4], ni = 0, no = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { if (in[v[k]]) ins[ni++] = v[k]; else outs[no++] = v[k]; }
            if (ni == 0 || ni == 4) continue;
            if (ni == 2) {
                // the quad (pr, ps, qs, qr) around the inside pair p, q; its normal leaves the inside when det(q - p, r - p, s - p) > 0
                const int p = ins[0], q = ins[1], r = outs[0], s = outs[1];
                const bool keep = corner_det(p, q, r, s) > 0;
                const uint32_t pr = mesh_edge_id(a, i, p, r), ps = mesh_edge_id(a, i, p, s), qs = mesh_edge_id(a, i, q, s), qr = mesh_edge_id(a, i, q, r);
                mesh_put_triangle(a, t_out++, pr, ps, qs, keep);
                mesh_put_triangle(a, t_out++, pr, qs, qr, keep);
            } else {
                // one corner p alone on its side: the triangle on its three edges points away from p when det > 0; it must point away from the inside
                const bool lone_inside = ni == 1;
                const int p = lone_inside ? ins[0] : outs[0];
                const int* o = lone_inside ? outs : ins;
                const bool keep = (corner_det(p, o[0], o[1], o[2]) > 0) == lone_inside;
                mesh_put_triangle(a, t_out++, mesh_edge_id(a, i, p, o[0]), mesh_edge_id(a, i, p, o[1]), mesh_edge_id(a, i, p, o[2]), keep);
            }
        }
    }
}

uint32_t mesh_blocks(uint32_t n_points) { return (n_points + kMeshBlock - 1u) / kMeshBlock; }

hipError_t launch_tsdf_mesh_count(const MeshArgs& a, hipStream_t s) {
    const uint32_t n = static_cast<uint32_t>(a.nx) * a.ny * a.nz;
    const uint32_t n_blocks = mesh_blocks(n);
    hipLaunchKernelGGL(mesh_classify_kernel, dim3(n_blocks), dim3(kMeshBlock), 0, s, a);
    hipLaunchKernelGGL(mesh_scan_blocks_kernel, dim3(1), dim3(kTileScanThreads), 0, s, a.block_sums, a.totals, n_blocks);
    return hipGetLastError();
}

hipError_t launch_tsdf_mesh_emit(const MeshArgs& a, hipStream_t s) {
    const uint32_t n = static_cast<uint32_t>(a.nx) * a.ny * a.nz;
    hipLaunchKernelGGL(mesh_emit_kernel, dim3(mesh_blocks(n)), dim3(kMeshBlock), 0, s, a);
    return hipGetLastError();
}

}  // namespace fgs

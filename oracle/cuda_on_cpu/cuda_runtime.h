// TEST-ONLY stand-in for <cuda_runtime.h>: lets g++ compile CUDA sources that use the documented runtime, cooperative-groups and CUB
// interfaces into a CPU library. Layered on the fiber-per-work-item workgroup emulator of tests/sim/include/hip/hip_runtime.h (its fibers,
// its workgroup barrier, its atomics); this file adds what CUDA text needs on top: the remaining vector types, two-dimensional blocks and
// grids, a 32-wide tile scope for collectives, the few runtime calls and device intrinsics, and a launcher for the rewritten `<<< >>>` syntax.
// Written from the CUDA C++ Programming Guide / CUDA Math API / CUB documentation; arithmetic is "as written" (build with -ffp-contract=off):
// __expf and its kin are the libm calls the fp32 oracle makes, not NVIDIA's approximations. See oracle/build_ref.py for the one user.
#pragma once
#include <hip/hip_runtime.h>      // tests/sim/include: fibers, sim::Block / sim::Lane, __syncthreads, __syncthreads_and, atomics, float2/float4/uint2/uint4/dim3

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#define __constant__
#define __align__(n) __attribute__((aligned(n)))

typedef unsigned int uint;
typedef unsigned short ushort;

struct float3 { float x, y, z; };
struct int2 { int x, y; };
struct int3 { int x, y, z; };
struct int4 { int x, y, z, w; };
struct uint3 { unsigned x, y, z; };
struct ushort4 { unsigned short x, y, z, w; };
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
inline int2 make_int2(int x, int y) { return int2{x, y}; }
inline int3 make_int3(int x, int y, int z) { return int3{x, y, z}; }
inline int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
inline uint3 make_uint3(unsigned x, unsigned y, unsigned z) { return uint3{x, y, z}; }
inline ushort4 make_ushort4(unsigned short x, unsigned short y, unsigned short z, unsigned short w) { return ushort4{x, y, z, w}; }

// ---- runtime calls: one address space, everything synchronous ---------------------------------------------------------------------------
typedef int cudaError_t;
enum { cudaSuccess = 0 };
enum cudaMemcpyKind { cudaMemcpyHostToHost, cudaMemcpyHostToDevice, cudaMemcpyDeviceToHost, cudaMemcpyDeviceToDevice, cudaMemcpyDefault };
typedef void* cudaStream_t;
inline cudaError_t cudaStreamCreate(cudaStream_t* s) { *s = nullptr; return cudaSuccess; }
inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
inline cudaError_t cudaDeviceSynchronize() { return cudaSuccess; }
inline const char* cudaGetErrorString(cudaError_t) { return "cuda_on_cpu"; }
inline cudaError_t cudaMemset(void* p, int v, size_t n) { if (n) memset(p, v, n); return cudaSuccess; }
inline cudaError_t cudaMemsetAsync(void* p, int v, size_t n, cudaStream_t = nullptr) { if (n) memset(p, v, n); return cudaSuccess; }
inline cudaError_t cudaMemcpy(void* d, const void* s, size_t n, cudaMemcpyKind) { if (n) memcpy(d, s, n); return cudaSuccess; }
template <class T> inline cudaError_t cudaMemcpyToSymbol(T& symbol, const void* s, size_t n) { memcpy(&symbol, s, n); return cudaSuccess; }

// ---- device intrinsics the emulator does not already have (CUDA Math API / Programming Guide semantics) ----------------------------------
inline int __float2int_rd(float x) { if (x != x) return 0; const float f = floorf(x); return f >= 2147483648.0f ? INT_MAX : f < -2147483648.0f ? INT_MIN : static_cast<int>(f); }
inline int __float2int_ru(float x) { if (x != x) return 0; const float f = ceilf(x); return f >= 2147483648.0f ? INT_MAX : f < -2147483648.0f ? INT_MIN : static_cast<int>(f); }
inline float __uint2float_rn(unsigned v) { return static_cast<float>(v); }
inline float __saturatef(float x) { return x != x ? 0.0f : x < 0.0f ? 0.0f : x > 1.0f ? 1.0f : x; }
inline int __ffs(int v) { return __builtin_ffs(v); }
inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
inline double rsqrt(double x) { return 1.0 / sqrt(x); }
// __fns: position of the |offset|-th set bit of `mask` counting from bit `base` (upwards for offset > 0, downwards for offset < 0; offset 0: `base` itself
// if set), 0xffffffff when there is none.
inline unsigned __fns(unsigned mask, unsigned base, int offset) {
    if (offset == 0) return (mask >> base) & 1u ? base : 0xffffffffu;
    int remaining = offset > 0 ? offset : -offset;
    for (int bit = static_cast<int>(base); bit >= 0 && bit < 32; bit += offset > 0 ? 1 : -1)
        if (((mask >> bit) & 1u) && --remaining == 0) return static_cast<unsigned>(bit);
    return 0xffffffffu;
}

// ---- two-dimensional launches, scheduled tile by tile -------------------------------------------------------------------------------------
namespace cuda_on_cpu {

constexpr int kTile = 32;
struct Config { dim3 grid, block, block_index; };
inline Config& cfg() { static Config c; return c; }

// One block. A 32-wide tile runs until every live work-item of it waits (at a tile collective for a tile-mate: never, they all arrive within a pass;
// at the workgroup barrier for another tile) or has returned, then the next tile runs: work-items pass every point of the kernel in rank order
// within a tile and tiles run in order between workgroup barriers, which makes the order of atomics -- and with it every compaction the
// kernels do with atomicAdd -- the order of the work-item ranks, run after run.
inline void run_block(unsigned linear_block, unsigned n_threads, unsigned n_blocks, const std::function<void()>& body) {
    sim::init_block(linear_block, n_threads, n_blocks, body);
    sim::Block& b = sim::blk();
    for (;;) {
        const unsigned long before = b.progress;
        int alive = 0;
        for (int w0 = 0; w0 < b.n; w0 += kTile) {
            const int w1 = std::min(w0 + kTile, b.n);
            for (;;) {
                const unsigned long p0 = b.progress;
                for (int i = w0; i < w1; ++i) {
                    if (!b.lanes[i].alive) continue;
                    b.cur = i;
                    fgs_sim_switch(&b.main_sp, &b.lanes[i].sp);
                }
                if (b.progress == p0) break;
            }
            for (int i = w0; i < w1; ++i) alive += b.lanes[i].alive ? 1 : 0;
        }
        if (alive == 0) break;
        if (b.progress == before) {
            fprintf(stderr, "[cuda_on_cpu] deadlock in block %u: %d work-items wait at a barrier the others never reach\n", linear_block, alive);
            abort();
        }
    }
}

struct Launch {
    dim3 grid, block;
    template <class K, class... A> void run(K kernel, A... args) const {
        Config& c = cfg();
        c.grid = grid; c.block = block;
        const unsigned n_threads = block.x * block.y * block.z, n_blocks = grid.x * grid.y * grid.z;
        if (n_threads == 0 || n_blocks == 0) return;                     // an invalid configuration launches nothing
        const std::function<void()> body = [=]() { kernel(args...); };
        unsigned linear = 0;
        for (unsigned bz = 0; bz < grid.z; ++bz)
            for (unsigned by = 0; by < grid.y; ++by)
                for (unsigned bx = 0; bx < grid.x; ++bx) {
                    c.block_index = dim3(bx, by, bz);
                    run_block(linear++, n_threads, n_blocks, body);
                }
    }
};
// `kernel<<<grid, block>>>(args...)` is rewritten to `cuda_on_cpu::launch(grid, block).run(kernel, args...)`.
inline Launch launch(dim3 grid, dim3 block) { return Launch{grid, block}; }

inline unsigned thread_rank() { return sim::tid(); }
inline sim::Idx3 thread_idx() {
    const dim3& d = cfg().block; const unsigned t = sim::tid();
    return sim::Idx3{t % d.x, (t / d.x) % d.y, t / (d.x * d.y)};
}
inline sim::Idx3 block_idx() { const dim3& i = cfg().block_index; return sim::Idx3{i.x, i.y, i.z}; }
inline sim::Idx3 block_dim() { const dim3& d = cfg().block; return sim::Idx3{d.x, d.y, d.z}; }
inline sim::Idx3 grid_dim() { const dim3& d = cfg().grid; return sim::Idx3{d.x, d.y, d.z}; }

// Tile-scope rendezvous: wait until every work-item of my 32-wide tile that has not returned reached my collective. A work-item took part in
// collective g iff its counter is >= g; what it published for g (slot parity g & 1) stays valid after it returned, and nobody can overwrite
// that parity before every live tile-mate has passed g + 1, i.e. after it has read g.
inline int tile_first() { return (sim::blk().cur / kTile) * kTile; }
inline int tile_last() { return std::min(tile_first() + kTile, sim::blk().n); }
inline unsigned tile_sync() {
    sim::Block& b = sim::blk();
    const unsigned g = ++sim::me().gen_wave;
    ++b.progress;
    const int first = tile_first(), last = tile_last();
    for (bool waited = false;; waited = true) {
        bool all = true;
        for (int i = first; i < last; ++i)
            if (b.lanes[i].alive && b.lanes[i].gen_wave < g) { all = false; break; }
        if (all) {
            // The work-item that completes the rendezvous steps aside once, so the tile leaves every collective in rank order, as it entered it. A
            // converged warp runs in lockstep; kernels written for one read shared memory after a collective that a tile-mate overwrites a few
            // statements later, with no barrier in between (the leader's read of the collected pixel data in the reference's blend backward is one).
            // Rank order between collectives keeps such a read ahead of the write, as lockstep does.
            if (!waited) sim::yield();
            return g;
        }
        sim::yield();
    }
}
inline int tile_parity() { return static_cast<int>((sim::me().gen_wave + 1u) & 1u); }

}  // namespace cuda_on_cpu

#undef threadIdx
#undef blockIdx
#undef blockDim
#undef gridDim
#define threadIdx (cuda_on_cpu::thread_idx())
#define blockIdx (cuda_on_cpu::block_idx())
#define blockDim (cuda_on_cpu::block_dim())
#define gridDim (cuda_on_cpu::grid_dim())

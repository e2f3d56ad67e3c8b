// Self-test of the CUDA-on-CPU stand-ins (tests/test_cuda_on_cpu.py compiles and runs it): own kernels written against the documented CUDA, cooperative
// groups and CUB interfaces, with the answers those documents give. Exit status 0 and "ok" when everything holds, otherwise one line per failure.
#include <cooperative_groups.h>
#include <cub/cub.cuh>

#include <cstdio>
#include <vector>

namespace cg = cooperative_groups;
static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); } } while (0)

// ---- two-dimensional blocks and grids --------------------------------------------------------------------------------------------------------
__global__ void index_kernel(unsigned* out) {
    auto block = cg::this_thread_block();
    auto warp = cg::tiled_partition<32>(block);
    const unsigned rank = threadIdx.y * blockDim.x + threadIdx.x;
    const unsigned linear_block = blockIdx.y * gridDim.x + blockIdx.x;
    unsigned ok = 1;
    ok &= block.thread_rank() == rank && warp.thread_rank() == rank % 32 && warp.meta_group_rank() == rank / 32;
    ok &= block.group_index().x == blockIdx.x && block.group_index().y == blockIdx.y;
    ok &= cg::this_grid().thread_rank() == static_cast<unsigned long long>(linear_block) * blockDim.x * blockDim.y + rank;
    ok &= blockDim.x == 16 && blockDim.y == 12 && gridDim.x == 3 && gridDim.y == 2 && threadIdx.x < 16 && threadIdx.y < 12;
    out[(blockIdx.y * blockDim.y + threadIdx.y) * (gridDim.x * blockDim.x) + blockIdx.x * blockDim.x + threadIdx.x] = ok ? 1 + linear_block : 0;
}

// ---- tile collectives, with work-items of the tile that have returned --------------------------------------------------------------------------
__global__ void collective_kernel(unsigned* ballots, unsigned* shuffles, float* ups, unsigned* second, unsigned* order, unsigned* counter) {
    auto block = cg::this_thread_block();
    auto warp = cg::tiled_partition<32>(block);
    const unsigned rank = block.thread_rank(), lane = warp.thread_rank();
    if (rank % 3 == 0) return;                                           // a third of every tile is gone before the first collective
    ballots[rank] = warp.ballot(lane % 2 == 1);
    shuffles[rank] = warp.shfl(1000u + rank, 4);                         // lane 4 of the tile: live in tiles 0 and 2 (ranks 4, 68), returned in tile 1 (rank 36)
    ups[rank] = warp.shfl_up(0.5f + static_cast<float>(rank), 1);
    order[atomicAdd(counter, 1)] = rank;                                 // compaction by atomics arrives in rank order
    if (lane >= 16) return;                                              // and half of the rest before the second
    warp.sync();
    second[rank] = warp.ballot(1);
}

__global__ void reduce_kernel(unsigned* out) {
    typedef cub::BlockReduce<unsigned, 16, cub::BLOCK_REDUCE_WARP_REDUCTIONS, 12> BlockReduce;
    __shared__ typename BlockReduce::TempStorage storage;
    auto block = cg::this_thread_block();
    const unsigned v = (block.thread_rank() * 37u) % 191u;               // maximum 190 at rank 36 * k ...
    const unsigned m = BlockReduce(storage).Reduce(v, cub::Max());
    if (block.thread_rank() == 0) out[blockIdx.x] = m;
    const bool all_in = __syncthreads_and(block.thread_rank() < 192), all_but_one = __syncthreads_and(block.thread_rank() != 77);
    if (block.thread_rank() == 5) out[2 + blockIdx.x] = all_in && !all_but_one ? 1u : 0u;
}

int main() {
    {   // 2-D
        std::vector<unsigned> out(48 * 24, 0);
        cuda_on_cpu::launch(dim3(3, 2), dim3(16, 12)).run(index_kernel, out.data());
        for (unsigned y = 0; y < 24; ++y)
            for (unsigned x = 0; x < 48; ++x) EXPECT(out[y * 48 + x] == 1 + (y / 12) * 3 + x / 16);
    }
    {   // collectives
        const unsigned n = 96;
        std::vector<unsigned> ballots(n, 77), shuffles(n, 77), second(n, 77), order(n, 77);
        std::vector<float> ups(n, -1.0f);
        unsigned counter = 0;
        cuda_on_cpu::launch(1, n).run(collective_kernel, ballots.data(), shuffles.data(), ups.data(), second.data(), order.data(), &counter);
        unsigned live = 0;
        for (unsigned r = 0; r < n; ++r) {
            const unsigned t0 = (r / 32) * 32, lane = r % 32;
            if (r % 3 == 0) { EXPECT(ballots[r] == 77 && second[r] == 77); continue; }
            EXPECT(order[live++] == r);
            unsigned odd_live = 0, low_live = 0;
            for (unsigned l = 0; l < 32; ++l) {
                if ((t0 + l) % 3 == 0) continue;
                if (l % 2 == 1) odd_live |= 1u << l;
                if (l < 16) low_live |= 1u << l;
            }
            EXPECT(ballots[r] == odd_live);
            EXPECT(shuffles[r] == ((t0 + 4) % 3 == 0 ? 1000u + r : 1000u + t0 + 4));             // from a returned work-item: the caller's own value
            const bool src_live = lane >= 1 && (r - 1) % 3 != 0;
            EXPECT(ups[r] == (src_live ? 0.5f + static_cast<float>(r - 1) : 0.5f + static_cast<float>(r)));
            if (lane < 16) EXPECT(second[r] == low_live); else EXPECT(second[r] == 77);
        }
        EXPECT(counter == live && live == 64);
    }
    {   // block reduce, __syncthreads_and on a 2-D block
        unsigned out[4] = {0, 0, 0, 0};
        cuda_on_cpu::launch(2, dim3(16, 12)).run(reduce_kernel, out);
        unsigned expect = 0;
        for (unsigned r = 0; r < 192; ++r) expect = std::max(expect, (r * 37u) % 191u);
        EXPECT(out[0] == expect && out[1] == expect && out[2] == 1 && out[3] == 1);
    }
    {   // CUB on the host: size queries, a stable sort over [begin_bit, end_bit), in-place scans
        unsigned short k0[8] = {0x25, 0x03, 0x45, 0x23, 0x01, 0x63, 0x05, 0x21}, k1[8] = {};
        unsigned v0[8] = {0, 1, 2, 3, 4, 5, 6, 7}, v1[8] = {};
        cub::DoubleBuffer<unsigned short> keys(k0, k1);
        cub::DoubleBuffer<unsigned> values(v0, v1);
        size_t bytes = 0;
        cub::DeviceRadixSort::SortPairs(nullptr, bytes, keys, values, 8, 0, 5);
        EXPECT(bytes > 0 && keys.selector == 0 && k1[0] == 0 && v0[1] == 1);                     // a size query touches nothing
        std::vector<char> ws(bytes);
        cub::DeviceRadixSort::SortPairs(ws.data(), bytes, keys, values, 8, 0, 5);                // the low five bits only: 5 3 5 3 1 3 5 1
        const unsigned expect_v[8] = {4, 7, 1, 3, 5, 0, 2, 6};
        for (int i = 0; i < 8; ++i) EXPECT(values.Current()[i] == expect_v[i] && keys.Current()[i] == k0[expect_v[i]]);
        EXPECT(keys.selector == values.selector && keys.Current() != keys.Alternate());
        unsigned a[5] = {3, 0, 4, 1, 5}, b[5] = {3, 0, 4, 1, 5}, c[5] = {};
        size_t sb = 0;
        cub::DeviceScan::ExclusiveSum(nullptr, sb, a, a, 5);
        EXPECT(sb > 0 && a[0] == 3);
        cub::DeviceScan::ExclusiveSum(ws.data(), sb, a, a, 5);
        cub::DeviceScan::InclusiveSum(ws.data(), sb, b, c, 5);
        const unsigned ex[5] = {0, 3, 3, 7, 8}, in[5] = {3, 3, 7, 8, 13};
        for (int i = 0; i < 5; ++i) EXPECT(a[i] == ex[i] && c[i] == in[i]);
    }
    {   // intrinsics
        EXPECT(__fns(0x16u, 0, 1) == 1 && __fns(0x16u, 0, 2) == 2 && __fns(0x16u, 0, 3) == 4 && __fns(0x16u, 0, 4) == 0xffffffffu);
        EXPECT(__fns(0x16u, 4, -2) == 2 && __fns(0x16u, 2, 0) == 2 && __fns(0x16u, 3, 0) == 0xffffffffu);
        EXPECT(__float2int_rd(-0.5f) == -1 && __float2int_ru(-0.5f) == 0 && __float2int_rd(2.0f) == 2 && __float2int_ru(2.0001f) == 3);
        EXPECT(__float2int_rd(NAN) == 0 && __float2int_ru(1e20f) == INT_MAX && __float2int_rd(-1e20f) == INT_MIN);
        EXPECT(__saturatef(NAN) == 0.0f && __saturatef(-1.0f) == 0.0f && __saturatef(2.0f) == 1.0f && __saturatef(0.25f) == 0.25f);
        EXPECT(__ffs(0) == 0 && __ffs(8) == 4 && __popc(0xf0u) == 4);
    }
    if (failures == 0) printf("ok\n");
    return failures ? 1 : 0;
}

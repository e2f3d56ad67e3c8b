// TEST-ONLY stand-in for <cooperative_groups.h> (see cuda_runtime.h in this directory): the thread block, its 32-wide tiles and the grid rank,
// as the CUDA C++ Programming Guide documents them. Tile collectives act over the 32 consecutive work-items of a tile on the fiber scheduler;
// work-items of the tile that have already returned do not take part (their ballot bit is 0, a shuffle from them returns the caller's own value).
#pragma once
#include "cuda_runtime.h"

namespace cooperative_groups {

struct thread_block {
    dim3 group_index() const { return cuda_on_cpu::cfg().block_index; }
    dim3 thread_index() const { const sim::Idx3 t = cuda_on_cpu::thread_idx(); return dim3(t.x, t.y, t.z); }
    unsigned thread_rank() const { return cuda_on_cpu::thread_rank(); }
    void sync() const { __syncthreads(); }
};
inline thread_block this_thread_block() { return thread_block{}; }

struct grid_group {
    unsigned long long thread_rank() const {
        const cuda_on_cpu::Config& c = cuda_on_cpu::cfg();
        const unsigned long long block = (static_cast<unsigned long long>(c.block_index.z) * c.grid.y + c.block_index.y) * c.grid.x + c.block_index.x;
        return block * (static_cast<unsigned long long>(c.block.x) * c.block.y * c.block.z) + cuda_on_cpu::thread_rank();
    }
};
inline grid_group this_grid() { return grid_group{}; }

template <unsigned Size>
struct thread_block_tile {
    static_assert(Size == cuda_on_cpu::kTile, "the CPU stand-in schedules 32-wide tiles only");
    unsigned thread_rank() const { return cuda_on_cpu::thread_rank() % Size; }
    unsigned meta_group_rank() const { return cuda_on_cpu::thread_rank() / Size; }
    unsigned size() const { return Size; }
    void sync() const { cuda_on_cpu::tile_sync(); }

    unsigned ballot(int predicate) const {
        const int par = cuda_on_cpu::tile_parity();
        sim::me().slot[par][0] = predicate ? 1u : 0u;
        const unsigned g = cuda_on_cpu::tile_sync();
        const sim::Block& b = sim::blk();
        const int first = cuda_on_cpu::tile_first(), last = cuda_on_cpu::tile_last();
        unsigned mask = 0;
        for (int i = first; i < last; ++i)
            if (b.lanes[i].gen_wave >= g && b.lanes[i].slot[par][0]) mask |= 1u << (i - first);
        return mask;
    }

    template <class T> T shfl(T value, int src_rank) const { return exchange(value, static_cast<int>(static_cast<unsigned>(src_rank) % Size)); }
    template <class T> T shfl_up(T value, unsigned delta) const {
        const unsigned rank = thread_rank();
        return exchange(value, rank >= delta ? static_cast<int>(rank - delta) : static_cast<int>(rank));
    }

private:
    template <class T> T exchange(T value, int src_rank) const {
        static_assert(sizeof(T) <= sizeof(uint64_t), "shuffles move up to 8 bytes");
        const int par = cuda_on_cpu::tile_parity();
        uint64_t bits = 0;
        memcpy(&bits, &value, sizeof(T));
        sim::me().slot[par][0] = bits;
        const unsigned g = cuda_on_cpu::tile_sync();
        const sim::Block& b = sim::blk();
        const int src = cuda_on_cpu::tile_first() + src_rank;
        if (src >= cuda_on_cpu::tile_last() || b.lanes[src].gen_wave < g) return value;
        T out;
        memcpy(&out, &b.lanes[src].slot[par][0], sizeof(T));
        return out;
    }
};

template <unsigned Size> inline thread_block_tile<Size> tiled_partition(const thread_block&) { return thread_block_tile<Size>{}; }

}  // namespace cooperative_groups

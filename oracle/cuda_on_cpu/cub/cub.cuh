// TEST-ONLY stand-in for <cub/cub.cuh> (see ../cuda_runtime.h): the handful of CUB entry points a rasterizer's host code and blend kernel use, from
// CUB's documentation. Device-wide algorithms run sequentially on the host and honour the two-call convention (a null workspace pointer asks for
// the workspace size and does nothing else); SortPairs is a stable least-significant-digit radix sort over [begin_bit, end_bit) that leaves its
// result in Current() of the double buffers, flipping the selectors once per 8-bit pass.
#pragma once
#include "../cuda_runtime.h"

#include <vector>

namespace cub {

template <class T>
struct DoubleBuffer {
    T* d_buffers[2];
    int selector;
    DoubleBuffer() : d_buffers{nullptr, nullptr}, selector(0) {}
    DoubleBuffer(T* current, T* alternate) : d_buffers{current, alternate}, selector(0) {}
    T* Current() { return d_buffers[selector]; }
    T* Alternate() { return d_buffers[selector ^ 1]; }
};

struct DeviceRadixSort {
    template <class KeyT, class ValueT>
    static cudaError_t SortPairs(void* d_temp_storage, size_t& temp_storage_bytes, DoubleBuffer<KeyT>& keys, DoubleBuffer<ValueT>& values, int num_items,
                                 int begin_bit = 0, int end_bit = static_cast<int>(sizeof(KeyT) * 8), cudaStream_t = nullptr) {
        if (d_temp_storage == nullptr) { temp_storage_bytes = 1; return cudaSuccess; }
        for (int bit = begin_bit; bit < end_bit; bit += 8) {
            const unsigned mask = (1u << std::min(8, end_bit - bit)) - 1u;
            const KeyT* k_in = keys.Current(); const ValueT* v_in = values.Current();
            KeyT* k_out = keys.Alternate(); ValueT* v_out = values.Alternate();
            size_t start[257] = {};
            for (int i = 0; i < num_items; ++i) ++start[((static_cast<unsigned long long>(k_in[i]) >> bit) & mask) + 1];
            for (int d = 0; d < 256; ++d) start[d + 1] += start[d];
            for (int i = 0; i < num_items; ++i) {
                const size_t at = start[(static_cast<unsigned long long>(k_in[i]) >> bit) & mask]++;
                k_out[at] = k_in[i]; v_out[at] = v_in[i];
            }
            keys.selector ^= 1; values.selector ^= 1;
        }
        return cudaSuccess;
    }
};

struct DeviceScan {
    template <class InT, class OutT>
    static cudaError_t ExclusiveSum(void* d_temp_storage, size_t& temp_storage_bytes, InT d_in, OutT d_out, int num_items, cudaStream_t = nullptr) {
        if (d_temp_storage == nullptr) { temp_storage_bytes = 1; return cudaSuccess; }
        auto sum = decltype(d_in[0] + d_in[0])(0);
        for (int i = 0; i < num_items; ++i) { const auto v = d_in[i]; d_out[i] = sum; sum += v; }      // in place is allowed
        return cudaSuccess;
    }
    template <class InT, class OutT>
    static cudaError_t InclusiveSum(void* d_temp_storage, size_t& temp_storage_bytes, InT d_in, OutT d_out, int num_items, cudaStream_t = nullptr) {
        if (d_temp_storage == nullptr) { temp_storage_bytes = 1; return cudaSuccess; }
        auto sum = decltype(d_in[0] + d_in[0])(0);
        for (int i = 0; i < num_items; ++i) { sum += d_in[i]; d_out[i] = sum; }
        return cudaSuccess;
    }
};

struct Max { template <class T> T operator()(const T& a, const T& b) const { return b > a ? b : a; } };

enum BlockReduceAlgorithm { BLOCK_REDUCE_WARP_REDUCTIONS };

// Block-wide reduction; as in CUB the result is defined in the work-item of rank 0 only.
template <class T, int BLOCK_DIM_X, BlockReduceAlgorithm = BLOCK_REDUCE_WARP_REDUCTIONS, int BLOCK_DIM_Y = 1, int BLOCK_DIM_Z = 1>
class BlockReduce {
public:
    struct TempStorage { T values[BLOCK_DIM_X * BLOCK_DIM_Y * BLOCK_DIM_Z]; };
    explicit BlockReduce(TempStorage& storage) : storage_(storage) {}
    template <class Op> T Reduce(T input, Op op) {
        const unsigned rank = cuda_on_cpu::thread_rank();
        storage_.values[rank] = input;
        __syncthreads();
        T out = input;
        if (rank == 0)
            for (int i = 1; i < BLOCK_DIM_X * BLOCK_DIM_Y * BLOCK_DIM_Z; ++i) out = op(out, storage_.values[i]);
        return out;
    }
private:
    TempStorage& storage_;
};

}  // namespace cub

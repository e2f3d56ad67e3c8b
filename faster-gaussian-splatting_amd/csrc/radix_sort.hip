// Stable LSD radix sort of (key, uint32 value) pairs for the two sorts of the binning stage (K2: 32-bit depth keys of the
// visible Gaussians; K6: tile keys of the instances), written for their sizes on gfx950.
//
// Why not rocPRIM: its onesweep sort is tuned for large inputs -- 16 384 items per 1024-thread workgroup (80 B of scratch per
// lane), one histogram fill plus two fills per 8-bit pass. The depth sort has ~2 M items: ~125 workgroups for 256 CUs behind a
// decoupled look-back chain, 14 launches, 0.167 ms for 32 MB of traffic; the tile sort moves 16 M items at 1.7 TB/s (0.266 ms).
// Here a pass is three launches over 8192-item workgroups (4096 until round 4) -- per-workgroup digit histogram -> one workgroup per digit scans its
// row of the [digit][workgroup] table -> stable scatter -- with ceil(end_bit / 8) passes of evenly split digit widths
// (depth keys 4 x 8 bits, tile keys at 1080p 2 x 7 bits); 8 / 16 / 24 items per thread measured 0.193 / 0.181 / 0.188 ms for the tile
// sort. Measured on MI355X (tools/ab_sort.py, S2): depth sort 0.135 ms,
// tile sort 0.173 ms with rocPRIM's scan between the kernels; wider (11-bit) digits were slower: without the LDS reorder below,
// 2 M x 2 scattered 4-byte stores per pass cost 55-72 us.
//
// Stability (equal keys keep their input order -- the tile sort relies on it to keep each tile's list in depth order,
// fwd:195-202) comes from ranking inside a workgroup in input order: a wave walks its 1024-item segment 64 consecutive items
// at a time; lanes holding the same digit find each other with one ballot per digit bit (the wave64 form of match_any),
// take the digit's running count from the wave's private LDS counters plus their position among the matching lanes, and the
// lowest matching lane advances the counter. Counts of the four waves are prefix-summed per digit afterwards, the items are
// reordered through LDS by digit, and leave so that consecutive lanes store to consecutive addresses of a digit's run.
#include <cstring>

#include "fgs_radix_sort.h"

namespace fgs {

namespace sortimpl {

// One workgroup per digit: exclusive scan of that digit's row of the table (over the workgroups of the sort), in place, and the
// row total. The scatter kernel adds the exclusive scan of the digit totals itself.
__global__ void __launch_bounds__(kSortThreads) radix_row_scan_kernel(uint32_t* __restrict__ table, uint32_t* __restrict__ totals, const uint32_t n_blocks) {
    __shared__ uint32_t s_part[kSortWaves];
    uint32_t* row = table + (size_t)blockIdx.x * n_blocks;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < n_blocks; c0 += kSortThreads * kScanPerThread) {        // workgroup-uniform trip count
        uint32_t v[kScanPerThread], sum = 0;
        const uint32_t first = c0 + threadIdx.x * kScanPerThread;
#pragma unroll
        for (int i = 0; i < kScanPerThread; ++i) { v[i] = first + i < n_blocks ? row[first + i] : 0u; sum += v[i]; }
        uint32_t chunk_total;
        uint32_t run = carry + block_exclusive_scan(sum, s_part, chunk_total);
#pragma unroll
        for (int i = 0; i < kScanPerThread; ++i) { if (first + i < n_blocks) row[first + i] = run; run += v[i]; }
        carry += chunk_total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}
void launch_row_scan(int bits, uint32_t* table, uint32_t* totals, uint32_t n_blocks, hipStream_t s) {
    hipLaunchKernelGGL(radix_row_scan_kernel, dim3(1u << bits), dim3(kSortThreads), 0, s, table, totals, n_blocks);
}

}  // namespace sortimpl
using namespace sortimpl;

// Workgroup shape of both sorts (the kernels are templates on it): **8192 items over 512 threads** (round 5; 4096 over 256 before). Twice the items per
// workgroup double the length of a digit's run in the scatter (depth sort, 512 digits: 8 -> 16 items = 32 -> 64-byte stores; tile sort, 128 digits:
// 32 -> 64 items) and halve the [digit][workgroup] table, its row scans and the histogram workgroups; twice the waves keep the ranking rounds per wave
// at 16. Measured on one box (profiles/r05_ab_sort_blocks.txt, S2): depth sort 0.128 -> 0.115 ms, tile sort 0.164 -> 0.148. Other shapes: depth sort
// 4096 items over 512 / 1024 threads 0.125 / 0.125, 8192 over 1024 0.117, 12288 over 1024 0.124; tile sort 4096 over 512 0.158, 8192 over 1024 0.197,
// 12288 over 512 (24 items per thread: registers) 0.217; 16384 items do not fit the LDS with 32-bit keys.
constexpr int kTileSortThreads = 512, kTileSortItems = 8192 / kTileSortThreads;

// Sized for the smallest workgroups any build launches (fgs_radix_sort.h: kSmallestSortBlock) and the full table: the blob layouts are the same in the
// product and the dev library
size_t own_sort_temp_bytes(uint32_t n, int end_bit) {
    const SortPlan p = plan_sort(n, end_bit, kGenericMaxBits, kSmallestSortBlock);
    return p.table_bytes + p.totals_bytes;
}

hipError_t own_sort_pairs_u32(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n, int end_bit, hipStream_t s) {
    return sort_pairs<uint32_t, kTileSortItems, kTileSortThreads>(temp, temp_bytes, keys, vals, selector, n, nullptr, 0u, end_bit, kGenericMaxBits, s);
}
hipError_t own_sort_pairs_u16(void* temp, size_t temp_bytes, uint16_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n, int end_bit, hipStream_t s) {
    return sort_pairs<uint16_t, kTileSortItems, kTileSortThreads>(temp, temp_bytes, keys, vals, selector, n, nullptr, 0u, end_bit, kGenericMaxBits, s);
}
hipError_t own_sort_pairs_u32_device_count(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t capacity,
                                           const uint32_t* n_ptr, int end_bit, hipStream_t s) {
    return sort_pairs<uint32_t, kTileSortItems, kTileSortThreads>(temp, temp_bytes, keys, vals, selector, capacity, n_ptr, 0u, end_bit, kGenericMaxBits, s);
}
hipError_t own_sort_pairs_u16_device_count(void* temp, size_t temp_bytes, uint16_t* keys[2], uint32_t* vals[2], int& selector, uint32_t capacity,
                                           const uint32_t* n_ptr, int end_bit, hipStream_t s) {
    return sort_pairs<uint16_t, kTileSortItems, kTileSortThreads>(temp, temp_bytes, keys, vals, selector, capacity, n_ptr, 0u, end_bit, kGenericMaxBits, s);
}

// Depth keys are the bit patterns of positive depths that passed the near / far cull (kf:67), i.e. values in [bits(near), bits(far)]:
// sorting key - bits(near) gives the same order in fewer bits.
DepthKeyRange depth_key_range(float near_plane, float far_plane) {
    DepthKeyRange r{0u, 32};
    if (!(near_plane >= 0.0f) || !(far_plane >= near_plane)) return r;                 // negative / NaN planes: no assumption, all 32 bits
    uint32_t lo, hi;
    std::memcpy(&lo, &near_plane, 4); std::memcpy(&hi, &far_plane, 4);
    const uint32_t span = hi - lo;
    int bits = 1;
    while (bits < 32 && (span >> bits) != 0u) ++bits;
    r.base = lo; r.bits = bits;
    return r;
}

// `n` = visible count, or with n_ptr != nullptr a bound of the count stored at n_ptr on the device. Sorted: key - bits(near) in 9-bit digits
// (near 0.2, far 1e4: 27 bits = 3 passes), 8192 items over 512 threads; what it was measured against is in sort_exhibits.hip.
hipError_t own_depth_sort(void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n, const uint32_t* n_ptr,
                          DepthKeyRange range, hipStream_t s, const SortPayload* payload) {
#ifdef FGS_DEV_SWITCHES      // the dev library's other formulations (sort_exhibits.hip); false: the switch selects this one
    hipError_t exhibit_result;
    if (depth_sort_exhibit(exhibit_result, temp, temp_bytes, keys, vals, selector, n, n_ptr, range, s, payload)) return exhibit_result;
#endif
    return sort_pairs<uint32_t, kDepthSortIpt, kDepthSortThreads>(temp, temp_bytes, keys, vals, selector, n, n_ptr, range.base, range.bits, kMaxBits, s, payload);
}

}  // namespace fgs

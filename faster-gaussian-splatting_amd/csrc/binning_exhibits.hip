// The binning chain's A/B exhibits. libfgs_hip_dev.so only (-DFGS_DEV_SWITCHES; the Makefile lists this unit in DEVOBJ and not in OBJ, with
// binning.o's flags); the product library has one formulation of K8+K9, the single-workgroup scan of binning.hip, and none of this file.
//   option 11        run_bucket_scan     the library scan (rocPRIM look-back, two launches) that the single-workgroup scan replaced
//   option 10 (12)   plan_tiles_kernel   the scan plus K10's device-side block plan, for the two mappings that read one (option 12: A/B of the deal)
#ifdef FGS_DEV_SWITCHES   // the whole unit: compiled without the define (the product flavour of the simulation does, it takes every csrc/*.hip) it is empty
#include "fgs_kernels.h"
#include <fgs_wave.h>
#include "fgs_tile_scan.h"
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

namespace fgs {

// ---- option 11: the library scan (rocPRIM), kept for A/B runs (fgs_debug_set_option(11, 1))
struct BucketsOfRange {
    __host__ __device__ uint32_t operator()(const uint2& r) const { return (r.y - r.x + kBucket - 1) / kBucket; }
};
size_t bucket_scan_temp_bytes(uint32_t n_tiles) {
    size_t bytes = 0;
    auto in = rocprim::make_transform_iterator(static_cast<const uint2*>(nullptr), BucketsOfRange{});
    (void)rocprim::inclusive_scan(nullptr, bytes, in, static_cast<uint32_t*>(nullptr), n_tiles, rocprim::plus<uint32_t>());
    return bytes;
}
hipError_t run_bucket_scan(void* temp, size_t temp_bytes, const uint2* ranges, uint32_t* bucket_offsets, uint32_t n_tiles, hipStream_t s) {
    auto in = rocprim::make_transform_iterator(ranges, BucketsOfRange{});
    return rocprim::inclusive_scan(temp, temp_bytes, in, bucket_offsets, n_tiles, rocprim::plus<uint32_t>(), s);
}

// ---- option 10 = 254 / 253: the tile -> workgroup plan of K10 ---------------------------------------------------------------------
// K8+K9's single-workgroup scan (fgs_tile_scan.h: scan_bucket_counts, the product's bucket_scan_kernel) followed, in the same kernel, by
// the plan that K10 reads to decide which tile a workgroup blends (fgs_k10_mappings.h: tile_of_workgroup, row_group == kPlannedBlocks).
// Why a plan: the hardware deals workgroups to the 8 XCDs round-robin (XCD = workgroup % 8), every XCD has its own L2, and a
// Gaussian's record is re-read by every tile it overlaps -- so an XCD should own compact pieces of the image. Round 1/2 gave every
// XCD one contiguous band of tile rows: good locality, but the bands differ in work (at S2 the top band has 30 ms of summed tile time
// against 44-47 ms for the others; on a layered scene 47 against 210-220: XCD 0 idles for two thirds of the kernel) and the heaviest
// rows came last in every band (profiles/archive/r02_k10_timeline_before.txt). Interleaving single rows balances but gives up vertical
// locality (+10 % layered, -9..16 % S2). The plan keeps both: the image is cut into 8 x 10 rectangular blocks of tiles (15 x 9 tiles
// at 1080p: every XCD gets exactly 10 blocks, i.e. the same number of workgroups, which the round-robin deal requires); a block's
// weight is its number of 64-Gaussian buckets (+ 1 per tile) -- known here, on the device, from the scan itself: no host read; the
// blocks are sorted by weight and dealt in 10 rounds of 8, heaviest block of a round to the XCD with the least work so far; an XCD
// walks its blocks in the order received = heaviest first, so the kernel's tail consists of the lightest blocks.
__global__ void __launch_bounds__(kTileScanThreads) plan_tiles_kernel(const uint2* __restrict__ ranges, uint32_t* __restrict__ bucket_offsets,
                                                                      uint32_t* __restrict__ tile_plan, const uint32_t n_tiles,
                                                                      const uint32_t grid_w, const uint32_t grid_h, const int experiment) {
    __shared__ TileScanShared s_scan;
    __shared__ uint32_t s_weight[kPlanBlocks], s_sorted[kPlanBlocks];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < kPlanBlocks) s_weight[tid] = 0u;
    scan_bucket_counts(ranges, bucket_offsets, n_tiles, s_scan);
    if (tile_plan == nullptr) return;                                                        // not from launch_plan_tiles, which runs the scan-only kernel then
    __syncthreads();                                                                        // bucket_offsets visible to the workgroup
    // block weights: one (block, tile row) pair per work item -- a difference of two scan values
    const uint32_t bw = (grid_w + kPlanBlocksX - 1) / kPlanBlocksX, bh = (grid_h + kPlanBlocksY - 1) / kPlanBlocksY;
    for (uint32_t i = tid; i < kPlanBlocks * bh; i += kTileScanThreads) {
        const uint32_t b = i / bh, r = i - b * bh;
        const uint32_t bx = b % kPlanBlocksX, by = b / kPlanBlocksX;
        const uint32_t ty = by * bh + r, x0 = bx * bw, x1 = min(x0 + bw, grid_w);
        if (ty < grid_h && x0 < x1) {
            const uint32_t last = ty * grid_w + x1 - 1u, first = ty * grid_w + x0;
            const uint32_t w = bucket_offsets[last] - (first != 0u ? bucket_offsets[first - 1u] : 0u) + (x1 - x0);
            atomicAdd(&s_weight[b], w);
        }
    }
    __syncthreads();
    // sort the blocks by weight (descending, ties by index): rank by counting -- 80 broadcast reads per thread
    if (tid < kPlanBlocks) {
        const uint32_t w = s_weight[tid];
        uint32_t rank = 0;
        for (uint32_t o = 0; o < kPlanBlocks; ++o) {
            const uint32_t wo = s_weight[o];
            rank += (wo > w || (wo == w && o < tid)) ? 1u : 0u;
        }
        s_sorted[(experiment & 1) ? tid : rank] = tid;                                       // experiment bit 0: no sort (blocks in natural order)
    }
    __syncthreads();
    if (tid < kWave) {                                                                       // wave 0: the deal, lanes 0..7 = the XCDs
        uint32_t load = 0;
        for (uint32_t round = 0; round < kPlanBlocksPerXcd; ++round) {
            uint32_t rank = 0;                                                               // my position among the XCDs by work so far
#pragma unroll
            for (int x = 0; x < kXcds; ++x) {
                const uint32_t lx = wave_read(load, x);
                rank += (lx < load || (lx == load && static_cast<uint32_t>(x) < lane)) ? 1u : 0u;
            }
            if (experiment & 1) rank = lane;                                                 // ... dealt statically: XCD x owns block column x
            if (lane < kXcds) {
                const uint32_t b = s_sorted[round * kXcds + rank];                           // least work so far <- heaviest block of the round
                load += s_weight[b];
                tile_plan[kPlanHeader + lane * kPlanBlocksPerXcd + round] = b;
            }
        }
        if (lane == 0) { tile_plan[0] = bw; tile_plan[1] = bh; tile_plan[2] = bw * bh; tile_plan[3] = kPlanBlocksPerXcd; }
    }
}

hipError_t launch_plan_tiles_exhibit(const uint2* ranges, uint32_t* bucket_offsets, uint32_t* tile_plan, uint32_t n_tiles, uint32_t grid_w, uint32_t grid_h,
                                     hipStream_t s) {
    hipLaunchKernelGGL(plan_tiles_kernel, dim3(1), dim3(kTileScanThreads), 0, s, ranges, bucket_offsets, tile_plan, n_tiles, grid_w, grid_h,
                       static_cast<int>(g_plan_experiment));
    return hipGetLastError();
}

}  // namespace fgs
#endif  // FGS_DEV_SWITCHES

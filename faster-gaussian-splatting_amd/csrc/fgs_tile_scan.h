// Prefix sums over the per-tile arrays (12 240 tiles at 1080p) by ONE 1024-thread workgroup -- the two planning passes of the pipeline
// (binning.hip: bucket scan after K7, scan_bucket_counts below; blend_backward.hip: plan_blend_backward_kernel before K11).
//
// Why a workgroup and not a device-wide scan: at this size the library scan (rocPRIM look-back, two launches) costs 15 us and two earlier
// own versions -- one barrier per 1024-tile chunk; sixteen strided wave scans through ds_bpermute -- 15-19 us: all latency. Here a thread
// owns kTileScanPerThread CONSECUTIVE tiles (16-byte loads, all issued at once), sums them serially, ONE DPP wave scan (6 instructions)
// ranks the threads, and the sixteen wave totals meet behind a single barrier.
#pragma once
#include <fgs_wave.h>
#include "fgs_config.h"

namespace fgs {

constexpr int kTileScanThreads = 1024;
constexpr int kTileScanPerThread = 16;                            // 16 Ki tiles per pass
constexpr int kTileScanWaves = kTileScanThreads / kWave;          // 16

struct TileScanShared { uint32_t wave_total[2][kTileScanWaves]; };   // double-buffered: one barrier per pass

// v[k] = value of tile first + tid * kTileScanPerThread + k (0 beyond the end). On return ex[k] = `base` + the sum of the values of all
// tiles in front of that tile; returns the sum of all values of the pass. Every thread of the 1024-thread workgroup must call it;
// `parity` alternates between consecutive passes of a kernel.
__device__ __forceinline__ uint32_t tile_scan_pass(const uint32_t (&v)[kTileScanPerThread], uint32_t (&ex)[kTileScanPerThread], TileScanShared& s,
                                                   const uint32_t base, const int parity) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t run = 0;
#pragma unroll
    for (int k = 0; k < kTileScanPerThread; ++k) { ex[k] = run; run += v[k]; }
    const uint32_t incl = wave_inclusive_sum(run);
    if (lane == 63u) s.wave_total[parity][wv] = incl;
    __syncthreads();
    uint32_t before = base + incl - run, total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kTileScanWaves; ++w) {               // 16 broadcast reads
        const uint32_t t = s.wave_total[parity][w];
        before += w < wv ? t : 0u;
        total += t;
    }
#pragma unroll
    for (int k = 0; k < kTileScanPerThread; ++k) ex[k] += before;
    return total;
}

// K8+K9 (kf:350-360, fwd:225-231): bucket_offsets[t] = the inclusive scan of ceil(len_t / kBucket) over the tiles' [start, end) ranges. Every thread
// of the 1024-thread workgroup must call it; a workgroup barrier stands between its stores and a read of them by another thread.
__device__ __forceinline__ void scan_bucket_counts(const uint2* ranges, uint32_t* bucket_offsets, const uint32_t n_tiles,
                                                   TileScanShared& s_scan) {
    const uint32_t tid = threadIdx.x;
    uint32_t base = 0;
    int parity = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kTileScanThreads * kTileScanPerThread, parity ^= 1) {   // one pass at 1080p (12 240 tiles)
        uint32_t nb[kTileScanPerThread], ex[kTileScanPerThread];
        const uint32_t first = t0 + tid * kTileScanPerThread;
        if (first + kTileScanPerThread <= n_tiles) {                                         // 128 contiguous bytes: eight 16-byte loads
            const uint4* q = reinterpret_cast<const uint4*>(ranges + first);
#pragma unroll
            for (int k = 0; k < kTileScanPerThread / 2; ++k) {
                const uint4 r = q[k];
                nb[2 * k] = (r.y - r.x + kBucket - 1) / kBucket;                              // kf:350-360
                nb[2 * k + 1] = (r.w - r.z + kBucket - 1) / kBucket;
            }
        } else {
#pragma unroll
            for (int k = 0; k < kTileScanPerThread; ++k) {
                uint2 r = make_uint2(0u, 0u);
                if (first + k < n_tiles) r = ranges[first + k];
                nb[k] = (r.y - r.x + kBucket - 1) / kBucket;
            }
        }
        const uint32_t total = tile_scan_pass(nb, ex, s_scan, base, parity);
        if (first + kTileScanPerThread <= n_tiles) {
            uint4* o = reinterpret_cast<uint4*>(bucket_offsets + first);                      // inclusive (fwd:225-231)
#pragma unroll
            for (int k = 0; k < kTileScanPerThread / 4; ++k)
                o[k] = make_uint4(ex[4 * k] + nb[4 * k], ex[4 * k + 1] + nb[4 * k + 1], ex[4 * k + 2] + nb[4 * k + 2], ex[4 * k + 3] + nb[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < kTileScanPerThread; ++k) if (first + k < n_tiles) bucket_offsets[first + k] = ex[k] + nb[k];
        }
        base += total;
    }
}

}  // namespace fgs

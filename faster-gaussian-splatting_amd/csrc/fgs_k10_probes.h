// Debug probes of K10 (blend_forward.hip: blend_tile; included by that unit alone -- the device arrays and the two read-back entries below are
// DEFINITIONS). blend_tile names five points, FGS_K10_PROBE_TILE_BEGIN .. FGS_K10_PROBE_TILE_END below; unless one of the two defines is set every
// one of them is empty, so the product kernels are token for token the kernels without probes.
//  * FGS_K10_TIMELINE (tools/k10_timeline.sh builds a separate library with it): per tile its start / end on the chip-wide 100 MHz counter, the
//    length of its list, the workgroup that ran it and the XCD that workgroup ran on.
//  * FGS_PAIR_STATS (tools/pair_stats.sh builds a separate library with it), counted over the training blend: [0] tiles, [1] instances staged,
//    [2] (Gaussian, 16x4 strip) pairs walked (the union of the two sub-tile masks), [3] lanes of walked pairs whose own 8x4 sub-tile is hit and whose
//    pixel is not finished, [4] lanes that blended (alpha test passed), [5] (Gaussian, strip) slots offered to the cull = 64-Gaussian chunks x 64
//    seen by a wave that still had a live pixel.
// The probes are macros over plain locals of blend_tile (st_*, t_start_), the form that left all three builds of K11 instruction for instruction
// what they were (fgs_k11_probes.h, profiles/k11_exhibits_split.txt); the same holds here (profiles/k10_exhibits_split.txt).
#pragma once
#include "fgs_kernels.h"
#include <fgs_wave.h>

#ifdef FGS_K10_TIMELINE
#define FGS_K10_IF_TIMELINE(...) __VA_ARGS__
#else
#define FGS_K10_IF_TIMELINE(...)
#endif
#ifdef FGS_PAIR_STATS
#define FGS_K10_IF_STATS(...) __VA_ARGS__
#else
#define FGS_K10_IF_STATS(...)
#endif

// the top of a tile, behind the early return of the padding workgroups
#define FGS_K10_PROBE_TILE_BEGIN() \
    FGS_K10_IF_TIMELINE(const unsigned long long t_start_ = __builtin_amdgcn_s_memrealtime();) \
    FGS_K10_IF_STATS(unsigned st_staged = 0, st_pairs = 0, st_mine = 0, st_pass = 0, st_offered = 0;)

// one 64-Gaussian chunk of a batch, behind its cull (done: this lane's pixel is finished)
#define FGS_K10_PROBE_CHUNK(wave, done, batch, chunk) FGS_K10_IF_STATS( \
    if (wave == 0) st_staged += min(static_cast<unsigned>(kBucket), batch - chunk); \
    if (wave_ballot(!done) != 0) st_offered += min(static_cast<unsigned>(kBucket), batch - chunk);)

// one trip of the walk: one list entry, or two (second)
#define FGS_K10_PROBE_TRIP(second) FGS_K10_IF_STATS(st_pairs += second ? 2u : 1u;)

// one list entry (bit k of the walked word), in front of its alpha test
#define FGS_K10_PROBE_ENTRY(not_mine, k, gate, tested) FGS_K10_IF_STATS( \
    st_mine += static_cast<unsigned>(__popcll(wave_ballot(((not_mine << k) & 0x80000000u) == 0u && gate < 1.0f))); \
    st_pass += static_cast<unsigned>(__popcll(wave_ballot(tested >= gate)));)

// the end of a tile: the write-out (timeline word 3: XCC_ID)
#define FGS_K10_PROBE_TILE_END(TRAINING, tid, wave, lane, tile, n_total) \
    FGS_K10_IF_STATS( \
        if (TRAINING && lane == 0) { \
            if (wave == 0) { atomicAdd(&g_k10_pair_stats[0], 1ull); atomicAdd(&g_k10_pair_stats[1], static_cast<unsigned long long>(st_staged)); } \
            atomicAdd(&g_k10_pair_stats[2], static_cast<unsigned long long>(st_pairs)); atomicAdd(&g_k10_pair_stats[3], static_cast<unsigned long long>(st_mine)); \
            atomicAdd(&g_k10_pair_stats[4], static_cast<unsigned long long>(st_pass)); atomicAdd(&g_k10_pair_stats[5], static_cast<unsigned long long>(st_offered)); \
        }) \
    FGS_K10_IF_TIMELINE( \
        if (tid == 0 && tile < kK10TimelineTiles) { \
            g_k10_timeline[tile * 4u] = t_start_; \
            g_k10_timeline[tile * 4u + 1u] = __builtin_amdgcn_s_memrealtime(); \
            g_k10_timeline[tile * 4u + 2u] = (static_cast<unsigned long long>(n_total) << 32) | blockIdx.x; \
            g_k10_timeline[tile * 4u + 3u] = static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11))); \
        })

namespace fgs {
#ifdef FGS_K10_TIMELINE
constexpr unsigned kK10TimelineTiles = 1u << 17;
__device__ unsigned long long g_k10_timeline[kK10TimelineTiles * 4];
#endif
#ifdef FGS_PAIR_STATS
__device__ unsigned long long g_k10_pair_stats[8];
#endif
}  // namespace fgs

// the read-back entries of the two probe libraries (tools/k10_timeline.py, tools/pair_stats.py)
#ifdef FGS_K10_TIMELINE
extern "C" __attribute__((visibility("default"))) int fgs_debug_k10_timeline(unsigned long long* out, unsigned n_tiles, int reset) {
    if (n_tiles > fgs::kK10TimelineTiles) n_tiles = fgs::kK10TimelineTiles;
    if (out != nullptr && hipMemcpyFromSymbol(out, HIP_SYMBOL(fgs::g_k10_timeline), sizeof(unsigned long long) * 4 * n_tiles) != hipSuccess) return -1;
    if (reset) {
        void* dev = nullptr;
        if (hipGetSymbolAddress(&dev, HIP_SYMBOL(fgs::g_k10_timeline)) != hipSuccess
            || hipMemset(dev, 0, sizeof(unsigned long long) * 4 * fgs::kK10TimelineTiles) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef FGS_PAIR_STATS
extern "C" __attribute__((visibility("default"))) int fgs_debug_k10_pair_stats(unsigned long long* out, int reset) {
    if (out != nullptr && hipMemcpyFromSymbol(out, HIP_SYMBOL(fgs::g_k10_pair_stats), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        void* dev = nullptr;
        if (hipGetSymbolAddress(&dev, HIP_SYMBOL(fgs::g_k10_pair_stats)) != hipSuccess || hipMemset(dev, 0, sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    }
    return 0;
}
#endif

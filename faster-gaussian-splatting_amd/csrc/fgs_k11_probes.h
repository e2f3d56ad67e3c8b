// Debug probes of K11's shipped kernel (blend_backward.hip: blend_backward_compact_kernel; included by that unit alone -- the device arrays and the
// two read-back entries below are DEFINITIONS). The kernel names five points, FGS_K11_PROBE_ITEM_BEGIN .. FGS_K11_PROBE_ITEM_END below; unless one of
// the two defines is set every one of them is empty, so the product kernel is token for token the kernel without probes.
//  * FGS_K11_TIMELINE (tools/k11_timeline.sh builds a separate library with it): per work item its start / end timestamp, the number of pipeline steps
//    and the hardware id of the wave -- concurrency over time, per-item durations, load per XCD / CU.
//  * FGS_PAIR_STATS (tools/pair_stats.sh builds a separate library with it): how many of the (pixel, Gaussian) lane-steps K11 issues pass the alpha
//    test -- [0] work items, [1] pipeline steps, [2] steps whose contribution block ran (at least one lane passed), [3] lane-steps with a real pixel in
//    front of its last contributor, [4] lane-steps that passed the alpha test, [5] live pixels outside the union of the bucket's screen bounds.
// The probes are macros over plain locals of the kernel (st_*, t_start_, c_start_), not an object with inline functions: the step lambda captures
// what it names by reference, and both forms were tried -- an object there, even an empty one, moved the register allocation of the product kernel,
// and helper functions moved that of the two probe builds. As macros all three builds are instruction for instruction what they were with the blocks inline.
#pragma once
#include "fgs_kernels.h"
#include <fgs_wave.h>

#ifdef FGS_K11_TIMELINE
#define FGS_K11_IF_TIMELINE(...) __VA_ARGS__
#else
#define FGS_K11_IF_TIMELINE(...)
#endif
#ifdef FGS_PAIR_STATS
#define FGS_K11_IF_STATS(...) __VA_ARGS__
#else
#define FGS_K11_IF_STATS(...)
#endif

// option 7 of the dev library (g_backward_ablate, blend_backward_exhibits.hip): timing experiments that switch parts of the kernels off
#ifdef FGS_DEV_SWITCHES
#define FGS_ABLATE(a) ((a).ablate)      // timing experiments of the dev build (fgs_debug_set_option key 7)
#else
#define FGS_ABLATE(a) 0
#endif

// the top of a work item (the timestamp counter runs at 100 MHz, the same clock on every CU; the cycle counter is not)
#define FGS_K11_PROBE_ITEM_BEGIN() \
    FGS_K11_IF_TIMELINE(const unsigned long long t_start_ = __builtin_amdgcn_s_memrealtime(); \
                        const unsigned long long c_start_ = __builtin_readcyclecounter();) \
    FGS_K11_IF_STATS(uint64_t st_live[kTilePixels / kWave] = {}; unsigned st_steps = 0, st_body = 0, st_elig = 0, st_pass = 0;)

// staging: the ballot of the live pixels of chunk c (64 pixels of the tile)
#define FGS_K11_PROBE_LIVE_PIXELS(c, m) FGS_K11_IF_STATS(st_live[c] = m;)

// once the lane's Gaussian is known -- st_trim, [5]: live pixels outside the union of the bucket's screen bounds
// (bx, by: x_min | x_max << 16, an empty box for lanes without a Gaussian)
#define FGS_K11_PROBE_BUCKET_BOUNDS(a, tile, lane, valid_prim, prim) FGS_K11_IF_STATS( \
    unsigned st_trim = 0; \
    { \
        unsigned bx = 0xffffu, by = 0xffffu; \
        if (valid_prim) { const float4 r2q = reinterpret_cast<const float4*>(a.rec + prim)[2]; bx = __float_as_uint(r2q.y); by = __float_as_uint(r2q.z); } \
        const unsigned ux0 = 0xffffu - wave_max(0xffffu - (bx & 0xffffu)), ux1 = wave_max(bx >> 16); \
        const unsigned uy0 = 0xffffu - wave_max(0xffffu - (by & 0xffffu)), uy1 = wave_max(by >> 16); \
        const unsigned tx_px = (tile % a.grid_w) * kTileW, ty_px = (tile / a.grid_w) * kTileH; \
        _Pragma("unroll") \
        for (int c = 0; c < kTilePixels / kWave; ++c) { \
            const unsigned p = static_cast<unsigned>(c) * kWave + lane; \
            const unsigned px_ = tx_px + (p & (kTileW - 1)), py_ = ty_px + p / kTileW; \
            const bool inside = px_ >= ux0 && px_ < ux1 && py_ >= uy0 && py_ < uy1; \
            st_trim += static_cast<unsigned>(__popcll(st_live[c] & wave_ballot(!inside))); \
        } \
    })

// one pipeline step, in front of its alpha test
#define FGS_K11_PROBE_STEP(lane_f, rel, alpha) FGS_K11_IF_STATS( \
    { \
        const uint64_t me_ = wave_ballot(lane_f < rel), mp_ = wave_ballot(lane_f < rel && alpha >= kMinAlphaThreshold); \
        st_steps += 1u; st_body += mp_ != 0 ? 1u : 0u; \
        st_elig += static_cast<unsigned>(__popcll(me_)); st_pass += static_cast<unsigned>(__popcll(mp_)); \
    })

// the end of a work item: the write-out (timeline word 3: HW_ID, all 32 bits, over XCC_ID (gfx94x+))
#define FGS_K11_PROBE_ITEM_END(lane, item, n_steps) \
    FGS_K11_IF_STATS( \
        if (lane == 0) { \
            atomicAdd(&g_k11_pair_stats[0], 1ull); atomicAdd(&g_k11_pair_stats[1], static_cast<unsigned long long>(st_steps)); \
            atomicAdd(&g_k11_pair_stats[2], static_cast<unsigned long long>(st_body)); atomicAdd(&g_k11_pair_stats[3], static_cast<unsigned long long>(st_elig)); \
            atomicAdd(&g_k11_pair_stats[4], static_cast<unsigned long long>(st_pass)); atomicAdd(&g_k11_pair_stats[5], static_cast<unsigned long long>(st_trim)); \
        }) \
    FGS_K11_IF_TIMELINE( \
        if (lane == 0 && item < kK11TimelineItems) { \
            g_k11_timeline[item * 4u] = t_start_; \
            g_k11_timeline[item * 4u + 1u] = __builtin_amdgcn_s_memrealtime(); \
            g_k11_timeline[item * 4u + 2u] = static_cast<unsigned long long>(n_steps) | ((__builtin_readcyclecounter() - c_start_) << 16); \
            g_k11_timeline[item * 4u + 3u] = (static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11))) << 32) \
                                            | static_cast<unsigned long long>(__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11))); \
        })

namespace fgs {
#ifdef FGS_K11_TIMELINE
constexpr unsigned kK11TimelineItems = 1u << 18;
__device__ unsigned long long g_k11_timeline[kK11TimelineItems * 4];
#endif
#ifdef FGS_PAIR_STATS
__device__ unsigned long long g_k11_pair_stats[8];
#endif
}  // namespace fgs

// the read-back entries of the two probe libraries (tools/k11_timeline.py, tools/pair_stats.py)
#ifdef FGS_K11_TIMELINE
extern "C" __attribute__((visibility("default"))) int fgs_debug_k11_timeline(unsigned long long* out, unsigned n_items, int reset) {
    if (n_items > fgs::kK11TimelineItems) n_items = fgs::kK11TimelineItems;
    if (out != nullptr && hipMemcpyFromSymbol(out, HIP_SYMBOL(fgs::g_k11_timeline), sizeof(unsigned long long) * 4 * n_items) != hipSuccess) return -1;
    if (reset) {
        void* dev = nullptr;
        if (hipGetSymbolAddress(&dev, HIP_SYMBOL(fgs::g_k11_timeline)) != hipSuccess
            || hipMemset(dev, 0, sizeof(unsigned long long) * 4 * fgs::kK11TimelineItems) != hipSuccess) return -1;
    }
    return 0;
}
#endif
#ifdef FGS_PAIR_STATS
extern "C" __attribute__((visibility("default"))) int fgs_debug_k11_pair_stats(unsigned long long* out, int reset) {
    if (out != nullptr && hipMemcpyFromSymbol(out, HIP_SYMBOL(fgs::g_k11_pair_stats), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) {
        void* dev = nullptr;
        if (hipGetSymbolAddress(&dev, HIP_SYMBOL(fgs::g_k11_pair_stats)) != hipSuccess || hipMemset(dev, 0, sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    }
    return 0;
}
#endif

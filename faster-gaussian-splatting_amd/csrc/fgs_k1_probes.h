// Debug probes of K1 (preprocess.hip: preprocess_body; included by that unit alone -- the device array and the two read-back entries below are
// DEFINITIONS). The body names the timer's marks, FGS_K1_START / FGS_K1_MARK(i) / FGS_K1_FLUSH, and takes its SH coefficients through
// FGS_K1_SH_COEFFICIENTS; unless one of the two defines is set the marks are empty and the coefficients are the Gaussian's own row, so the product
// kernels are token for token the kernels without probes (macros over plain locals of the body, the form of fgs_k11_probes.h / fgs_k10_probes.h).
#pragma once
#include "fgs_kernels.h"
#include <fgs_wave.h>

namespace fgs {

// Debug-only phase timer (tools/k1_phase_timer.sh builds a separate library with -DFGS_K1_PHASE_TIMER; the product build has none of it):
// every wave keeps the cycles it spent between two marks in (scalar) registers and stores them ONCE, to its own slot of g_k1_phase, at the
// end -- a first version with one atomic per mark onto eight shared words slowed the kernel 9x and measured only itself. A wave's memory
// waits land in the phase that first uses the data, i.e. where the wave stalls. Result at S2 (profiles/archive/r02_k1_phases.txt): loads +
// projection 20 %, flattened tile count 26 %, SH colour + record 23 %, and 24 % in the last phase -- waves waiting at the workgroup
// barrier of the compaction for slower siblings, not the counter's round trip: requesting the counter before the colour phase so that
// the round trip overlaps with it made the kernel 6.5 % SLOWER (profiles/archive/r02_ab_k1_early_counter.txt) and was reverted.
#ifdef FGS_K1_PHASE_TIMER
constexpr unsigned kK1TimerWaves = 1u << 17;
__device__ unsigned long long g_k1_phase[kK1TimerWaves * 8];
#define FGS_K1_MARK(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); t_phase_[i] += now_ - t_prev_; t_prev_ = now_; } while (0)
#define FGS_K1_START unsigned long long t_phase_[8] = {}; unsigned long long t_prev_ = __builtin_readcyclecounter()
#define FGS_K1_FLUSH do { const unsigned w_ = (blockIdx.x * kPreprocessBlock + threadIdx.x) >> 6; \
                          if (lane_id() < 8u && w_ < kK1TimerWaves) g_k1_phase[w_ * 8u + lane_id()] += t_phase_[0] * (lane_id() == 0) + t_phase_[1] * (lane_id() == 1) + \
                              t_phase_[2] * (lane_id() == 2) + t_phase_[3] * (lane_id() == 3) + t_phase_[4] * (lane_id() == 4) + t_phase_[5] * (lane_id() == 5); } while (0)
#else
#define FGS_K1_MARK(i) do { } while (0)
#define FGS_K1_START do { } while (0)
#define FGS_K1_FLUSH do { } while (0)
#endif

// `const float* k` = the 45 SH-rest coefficients sh_to_color reads for Gaussian idx (a: PreprocessArgs, cam: the loaded camera, lane: lane_id())
#if defined(FGS_K1_SH_PROBE)
// TIMING PROBE, wrong colours (tools/build_variant.sh k1probe preprocess.hip -DFGS_K1_SH_PROBE): the lane's 45 coefficients are taken from the
// wave's 11.25 KB block with perfectly coalesced 16-byte loads (lane l takes float4 i*64 + l of the block) -- what staging the block through LDS
// could reach at most, without the LDS traffic. Measured: 0.198-0.201 -> 0.188-0.189 ms (profiles/r06_ab_k1_sh_probe.txt): the staging was not built.
#define FGS_K1_SH_COEFFICIENTS(k, a, cam, idx, lane) \
                float kk[48]; \
                { \
                    const size_t wave_first = (size_t)(idx & ~63u) * 45u; \
                    const size_t total = (size_t)a.n * 45u; \
                    const float* blk = a.sh_rest + wave_first; \
                    _Pragma("unroll") \
                    for (int i = 0; i < 12; ++i) { \
                        const size_t e = ((size_t)i * 64u + lane) * 4u; \
                        const bool in = i < 11 ? (wave_first + e + 3u < total) : (lane < 16u && wave_first + e + 3u < total); \
                        const float4 v = in ? *reinterpret_cast<const float4*>(blk + e) : make_float4(0.f, 0.f, 0.f, 0.f); \
                        kk[4 * i] = v.x; kk[4 * i + 1] = v.y; kk[4 * i + 2] = v.z; kk[4 * i + 3] = v.w; \
                    } \
                } \
                const float* k = kk
#else
#define FGS_K1_SH_COEFFICIENTS(k, a, cam, idx, lane) const float* k = a.sh_rest + (size_t)idx * cam.total_sh_rest * 3
#endif

}  // namespace fgs

#ifdef FGS_K1_PHASE_TIMER
// debug build only: sum (and optionally clear) the per-wave, per-phase cycle counts of preprocess_body
extern "C" __attribute__((visibility("default"))) int fgs_debug_k1_phases(unsigned long long* out8, int reset) {
    static unsigned long long host[fgs::kK1TimerWaves * 8];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(fgs::g_k1_phase), sizeof(host)) != hipSuccess) return -1;
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    for (unsigned w = 0; w < fgs::kK1TimerWaves; ++w) for (int i = 0; i < 8; ++i) out8[i] += host[w * 8u + i];
    if (reset) {
        void* dev = nullptr;
        if (hipGetSymbolAddress(&dev, HIP_SYMBOL(fgs::g_k1_phase)) != hipSuccess || hipMemset(dev, 0, sizeof(host)) != hipSuccess) return -1;
    }
    return 0;
}
// the raw per-wave table ([wave][8] cycles, waves in launch order): for the distribution of a phase over the waves (is the kernel's time a tail?)
extern "C" __attribute__((visibility("default"))) int fgs_debug_k1_phase_waves(unsigned long long* out, unsigned n_waves) {
    if (n_waves > fgs::kK1TimerWaves) n_waves = fgs::kK1TimerWaves;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fgs::g_k1_phase), sizeof(unsigned long long) * 8u * n_waves) == hipSuccess ? 0 : -1;
}
#endif

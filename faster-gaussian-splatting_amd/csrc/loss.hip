// Fused photometric loss  lambda_l1 * L1 + lambda_dssim * (1 - SSIM)  and its gradient w.r.t. the rendered image, for
// gfx950: the step between the two halves of the hot path in every training iteration (Trainer.py:190-196, Loss.py:15-16;
// SURVEY.md 8f rank 2). The reference calls `fused_dssim` from the un-vendored NeRFICG framework; this implements the
// published SSIM as used by 3D Gaussian Splatting (11x11 Gaussian window, sigma 1.5, zero padding, C1 = 0.01^2,
// C2 = 0.03^2, mean over channels and pixels); tests/test_loss.py pins it against a torch conv2d + autograd implementation.
//
// Two launches replace the ~30 elementwise/conv kernels of a framework-level SSIM, and both STREAM: a wave owns a strip of 64 columns of one
// channel and a band of rows, and marches down it one input row at a time (lane = column). No workgroup barrier and no tile in LDS:
//   per input row   the strip + a 5-column halo on each side is loaded (zero padding; the loads run kPrefetch rows ahead of their use), written to
//                   the wave's own LDS row, and filtered horizontally from there: 11 taps per map, read straight from LDS;
//   register ring   the horizontally filtered values of the last 11 rows stay in registers (five maps forward, three backward). The row loop is
//                   unrolled 11 times so that every ring index is a constant;
//   per output row  from the 11th input row on, the vertical taps over the ring give one output row.
//   ssim_forward_kernel : SSIM value + the three partial derivative maps (d/dmu1, d/dE[x^2], d/dE[xy]); one pair of partial sums per wave.
//   ssim_backward_kernel: filters the three derivative maps with the same (self-adjoint) window and combines them with
//                         x, y and the L1 sign: dloss/dimage, no dependence on the loss value -> no host sync anywhere.
// The vertical halo is paid once per band -- (B + 10) / B on the horizontal half of the work -- instead of once per 32-row tile, and a wave that waits
// for memory stalls alone. The tiled formulation this replaced (32 x 32 and 64 x 32 tiles staged in 36 KB of LDS, five barriers per tile) is the dev
// library's exhibit, loss_exhibits.hip; what the two share, the per-pixel algebra included, is fgs_loss.h. Figures: profiles/loss_streaming.txt.
// Each kernel is a template <bool WEIGHTED>: false is the loss above, true the same loss with a per-pixel weight / mask (INTEGRATION.md 'Weighted loss').
#include "fgs_loss.h"
#include <type_traits>

namespace fgs {

// Band heights: rows of output per wave. 1080p has 90 strip-channels; the grid should fill the chip's wave slots once and evenly, and the halo rows
// cost (B + 10) / B on the horizontal part. Measured (profiles/loss_streaming.txt).
#ifndef FGS_LOSS_BAND_H
#define FGS_LOSS_BAND_H 24
#endif
#ifndef FGS_LOSS_BWD_BAND_H
#define FGS_LOSS_BWD_BAND_H 24
#endif
#ifndef FGS_LOSS_PREFETCH
#define FGS_LOSS_PREFETCH 2      // input rows whose global loads are in flight ahead of the row being filtered
#endif
constexpr int kStripW = 64, kRowFloats = kStripW + 2 * kHalo, kRowPitch = 80;      // one LDS row: 74 floats, padded
constexpr int kBandH = FGS_LOSS_BAND_H, kBwdBandH = FGS_LOSS_BWD_BAND_H, kPrefetch = FGS_LOSS_PREFETCH;
constexpr unsigned kStripWaves = 4;                                                 // waves per workgroup, each with a strip-band of its own
static_assert(kPrefetch >= 1 && kBandH >= 1 && kBwdBandH >= 1 && kRowFloats <= kRowPitch, "at least the next row is in flight; a row fits its LDS pitch");

// The strip-bands of an image in (channel, band, strip) order; a workgroup takes four consecutive ones, an XCD a contiguous run of workgroups.
struct StripGrid {
    unsigned strips, bands, band_h;
    __host__ __device__ StripGrid(int width, int height, int band_h_) : strips((width + kStripW - 1) / kStripW), bands((height + band_h_ - 1) / band_h_), band_h(band_h_) {}
    __host__ __device__ unsigned units() const { return strips * bands * 3u; }
    __host__ __device__ unsigned groups() const { return (units() + kStripWaves - 1u) / kStripWaves; }
};
struct StripBand { int x0, y0, y1, c; unsigned unit; };
// wave-uniform. false: a spare workgroup or a spare wave of the last one -- nothing to do
__device__ __forceinline__ bool strip_band_of(const StripGrid g, const int height, StripBand& b) {
    unsigned group;
    if (!xcd_region_unit(blockIdx.x, g.groups(), group)) return false;
    b.unit = group * kStripWaves + wave_uniform(static_cast<unsigned>(threadIdx.x) >> 6);
    if (b.unit >= g.units()) return false;
    const unsigned per_plane = g.strips * g.bands;
    const unsigned c = b.unit / per_plane, in_plane = b.unit - c * per_plane, band = in_plane / g.strips;
    b.c = c; b.x0 = (in_plane - band * g.strips) * kStripW; b.y0 = band * g.band_h;
    b.y1 = b.y0 + static_cast<int>(g.band_h) < height ? b.y0 + static_cast<int>(g.band_h) : height;
    return true;
}

// Which element of an input row does this lane load besides its own column x0 + lane? Lanes 0..4 the left halo, 5..9 the right one.
struct HaloLane { bool active; int gx, slot; };
__device__ __forceinline__ HaloLane halo_lane_of(const int lane, const int x0, const int width) {
    HaloLane h;
    h.gx = lane < kHalo ? x0 - kHalo + lane : x0 + kStripW + lane - kHalo;
    h.slot = lane < kHalo ? lane : kStripW + lane;                      // LDS row: column x0 - 5 + slot
    h.active = lane < 2 * kHalo && h.gx >= 0 && h.gx < width;
    return h;
}

// One turn of the ring: the step of ring slot PH runs for input row k with k % 11 == PH -- k starts at 0 in front of slot 0 and every step is followed by
// ++k -- and the enclosing for (;;) is left by the `break` in here after the band's last input row (n_in = rows + 10 >= 11, so slot 0 always runs).
#define FGS_RING_STEPS(step) \
    step(std::integral_constant<int, 0>{}); if (++k >= n_in) break; step(std::integral_constant<int, 1>{}); if (++k >= n_in) break; \
    step(std::integral_constant<int, 2>{}); if (++k >= n_in) break; step(std::integral_constant<int, 3>{}); if (++k >= n_in) break; \
    step(std::integral_constant<int, 4>{}); if (++k >= n_in) break; step(std::integral_constant<int, 5>{}); if (++k >= n_in) break; \
    step(std::integral_constant<int, 6>{}); if (++k >= n_in) break; step(std::integral_constant<int, 7>{}); if (++k >= n_in) break; \
    step(std::integral_constant<int, 8>{}); if (++k >= n_in) break; step(std::integral_constant<int, 9>{}); if (++k >= n_in) break; \
    step(std::integral_constant<int, 10>{}); if (++k >= n_in) break;

// WEIGHTED (a.weight, [H,W]; INTEGRATION.md 'Weighted loss'): the same strips and the same order of every sum, so all-ones weights reproduce the
// unweighted bits. Three differences: a row is loaded with its weights and x' = the target where the weight is not positive (a select: whatever x holds
// there, NaN included, goes nowhere), the L1 term carries the weight of its pixel and the output row reads the weights of ITS pixels (lines this wave
// brought in five rows earlier) and multiplies the SSIM value and the three derivative maps by them, and the waves of channel 0 leave their sum of
// weights in a.wpartials.
struct FwdRow { float x, y, hx, hy, w; };      // the lane's own column and its halo element of one input row; w: the weight of (row, own column)
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_forward_kernel(const LossArgs a, const GaussWindow gw) {
    __shared__ float s_rows[kStripWaves][2][2][kRowPitch];                             // per wave: two rows in turn (no fence between a row's reads and the next row's writes), x and y
    StripBand sb;
    if (!strip_band_of(StripGrid(a.width, a.height, kBandH), a.height, sb)) return;    // wave-uniform; the kernel has no workgroup barrier
    const int lane = static_cast<int>(lane_id()), gx = sb.x0 + lane, width = a.width, height = a.height;
    const HaloLane halo = halo_lane_of(lane, sb.x0, width);
    const bool own = gx < width;
    const size_t plane = (size_t)width * height;
    const float* __restrict__ X = a.image + sb.c * plane; const float* __restrict__ Y = a.target + sb.c * plane;
    const float* __restrict__ Wt = a.weight;
    float (*const rows)[2][kRowPitch] = s_rows[threadIdx.x >> 6];
    const int n_in = sb.y1 - sb.y0 + 2 * kHalo;                                        // input rows y0 - 5 .. y1 + 4

    auto load_row = [&](const int iy) {
        FwdRow r{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (iy >= 0 && iy < height && iy < sb.y1 + kHalo) {                            // wave-uniform; zero padding outside, nothing past the band's last input row
            const size_t at = (size_t)iy * width;
            if (own) {
                r.y = Y[at + gx];
                if constexpr (WEIGHTED) { r.w = Wt[at + gx]; r.x = r.w > 0.0f ? X[at + gx] : r.y; } else r.x = X[at + gx];
            }
            if (halo.active) {
                r.hy = Y[at + halo.gx];
                if constexpr (WEIGHTED) r.hx = Wt[at + halo.gx] > 0.0f ? X[at + halo.gx] : r.hy; else r.hx = X[at + halo.gx];
            }
        }
        return r;
    };
    FwdRow ahead[kPrefetch];
#pragma unroll
    for (int d = 0; d < kPrefetch; ++d) ahead[d] = load_row(sb.y0 - kHalo + d);

    float ring[5][kTaps];
    float l1_sum = 0.0f, ssim_sum = 0.0f;
    [[maybe_unused]] float w_sum = 0.0f;
    int k = 0;                                                                         // input row y0 - 5 + k
    auto step = [&](auto phase) {
        constexpr int PH = decltype(phase)::value;                                     // == k % 11: the ring slot of this input row
        const int iy = sb.y0 - kHalo + k, oy = iy - kHalo;
        const bool emits = k >= kTaps - 1;                                             // the ring is full: output row oy
        const FwdRow cur = ahead[0];
#pragma unroll
        for (int d = 0; d + 1 < kPrefetch; ++d) ahead[d] = ahead[d + 1];
        ahead[kPrefetch - 1] = load_row(iy + kPrefetch);
        [[maybe_unused]] float wp = 0.0f;
        if constexpr (WEIGHTED) { if (emits && own) wp = effective_weight(Wt[(size_t)oy * width + gx]); }
        float* const sx = rows[k & 1][0]; float* const sy = rows[k & 1][1];
        sx[lane + kHalo] = cur.x; sy[lane + kHalo] = cur.y;
        if (lane < 2 * kHalo) { sx[halo.slot] = cur.hx; sy[halo.slot] = cur.hy; }
        wave_lds_fence();
        float m1 = 0.0f, m2 = 0.0f, m11 = 0.0f, m22 = 0.0f, m12 = 0.0f;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {                                              // horizontal taps; the three products once per staged value read
            const float p = sx[lane + t], q = sy[lane + t], w = gw.w[t];
            m1 = tap(w, p, m1); m2 = tap(w, q, m2); m11 = tap(w, p * p, m11); m22 = tap(w, q * q, m22); m12 = tap(w, p * q, m12);
        }
        ring[0][PH] = m1; ring[1][PH] = m2; ring[2][PH] = m11; ring[3][PH] = m22; ring[4][PH] = m12;
        if (own && iy >= sb.y0 && iy < sb.y1) {                                        // the L1 term of the band's own pixel
            if constexpr (WEIGHTED) l1_sum += effective_weight(cur.w) * fabsf(cur.x - cur.y);
            else l1_sum += fabsf(cur.x - cur.y);
        }
        if (emits) {                                                                   // wave-uniform
            float v[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                float acc = 0.0f;
#pragma unroll
                for (int t = 0; t < kTaps; ++t) acc = tap(gw.w[t], ring[m][(PH + 1 + t) % kTaps], acc);   // tap t: input row k - 10 + t
                v[m] = acc;
            }
            if (own) {
                const SsimPoint s = ssim_point(v[0], v[1], v[2], v[3], v[4]);
                const size_t e = sb.c * plane + (size_t)oy * width + gx;
                if constexpr (WEIGHTED) {        // the weight of the OUTPUT pixel on the SSIM value and on its three derivatives: the backward filter stays what it is
                    w_sum += wp;
                    ssim_sum += wp * s.value;
                    a.d_mu[e] = wp * s.d_mu; a.d_m11[e] = wp * s.d_m11; a.d_m12[e] = wp * s.d_m12;
                } else {
                    ssim_sum += s.value;
                    a.d_mu[e] = s.d_mu; a.d_m11[e] = s.d_m11; a.d_m12[e] = s.d_m12;
                }
            }
        }
    };
    for (;;) { FGS_RING_STEPS(step) }
    // per-wave partial sums at the wave's unit index, reduced in that order by reduce_loss_partials: thousands of waves adding to two words would
    // serialise on the same-address atomic rate (measured 0.28 ms at 1080p), and a fixed order makes the loss reproducible
    const float wl = wave_sum_to_lane63(l1_sum), ws = wave_sum_to_lane63(ssim_sum);
    if constexpr (WEIGHTED) {
        const float ww = wave_sum_to_lane63(w_sum);
        if (lane == 63 && sb.c == 0) a.wpartials[sb.unit] = ww;                        // once, not once per channel: channel 0's unit index IS the unit's index in the plane
    }
    if (lane == 63) { a.partials[2 * sb.unit] = wl; a.partials[2 * sb.unit + 1] = ws; }
}

#ifndef FGS_LOSS_SEPARATE_REDUCE
#define FGS_LOSS_SEPARATE_REDUCE 0       // A/B knob: 1 = the reduction as a launch of its own between the two filter kernels (until round 6)
#endif
// Loss value only (no gradient asked for: the autograd form, whose forward call must leave a valid value). With a gradient in the same call, workgroup 0 of
// the backward kernel does this on its way in (round 6: one launch less, -12 us per fused iteration, profiles/r06_ab_loss_reduce.txt).
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_reduce_kernel(const LossArgs a, const unsigned n_partials) {
    __shared__ float s_red[WEIGHTED ? 12 : 8];
    if constexpr (WEIGHTED) reduce_loss_partials<true>(a, n_partials, s_red, weight_total(a, n_partials / 3u, s_red + 8));
    else reduce_loss_partials<false>(a, n_partials, s_red);
}

// The weighted backward kernel needs S in EVERY workgroup, and S is a reduction over the forward launch: workgroup 0 cannot produce it for the others
// without them waiting on it (no inter-workgroup waits here). One call with a gradient therefore either launches ssim_reduce_kernel between the two
// filter kernels (0) or has every backward workgroup re-sum the units' weight sums itself (1: a couple of thousand L2-resident floats at 1080p, the
// same weight_total, so the same bits). Measured by tools/ab_weighted_loss.py (profiles/weighted_loss_ab.json).
#ifndef FGS_LOSS_WEIGHTED_RESUM
#define FGS_LOSS_WEIGHTED_RESUM 1
#endif

// WEIGHTED: the maps arrive weighted, so the filter is the unweighted one; the gradient is SELECTED to 0.0f where the weight is not positive (there x'
// is the target, not the image: nothing of the image is read into the result) and the L1 sign carries the pixel's weight elsewhere. 3 S takes the place of
// 3 W H: from a.total_weight, or with n_reduce != 0 re-summed by this workgroup (FGS_LOSS_WEIGHTED_RESUM).
struct BwdRow { float d[3], h[3], p, q, w; };  // an input row of the three maps (own column, halo element) and the image, target and weight of the output row it completes
template <bool WEIGHTED>
__global__ void __launch_bounds__(256) ssim_backward_kernel(const LossArgs a, const GaussWindow gw, const unsigned n_reduce) {
    __shared__ float s_rows[kStripWaves][2][3][kRowPitch];
    const float n_total = backward_head<WEIGHTED>(a, n_reduce, &s_rows[0][0][0][0]);   // the only workgroup barriers of the kernel
    StripBand sb;
    if (!strip_band_of(StripGrid(a.width, a.height, kBwdBandH), a.height, sb)) return; // wave-uniform
    const int lane = static_cast<int>(lane_id()), gx = sb.x0 + lane, width = a.width, height = a.height;
    const HaloLane halo = halo_lane_of(lane, sb.x0, width);
    const bool own = gx < width;
    const size_t plane = (size_t)width * height;
    const float* __restrict__ D[3] = {a.d_mu + sb.c * plane, a.d_m11 + sb.c * plane, a.d_m12 + sb.c * plane};
    const float* __restrict__ X = a.image + sb.c * plane; const float* __restrict__ Y = a.target + sb.c * plane;
    float (*const rows)[3][kRowPitch] = s_rows[threadIdx.x >> 6];
    const int n_in = sb.y1 - sb.y0 + 2 * kHalo;
    // the upstream gradient dL/dloss (a device scalar: no host read) is folded into the two constants -- a framework-level
    // `grad * upstream` is one more pass over the 25 MB gradient image (11 us per iteration at 1080p)
    const float up = a.upstream != nullptr ? *a.upstream : 1.0f;
    const float ks = -a.lambda_dssim / n_total * up, kl = a.lambda_l1 / n_total * up;

    auto load_row = [&](const int iy) {
        BwdRow r{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f};
        if (iy >= 0 && iy < height && iy < sb.y1 + kHalo) {                            // wave-uniform; zero padding outside, nothing past the band's last input row
            const size_t at = (size_t)iy * width;
#pragma unroll
            for (int m = 0; m < 3; ++m) { if (own) r.d[m] = D[m][at + gx]; if (halo.active) r.h[m] = D[m][at + halo.gx]; }
        }
        const int oy = iy - kHalo;                                                     // the output row this input row completes
        if (own && oy >= sb.y0 && oy < sb.y1) {
            const size_t e = (size_t)oy * width + gx;
            r.p = X[e]; r.q = Y[e];
            if constexpr (WEIGHTED) r.w = a.weight[e];
        }
        return r;
    };
    BwdRow ahead[kPrefetch];
#pragma unroll
    for (int d = 0; d < kPrefetch; ++d) ahead[d] = load_row(sb.y0 - kHalo + d);

    float ring[3][kTaps];
    int k = 0;
    auto step = [&](auto phase) {
        constexpr int PH = decltype(phase)::value;
        const int iy = sb.y0 - kHalo + k, oy = iy - kHalo;
        const BwdRow cur = ahead[0];
#pragma unroll
        for (int d = 0; d + 1 < kPrefetch; ++d) ahead[d] = ahead[d + 1];
        ahead[kPrefetch - 1] = load_row(iy + kPrefetch);
        float (*const sd)[kRowPitch] = rows[k & 1];
#pragma unroll
        for (int m = 0; m < 3; ++m) { sd[m][lane + kHalo] = cur.d[m]; if (lane < 2 * kHalo) sd[m][halo.slot] = cur.h[m]; }
        wave_lds_fence();
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float f = 0.0f;
#pragma unroll
            for (int t = 0; t < kTaps; ++t) f = tap(gw.w[t], sd[m][lane + t], f);
            ring[m][PH] = f;
        }
        if (k >= kTaps - 1) {                                                          // wave-uniform
            float v[3];
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                float acc = 0.0f;
#pragma unroll
                for (int t = 0; t < kTaps; ++t) acc = tap(gw.w[t], ring[m][(PH + 1 + t) % kTaps], acc);
                v[m] = acc;
            }
            if (own) a.grad[sb.c * plane + (size_t)oy * width + gx] = loss_gradient<WEIGHTED>(ks, kl, v[0], v[1], v[2], cur.p, cur.q, cur.w);
        }
    };
    for (;;) { FGS_RING_STEPS(step) }
}

// In the dev library the scratch holds whichever forward formulation option 16 selects
size_t l1_dssim_partials(int width, int height) {
    size_t n = 2 * static_cast<size_t>(StripGrid(width, height, kBandH).units());
#ifdef FGS_DEV_SWITCHES
    n = std::max(n, loss_exhibit_partials(width, height));
#endif
    return n;
}
size_t l1_dssim_weight_partials(int width, int height) { return l1_dssim_partials(width, height) / 6; }

// option 16 (dev library): bit 0 the forward kernel, bit 1 the backward kernel of loss_exhibits.hip
static bool exhibit_selected([[maybe_unused]] const int bit) {
#ifdef FGS_DEV_SWITCHES
    return (g_loss_form & bit) != 0;
#else
    return false;
#endif
}

// Enqueues the forward kernel; returns the number of partial-sum pairs it leaves
template <bool WEIGHTED>
static unsigned launch_forward(const LossArgs& a, const GaussWindow& gw, hipStream_t s) {
#ifdef FGS_DEV_SWITCHES
    if (exhibit_selected(1)) { (void)launch_loss_forward_exhibit(a, gw, s); return static_cast<unsigned>(loss_exhibit_partials(a.width, a.height) / 2); }
#endif
    const StripGrid g(a.width, a.height, kBandH);
    hipLaunchKernelGGL(ssim_forward_kernel<WEIGHTED>, loss_grid(g.groups()), dim3(256), 0, s, a, gw);
    return g.units();
}

template <bool WEIGHTED>
static hipError_t launch_backward(const LossArgs& a, const GaussWindow& gw, const unsigned n_reduce, hipStream_t s) {
#ifdef FGS_DEV_SWITCHES
    if (exhibit_selected(2)) return launch_loss_backward_exhibit(a, gw, n_reduce, s);
#endif
    hipLaunchKernelGGL(ssim_backward_kernel<WEIGHTED>, loss_grid(StripGrid(a.width, a.height, kBwdBandH).groups()), dim3(256), 0, s, a, gw, n_reduce);
    return hipGetLastError();
}

template <bool WEIGHTED>
static hipError_t launch_loss(const LossArgs& a, hipStream_t s) {
    constexpr bool kSeparateReduce = WEIGHTED ? !FGS_LOSS_WEIGHTED_RESUM : FGS_LOSS_SEPARATE_REDUCE != 0;
    const GaussWindow gw = make_window();
    const unsigned n_partials = launch_forward<WEIGHTED>(a, gw, s);
    if (a.grad == nullptr || kSeparateReduce) {
        hipLaunchKernelGGL(ssim_reduce_kernel<WEIGHTED>, dim3(1), dim3(256), 0, s, a, n_partials);
        if (a.grad == nullptr) return hipGetLastError();
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_backward<WEIGHTED>(a, gw, kSeparateReduce ? 0u : n_partials, s);
}

// a.weight != nullptr: the weighted instantiations (a.wpartials and a.total_weight are then scratch too)
hipError_t launch_l1_dssim(const LossArgs& a, hipStream_t s) { return a.weight != nullptr ? launch_loss<true>(a, s) : launch_loss<false>(a, s); }
hipError_t launch_l1_dssim_backward(const LossArgs& a, hipStream_t s) {
    const GaussWindow gw = make_window();
    return a.weight != nullptr ? launch_backward<true>(a, gw, 0u, s) : launch_backward<false>(a, gw, 0u, s);
}

}  // namespace fgs

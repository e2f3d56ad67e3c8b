// The depth-distortion regulariser of the training render (blend_distortion.hip, api_distortion.hip): what the kernel unit and its host unit share.
// A header of its own, seen by those two units only: every other unit is built from the sources it had.
#pragma once
#include "fgs_kernels.h"

namespace fgs {

// X(p) = sum_a sum_b w_a w_b |t_a - t_b| over the pairs K10 blended in pixel p (fgs_blend_distortion), and its backward pass, which runs between K11
// and K12 (fgs_backward_distortion). Both walk the tile lists K10 built, bounded per pixel by n_processed.
struct DistortionArgs {
    const uint2* ranges; const uint32_t* inst_prims; const PrimRec* rec;
    const uint32_t* n_processed; const uint32_t* max_n_processed;          // tile-major [T][192], [T]: what K10 left
    const float* means; const float* w2c;  // z of a Gaussian = view_depth(mean): row 2 of w2c
    float* state;                         // forward: [3][H][W] = (X, sum w, sum w (t - t0 of the tile)), every element written
    const float* state_in;                // backward: the forward pass's state
    const float* grad;                    // backward: [H][W] upstream gradient of X
    float* acc;                           // backward: K11's accumulator records [N][9]; words 0..5 are added to
    float* acc_z;                         // backward: [N] dL/dz, zero or K11's at launch, added to with float atomics
    float depth_scale;                    // normalized mode: far near / (far - near), so that t - t0 = depth_scale (z - z0) / (z z0)
    uint32_t width, height, grid_w, grid_h, n_tiles;
    int normalized, proper_aa;
};
hipError_t launch_blend_distortion(const DistortionArgs& a, hipStream_t s);
hipError_t launch_blend_distortion_backward(const DistortionArgs& a, hipStream_t s);

}  // namespace fgs

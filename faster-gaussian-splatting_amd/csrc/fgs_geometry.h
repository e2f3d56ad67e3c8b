// The one render of the 2DGS regularisers (blend_geometry.hip, api_geometry.hip): what the kernel unit and its host unit share.
// A header of its own, seen by those two units only: every other unit is built from the sources it had.
#pragma once
#include "fgs_kernels.h"

namespace fgs {

constexpr unsigned kGeometryChannels = 5;      // the surface features: normal (3), depth, one
// The state the forward walk hands to the backward walk and to fgs_normal_consistency, fp32 [kGeometryPlanes][H][W], every element written:
//   plane 0      X, the depth-distortion map                                                    (public)
//   plane 1      D_n = sum w (t - t0 of the tile)                                               (private)
//   planes 2..6  M_c = sum w f_c, the surface map: a contiguous [5][H][W]                       (public)
//   plane 7      A_n = sum w, kept beside M_4 so that X does not depend on channel 4 holding ones (private)
constexpr unsigned kGeometryPlanes = 8;
constexpr unsigned kGeometryPlaneD = 1, kGeometryPlaneM = 2, kGeometryPlaneA = 7;

// X(p) = sum_a sum_b w_a w_b |t_a - t_b| and M_c(p) = sum_i w_i f_{i,c} over the pairs K10 blended in pixel p, in ONE walk of the tile lists K10 built
// (fgs_blend_geometry), and the backward pass of both, one walk between K11 and K12 (fgs_backward_geometry).
struct GeometryArgs {
    const uint2* ranges; const uint32_t* inst_prims; const PrimRec* rec;
    const uint32_t* n_processed; const uint32_t* max_n_processed;          // tile-major [T][192], [T]: what K10 left
    const float* means; const float* w2c;  // z of a Gaussian = view_depth(mean): row 2 of w2c
    const float* features;                // [N][5]
    float* state;                         // forward: [8][H][W], the layout above
    const float* state_in;                // backward: the forward pass's state
    const float* grad_x;                  // backward: [H][W] upstream gradient of X, or nullptr
    const float* grad_m;                  // backward: [5][H][W] upstream gradient of M, or nullptr
    float* acc;                           // backward: K11's accumulator records [N][9]; words 0..5 are added to
    float* acc_z;                         // backward: [N] dL/dz, zero or K11's at launch, added to with float atomics
    float* grad_features;                 // backward: [N][5], zero at launch, added to with float atomics
    float depth_scale;                    // normalized mode: far near / (far - near), so that t - t0 = depth_scale (z - z0) / (z z0)
    uint32_t width, height, grid_w, grid_h, n_tiles;
    int normalized, proper_aa;
};
hipError_t launch_blend_geometry(const GeometryArgs& a, hipStream_t s);
hipError_t launch_blend_geometry_backward(const GeometryArgs& a, hipStream_t s);

}  // namespace fgs

// K1's A/B exhibit: the reference's tile-counting scheme, option 5 of the dev library (g_seq_tiles; tools/ab_preprocess.py). Included by preprocess.hip
// alone. preprocess_body<INFERENCE, true> counts with it, and only libfgs_hip_dev.so instantiates that (preprocess.hip: the *_sequential_* kernels,
// launched when the switch is not 0); the product's kernels contain the flattened count and nothing of this file.
#pragma once
#include "fgs_kernels.h"

namespace fgs {

// The reference's scheme: every lane tests the first n candidates of its own Gaussian (cfg:54: 4), the wave cooperates on the rest (the loop of
// preprocess_body that both schemes share, which then starts at candidate n). At a mean footprint of 9 candidates a wave runs all n rounds with half
// of its lanes idle. Measured on S2, n = 4: 0.355 ms, 8: 0.300, 12: 0.252, 16: 0.248, 24: 0.256, 32: 0.269; the flattened count replaced it.
// Returns n: candidates below that index are counted here (cnt, and their bits of hit_mask), the others by the wave.
__device__ __forceinline__ unsigned count_tiles_sequential(const int seq_tiles, const bool active, const TileTest& tt, const unsigned tx0, const unsigned ty0,
                                                           const unsigned tbw, const unsigned n_max, unsigned& cnt, uint64_t& hit_mask) {
    const unsigned first_shared = static_cast<unsigned>(seq_tiles);
    if (active) {
        const unsigned n_seq = n_max < first_shared ? n_max : first_shared;
        for (unsigned t = 0; t < n_seq; ++t)
            if (tile_contributes(tt, tx0 + t % tbw, ty0 + t / tbw)) { ++cnt; hit_mask |= 1ull << t; }
    }
    return first_shared;
}

}  // namespace fgs

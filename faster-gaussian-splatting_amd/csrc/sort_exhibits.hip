// The depth sort's A/B exhibits. libfgs_hip_dev.so only (-DFGS_DEV_SWITCHES; the Makefile lists this unit in DEVOBJ and not in OBJ, with radix_sort.o's
// flags); the product library has one formulation of the depth sort, own_depth_sort of radix_sort.hip (mode 1 below), and none of this file.
//   option 9   g_depth_sort_mode -- bit 0: sort key - bits(near) in ceil(bits / 9) passes (near 0.2, far 1e4: 27 bits = 3 passes instead of 4);
//              bit 1: 2048-item workgroups (8 items per thread over 256 threads) where the sort carries no payload; 0 = round 1 (4 x 8 bits over all 32).
//   tools/ab_depth_sort.py, S2 (2 M keys), one process: mode 0 0.108 ms, 1 0.096, 2 0.119, 3 0.117
#ifdef FGS_DEV_SWITCHES   // the whole unit: compiled without the define (the product flavour of the simulation does, it takes every csrc/*.hip) it is empty
#include "fgs_radix_sort.h"

namespace fgs {
using namespace sortimpl;

constexpr int kDepthSortItems = 8;                    // bit 1: items per thread of the 2048-item shape (kSmallestSortBlock)

// false: the switch selects the product's formulation and nothing was enqueued; true: `result` is that of the mode's sort
bool depth_sort_exhibit(hipError_t& result, void* temp, size_t temp_bytes, uint32_t* keys[2], uint32_t* vals[2], int& selector, uint32_t n,
                        const uint32_t* n_ptr, DepthKeyRange range, hipStream_t s, const SortPayload* payload) {
    const int mode = g_depth_sort_mode;
    if (mode == 1) return false;
    const uint32_t base = (mode & 1) ? range.base : 0u;
    const int end_bit = (mode & 1) ? range.bits : 32, max_bits = (mode & 1) ? kMaxBits : kGenericMaxBits;
    if ((mode & 2) && payload == nullptr) result = sort_pairs<uint32_t, kDepthSortItems>(temp, temp_bytes, keys, vals, selector, n, n_ptr, base, end_bit, max_bits, s);
    else result = sort_pairs<uint32_t, kDepthSortIpt, kDepthSortThreads>(temp, temp_bytes, keys, vals, selector, n, n_ptr, base, end_bit, max_bits, s, payload);
    return true;
}

}  // namespace fgs
#endif  // FGS_DEV_SWITCHES

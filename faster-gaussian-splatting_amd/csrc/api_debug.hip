// The dev build's A/B switchboard (libfgs_hip_dev.so only: FGS_SWITCH, fgs_kernels.h) and the always-present hooks the tests reach the sorts and
// the wave collectives through.
#include "fgs_host.h"

using namespace fgs;
extern "C" {
#pragma GCC visibility push(default)
#ifdef FGS_DEV_SWITCHES      // the A/B switchboard exists in libfgs_hip_dev.so only (tools/, the variant tests); the product library has no process-wide knobs
int32_t fgs_debug_set_backward_variant(int32_t variant) {
    if (variant < 0 || variant > 5) return fail(FGS_ERR_INVALID_ARGUMENT, "variant must be 0 (systolic), 1 (strip), 2 (systolic, global dL/dC), 3 (live list + compacted pixels), 4 (lane = pixel, matrix-core reduction) or 5 (3 with the items of a wave chained through the lanes)");
    fgs::g_backward_variant = variant;
    return FGS_OK;
}

int32_t fgs_debug_set_option(int32_t key, int32_t value) {
    switch (key) {
        case 0: return fgs_debug_set_backward_variant(value);
        case 1: if (value != 1 && value != 2 && value != 4) return fail(FGS_ERR_INVALID_ARGUMENT, "adam unroll must be 1, 2 or 4");
                fgs::g_adam_unroll = value; return FGS_OK;
        case 2: fgs::g_adam_nontemporal = value ? 1 : 0; return FGS_OK;
        case 3: g_fused_single_kernel = value ? 1 : 0; return FGS_OK;
        case 7: fgs::g_backward_ablate = value & 15; return FGS_OK;
        case 13: if (value < 1) return fail(FGS_ERR_INVALID_ARGUMENT, "K11 variant 4 needs at least one workgroup"); fgs::g_k11m_max_blocks = value; return FGS_OK;
        case 8: fgs::g_adam_reverse = value ? 1 : 0; return FGS_OK;
        case 9: fgs::g_depth_sort_mode = value & 3; return FGS_OK;
        case 10: if (value < 0 || (value > 64 && (value < 251 || value > 255))) return fail(FGS_ERR_INVALID_ARGUMENT, "tile mapping must be 252 (one strip of tile columns per XCD, default), 254 (device-side block plan), 0 (bands), 255 (bands, bottom first) or 1..64 (row groups)");
                 fgs::g_tile_row_group = value; return FGS_OK;
        case 11: g_library_bucket_scan = value ? 1 : 0; return FGS_OK;
        case 12: fgs::g_plan_experiment = value & 3; return FGS_OK;
        case 14: if (value < 1) return fail(FGS_ERR_INVALID_ARGUMENT, "the chained K11 needs at least one wave"); fgs::g_k11_chain_waves = value; return FGS_OK;
        case 15: if (value < 1 || value > 32) return fail(FGS_ERR_INVALID_ARGUMENT, "the Adam span must be 1..32 chunks of 1024 floats");
                 fgs::g_adam_span = value; return FGS_OK;
        case 16: fgs::g_loss_form = value & 3; return FGS_OK;
        case 5: if (value < 0 || value > 32) return fail(FGS_ERR_INVALID_ARGUMENT, "seq_tiles must be 0 (flattened counting) or 1..32");
                g_seq_tiles = value; return FGS_OK;
        default: return fail(FGS_ERR_INVALID_ARGUMENT, "unknown option %d", key);
    }
}

#endif  // FGS_DEV_SWITCHES

size_t fgs_debug_radix_sort_temp_bytes(int32_t n, int32_t end_bit) {
    return n < 0 ? 0 : own_sort_temp_bytes(static_cast<uint32_t>(n), end_bit);
}

int32_t fgs_debug_radix_sort(void* keys0, void* keys1, uint32_t* vals0, uint32_t* vals1, int32_t n, int32_t key_bytes, int32_t end_bit,
                             void* temp, size_t temp_bytes, void* stream) {
    if (n < 0 || (key_bytes != 2 && key_bytes != 4) || end_bit < 1 || end_bit > 8 * key_bytes)
        return fail(FGS_ERR_INVALID_ARGUMENT, "bad sort arguments");
    if (n > 0 && (!keys0 || !keys1 || !vals0 || !vals1 || !temp)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL buffer");
    int selector = 0;
    uint32_t* vals[2] = {vals0, vals1};
    if (key_bytes == 2) {
        uint16_t* k[2] = {static_cast<uint16_t*>(keys0), static_cast<uint16_t*>(keys1)};
        FGS_HIP(own_sort_pairs_u16(temp, temp_bytes, k, vals, selector, static_cast<uint32_t>(n), end_bit, static_cast<hipStream_t>(stream)));
    } else {
        uint32_t* k[2] = {static_cast<uint32_t*>(keys0), static_cast<uint32_t*>(keys1)};
        FGS_HIP(own_sort_pairs_u32(temp, temp_bytes, k, vals, selector, static_cast<uint32_t>(n), end_bit, static_cast<hipStream_t>(stream)));
    }
    return selector;                     // 0 / 1: which buffer pair holds the sorted result
}

int32_t fgs_debug_depth_sort(uint32_t* keys0, uint32_t* keys1, uint32_t* vals0, uint32_t* vals1, int32_t n, float near_plane, float far_plane,
                             void* temp, size_t temp_bytes, void* stream) {
    if (n < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad sort arguments");
    if (n > 0 && (!keys0 || !keys1 || !vals0 || !vals1 || !temp)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL buffer");
    int selector = 0;
    uint32_t* k[2] = {keys0, keys1};
    uint32_t* vals[2] = {vals0, vals1};
    FGS_HIP(own_depth_sort(temp, temp_bytes, k, vals, selector, static_cast<uint32_t>(n), nullptr, depth_key_range(near_plane, far_plane),
                           static_cast<hipStream_t>(stream)));
    return selector;
}

int32_t fgs_debug_wave_selftest(uint32_t* out_device_256, void* stream) {
    if (!out_device_256) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL output");
    FGS_HIP(launch_wave_selftest(out_device_256, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}
#pragma GCC visibility pop
}  // extern "C"

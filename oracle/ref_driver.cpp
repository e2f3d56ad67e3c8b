// TEST INFRASTRUCTURE: C-ABI driver of the reference rasterizer built for the CPU (oracle/build_ref.py). It calls the reference's host functions
// the way its torch entry points route them (rasterization_api.cu / densification_api.cu: zero-filled gradient and helper tensors, byte blobs grown
// through resize callbacks, the three integers of the forward handed to the backward) and keeps the blobs, so that oracle/reference.py can decode
// every intermediate through the offsets the reference's own from_blob layouts give. Nothing here restates a kernel.
#include "forward.h"
#include "backward.h"
#include "inference.h"
#include "pruning_scores.h"
#include "mcmc.h"
#include "buffer_utils.h"

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <tuple>

namespace {

namespace fr = faster_gs::rasterization;

// A byte tensor of the torch glue: 256-byte aligned like a device allocation, so the layouts' 128-byte alignment starts at offset 0.
struct Blob {
    char* data = nullptr;
    size_t size = 0;
    char* resize(size_t n) {
        free(data);
        size = n;
        data = static_cast<char*>(aligned_alloc(256, ((n + 255) / 256 + 1) * 256));
        memset(data, 0xA5, ((n + 255) / 256 + 1) * 256);          // torch::empty: no promise about the contents; a recognisable pattern
        return data;
    }
    std::function<char*(size_t)> resizer() { return [this](size_t n) { return resize(n); }; }
};
Blob g_blobs[4];          // primitive, tile, instance, bucket -- of the latest forward / inference / pruning-scores call

}  // namespace

extern "C" {

const char* ref_blob(int which, size_t* size) { *size = g_blobs[which].size; return g_blobs[which].data; }

// Offsets of every field in the four blobs, from the reference's own layouts applied to a null base.
void ref_layout(int n_primitives, int n_tiles, int n_instances, int n_buckets, int end_bit, size_t* primitive, size_t* tile, size_t* instance, size_t* bucket) {
    auto off = [](const void* p) { return reinterpret_cast<size_t>(p); };
    char* base = nullptr;
    fr::PrimitiveBuffers p = fr::PrimitiveBuffers::from_blob(base, n_primitives);
    const size_t po[] = {off(p.depth_keys.d_buffers[0]), off(p.depth_keys.d_buffers[1]), off(p.primitive_indices.d_buffers[0]), off(p.primitive_indices.d_buffers[1]),
                         off(p.n_touched_tiles), off(p.offset), off(p.screen_bounds), off(p.mean2d), off(p.conic_opacity), off(p.color),
                         off(p.n_visible_primitives), off(p.n_instances), off(base)};
    memcpy(primitive, po, sizeof(po));
    base = nullptr;
    fr::TileBuffers t = fr::TileBuffers::from_blob(base, n_tiles);
    const size_t to[] = {off(t.instance_ranges), off(t.final_transmittances), off(t.n_buckets), off(t.buckets_offset), off(t.max_n_processed), off(t.n_processed), off(base)};
    memcpy(tile, to, sizeof(to));
    base = nullptr;
    if (end_bit <= 16) {
        auto i = fr::InstanceBuffers<ushort>::from_blob(base, n_instances, end_bit);
        const size_t io[] = {off(i.keys.d_buffers[0]), off(i.keys.d_buffers[1]), off(i.primitive_indices.d_buffers[0]), off(i.primitive_indices.d_buffers[1]), off(base)};
        memcpy(instance, io, sizeof(io));
    } else {
        auto i = fr::InstanceBuffers<uint>::from_blob(base, n_instances, end_bit);
        const size_t io[] = {off(i.keys.d_buffers[0]), off(i.keys.d_buffers[1]), off(i.primitive_indices.d_buffers[0]), off(i.primitive_indices.d_buffers[1]), off(base)};
        memcpy(instance, io, sizeof(io));
    }
    base = nullptr;
    fr::BucketBuffers b = fr::BucketBuffers::from_blob(base, n_buckets);
    const size_t bo[] = {off(b.tile_index), off(b.color_transmittance), off(base)};
    memcpy(bucket, bo, sizeof(bo));
}

int ref_extract_end_bit(unsigned n) { return fr::extract_end_bit(n); }

// rasterization_api.cu: forward_wrapper. out3 = (n_instances, n_buckets, instance_primitive_indices_selector).
void ref_forward(const float* means, const float* scales, const float* rotations, const float* opacities, const float* sh0, const float* sh_rest,
                 const float* w2c, const float* cam_position, const float* bg_color, float* image, int n_primitives, int active_sh_bases,
                 int total_sh_bases, int width, int height, float focal_x, float focal_y, float center_x, float center_y, float near_plane,
                 float far_plane, int proper_antialiasing, int* out3) {
    auto [n_instances, n_buckets, selector] = fr::forward(
        g_blobs[0].resizer(), g_blobs[1].resizer(), g_blobs[2].resizer(), g_blobs[3].resizer(),
        reinterpret_cast<const float3*>(means), reinterpret_cast<const float3*>(scales), reinterpret_cast<const float4*>(rotations), opacities,
        reinterpret_cast<const float3*>(sh0), reinterpret_cast<const float3*>(sh_rest), reinterpret_cast<const float4*>(w2c),
        reinterpret_cast<const float3*>(cam_position), reinterpret_cast<const float3*>(bg_color), image, n_primitives, active_sh_bases, total_sh_bases,
        width, height, focal_x, focal_y, center_x, center_y, near_plane, far_plane, proper_antialiasing != 0);
    out3[0] = n_instances; out3[1] = n_buckets; out3[2] = selector;
}

// rasterization_api.cu: backward_wrapper, on the blobs of the latest ref_forward. The caller passes zero-filled gradients and helpers (torch::zeros there);
// densification_info may be null (a tensor of size 0 there).
void ref_backward(const float* grad_image, const float* image, const float* means, const float* scales, const float* rotations, const float* opacities,
                  const float* sh_rest, const float* w2c, const float* cam_position, const float* bg_color, float* grad_means, float* grad_scales,
                  float* grad_rotations, float* grad_opacities, float* grad_sh0, float* grad_sh_rest, float* grad_mean2d_helper, float* grad_conic_helper,
                  float* densification_info, int n_primitives, int n_instances, int n_buckets, int selector, int active_sh_bases, int total_sh_bases,
                  int width, int height, float focal_x, float focal_y, float center_x, float center_y, int proper_antialiasing) {
    fr::backward(grad_image, image, reinterpret_cast<const float3*>(means), reinterpret_cast<const float3*>(scales), reinterpret_cast<const float4*>(rotations),
                 opacities, reinterpret_cast<const float3*>(sh_rest), reinterpret_cast<const float4*>(w2c), reinterpret_cast<const float3*>(cam_position),
                 reinterpret_cast<const float3*>(bg_color), g_blobs[0].data, g_blobs[1].data, g_blobs[2].data, g_blobs[3].data,
                 reinterpret_cast<float3*>(grad_means), reinterpret_cast<float3*>(grad_scales), reinterpret_cast<float4*>(grad_rotations), grad_opacities,
                 reinterpret_cast<float3*>(grad_sh0), reinterpret_cast<float3*>(grad_sh_rest), reinterpret_cast<float2*>(grad_mean2d_helper), grad_conic_helper,
                 densification_info, n_primitives, n_instances, n_buckets, selector, active_sh_bases, total_sh_bases, width, height, focal_x, focal_y,
                 center_x, center_y, proper_antialiasing != 0);
}

// rasterization_api.cu: inference_wrapper.
void ref_inference(const float* means, const float* scales, const float* rotations, const float* opacities, const float* sh0, const float* sh_rest,
                   const float* w2c, const float* cam_position, const float* bg_color, float* image, int n_primitives, int active_sh_bases,
                   int total_sh_bases, int width, int height, float focal_x, float focal_y, float center_x, float center_y, float near_plane,
                   float far_plane, int proper_antialiasing, int to_chw, int clamp_output) {
    fr::inference(g_blobs[0].resizer(), g_blobs[1].resizer(), g_blobs[2].resizer(),
                  reinterpret_cast<const float3*>(means), reinterpret_cast<const float3*>(scales), reinterpret_cast<const float4*>(rotations), opacities,
                  reinterpret_cast<const float3*>(sh0), reinterpret_cast<const float3*>(sh_rest), reinterpret_cast<const float4*>(w2c),
                  reinterpret_cast<const float3*>(cam_position), reinterpret_cast<const float3*>(bg_color), image, n_primitives, active_sh_bases,
                  total_sh_bases, width, height, focal_x, focal_y, center_x, center_y, near_plane, far_plane, proper_antialiasing != 0, to_chw != 0,
                  clamp_output != 0);
}

// rasterization_api.cu: pruning_scores_wrapper (accumulates into `scores`).
void ref_pruning_scores(float* scores, const float* means, const float* scales, const float* rotations, const float* opacities, const float* sh0,
                        const float* sh_rest, const float* w2c, const float* cam_position, const float* bg_color, int n_primitives, int active_sh_bases,
                        int total_sh_bases, int width, int height, float focal_x, float focal_y, float center_x, float center_y, float near_plane,
                        float far_plane, int proper_antialiasing) {
    fr::pruning_scores(g_blobs[0].resizer(), g_blobs[1].resizer(), g_blobs[2].resizer(),
                       reinterpret_cast<const float3*>(means), reinterpret_cast<const float3*>(scales), reinterpret_cast<const float4*>(rotations), opacities,
                       reinterpret_cast<const float3*>(sh0), reinterpret_cast<const float3*>(sh_rest), reinterpret_cast<const float4*>(w2c),
                       reinterpret_cast<const float3*>(cam_position), reinterpret_cast<const float3*>(bg_color), scores, n_primitives, active_sh_bases,
                       total_sh_bases, width, height, focal_x, focal_y, center_x, center_y, near_plane, far_plane, proper_antialiasing != 0);
}

// densification_api.cu: relocation_adjustment_wrapper / add_noise_wrapper.
void ref_relocation_adjustment(const float* old_opacities, const float* old_scales, const int64_t* n_samples, float* new_opacities, float* new_scales, int n) {
    faster_gs::densification::relocation_adjustment(old_opacities, reinterpret_cast<const float3*>(old_scales), n_samples, new_opacities,
                                                    reinterpret_cast<float3*>(new_scales), n);
}
void ref_add_noise(const float* raw_scales, const float* raw_rotations, const float* raw_opacities, const float* random_samples, float* means, int n, float current_lr) {
    faster_gs::densification::add_noise(reinterpret_cast<const float3*>(raw_scales), reinterpret_cast<const float4*>(raw_rotations), raw_opacities,
                                        reinterpret_cast<const float3*>(random_samples), reinterpret_cast<float3*>(means), n, current_lr);
}

}  // extern "C"

#ifdef REF_DRIVER_MAIN
// Stand-alone run of one scene (oracle/build_ref.py: build_sanitized_program builds this with -fsanitize=undefined; oracle/reference.py: dump_scene writes
// the input file): forward, backward with densification_info, pruning scores; prints a few sums. Sanitizers check it as an ordinary program.
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s scene.bin\n", argv[0]); return 2; }
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) { perror(argv[1]); return 2; }
    int hdr[6];                      // N, total_sh_bases, width, height, active_sh_bases, proper_antialiasing
    float cam[6];                    // focal_x, focal_y, center_x, center_y, near_plane, far_plane
    if (fread(hdr, sizeof(int), 6, fh) != 6 || fread(cam, sizeof(float), 6, fh) != 6) return 2;
    const int N = hdr[0], R = hdr[1], W = hdr[2], H = hdr[3];
    auto take = [&](size_t n) { std::vector<float> v(n); if (n && fread(v.data(), sizeof(float), n, fh) != n) { fprintf(stderr, "short file\n"); exit(2); } return v; };
    auto means = take(3 * N), scales = take(3 * N), rotations = take(4 * N), opacities = take(N), sh0 = take(3 * N), sh_rest = take(3 * (size_t)R * N);
    auto w2c = take(12), pos = take(3), bg = take(3), grad_image = take(3 * (size_t)W * H);
    fclose(fh);
    std::vector<float> image(3 * (size_t)W * H);
    int st[3];
    ref_forward(means.data(), scales.data(), rotations.data(), opacities.data(), sh0.data(), sh_rest.data(), w2c.data(), pos.data(), bg.data(), image.data(), N,
                hdr[4], R, W, H, cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], hdr[5], st);
    std::vector<float> gm(3 * N), gs(3 * N), gr(4 * N), go(N), g0(3 * N), grest(3 * (size_t)R * N), h2(2 * N), hc(3 * N), dens(2 * N), scores(N, 1.0f);
    ref_backward(grad_image.data(), image.data(), means.data(), scales.data(), rotations.data(), opacities.data(), sh_rest.data(), w2c.data(), pos.data(), bg.data(),
                 gm.data(), gs.data(), gr.data(), go.data(), g0.data(), grest.data(), h2.data(), hc.data(), dens.data(), N, st[0], st[1], st[2], hdr[4], R, W, H,
                 cam[0], cam[1], cam[2], cam[3], hdr[5]);
    ref_pruning_scores(scores.data(), means.data(), scales.data(), rotations.data(), opacities.data(), sh0.data(), sh_rest.data(), w2c.data(), pos.data(), bg.data(), N,
                       hdr[4], R, W, H, cam[0], cam[1], cam[2], cam[3], cam[4], cam[5], hdr[5]);
    auto sum = [](const std::vector<float>& v) { double s = 0; for (float x : v) s += x; return s; };
    printf("instances %d buckets %d selector %d | image %.9g | grad means %.9g scales %.9g opacities %.9g | visits %.9g | scores %.9g\n", st[0], st[1], st[2],
           sum(image), sum(gm), sum(gs), sum(go), sum(dens), sum(scores));
    return 0;
}
#endif

// C-ABI entry points of the Gaussian-sharded multi-GPU path (shard_exchange.hip; no reference counterpart, the reference is single-GPU):
// the owners' K1 over all views of a step, the renderer's forward and backward passes over received records, the owners' K12 / K13.
#include "fgs_host.h"

using namespace fgs;
namespace {
// records of the shards, concatenated -> ShardOrder (nullptr / fewer than two segments / more than kMaxBatchViews: the order as received)
int shard_order_of(ShardOrder& order, const int32_t* shard_counts, int32_t n_shards, int32_t n_records) {
    order = ShardOrder{};
    if (!shard_counts || n_shards <= 1) return FGS_OK;
    int64_t total = 0;
    for (int32_t k = 0; k < n_shards; ++k) {
        if (shard_counts[k] < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "shard_counts[%d] = %d", k, shard_counts[k]);
        total += shard_counts[k];
    }
    if (total != n_records) return fail(FGS_ERR_INVALID_ARGUMENT, "shard_counts sum to %lld, n_records = %d", static_cast<long long>(total), n_records);
    if (n_shards > kMaxBatchViews) return FGS_OK;
    order.n_shards = n_shards;
    for (int32_t k = 0; k < n_shards; ++k) order.count[k] = static_cast<uint32_t>(shard_counts[k]);
    return FGS_OK;
}

struct ShardBackward {                // one owner-side backward pass; adam != nullptr: the fused form (no gradient outputs)
    const float* acc_records; const int32_t* n_visible; const void* primitive_buffers;
    GaussianParams params;
    float* grad_means; float* grad_scales; float* grad_rotations; float* grad_opacities; float* grad_sh0; float* grad_sh_rest;
    float* densification_info; void* scratch; int32_t n_primitives, n_views; const fgs_settings* settings;
    const FusedAdam* adam; hipStream_t stream;
};

int run_shard_backward(const ShardBackward& rq) {
    const fgs_settings* settings = rq.settings;
    const int32_t n_primitives = rq.n_primitives, n_views = rq.n_views;
    const FusedAdam* adam = rq.adam;
    if (n_views < 1 || !settings || !rq.n_visible) return fail(FGS_ERR_INVALID_ARGUMENT, "n_views %d / settings / n_visible", n_views);
    int64_t total_visible = 0;
    for (int v = 0; v < n_views; ++v) {
        if (int rc = check_settings(settings + v)) return rc;
        if (rq.n_visible[v] < 0 || rq.n_visible[v] > n_primitives) return fail(FGS_ERR_INVALID_ARGUMENT, "view %d: n_visible %d of %d primitives", v, rq.n_visible[v], n_primitives);
        total_visible += rq.n_visible[v];
    }
    if (n_primitives < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "n_primitives %d", n_primitives);
    if (n_primitives == 0) return FGS_OK;
    if (!rq.primitive_buffers || !rq.scratch || (total_visible > 0 && !rq.acc_records)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL buffer");
    if (!rq.params.means || !rq.params.scales || !rq.params.rotations || !rq.params.opacities) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL parameter tensor");
    if (!adam && (!rq.grad_means || !rq.grad_scales || !rq.grad_rotations || !rq.grad_opacities || !rq.grad_sh0 ||
                  (settings->total_sh_bases_rest > 0 && !rq.grad_sh_rest)))
        return fail(FGS_ERR_INVALID_ARGUMENT, "NULL gradient tensor");
    if (adam && n_views > kMaxBatchViews) return fail(FGS_ERR_INVALID_ARGUMENT, "the fused form sums at most %d views in registers (got %d)", kMaxBatchViews, n_views);
    hipStream_t stream = rq.stream;
    const uint32_t n = static_cast<uint32_t>(n_primitives);
    const Geometry geo = geometry_of(settings->width, settings->height);
    const size_t per_view = primitive_view_bytes(n);
    const size_t dir_stride = ((size_t)n * 3 * sizeof(float) + 255) / 256 * 256;
    char* const dir_base = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(rq.scratch) + 255) & ~static_cast<uintptr_t>(255));
    size_t first_record = 0;
    for (int v0 = 0; v0 < n_views; v0 += kMaxBatchViews) {
        PreprocessBackwardArgs a{};
        ShRestArgs sh{};
        fill_backward_args(a, sh, rq.params, n, n_views - v0 < kMaxBatchViews ? n_views - v0 : kMaxBatchViews, *settings);
        a.grad_means = rq.grad_means; a.grad_scales = rq.grad_scales; a.grad_rotations = rq.grad_rotations; a.grad_opacities = rq.grad_opacities;
        a.grad_sh0 = rq.grad_sh0; a.densification_info = rq.densification_info; sh.grad_sh_rest = rq.grad_sh_rest;
        a.accumulate = sh.accumulate = v0 > 0 ? 1 : 0;    // gradients of a batch of views are summed in registers; later batches add
        for (int k = 0; k < a.n_views; ++k) {
            const int v = v0 + k;
            const PrimitiveBuffers b = primitive_view(rq.primitive_buffers, per_view, v, n);
            // accumulator records are read in place through the slot table K1 left behind: no scatter pass, no dense copy
            set_backward_view(a, sh, k, backward_view(settings[v], geo, b.n_touched, b.keys[1], rq.acc_records + first_record * kAccRecordWords,
                                                      reinterpret_cast<float*>(dir_base + dir_stride * v)));
            first_record += static_cast<size_t>(rq.n_visible[v]);
        }
        if (adam) fill_fused_adam(a, sh, *adam);
        // fused: the geometry kernel reads sh_rest (pre-update) and leaves the view directions, then the SH-rest pass updates it
        { StageScope t(ST_PREPROCESS_BACKWARD, stream); FGS_HIP(launch_preprocess_backward(adam != nullptr, a, stream)); }
        if (settings->total_sh_bases_rest > 0) { StageScope t(ST_SH_REST_BACKWARD, stream); FGS_HIP(launch_sh_rest_backward(adam != nullptr, sh, stream)); }
    }
    return FGS_OK;
}
}  // namespace

extern "C" {
#pragma GCC visibility push(default)
int32_t fgs_shard_preprocess(const float* means, const float* scales, const float* rotations, const float* opacities,
                             const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                             int32_t n_views, const fgs_settings* settings, void* records_out, uint32_t* counts_out,
                             fgs_resize_fn resize, void* resize_user, void* stream_) {
    if (n_views < 1 || !settings) return fail(FGS_ERR_INVALID_ARGUMENT, "n_views %d / settings", n_views);
    for (int v = 0; v < n_views; ++v) {
        if (int rc = check_settings(settings + v)) return rc;
        if (settings[v].width != settings[0].width || settings[v].height != settings[0].height || settings[v].total_sh_bases_rest != settings[0].total_sh_bases_rest)
            return fail(FGS_ERR_INVALID_ARGUMENT, "all views of a step must share the image size and SH layout");
    }
    if (n_primitives < 0 || !counts_out || !resize || (n_primitives > 0 && !records_out)) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument (n_primitives=%d)", n_primitives);
    const GaussianParams params{means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest};
    if (n_primitives > 0 && !params.complete(settings->total_sh_bases_rest)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL parameter tensor");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t n = static_cast<uint32_t>(n_primitives);
    const Geometry geo = geometry_of(settings->width, settings->height);
    const size_t per_view = primitive_view_bytes(n);
    void* prim_blob = resize(resize_user, FGS_BUF_PRIMITIVE, per_view * n_views);
    if (!prim_blob && per_view > 0) return fail(FGS_ERR_ALLOC, "resize(primitive, %zu) returned NULL", per_view * n_views);
    for (int v0 = 0; v0 < n_views; v0 += kMaxBatchViews) {
        PreprocessBatch pb{};
        PackRecordsBatch rb{};
        pb.n_views = rb.n_views = n_views - v0 < kMaxBatchViews ? n_views - v0 : kMaxBatchViews;
        rb.capacity = n;
        for (int k = 0; k < pb.n_views; ++k) {
            const int v = v0 + k;
            const PrimitiveBuffers b = primitive_view(prim_blob, per_view, v, n);
            FGS_HIP(hipMemsetAsync(b.counters, 0, kCounterWords * sizeof(uint32_t), stream));
            PreprocessArgs& pa = pb.v[k];
            params.write(pa);
            pa.rec = b.rec; pa.n_touched = b.n_touched; pa.depth_keys = b.keys[0]; pa.prim_idx = b.prims[0]; pa.counters = b.counters; pa.huge_list = b.offsets; pa.hot_list = b.hot_list; pa.foot = nullptr;
            pa.count_appended = 1;
            pa.n = n; pa.cam = camera_of(settings[v], geo); pa.ranges = nullptr; pa.n_tiles = 0;   // the tile ranges belong to the renderer of the view
            // slot table for fgs_shard_backward: the second depth-key buffer is free on this path (no sort on the owner)
            rb.v[k] = PackRecordsView{b.rec, b.n_touched, b.keys[0], b.prims[0], b.counters, b.keys[1],
                                      static_cast<uint32_t*>(records_out) + (size_t)v * n * kSplatRecordWords, counts_out + 2 * v};
        }
        if (n == 0) { FGS_HIP(hipMemsetAsync(counts_out + 2 * v0, 0, 2 * sizeof(uint32_t) * pb.n_views, stream)); continue; }
        { StageScope t(ST_PREPROCESS, stream); FGS_HIP(launch_preprocess_batch(pb, stream)); }
        { StageScope t(ST_RECORDS, stream); FGS_HIP(launch_pack_splat_records(rb, stream)); }
    }
    return FGS_OK;
}

int32_t fgs_forward_from_records(const void* records, int32_t n_records, int32_t n_instances, const fgs_settings* settings, float* image,
                                 fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream_) {
    return fgs_forward_from_shard_records(records, n_records, n_instances, nullptr, 0, settings, image, resize, resize_user, state_out, stream_);
}

int32_t fgs_forward_from_shard_records(const void* records, int32_t n_records, int32_t n_instances, const int32_t* shard_counts, int32_t n_shards,
                                       const fgs_settings* settings, float* image, fgs_resize_fn resize, void* resize_user,
                                       fgs_forward_state* state_out, void* stream_) {
    if (int rc = check_settings(settings)) return rc;
    ShardOrder order;
    if (int rc = shard_order_of(order, shard_counts, n_shards, n_records)) return rc;
    if (n_records < 0 || n_instances < 0 || !image || !resize || !state_out || (n_records > 0 && !records))
        return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument (n_records=%d, n_instances=%d)", n_records, n_instances);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const uint32_t n = static_cast<uint32_t>(n_records);
    const Geometry geo = geometry_of(settings->width, settings->height);
    TileBuffers tb;
    if (int rc = acquire(tb, resize, resize_user, FGS_BUF_TILE, geo.n_tiles, true)) return rc;
    PrimitiveBuffers pb;
    if (int rc = acquire(pb, resize, resize_user, FGS_BUF_PRIMITIVE, n, true)) return rc;
    FGS_HIP(hipMemsetAsync(pb.counters, 0, kCounterWords * sizeof(uint32_t), stream));
    { StageScope t(ST_RECORDS, stream);
      FGS_HIP(launch_unpack_splat_records(static_cast<const uint32_t*>(records), n, pb.rec, pb.n_touched, pb.keys[0], pb.prims[0], pb.foot[0], tb.ranges, geo.n_tiles, pb.hot_list, pb.counters + 4, order, stream)); }
    const ForwardRequest rq{MODE_TRAINING, {}, n_records, settings, image, 1, 0, resize, resize_user, state_out, stream, nullptr, 0};
    return forward_tail(rq, pb, tb, geo, {n, static_cast<uint32_t>(n_instances), -1, false});
}

int32_t fgs_backward_to_records(const float* grad_image, const float* image,
                                void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                void* scratch, float* acc_records_out, int32_t n_records,
                                const fgs_settings* settings, const fgs_forward_state* state, void* stream_) {
    return fgs_backward_to_shard_records(grad_image, image, primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, scratch, acc_records_out,
                                         n_records, nullptr, 0, settings, state, stream_);
}

int32_t fgs_backward_to_shard_records(const float* grad_image, const float* image,
                                      void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                      void* scratch, float* acc_records_out, int32_t n_records, const int32_t* shard_counts, int32_t n_shards,
                                      const fgs_settings* settings, const fgs_forward_state* state, void* stream_) {
    ShardOrder order;
    if (int rc = shard_order_of(order, shard_counts, n_shards, n_records)) return rc;
    BackwardPlan P;
    if (int rc = plan_backward(P, {primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, scratch}, n_records, settings, state)) return rc;
    if (!grad_image || !image) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL image / grad_image");
    if (n_records == 0) return FGS_OK;
    if (!acc_records_out) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL acc_records_out");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = run_blend_backward(P, grad_image, image, stream, false)) return rc;      // no K1 of this library wrote this blob
    { StageScope t(ST_RECORDS, stream); FGS_HIP(launch_pack_acc(P.pb.acc, static_cast<uint32_t>(n_records), acc_records_out, order, stream)); }
    return FGS_OK;
}

size_t fgs_shard_backward_scratch_bytes(int32_t n_primitives, int32_t n_views) {
    if (n_primitives < 0 || n_views < 1) return 0;
    return ((size_t)n_primitives * 3 * sizeof(float) + 255) / 256 * 256 * (size_t)n_views + 256;     // one view-direction array per view
}

int32_t fgs_shard_backward(const float* acc_records, const int32_t* n_visible, const void* primitive_buffers,
                           const float* means, const float* scales, const float* rotations, const float* opacities,
                           const float* sh_coefficients_rest,
                           float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                           float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                           float* densification_info, void* scratch, int32_t n_primitives, int32_t n_views,
                           const fgs_settings* settings, void* stream) {
    return run_shard_backward({acc_records, n_visible, primitive_buffers, {means, scales, rotations, opacities, nullptr, sh_coefficients_rest},
                               grad_means, grad_scales, grad_rotations, grad_opacities, grad_sh_coefficients_0, grad_sh_coefficients_rest,
                               densification_info, scratch, n_primitives, n_views, settings, nullptr, static_cast<hipStream_t>(stream)});
}

int32_t fgs_shard_backward_adam_fused(const float* acc_records, const int32_t* n_visible, const void* primitive_buffers,
                                      float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                                      float* densification_info, void* scratch, int32_t n_primitives, int32_t n_views,
                                      const fgs_settings* settings, int32_t step, const double* lrs, double beta1, double beta2, double eps,
                                      void* stream) {
    const FusedAdam adam{params, exp_avgs, exp_avg_sqs, step, lrs, beta1, beta2, eps};
    if (!adam.valid() || !settings) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    if (n_primitives > 0) { if (int rc = check_adam_groups(adam, settings->total_sh_bases_rest)) return rc; }
    return run_shard_backward({acc_records, n_visible, primitive_buffers, adam.gaussians(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               densification_info, scratch, n_primitives, n_views, settings, &adam, static_cast<hipStream_t>(stream)});
}
#pragma GCC visibility pop
}  // extern "C"

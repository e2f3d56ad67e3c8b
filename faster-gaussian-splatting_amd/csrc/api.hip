// C-ABI entry points of libfgs_hip.so (declared in include/fgs_hip.h) and the host-side orchestration of the pipeline. This unit: the library's
// state (error text, stage recorder) and the single-GPU passes. api_shard.hip: the Gaussian-sharded multi-GPU entry points; api_ops.hip: optimizer,
// loss, maintenance operators; api_debug.hip: the dev build's switchboard and the test hooks. What they share is in fgs_host.h.
// Replaces the reference's C++ wrappers + host code: rasterization_api.cu:13-247, rasterization/src/forward.cu:11-259,
// backward.cu:8-125, inference.cu:11-226, adam/src/adam.cu:36-71.
//
// Host-side differences that are deliberate (MI355X-first), not omissions:
//  * every launch goes to the caller's hipStream_t (the reference uses the legacy default stream + a static side stream);
//  * ONE device->host read per forward (n_visible, n_instances through pinned memory) instead of three blocking copies:
//    the bucket buffer is sized by the bound B <= I/64 + min(T, I) and kernels read the exact bucket count on the device;
//  * no zero-fill of the 59-float gradients (the backward kernels write every element), only the 9-float atomic
//    accumulators are cleared.
#include "fgs_host.h"
#include <cstdarg>
#include <cstdio>
#include <vector>

using namespace fgs;
namespace {
thread_local char g_error[512] = "";

const char* const kStageNames[ST_COUNT] = {"preprocess", "depth_sort", "offsets_scan", "create_instances", "tile_sort", "extract_ranges",
                                           "bucket_scan", "blend_forward", "stage_pixels", "blend_backward", "preprocess_backward",
                                           "sh_rest_backward", "adam", "l1_dssim_loss", "shard_records", "fused_backward_adam"};
struct StageRecord { int stage; hipEvent_t start, stop; };
struct Profiler {
    bool enabled = false;
    int only = -1;                     // >= 0: record this stage only (two events per launch of ONE stage perturb a timed loop far less than 30)
    std::vector<StageRecord> records;
    std::vector<hipEvent_t> pool;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
};
Profiler g_prof;

// The one D2H read of a forward pass goes through 16 bytes of pinned host memory and an event; both belong to the device that
// was current when they were created, so they are kept per (host thread, device) -- a thread driving two GPUs gets two sets.
constexpr int kMaxDevices = 64;
struct CounterReadback { uint32_t* host = nullptr; hipEvent_t ready = nullptr; };
CounterReadback* counter_readback() {
    thread_local CounterReadback slots[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
    CounterReadback& c = slots[dev];
    if (!c.host && hipHostMalloc(reinterpret_cast<void**>(&c.host), 16, hipHostMallocDefault) != hipSuccess) c.host = nullptr;
    if (!c.ready && hipEventCreateWithFlags(&c.ready, hipEventDisableTiming) != hipSuccess) c.ready = nullptr;
    return (c.host && c.ready) ? &c : nullptr;
}

// K2 over the primitive blob. count_ptr != nullptr: `count` is a bound and the sort reads the exact count there on the device
int enqueue_depth_sort(PrimitiveBuffers& pb, const fgs_settings* settings, int& depth_sel, uint32_t count, const uint32_t* count_ptr, hipStream_t stream) {
    StageScope t(ST_DEPTH_SORT, stream);
    FGS_HIP(run_depth_sort(pb.temp, pb.temp_bytes, pb.keys, pb.prims, depth_sel, count, count_ptr, depth_key_range(settings->near_plane, settings->far_plane),
                           pb.foot, pb.tile_counts, pb.big_list, pb.counters + 2, stream));
    return FGS_OK;
}
}  // namespace

namespace fgs {
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}

StageScope::StageScope(int stage, hipStream_t s) : stream(s) {
    if (!g_prof.enabled || (g_prof.only >= 0 && g_prof.only != stage)) return;
    StageRecord r{stage, g_prof.get(), g_prof.get()};
    if (!r.start || !r.stop) return;
    (void)hipEventRecord(r.start, stream);
    g_prof.records.push_back(r);
    idx = static_cast<int>(g_prof.records.size()) - 1;
}
StageScope::~StageScope() { if (idx >= 0) (void)hipEventRecord(g_prof.records[idx].stop, stream); }

// shared by fgs_forward (training), fgs_inference, fgs_inference_aux and fgs_pruning_scores
int run_forward(const ForwardRequest& rq) {
    const bool training = rq.mode == MODE_TRAINING;
    const fgs_settings* settings = rq.settings;
    if (int rc = check_settings(settings)) return rc;
    if (rq.n < 0 || (!rq.image && rq.mode != MODE_SCORES) || (!rq.scores && rq.mode == MODE_SCORES) || !rq.resize || !rq.state_out) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument (n_primitives=%d)", rq.n);
    if (rq.n > 0 && !rq.params.complete(settings->total_sh_bases_rest)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL parameter tensor");
    if (rq.aux && rq.mode == MODE_SCORES) return fail(FGS_ERR_INVALID_ARGUMENT, "auxiliary maps belong to the inference and training passes (mode %d)", static_cast<int>(rq.mode));
    if (rq.aux && training && (rq.instance_capacity > 0 || rq.aux_median))
        return fail(FGS_ERR_INVALID_ARGUMENT, "the training pass returns alpha and depth_expected through fgs_forward_aux only: no median depth, no asynchronous form");
    if (rq.aux && training && !rq.aux_alpha && !rq.aux_depth)
        return fail(FGS_ERR_INVALID_ARGUMENT, "alpha and depth_expected are both NULL: no auxiliary map requested (use fgs_forward)");
    if (rq.aux && !rq.aux_alpha && !rq.aux_depth && !rq.aux_median)
        return fail(FGS_ERR_INVALID_ARGUMENT, "alpha, depth_expected and depth_median are all NULL: no auxiliary map requested (use fgs_inference)");
    hipStream_t stream = rq.stream;
    const uint32_t n = static_cast<uint32_t>(rq.n);
    const Geometry geo = geometry_of(settings->width, settings->height);
    TileBuffers tb;                    // tile buffers + K0 (fwd:44-55)
    if (int rc = acquire(tb, rq.resize, rq.user, FGS_BUF_TILE, geo.n_tiles, training)) return rc;
    PrimitiveBuffers pb;               // primitive buffers + K1 (fwd:58-98)
    if (int rc = acquire(pb, rq.resize, rq.user, FGS_BUF_PRIMITIVE, n, training)) return rc;
    FGS_HIP(hipMemsetAsync(pb.counters, 0, kCounterWords * sizeof(uint32_t), stream));      // incl. counters[7]: "the accumulator records are dirty"
    PreprocessArgs pa{};
    pa.acc = pb.acc;                                   // training: K1 clears the accumulator record of every visible Gaussian
    rq.params.write(pa);
    pa.rec = pb.rec; pa.n_touched = pb.n_touched; pa.depth_keys = pb.keys[0]; pa.prim_idx = pb.prims[0]; pa.counters = pb.counters; pa.huge_list = pb.offsets;   // `offsets` is free until the K4 scan writes it
    pa.hot_list = pb.hot_list; pa.foot = pb.foot[0];
    pa.n = n; pa.cam = camera_of(*settings, geo); pa.ranges = tb.ranges; pa.n_tiles = geo.n_tiles;
    if (n == 0) FGS_HIP(hipMemsetAsync(tb.ranges, 0, sizeof(uint2) * geo.n_tiles, stream));   // no preprocess launch to clear them
    { StageScope t(ST_PREPROCESS, stream); FGS_HIP(launch_preprocess(!training, pa, stream)); }
    // Host-synchronisation-free form (fgs_forward_async): nothing is read back. Every launch behind K1 is sized by a bound -- the primitive
    // count for the visible list, the caller's capacity for the instance stages -- and reads the exact count on the device.
    // Synchronous form: the one host read of the pass, V and I (fwd:99-102). The depth sort does not need them on the host (radix_sort.hip
    // reads the count on the device), so it is enqueued BEHIND the copy and runs while the host waits for the two words.
    const bool async = rq.instance_capacity > 0;
    CounterReadback* rb = nullptr;
    if (!async) {
        rb = counter_readback();
        if (!rb) return fail(FGS_ERR_HIP, "pinned memory / event for the counter read-back unavailable on the current device");
        FGS_HIP(hipMemcpyAsync(rb->host, pb.counters, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        FGS_HIP(hipEventRecord(rb->ready, stream));
    }
    int depth_sel = async ? 0 : -1;                    // n == 0: no sort here; the synchronous form leaves it to forward_tail (a sort of nothing), the other does without
    if (n > 0) { if (int rc = enqueue_depth_sort(pb, settings, depth_sel, n, pb.counters, stream)) return rc; }
    if (async) return forward_tail(rq, pb, tb, geo, {n, static_cast<uint32_t>(rq.instance_capacity), depth_sel, true});
    FGS_HIP(hipEventSynchronize(rb->ready));
    return forward_tail(rq, pb, tb, geo, {rb->host[0], rb->host[1], depth_sel, false});
}

// K8+K9, and which tile -> workgroup mapping K10 runs with (ba.row_group, ba.tile_plan).
#ifndef FGS_DEV_SWITCHES
// The product: the training blend needs the per-tile bucket offsets for its checkpoints; always the columns mapping, which reads no plan.
static int bucket_scan_and_mapping(bool training, const TileBuffers& tb, const Geometry& geo, BlendArgs& ba, hipStream_t stream) {
    ba.row_group = kColumnsTopDown;
    if (!training) return FGS_OK;
    StageScope t(ST_BUCKET_SCAN, stream);
    FGS_HIP(launch_plan_tiles(tb.ranges, tb.bucket_offsets, nullptr, geo.n_tiles, geo.grid_w, geo.grid_h, stream));
    return FGS_OK;
}
#else
// The dev library: the mapping is a process-wide A/B switch another thread may flip, so it is read ONCE per pass and travels in BlendArgs -- planning
// and launch see the same value. The two mappings that read a device-side table get it from the scan's own kernel (binning_exhibits.hip), in inference
// passes too; the library scan (option 11) makes none, and they fall back to the bands.
static int bucket_scan_and_mapping(bool training, const TileBuffers& tb, const Geometry& geo, BlendArgs& ba, hipStream_t stream) {
    ba.row_group = static_cast<uint32_t>(static_cast<int>(g_tile_row_group));
    const bool need_plan = ba.row_group == kPlannedBlocks || ba.row_group == kBandsThroughPlan;
    if (!training && !need_plan) return FGS_OK;
    StageScope t(ST_BUCKET_SCAN, stream);
    if (g_library_bucket_scan && training) {
        FGS_HIP(run_bucket_scan(tb.temp, tb.temp_bytes, tb.ranges, tb.bucket_offsets, geo.n_tiles, stream));
        if (need_plan) ba.row_group = 0u;
        return FGS_OK;
    }
    uint32_t* const plan = need_plan ? tb.tile_plan : nullptr;
    FGS_HIP(launch_plan_tiles(tb.ranges, tb.bucket_offsets, plan, geo.n_tiles, geo.grid_w, geo.grid_h, stream));
    ba.tile_plan = plan;
    return FGS_OK;
}
#endif

// K2..K10 over a filled primitive buffer (rec, n_touched, depth keys + indices of the visible entries)
int forward_tail(const ForwardRequest& rq, PrimitiveBuffers& pb, const TileBuffers& tb, const Geometry& geo, ForwardCounts counts) {
    const bool training = rq.mode == MODE_TRAINING;
    const fgs_settings* settings = rq.settings;
    hipStream_t stream = rq.stream;
    const uint32_t n_visible = counts.n_visible, n_instances = counts.n_instances;
    // on_device: counters[0] = visible, counters[5] = min(instances, capacity) (written by K5), counters[6] = the capacity was exceeded
    const uint32_t* const visible_ptr = counts.on_device ? pb.counters : nullptr;
    const uint32_t* const instances_ptr = counts.on_device ? pb.counters + 5 : nullptr;
    // K2-K4 (fwd:104-127)
    if (counts.depth_sel < 0) { if (int rc = enqueue_depth_sort(pb, settings, counts.depth_sel, n_visible, visible_ptr, stream)) return rc; }
    { StageScope t(ST_OFFSETS_SCAN, stream); FGS_HIP(launch_tile_count_sums(pb.tile_counts, pb.wave_sums, pb.block_sums, n_visible, visible_ptr, stream)); }
    InstanceBuffers ib;                // K5-K7 (fwd:179-216)
    if (int rc = acquire(ib, rq.resize, rq.user, FGS_BUF_INSTANCE, n_instances, geo.key_bytes, geo.end_bit)) return rc;
    { StageScope t(ST_CREATE_INSTANCES, stream); FGS_HIP(launch_create_instances(geo.key_bytes, pb.foot[1], pb.wave_sums, pb.block_sums, pb.offsets, pb.rec, ib.keys[0], ib.prims[0], geo.grid_w, n_visible,
                                                                                 visible_ptr, counts.on_device ? n_instances : 0xffffffffu, pb.counters,
                                                                                 pb.big_list, pb.counters + 2, stream)); }
    int tile_sel = 0;
    { StageScope t(ST_TILE_SORT, stream); FGS_HIP(run_tile_sort(ib.temp, ib.temp_bytes, geo.key_bytes, ib.keys, ib.prims, tile_sel, n_instances, instances_ptr, geo.end_bit, stream)); }
    // the key double buffer flips together with the value double buffer
    { StageScope t(ST_RANGES, stream); FGS_HIP(launch_extract_ranges(geo.key_bytes, ib.keys[tile_sel], tb.ranges, n_instances, instances_ptr, stream)); }

    BlendArgs ba{};
    ba.ranges = tb.ranges; ba.inst_prims = ib.prims[tile_sel]; ba.rec = pb.rec; ba.bg = settings->bg_color; ba.image = rq.image;
    ba.width = settings->width; ba.height = settings->height; ba.grid_w = geo.grid_w; ba.grid_h = geo.grid_h; ba.n_tiles = geo.n_tiles;
    ba.to_chw = rq.to_chw; ba.clamp_output = rq.clamp_output;
    uint32_t n_buckets_cap = 0;
    if (int rc = bucket_scan_and_mapping(training, tb, geo, ba, stream)) return rc;           // K8+K9 (fwd:218-231)
    BucketBuffers bb{};
    if (training) {
        // the bucket buffer sized by its bound (no read-back of n_buckets, fwd:234)
        n_buckets_cap = bucket_capacity(n_instances, geo.n_tiles);
        if (int rc = acquire(bb, rq.resize, rq.user, FGS_BUF_BUCKET, n_buckets_cap, rq.aux)) return rc;
        ba.bucket_offsets = tb.bucket_offsets; ba.final_T = tb.final_T; ba.n_processed = tb.n_processed;
        ba.max_n_processed = tb.max_n_processed; ba.bucket_tile = bb.tile_index; ba.ckpt = bb.ckpt;
    }
    if (rq.mode == MODE_SCORES) { ba.scores = rq.scores; StageScope t(ST_BLEND_FORWARD, stream); FGS_HIP(launch_pruning_scores(ba, stream)); }
    else if (rq.aux && training) {                     // the training blend that also writes alpha / expected depth and the depth checkpoints
        ba.means = rq.params.means; ba.w2c = settings->w2c; ba.aux_alpha = rq.aux_alpha; ba.aux_depth = rq.aux_depth;
        StageScope t(ST_BLEND_FORWARD, stream); FGS_HIP(launch_blend_training_aux(BlendDepthArgs{ba, bb.ckpt_d}, stream));
        *rq.state_out = fgs_forward_state{static_cast<int32_t>(n_visible), static_cast<int32_t>(n_instances), static_cast<int32_t>(n_buckets_cap), tile_sel | kStateDepthCheckpoints};
        return FGS_OK;
    }
    else if (rq.aux) {                                 // the inference blend that also writes the requested maps; z from the means and w2c's depth row
        ba.means = rq.params.means; ba.w2c = settings->w2c;
        ba.aux_alpha = rq.aux_alpha; ba.aux_depth = rq.aux_depth; ba.aux_median = rq.aux_median;
        StageScope t(ST_BLEND_FORWARD, stream); FGS_HIP(launch_blend_aux(ba, stream));
    }
    else { StageScope t(ST_BLEND_FORWARD, stream); FGS_HIP(launch_blend(training, ba, stream)); }   // K10 (fwd:239)
    const int32_t origin = (counts.on_device ? kStateAsyncCounts : 0) | (training && rq.n > 0 && !rq.params.means ? kStateFromRecords : 0);
    *rq.state_out = fgs_forward_state{static_cast<int32_t>(n_visible), static_cast<int32_t>(n_instances), static_cast<int32_t>(n_buckets_cap), tile_sel | origin};
    return FGS_OK;
}

int plan_backward(BackwardPlan& P, const BackwardBlobs& blobs, int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, bool with_depth,
                  bool with_abs) {
    if (int rc = check_settings(settings)) return rc;
    if (!state || n_primitives < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad state / n_primitives");
    if (static_cast<uint64_t>(n_primitives) * kAccRecordWords + PrimitiveBuffers::kHotFloats > 0xfffffff0ull)      // K11 addresses the accumulator records by 32-bit float offsets
        return fail(FGS_ERR_INVALID_ARGUMENT, "n_primitives %d: more than 477 M Gaussians per backward pass are not supported", n_primitives);
    if (!blobs.primitive || !blobs.tile || !blobs.scratch || (state->n_instances > 0 && !blobs.instance) || (state->n_buckets > 0 && !blobs.bucket))
        return fail(FGS_ERR_INVALID_ARGUMENT, "NULL scratch buffer");
    P.n = n_primitives; P.settings = settings; P.state = state;
    P.geo = geometry_of(settings->width, settings->height);
    Carver pc(blobs.primitive), tc(blobs.tile), ic(blobs.instance), bc(blobs.bucket), sc(blobs.scratch);   // same carve order as the forward pass (bwd:46-52)
    P.pb = PrimitiveBuffers::carve(pc, static_cast<uint32_t>(n_primitives));
    P.tb = TileBuffers::carve(tc, P.geo.n_tiles, true);
    P.ib = InstanceBuffers::carve(ic, static_cast<uint32_t>(state->n_instances), P.geo.key_bytes, P.geo.end_bit);
    P.bb = BucketBuffers::carve(bc, static_cast<uint32_t>(state->n_buckets), (state->selector & kStateDepthCheckpoints) != 0);
    P.sc = BackwardScratch::carve(sc, static_cast<uint32_t>(n_primitives), P.geo.n_tiles, with_depth, with_abs);
    return FGS_OK;
}

static BlendBackwardArgs blend_backward_args(const BackwardPlan& P, const float* grad_image, const float* image, bool cleared_by_preprocess) {
    BlendBackwardArgs a{};
    // replaces api:127-134. K11 adds into 9-float records that must start at zero. The records of the visible Gaussians were cleared by K1 during the
    // forward pass (PrimitiveBuffers::acc); what is left for the staging kernel is the hot replicas (9 MB) -- or everything, when no K1 of this
    // library filled the blob (the sharded renderer: records arrive from the owners) or when these buffers already went through a backward pass
    // (a retained graph differentiated twice): counters[7], set by the last kernel of a backward pass, read on the device.
    static_assert(PrimitiveBuffers::kHotFloats % 4 == 0, "the cleared regions are whole numbers of 16-byte pieces");
    const size_t all_bytes = P.n > 0 ? static_cast<size_t>(reinterpret_cast<char*>(P.pb.acc_hot + PrimitiveBuffers::kHotFloats) - reinterpret_cast<char*>(P.pb.acc)) : 0;
    a.clear_all_f4 = static_cast<uint32_t>(all_bytes / 16);          // n <= 477 M (plan_backward): < 2^32 pieces
    a.clear_hot_f4 = P.n > 0 ? static_cast<uint32_t>(PrimitiveBuffers::kHotFloats / 4) : 0u;
    a.clear_everything = cleared_by_preprocess ? 0 : 1;
    a.dirty_flag = P.pb.counters + 7;
    a.ranges = P.tb.ranges; a.bucket_offsets = P.tb.bucket_offsets; a.inst_prims = P.ib.prims[P.state->selector & 1]; a.rec = P.pb.rec;
    a.bg = P.settings->bg_color; a.grad_image = grad_image; a.image = image;
    a.final_T = P.tb.final_T; a.n_processed = P.tb.n_processed; a.max_n_processed = P.tb.max_n_processed;
    a.bucket_tile = P.bb.tile_index; a.ckpt = P.bb.ckpt; a.pixrec = P.sc.pixrec; a.acc = P.pb.acc;
    a.work_list = P.bb.work_list; a.live_count = P.tb.live_count; a.live_offsets = P.tb.live_offsets;
    a.acc_hot = P.pb.acc_hot; a.hot_list = P.pb.hot_list; a.hot_count = P.pb.counters + 4;
    a.n = static_cast<uint32_t>(P.n); a.width = P.settings->width; a.height = P.settings->height;
    a.grid_w = P.geo.grid_w; a.n_tiles = P.geo.n_tiles; a.n_buckets_cap = static_cast<uint32_t>(P.state->n_buckets);
    a.proper_aa = P.settings->proper_antialiasing ? 1 : 0;
    a.variant = blend_backward_variant();           // once per pass: the planning pass and the kernel see the same formulation
    return a;
}

int run_blend_backward(const BackwardPlan& P, const float* grad_image, const float* image, hipStream_t stream, bool cleared_by_preprocess) {
    const BlendBackwardArgs a = blend_backward_args(P, grad_image, image, cleared_by_preprocess);
    { StageScope t(ST_STAGE_PIXELS, stream); FGS_HIP(launch_stage_pixels(a, stream)); }
    { StageScope t(ST_BLEND_BACKWARD, stream); FGS_HIP(launch_blend_backward(a, stream)); }     // K11 (bwd:56)
    return FGS_OK;
}

static BlendDepthPart blend_depth_part(const BackwardPlan& P, const float* grad_alpha, const float* grad_depth, const float* depth, const float* means) {
    BlendDepthPart d{};
    d.grad_alpha = grad_alpha; d.grad_depth = grad_depth; d.depth = depth;
    d.ckpt_d = grad_depth ? P.bb.ckpt_d : nullptr;
    d.pixaux = P.sc.pixaux; d.means = means; d.w2c = P.settings->w2c;
    d.acc_z = P.sc.acc_z; d.acc_z_hot = P.sc.acc_z_hot;
    d.clear_z_f4 = static_cast<uint32_t>(static_cast<size_t>(reinterpret_cast<char*>(P.sc.acc_z_hot + BackwardScratch::kHotDepthFloats) - reinterpret_cast<char*>(P.sc.acc_z)) / 16);
    return d;
}

int run_blend_backward_aux(const BackwardPlan& P, const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth,
                           const float* depth, const float* means, hipStream_t stream) {
    const BlendBackwardDepthArgs a{blend_backward_args(P, grad_image, image, true), blend_depth_part(P, grad_alpha, grad_depth, depth, means)};
    { StageScope t(ST_STAGE_PIXELS, stream); FGS_HIP(launch_stage_pixels_depth(a, stream)); }
    { StageScope t(ST_BLEND_BACKWARD, stream); FGS_HIP(launch_blend_backward_depth(a, stream)); }
    return FGS_OK;
}

int run_blend_backward_abs(const BackwardPlan& P, const float* grad_image, const float* image, bool with_maps, const float* grad_alpha, const float* grad_depth,
                           const float* depth, const float* means, hipStream_t stream) {
    static_assert(BackwardScratch::kHotAbsFloats % 4 == 0, "the cleared region is a whole number of 16-byte pieces");
    BlendAbsPart y{};
    y.acc_abs = P.sc.acc_abs; y.acc_abs_hot = P.sc.acc_abs_hot;      // 2 n + the replicas < 2^32 floats: n <= 477 M (plan_backward)
    y.clear_abs_f4 = static_cast<uint32_t>(static_cast<size_t>(reinterpret_cast<char*>(P.sc.acc_abs_hot + BackwardScratch::kHotAbsFloats) - reinterpret_cast<char*>(P.sc.acc_abs)) / 16);
    const BlendBackwardArgs blend = blend_backward_args(P, grad_image, image, true);
    if (with_maps) {
        const BlendBackwardDepthAbsArgs a{blend, blend_depth_part(P, grad_alpha, grad_depth, depth, means), y};
        { StageScope t(ST_STAGE_PIXELS, stream); FGS_HIP(launch_stage_pixels_depth_abs(a, stream)); }
        { StageScope t(ST_BLEND_BACKWARD, stream); FGS_HIP(launch_blend_backward_depth_abs(a, stream)); }
    } else {
        const BlendBackwardAbsArgs a{blend, y};
        { StageScope t(ST_STAGE_PIXELS, stream); FGS_HIP(launch_stage_pixels_abs(a, stream)); }
        { StageScope t(ST_BLEND_BACKWARD, stream); FGS_HIP(launch_blend_backward_abs(a, stream)); }
    }
    return FGS_OK;
}

// ---- the feature-channel render (blend_features.hip) ----
// What fgs_backward_features adds to a backward pass. n: the Gaussian count, for the clear of grad_features.
struct FeatureGradient { const float* features; int32_t n_channels; const float* feature_map; const float* grad_feature_map; float* grad_features;
                         int32_t detach_geometry; int32_t n; };

static int check_feature_channels(int32_t n_channels, const fgs_forward_state* state) {
    if (n_channels < 1 || n_channels > kMaxFeatureChannels)
        return fail(FGS_ERR_INVALID_ARGUMENT, "n_channels %d: the feature render takes 1..%d channels", n_channels, kMaxFeatureChannels);
    if (state->selector & kStateAsyncCounts)
        return fail(FGS_ERR_INVALID_ARGUMENT, "the feature render needs the buffers of a synchronous forward pass (fgs_forward / fgs_forward_aux), these are fgs_forward_async's");
    if (state->selector & kStateFromRecords)
        return fail(FGS_ERR_INVALID_ARGUMENT, "the feature render does not take the sharded / record paths: these buffers were filled from splat records");
    return FGS_OK;
}

static int check_feature_gradient(const FeatureGradient& f, const fgs_forward_state* state) {
    if (int rc = check_feature_channels(f.n_channels, state)) return rc;
    if (f.n > 0 && (!f.features || !f.feature_map || !f.grad_features)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL features / feature_map / grad_features");
    return FGS_OK;
}

static FeatureBlendArgs feature_blend_args(const PrimitiveBuffers& pb, const TileBuffers& tb, const InstanceBuffers& ib, const Geometry& geo,
                                           const fgs_settings& settings, const fgs_forward_state& state, const float* features, int32_t n_channels) {
    FeatureBlendArgs a{};
    a.ranges = tb.ranges; a.inst_prims = ib.prims[state.selector & 1]; a.rec = pb.rec;
    a.n_processed = tb.n_processed; a.max_n_processed = tb.max_n_processed;
    a.features = features; a.n_channels = static_cast<uint32_t>(n_channels);
    a.width = settings.width; a.height = settings.height; a.grid_w = geo.grid_w; a.grid_h = geo.grid_h; a.n_tiles = geo.n_tiles;
    a.proper_aa = settings.proper_antialiasing ? 1 : 0;
    return a;
}

static int run_blend_features_backward(const BackwardPlan& P, const FeatureGradient& f, hipStream_t stream) {
    FeatureBlendArgs a = feature_blend_args(P.pb, P.tb, P.ib, P.geo, *P.settings, *P.state, f.features, f.n_channels);
    a.feature_map_in = f.feature_map; a.grad_feature_map = f.grad_feature_map; a.grad_features = f.grad_features; a.acc = P.pb.acc;
    a.detach_geometry = f.detach_geometry ? 1 : 0;
    FGS_HIP(hipMemsetAsync(f.grad_features, 0, sizeof(float) * static_cast<size_t>(f.n) * f.n_channels, stream));
    StageScope t(ST_BLEND_BACKWARD, stream);
    FGS_HIP(launch_blend_features_backward(a, stream));
    return FGS_OK;
}
}  // namespace fgs

extern "C" {
#pragma GCC visibility push(default)
int32_t fgs_abi_version(void) { return FGS_ABI_VERSION; }
const char* fgs_last_error(void) { return g_error; }
#ifdef FGS_DEV_SWITCHES
const char* fgs_build_info(void) { return "libfgs_hip_dev gfx950 wave64 tile16x12 bucket64 radix-sort-v1 +dev-switches"; }
#else
const char* fgs_build_info(void) { return "libfgs_hip gfx950 wave64 tile16x12 bucket64 radix-sort-v1"; }
#endif

int32_t fgs_forward(const float* means, const float* scales, const float* rotations, const float* opacities,
                    const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                    const fgs_settings* settings, float* image, fgs_resize_fn resize, void* resize_user,
                    fgs_forward_state* state_out, void* stream) {
    return run_forward({MODE_TRAINING, {means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest}, n_primitives, settings,
                        image, 1, 0, resize, resize_user, state_out, static_cast<hipStream_t>(stream), nullptr, 0});
}

int32_t fgs_forward_aux(const float* means, const float* scales, const float* rotations, const float* opacities,
                        const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                        const fgs_settings* settings, float* image, float* alpha, float* depth_expected,
                        fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream) {
    ForwardRequest rq{MODE_TRAINING, {means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest}, n_primitives, settings,
                      image, 1, 0, resize, resize_user, state_out, static_cast<hipStream_t>(stream), nullptr, 0};
    rq.aux = true; rq.aux_alpha = alpha; rq.aux_depth = depth_expected;
    return run_forward(rq);
}

int32_t fgs_forward_async(const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                          const fgs_settings* settings, float* image, int32_t instance_capacity, fgs_resize_fn resize, void* resize_user,
                          fgs_forward_state* state_out, void* stream) {
    if (instance_capacity <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "instance_capacity %d", instance_capacity);
    return run_forward({MODE_TRAINING, {means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest}, n_primitives, settings,
                        image, 1, 0, resize, resize_user, state_out, static_cast<hipStream_t>(stream), nullptr, instance_capacity});
}

int32_t fgs_forward_counts(const void* primitive_buffers, int32_t n_primitives, int32_t* host_out, void* stream_) {
    if (!primitive_buffers || n_primitives < 0 || !host_out) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    Carver c(const_cast<void*>(primitive_buffers));
    const PrimitiveBuffers pb = PrimitiveBuffers::carve(c, static_cast<uint32_t>(n_primitives));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    // counters: [0] visible, [1] instances; [6] overflow flag of fgs_forward_async. Two small copies, no synchronisation here.
    FGS_HIP(hipMemcpyAsync(host_out, pb.counters, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    FGS_HIP(hipMemcpyAsync(host_out + 2, pb.counters + 6, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    return FGS_OK;
}

int32_t fgs_inference(const float* means, const float* scales, const float* rotations, const float* opacities,
                      const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                      const fgs_settings* settings, float* image, int32_t to_chw, int32_t clamp_output,
                      fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream) {
    return run_forward({MODE_INFERENCE, {means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest}, n_primitives, settings,
                        image, to_chw, clamp_output, resize, resize_user, state_out, static_cast<hipStream_t>(stream), nullptr, 0});
}

int32_t fgs_inference_aux(const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                          const fgs_settings* settings, float* image, int32_t to_chw, int32_t clamp_output,
                          float* alpha, float* depth_expected, float* depth_median,
                          fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream) {
    ForwardRequest rq{MODE_INFERENCE, {means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest}, n_primitives, settings,
                      image, to_chw, clamp_output, resize, resize_user, state_out, static_cast<hipStream_t>(stream), nullptr, 0};
    rq.aux = true; rq.aux_alpha = alpha; rq.aux_depth = depth_expected; rq.aux_median = depth_median;
    return run_forward(rq);
}

int32_t fgs_pruning_scores(float* scores, const float* means, const float* scales, const float* rotations, const float* opacities,
                           const float* sh_coefficients_0, const float* sh_coefficients_rest, int32_t n_primitives,
                           const fgs_settings* settings, fgs_resize_fn resize, void* resize_user, fgs_forward_state* state_out, void* stream) {
    return run_forward({MODE_SCORES, {means, scales, rotations, opacities, sh_coefficients_0, sh_coefficients_rest}, n_primitives, settings,
                        nullptr, 1, 0, resize, resize_user, state_out, static_cast<hipStream_t>(stream), scores, 0});
}

size_t fgs_backward_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height) {
    if (n_primitives < 0 || width <= 0 || height <= 0) return 0;
    Carver c(nullptr);
    BackwardScratch::carve(c, static_cast<uint32_t>(n_primitives), geometry_of(width, height).n_tiles);
    return c.total();
}

size_t fgs_backward_aux_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height) {
    if (n_primitives < 0 || width <= 0 || height <= 0) return 0;
    Carver c(nullptr);
    BackwardScratch::carve(c, static_cast<uint32_t>(n_primitives), geometry_of(width, height).n_tiles, true);
    return c.total();
}

size_t fgs_backward_absgrad_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height) {
    if (n_primitives < 0 || width <= 0 || height <= 0) return 0;
    Carver c(nullptr);
    BackwardScratch::carve(c, static_cast<uint32_t>(n_primitives), geometry_of(width, height).n_tiles, true, true);
    return c.total();
}

int32_t fgs_backward_live(const float* grad_image, const float* image,
                          const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_rest,
                          void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                          float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                          float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                          float* densification_info, void* scratch,
                          int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks, void* stream_) {
    return fgs_backward_aux(grad_image, image, nullptr, nullptr, nullptr, means, scales, rotations, opacities, sh_coefficients_rest, primitive_buffers,
                            tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities, grad_sh_coefficients_0,
                            grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks, stream_);
}

int32_t fgs_backward_aux(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                         const float* means, const float* scales, const float* rotations, const float* opacities,
                         const float* sh_coefficients_rest,
                         void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                         float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                         float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                         float* densification_info, void* scratch,
                         int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks, void* stream_) {
    return fgs_backward_reached(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                                primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                                grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                                nullptr, stream_);
}

// K11 and K12 of the single-GPU path. Without map gradients this IS fgs_backward_live: the plain staging pass and K11, the plain scratch layout.
// reached_blocks: K12's second flag per block of 64 ("K11 reached a Gaussian of it"); with a depth gradient the per-lane test includes dL/dz (acc_z), so a
// block flagged 0 stays zero through launch_depth_mean_gradient as well.
int32_t fgs_backward_reached(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                             const float* means, const float* scales, const float* rotations, const float* opacities,
                             const float* sh_coefficients_rest,
                             void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                             float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                             float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                             float* densification_info, void* scratch,
                             int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                             uint8_t* reached_blocks, void* stream_) {
    return fgs_backward_recycled(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                                 primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                                 grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                                 reached_blocks, nullptr, stream_);
}

// fgs_backward_reached for gradient tensors whose content the caller knows: prior_blocks[b] == 0 promises that block b of all six is zero NOW, and the
// one-kernel K12 leaves such a block alone if it reaches none of its Gaussians (backward_gradients_kernel). The promise holds through the depth term as
// well: launch_depth_mean_gradient adds to reached Gaussians only, and the reached test includes dL/dz.
int32_t fgs_backward_recycled(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                              const float* means, const float* scales, const float* rotations, const float* opacities,
                              const float* sh_coefficients_rest,
                              void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                              float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                              float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                              float* densification_info, void* scratch,
                              int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                              uint8_t* reached_blocks, const uint8_t* prior_blocks, void* stream_) {
    return fgs_backward_pose(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                             primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                             grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                             reached_blocks, prior_blocks, nullptr, nullptr, stream_);
}

size_t fgs_backward_pose_scratch_bytes(int32_t n_primitives, int32_t width, int32_t height) {
    if (n_primitives < 0 || width <= 0 || height <= 0) return 0;
    Carver c(nullptr);
    BackwardScratch::carve(c, static_cast<uint32_t>(n_primitives), geometry_of(width, height).n_tiles, true);
    PoseScratch::carve(c, static_cast<uint32_t>(n_primitives));
    return c.total();
}

// The materialised-gradient backward pass of the single-GPU path: staging + K11, the feature backward blend if `feat` brings an upstream gradient of a
// feature map, K12. Behind fgs_backward_pose (feat == nullptr) and fgs_backward_features.
static int backward_pass(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                         const float* means, const float* scales, const float* rotations, const float* opacities,
                         const float* sh_coefficients_rest,
                         void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                         float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                         float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                         float* densification_info, void* scratch,
                         int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                         uint8_t* reached_blocks, const uint8_t* prior_blocks, float* grad_w2c, float* grad_cam_position, const FeatureGradient* feat,
                         float* abs_densification_info, void* stream_) {
    const bool with_pose = grad_w2c != nullptr || grad_cam_position != nullptr;
    const bool with_abs = abs_densification_info != nullptr;
    if (prior_blocks != nullptr && reached_blocks == nullptr)
        return fail(FGS_ERR_INVALID_ARGUMENT, "prior_blocks without reached_blocks: the caller could not make the promise again for the next pass");
    if (prior_blocks != nullptr && (prior_blocks == reached_blocks || prior_blocks == live_blocks))
        return fail(FGS_ERR_INVALID_ARGUMENT, "prior_blocks aliases %s: the pass reads the one while it writes the other", prior_blocks == reached_blocks ? "reached_blocks" : "live_blocks");
    const bool with_maps = grad_alpha != nullptr || grad_depth != nullptr;
    BackwardPlan P;
    if (int rc = plan_backward(P, {primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, scratch}, n_primitives, settings, state, with_maps, with_abs)) return rc;
    if (!grad_image || !image) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL image / grad_image");
    if (with_abs) {
        if (state->selector & kStateAsyncCounts)
            return fail(FGS_ERR_INVALID_ARGUMENT, "abs_densification_info needs the buffers of a synchronous forward pass (fgs_forward / fgs_forward_aux), these are fgs_forward_async's");
        if (state->selector & kStateFromRecords)
            return fail(FGS_ERR_INVALID_ARGUMENT, "abs_densification_info does not take the sharded / record paths: these buffers were filled from splat records");
        const uintptr_t lo_a = reinterpret_cast<uintptr_t>(abs_densification_info), lo_d = reinterpret_cast<uintptr_t>(densification_info);
        const uintptr_t info_bytes = 2 * sizeof(float) * static_cast<uintptr_t>(n_primitives);
        if (densification_info != nullptr && (lo_a == lo_d || (lo_a < lo_d + info_bytes && lo_d < lo_a + info_bytes)))
            return fail(FGS_ERR_INVALID_ARGUMENT, "abs_densification_info aliases densification_info: the signed and the absolute statistic are two tensors");
    }
    if (grad_depth && !(state->selector & kStateDepthCheckpoints))
        return fail(FGS_ERR_INVALID_ARGUMENT, "grad_depth needs the depth checkpoints that fgs_forward_aux writes: these buffers were filled by a forward pass without them");
    if (grad_depth && !depth_expected) return fail(FGS_ERR_INVALID_ARGUMENT, "grad_depth without depth_expected (the map fgs_forward_aux returned)");
    if (feat) { if (int rc = check_feature_gradient(*feat, state)) return rc; }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n_primitives == 0) {               // no Gaussian, no term: the camera gradients are zero
        if (grad_w2c) FGS_HIP(hipMemsetAsync(grad_w2c, 0, 12 * sizeof(float), stream));
        if (grad_cam_position) FGS_HIP(hipMemsetAsync(grad_cam_position, 0, 3 * sizeof(float), stream));
        return FGS_OK;
    }
    if (!means || !scales || !rotations || !opacities || !grad_means || !grad_scales || !grad_rotations || !grad_opacities || !grad_sh_coefficients_0)
        return fail(FGS_ERR_INVALID_ARGUMENT, "NULL parameter / gradient tensor");
    if (with_pose && !g_fused_single_kernel) return fail(FGS_ERR_INVALID_ARGUMENT, "pose gradients are reduced by the one-kernel K12 only (dev option: the two-kernel form is selected)");
    if (with_abs) { if (int rc = run_blend_backward_abs(P, grad_image, image, with_maps, grad_alpha, grad_depth, depth_expected, means, stream)) return rc; }
    else if (with_maps) { if (int rc = run_blend_backward_aux(P, grad_image, image, grad_alpha, grad_depth, depth_expected, means, stream)) return rc; }
    else if (int rc = run_blend_backward(P, grad_image, image, stream)) return rc;
    // behind K11's last kernel (the hot replicas are folded, the records are marked dirty), in front of K12: the feature term adds into the same records
    if (feat) { if (int rc = run_blend_features_backward(P, *feat, stream)) return rc; }

    PreprocessBackwardArgs a{};
    ShRestArgs sh{};
    fill_backward_args(a, sh, {means, scales, rotations, opacities, nullptr, sh_coefficients_rest}, static_cast<uint32_t>(n_primitives), 1, *settings);
    set_backward_view(a, sh, 0, backward_view(*settings, P.geo, P.pb.n_touched, nullptr, P.pb.acc, P.sc.view_dir));
    if (grad_depth) a.view[0].acc_z = P.sc.acc_z;
    a.grad_means = grad_means; a.grad_scales = grad_scales; a.grad_rotations = grad_rotations; a.grad_opacities = grad_opacities;
    a.grad_sh0 = grad_sh_coefficients_0; a.densification_info = densification_info;
    if (settings->total_sh_bases_rest > 0 && !grad_sh_coefficients_rest) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL grad_sh_coefficients_rest");
    sh.grad_sh_rest = grad_sh_coefficients_rest;
    if (g_fused_single_kernel) {           // K12 (bwd:94) as one kernel
        StageScope t(ST_PREPROCESS_BACKWARD, stream);
        a.live_blocks = live_blocks;
        a.reached_blocks = reached_blocks;
        a.prior_blocks = prior_blocks;
        if (with_pose) {
            Carver sc(scratch);
            BackwardScratch::carve(sc, static_cast<uint32_t>(n_primitives), P.geo.n_tiles, true);
            const PoseScratch ps = PoseScratch::carve(sc, static_cast<uint32_t>(n_primitives));
            FGS_HIP(launch_backward_gradients_pose(a, sh, PosePart{ps.partials, ps.chunk_sums, grad_w2c, grad_cam_position}, stream));
        }
        else FGS_HIP(launch_backward_gradients(a, sh, stream));
    } else {                               // the two-kernel form writes every element and publishes all-ones flags: prior_blocks is not looked at
        if (live_blocks != nullptr) FGS_HIP(hipMemsetAsync(live_blocks, 1, (static_cast<size_t>(n_primitives) + 63) / 64, stream));   // A/B form: no flags, every block "live"
        if (reached_blocks != nullptr) FGS_HIP(hipMemsetAsync(reached_blocks, 1, (static_cast<size_t>(n_primitives) + 63) / 64, stream));   // ... and "reached"
        { StageScope t(ST_PREPROCESS_BACKWARD, stream); FGS_HIP(launch_preprocess_backward(false, a, stream)); }   // round-1 form: geometry kernel + SH-rest kernel
        if (settings->total_sh_bases_rest > 0) { StageScope t(ST_SH_REST_BACKWARD, stream); FGS_HIP(launch_sh_rest_backward(false, sh, stream)); }
    }
    // z_i's own dependence on mean_i: grad_means += dL/dz w2c[2, 0:3], after K12 has written every element. Not launched without a depth gradient.
    if (grad_depth) { StageScope t(ST_PREPROCESS_BACKWARD, stream); FGS_HIP(launch_depth_mean_gradient(P.sc.acc_z, P.pb.n_touched, settings->w2c, grad_means, static_cast<uint32_t>(n_primitives), stream)); }
    // the absolute-gradient statistic, from K11's two extra sums: never enters K12, so either form of it above serves
    if (with_abs) { StageScope t(ST_PREPROCESS_BACKWARD, stream); FGS_HIP(launch_abs_densification(P.sc.acc_abs, P.pb.n_touched, abs_densification_info, static_cast<uint32_t>(n_primitives),
                                                                                                    static_cast<float>(settings->width), static_cast<float>(settings->height), stream)); }
    return FGS_OK;
}

// fgs_backward_recycled that also accumulates the absolute-gradient densification statistic (AbsGS; include/fgs_hip.h): K11 with two more per-Gaussian sums,
// one small kernel behind K12. abs_densification_info == NULL is fgs_backward_recycled exactly: the same kernels, the plain or the aux scratch layout.
int32_t fgs_backward_absgrad(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                             const float* means, const float* scales, const float* rotations, const float* opacities,
                             const float* sh_coefficients_rest,
                             void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                             float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                             float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                             float* densification_info, void* scratch,
                             int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                             uint8_t* reached_blocks, const uint8_t* prior_blocks, float* abs_densification_info, void* stream_) {
    return backward_pass(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                         primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                         grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                         reached_blocks, prior_blocks, nullptr, nullptr, nullptr, abs_densification_info, stream_);
}

// fgs_backward_recycled that also reduces, inside K12, what the per-Gaussian chains say about the camera: dL/dw2c (rows 0..2) and dL/dcam_position.
// Both outputs NULL: the pass is fgs_backward_recycled's, kernel for kernel, on the plain (or aux) scratch layout. Otherwise the scratch has the aux
// layout -- whether or not map gradients arrive: the plain layout is its prefix -- with the pose partials behind it.
int32_t fgs_backward_pose(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                          const float* means, const float* scales, const float* rotations, const float* opacities,
                          const float* sh_coefficients_rest,
                          void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                          float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                          float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                          float* densification_info, void* scratch,
                          int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                          uint8_t* reached_blocks, const uint8_t* prior_blocks, float* grad_w2c, float* grad_cam_position, void* stream_) {
    return backward_pass(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                         primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                         grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                         reached_blocks, prior_blocks, grad_w2c, grad_cam_position, nullptr, nullptr, stream_);
}

// fgs_backward_reached with the upstream gradient of a feature map of fgs_blend_features: K11 as always, then the feature backward blend -- grad_features
// by atomics into memory zeroed here, its geometry term into words 0..5 of K11's accumulator records unless detach_geometry -- then K12, which turns the
// records into the six gradients unchanged. grad_feature_map == NULL is fgs_backward_reached exactly: the feature arguments are not looked at.
int32_t fgs_backward_features(const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth, const float* depth_expected,
                              const float* means, const float* scales, const float* rotations, const float* opacities,
                              const float* sh_coefficients_rest,
                              void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                              float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                              float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                              float* densification_info, void* scratch,
                              int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, uint8_t* live_blocks,
                              uint8_t* reached_blocks, const float* features, int32_t n_channels, const float* feature_map,
                              const float* grad_feature_map, float* grad_features, int32_t detach_geometry, void* stream_) {
    const FeatureGradient feat{features, n_channels, feature_map, grad_feature_map, grad_features, detach_geometry, n_primitives};
    return backward_pass(grad_image, image, grad_alpha, grad_depth, depth_expected, means, scales, rotations, opacities, sh_coefficients_rest,
                         primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities,
                         grad_sh_coefficients_0, grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, live_blocks,
                         reached_blocks, nullptr, nullptr, nullptr, grad_feature_map ? &feat : nullptr, nullptr, stream_);
}

// The F-channel blend over the buffers of a completed synchronous training forward pass (fgs_forward / fgs_forward_aux): feature_map [F,H,W].
int32_t fgs_blend_features(const float* features, int32_t n_channels, const void* primitive_buffers, const void* tile_buffers, const void* instance_buffers,
                           int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, float* feature_map, void* stream_) {
    if (int rc = check_settings(settings)) return rc;
    if (!state || n_primitives < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad state / n_primitives");
    if (int rc = check_feature_channels(n_channels, state)) return rc;
    if (!feature_map) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL feature_map");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const Geometry geo = geometry_of(settings->width, settings->height);
    if (n_primitives == 0) {               // nothing was blended: a zero map, nothing else is touched
        FGS_HIP(hipMemsetAsync(feature_map, 0, sizeof(float) * n_channels * static_cast<size_t>(settings->width) * settings->height, stream));
        return FGS_OK;
    }
    if (!features) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL features");
    if (!primitive_buffers || !tile_buffers || (state->n_instances > 0 && !instance_buffers)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL scratch buffer");
    Carver pc(const_cast<void*>(primitive_buffers)), tc(const_cast<void*>(tile_buffers)), ic(const_cast<void*>(instance_buffers));
    const PrimitiveBuffers pb = PrimitiveBuffers::carve(pc, static_cast<uint32_t>(n_primitives));
    const TileBuffers tb = TileBuffers::carve(tc, geo.n_tiles, true);
    const InstanceBuffers ib = InstanceBuffers::carve(ic, static_cast<uint32_t>(state->n_instances), geo.key_bytes, geo.end_bit);
    FeatureBlendArgs a = feature_blend_args(pb, tb, ib, geo, *settings, *state, features, n_channels);
    a.feature_map = feature_map;
    StageScope t(ST_BLEND_FORWARD, stream);
    FGS_HIP(launch_blend_features(a, stream));
    return FGS_OK;
}

int32_t fgs_backward(const float* grad_image, const float* image,
                     const float* means, const float* scales, const float* rotations, const float* opacities,
                     const float* sh_coefficients_rest,
                     void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                     float* grad_means, float* grad_scales, float* grad_rotations, float* grad_opacities,
                     float* grad_sh_coefficients_0, float* grad_sh_coefficients_rest,
                     float* densification_info, void* scratch,
                     int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, void* stream) {
    return fgs_backward_live(grad_image, image, means, scales, rotations, opacities, sh_coefficients_rest, primitive_buffers, tile_buffers,
                             instance_buffers, bucket_buffers, grad_means, grad_scales, grad_rotations, grad_opacities, grad_sh_coefficients_0,
                             grad_sh_coefficients_rest, densification_info, scratch, n_primitives, settings, state, nullptr, stream);
}

int32_t fgs_backward_adam_fused(const float* grad_image, const float* image,
                                float* const* params, float* const* exp_avgs, float* const* exp_avg_sqs,
                                void* primitive_buffers, void* tile_buffers, void* instance_buffers, void* bucket_buffers,
                                float* densification_info, void* scratch,
                                int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state,
                                int32_t step, const double* lrs, double beta1, double beta2, double eps, void* stream_) {
    BackwardPlan P;
    if (int rc = plan_backward(P, {primitive_buffers, tile_buffers, instance_buffers, bucket_buffers, scratch}, n_primitives, settings, state)) return rc;
    const FusedAdam adam{params, exp_avgs, exp_avg_sqs, step, lrs, beta1, beta2, eps};
    if (!grad_image || !image || !adam.valid()) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    if (n_primitives == 0) return FGS_OK;
    if (int rc = check_adam_groups(adam, settings->total_sh_bases_rest)) return rc;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (int rc = run_blend_backward(P, grad_image, image, stream)) return rc;

    PreprocessBackwardArgs a{};
    ShRestArgs sh{};
    fill_backward_args(a, sh, adam.gaussians(), static_cast<uint32_t>(n_primitives), 1, *settings);
    set_backward_view(a, sh, 0, backward_view(*settings, P.geo, P.pb.n_touched, nullptr, P.pb.acc, P.sc.view_dir));
    a.densification_info = densification_info;
    fill_fused_adam(a, sh, adam);
    if (g_fused_single_kernel) {
        // one kernel for all 59 floats: a wave gathers its Gaussians' sh_rest once, keeps the view direction in registers
        StageScope t(ST_FUSED_BACKWARD_ADAM, stream);
        FGS_HIP(launch_fused_backward_adam(a, sh, stream));
        return FGS_OK;
    }
    // Two-kernel form (round 1, kept for A/B): the geometry kernel reads sh_rest (pre-update) and leaves the view direction for
    // the SH-rest pass, which then updates sh_rest in place; means are updated by the geometry kernel after it has taken the direction.
    { StageScope t(ST_PREPROCESS_BACKWARD, stream); FGS_HIP(launch_preprocess_backward(true, a, stream)); }
    if (settings->total_sh_bases_rest > 0) { StageScope t(ST_SH_REST_BACKWARD, stream); FGS_HIP(launch_sh_rest_backward(true, sh, stream)); }
    return FGS_OK;
}

int32_t fgs_blob_layout(int32_t which, int32_t n_primitives, int32_t width, int32_t height, int32_t n_instances,
                        int32_t n_buckets, fgs_blob_entry* entries, int32_t max_entries) {
    if (width <= 0 || height <= 0 || n_primitives < 0 || n_instances < 0 || n_buckets < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad sizes");
    const Geometry geo = geometry_of(width, height);
    Carver c(nullptr, entries, max_entries);
    switch (which) {
        case FGS_BUF_PRIMITIVE: PrimitiveBuffers::carve(c, n_primitives); break;
        case FGS_BUF_TILE: TileBuffers::carve(c, geo.n_tiles, true); break;
        case FGS_BUF_INSTANCE: InstanceBuffers::carve(c, n_instances, geo.key_bytes, geo.end_bit); break;
        case FGS_BUF_BUCKET: BucketBuffers::carve(c, n_buckets); break;
        case FGS_BUF_COUNT: BackwardScratch::carve(c, n_primitives, geo.n_tiles); break;   // the backward scratch buffer
        default: return fail(FGS_ERR_INVALID_ARGUMENT, "unknown buffer %d", which);
    }
    return c.n < max_entries ? c.n : max_entries;
}

int32_t fgs_profile_enable(int32_t enable) {
    g_prof.enabled = enable != 0;
    g_prof.only = enable >= 2 ? enable - 2 : -1;          // 1: every stage; 2 + k: stage k only (index into fgs_profile_read's table)
    if (g_prof.only >= ST_COUNT) return fail(FGS_ERR_INVALID_ARGUMENT, "stage index %d", g_prof.only);
    return FGS_OK;
}

int32_t fgs_profile_read(fgs_stage_time* out, int32_t max_entries) {
    if (!out || max_entries < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad output array");
    double ms[ST_COUNT] = {0}; int64_t calls[ST_COUNT] = {0};
    for (StageRecord& r : g_prof.records) {
        float t = 0.0f;
        if (hipEventSynchronize(r.stop) == hipSuccess && hipEventElapsedTime(&t, r.start, r.stop) == hipSuccess) { ms[r.stage] += t; ++calls[r.stage]; }
        g_prof.pool.push_back(r.start); g_prof.pool.push_back(r.stop);
    }
    g_prof.records.clear();
    int n = 0;
    for (int k = 0; k < ST_COUNT && n < max_entries; ++k) { out[n].name = kStageNames[k]; out[n].total_ms = ms[k]; out[n].calls = calls[k]; ++n; }
    return n;
}
#pragma GCC visibility pop
}  // extern "C"

// What the host units of the C ABI share (api.hip, api_shard.hip, api_ops.hip, api_bilagrid.hip, api_normals.hip, api_tsdf.hip, api_debug.hip): the error channel, the stage timer, the blob
// carver with the five buffer layouts, and the argument builders. Internal: not installed, not seen by the kernel units.
// The error text and the stage recorder are the library's only state; both live in api.hip, behind fail() and StageScope.
#pragma once
#include <fgs_hip.h>
#include "fgs_kernels.h"

namespace fgs {
int fail(int code, const char* fmt, ...);
#define FGS_HIP(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(FGS_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// ---- optional per-stage timing with HIP events recorded on the caller's stream (fgs_profile_enable / fgs_profile_read) ----
enum Stage { ST_PREPROCESS, ST_DEPTH_SORT, ST_OFFSETS_SCAN, ST_CREATE_INSTANCES, ST_TILE_SORT, ST_RANGES, ST_BUCKET_SCAN,
             ST_BLEND_FORWARD, ST_STAGE_PIXELS, ST_BLEND_BACKWARD, ST_PREPROCESS_BACKWARD, ST_SH_REST_BACKWARD, ST_ADAM, ST_LOSS, ST_RECORDS, ST_FUSED_BACKWARD_ADAM, ST_COUNT };
struct StageScope { hipStream_t stream; int idx = -1; StageScope(int stage, hipStream_t s); ~StageScope(); };   // records start now and stop at scope exit, both on `stream`

struct Carver {                       // 256-byte aligned bump allocation inside a caller-owned byte buffer (cf. bu:30-36)
    char* base; size_t off = 0;
    fgs_blob_entry* entries; int max_entries; int n = 0;
    explicit Carver(void* b, fgs_blob_entry* e = nullptr, int m = 0) : base(static_cast<char*>(b)), entries(e), max_entries(m) {}
    template <typename T> T* take(const char* name, size_t count) {
        off = (off + 255) & ~static_cast<size_t>(255);
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        if (entries && n < max_entries) { entries[n].name = name; entries[n].offset = off; entries[n].bytes = count * sizeof(T); }
        ++n;
        off += count * sizeof(T);
        return p;
    }
    size_t total() const { return (off + 255) & ~static_cast<size_t>(255); }
};

constexpr size_t kCounterWords = 8;      // PreprocessArgs::counters
struct Geometry { uint32_t grid_w, grid_h, n_tiles; int end_bit, key_bytes; };
inline Geometry geometry_of(int width, int height) {
    Geometry g;
    g.grid_w = (width + kTileW - 1) / kTileW;
    g.grid_h = (height + kTileH - 1) / kTileH;
    g.n_tiles = g.grid_w * g.grid_h;
    g.end_bit = 0;                                        // bits of the largest tile index (fwd:42, bu:10-18); 1 for a single tile, as in the reference
    for (uint32_t m = g.n_tiles - 1; m != 0; m >>= 1) ++g.end_bit;
    if (g.end_bit == 0) g.end_bit = 1;
    g.key_bytes = g.end_bit <= 16 ? 2 : 4;                // fwd:152-153
    return g;
}

struct PrimitiveBuffers {             // cf. bu:45-94
    PrimRec* rec; uint32_t* n_touched; uint32_t* keys[2]; uint32_t* prims[2]; uint32_t* offsets; uint32_t* counters; uint32_t* hot_list;
    uint4* foot[2]; uint32_t* tile_counts;      // footprint rows in compaction / depth order, tile counts in depth order (fgs_math.h, radix_sort.hip)
    uint32_t* wave_sums; uint32_t* block_sums;  // their sums per 64-Gaussian wave segment / per 4096-Gaussian block (binning.hip)
    uint32_t* big_list;                         // depth-order positions of the footprints of more than kBigInstanceFootprint candidate tiles (counters[2] of them)
    char* temp; size_t temp_bytes;
    // K11's accumulator records [N][9] and the hot Gaussians' replicas behind them (K11 addresses both as 32-bit float offsets from `acc`). Round 6:
    // they live HERE, at the end of the forward pass's primitive blob, not in the backward scratch -- K1 clears the record of every Gaussian it
    // finds visible on the side of its own (latency-bound) work, so the backward pass starts without a 117 MB clear on its critical path. Passes
    // that are never differentiated (inference, pruning scores, the sharded owner's K1) carve the blob without them.
    float* acc; float* acc_hot;
    static constexpr size_t kHotFloats = (size_t)kHotReplicas * 9 * kMaxHot;
    static PrimitiveBuffers carve(Carver& c, uint32_t n, bool with_acc = true) {
        PrimitiveBuffers b;
        b.rec = c.take<PrimRec>("rec", n);
        b.n_touched = c.take<uint32_t>("n_touched", n);
        b.keys[0] = c.take<uint32_t>("depth_keys0", n); b.keys[1] = c.take<uint32_t>("depth_keys1", n);
        b.prims[0] = c.take<uint32_t>("prim_idx0", n); b.prims[1] = c.take<uint32_t>("prim_idx1", n);
        b.offsets = c.take<uint32_t>("offsets", n);
        b.counters = c.take<uint32_t>("counters", kCounterWords);
        b.hot_list = c.take<uint32_t>("hot_list", kMaxHot);
        b.foot[0] = c.take<uint4>("foot0", n); b.foot[1] = c.take<uint4>("foot1", n);
        b.tile_counts = c.take<uint32_t>("tile_counts", n);
        b.wave_sums = c.take<uint32_t>("wave_sums", (static_cast<size_t>(n) + 63) / 64 + 64);
        b.block_sums = c.take<uint32_t>("block_sums", (static_cast<size_t>(n) + 4095) / 4096 + 1);
        b.big_list = c.take<uint32_t>("big_list", n);
        b.temp_bytes = depth_sort_temp_bytes(n);
        b.temp = c.take<char>("sort_temp", b.temp_bytes);
        b.acc = with_acc ? c.take<float>("acc", (size_t)n * 9) : nullptr;
        b.acc_hot = with_acc ? c.take<float>("acc_hot", kHotFloats) : nullptr;
        return b;
    }
};
struct TileBuffers {                  // cf. bu:126-152; final_T / n_processed are tile-major here
    uint2* ranges; uint32_t* bucket_offsets; uint32_t* max_n_processed; float* final_T; uint32_t* n_processed;
    uint32_t* tile_plan;              // K10's tile -> workgroup plan (dev library: plan_tiles_kernel); carved in both flavours, the blob layout is one
    uint32_t* live_count;             // backward: number of live buckets (K11 planning pass)
    uint32_t* live_offsets;           // backward: first slot of each tile in the live-bucket list
    char* temp; size_t temp_bytes;
    static TileBuffers carve(Carver& c, uint32_t t, bool training) {
        TileBuffers b{};
        b.ranges = c.take<uint2>("ranges", t);
        b.bucket_offsets = c.take<uint32_t>("bucket_offsets", t);         // inference too: the dev library's block plan weighs its blocks by differences of this scan
        b.tile_plan = c.take<uint32_t>("tile_plan", kPlanWords);
        if (training) {
            b.max_n_processed = c.take<uint32_t>("max_n_processed", t);
            b.final_T = c.take<float>("final_T", (size_t)t * kTilePixels);
            b.n_processed = c.take<uint32_t>("n_processed", (size_t)t * kTilePixels);
#ifdef FGS_DEV_SWITCHES
            b.temp_bytes = bucket_scan_temp_bytes(t);      // the library scan, an A/B option of the dev build
#else
            b.temp_bytes = 0;
#endif
            b.temp = c.take<char>("scan_temp", b.temp_bytes);
            b.live_count = c.take<uint32_t>("live_count", 4);
            b.live_offsets = c.take<uint32_t>("live_offsets", t);
        }
        return b;
    }
};
struct InstanceBuffers {              // cf. bu:96-124
    void* keys[2]; uint32_t* prims[2]; char* temp; size_t temp_bytes;
    static InstanceBuffers carve(Carver& c, uint32_t n, int key_bytes, int end_bit) {
        InstanceBuffers b;
        b.keys[0] = c.take<char>("keys0", (size_t)n * key_bytes); b.keys[1] = c.take<char>("keys1", (size_t)n * key_bytes);
        b.prims[0] = c.take<uint32_t>("prims0", n); b.prims[1] = c.take<uint32_t>("prims1", n);
        b.temp_bytes = tile_sort_temp_bytes(n, key_bytes, end_bit);
        b.temp = c.take<char>("sort_temp", b.temp_bytes);
        return b;
    }
};
struct BucketBuffers {                // cf. bu:154-163
    uint32_t* tile_index; float4* ckpt; uint2* work_list;
    float* ckpt_d;                    // fgs_forward_aux only: the running depth sum beside every checkpoint, [B][192]. At the TAIL: the plain layout is a prefix,
                                      // so buffers filled by fgs_forward_aux are valid input to every plain backward pass
    static BucketBuffers carve(Carver& c, uint32_t n, bool with_depth = false) {
        BucketBuffers b;
        b.tile_index = c.take<uint32_t>("tile_index", n);
        b.ckpt = c.take<float4>("ckpt", (size_t)n * kTilePixels);
        b.work_list = c.take<uint2>("work_list", n);        // backward: the live (tile, bucket) pairs
        b.ckpt_d = with_depth ? c.take<float>("ckpt_d", (size_t)n * kTilePixels) : nullptr;
        return b;
    }
};
struct BackwardScratch {
    float* view_dir; float4* pixrec;
    // fgs_backward_aux only (behind the plain layout): staged (gD, gA, D_final, T_final) per pixel, dL/dz per Gaussian and the hot Gaussians' replicas of it
    float4* pixaux; float* acc_z; float* acc_z_hot;
    // fgs_backward_absgrad only (behind the aux layout, whether or not map gradients arrive: both smaller layouts stay prefixes): the absolute sums
    // (ax, ay) per Gaussian, interleaved, and the hot Gaussians' replicas of them
    float* acc_abs; float* acc_abs_hot;
    static constexpr size_t kHotDepthFloats = (size_t)kHotReplicas * kMaxHot;
    static constexpr size_t kHotAbsFloats = (size_t)kHotReplicas * kMaxHot * 2;
    static BackwardScratch carve(Carver& c, uint32_t n, uint32_t t, bool with_depth = false, bool with_abs = false) {
        BackwardScratch b{};
        b.view_dir = c.take<float>("view_dir", (size_t)n * 3);
        b.pixrec = c.take<float4>("pixrec", (size_t)t * kTilePixels * 2);
        if (with_depth || with_abs) {
            b.pixaux = c.take<float4>("pixaux", (size_t)t * kTilePixels);
            b.acc_z = c.take<float>("acc_z", ((size_t)n + 3) / 4 * 4);
            b.acc_z_hot = c.take<float>("acc_z_hot", kHotDepthFloats);
        }
        if (with_abs) {
            b.acc_abs = c.take<float>("acc_abs", ((size_t)n * 2 + 3) / 4 * 4);
            b.acc_abs_hot = c.take<float>("acc_abs_hot", kHotAbsFloats);
        }
        return b;
    }
};
// fgs_backward_pose only, behind the aux layout of BackwardScratch (fgs_backward_pose_scratch_bytes): one 64-byte line of partial sums per wave of
// K12 and the fp64 sums of the reduction's first stage (PosePart). Every element that is read is written by the pass itself.
struct PoseScratch {
    float* partials; double* chunk_sums;
    static PoseScratch carve(Carver& c, uint32_t n) {
        PoseScratch b;
        b.partials = c.take<float>("pose_partials", ((size_t)n + 63) / 64 * kPoseLineFloats);
        b.chunk_sums = c.take<double>("pose_chunk_sums", (size_t)kPoseMaxChunks * kPoseLineFloats);
        return b;
    }
};
// fgs_forward_state::selector, bit 1: the bucket buffer carries ckpt_d (fgs_forward_aux filled it). Bit 0 is the half of the instance double buffer.
constexpr int32_t kStateDepthCheckpoints = 2;
// bit 2: the counts of the state are bounds (fgs_forward_async); bit 3: the primitive blob was filled from splat records, not by K1 over the caller's
// Gaussians (fgs_forward_from_records / _shard_records). Read by the feature render, which takes neither.
constexpr int32_t kStateAsyncCounts = 4, kStateFromRecords = 8;

// One blob from the caller's allocator: size it for B::carve(args...), ask `resize` for buffer `which`, carve it into `out`.
template <class B, class... A>
int acquire(B& out, fgs_resize_fn resize, void* user, int which, A... args) {
    static const char* const kBlobNames[] = {"primitive", "tile", "instance", "bucket"};      // indexed by FGS_BUF_*
    static_assert(sizeof(kBlobNames) / sizeof(kBlobNames[0]) == FGS_BUF_COUNT, "one name per FGS_BUF_* blob");
    if (which < 0 || which >= FGS_BUF_COUNT) return fail(FGS_ERR_INVALID_ARGUMENT, "unknown buffer %d", which);
    Carver size(nullptr);
    B::carve(size, args...);
    void* blob = resize(user, which, size.total());
    if (!blob && size.total() > 0) return fail(FGS_ERR_ALLOC, "resize(%s, %zu) returned NULL", kBlobNames[which], size.total());
    Carver c(blob);
    out = B::carve(c, args...);
    return FGS_OK;
}
// Sharded owner: one primitive blob holds the buffers of every view of the step back to back, each carved without accumulator records
inline size_t primitive_view_bytes(uint32_t n) { Carver c(nullptr); PrimitiveBuffers::carve(c, n, false); return c.total(); }
inline PrimitiveBuffers primitive_view(const void* blob, size_t per_view, int v, uint32_t n) {
    Carver c(const_cast<char*>(static_cast<const char*>(blob)) + per_view * v);
    return PrimitiveBuffers::carve(c, n, false);
}
inline uint32_t bucket_capacity(uint32_t n_instances, uint32_t n_tiles) {   // sum_t ceil(len_t/64) <= I/64 + #non-empty tiles
    return n_instances / kBucket + (n_instances < n_tiles ? n_instances : n_tiles);
}
inline CameraArgs camera_of(const fgs_settings& s, const Geometry& g) {
    CameraArgs c;
    c.w2c = s.w2c; c.cam_pos = s.cam_position;
    c.width = static_cast<float>(s.width); c.height = static_cast<float>(s.height);   // fwd:82-83
    c.fx = s.focal_x; c.fy = s.focal_y; c.cx = s.center_x; c.cy = s.center_y;
    c.near_plane = s.near_plane; c.far_plane = s.far_plane; c.proper_aa = s.proper_antialiasing ? 1 : 0;
    c.active_sh_bases = s.active_sh_bases; c.total_sh_rest = s.total_sh_bases_rest;
    c.grid_w = g.grid_w; c.grid_h = g.grid_h;
    return c;
}
inline BackwardView backward_view(const fgs_settings& s, const Geometry& g, const uint32_t* n_touched, const uint32_t* slot, const float* acc, float* view_dir) {
    return BackwardView{camera_of(s, g), n_touched, acc, slot, view_dir, nullptr};
}
inline int check_settings(const fgs_settings* s) {
    if (!s) return fail(FGS_ERR_INVALID_ARGUMENT, "settings is NULL");
    if (!s->w2c || !s->cam_position || !s->bg_color) return fail(FGS_ERR_INVALID_ARGUMENT, "w2c / cam_position / bg_color must be device pointers");
    if (s->width <= 0 || s->height <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "image size %dx%d", s->width, s->height);
    if (s->active_sh_bases < 1 || s->active_sh_bases > 16) return fail(FGS_ERR_INVALID_ARGUMENT, "active_sh_bases %d", s->active_sh_bases);
    if (s->total_sh_bases_rest > 15) return fail(FGS_ERR_INVALID_ARGUMENT, "sh_coefficients_rest has %d bases (SH degree 3 = 15 is the maximum)", s->total_sh_bases_rest);
    if (s->total_sh_bases_rest < 0 || (s->active_sh_bases > 1 && s->total_sh_bases_rest < s->active_sh_bases - 1))
        return fail(FGS_ERR_INVALID_ARGUMENT, "sh_coefficients_rest has %d bases, active_sh_bases %d", s->total_sh_bases_rest, s->active_sh_bases);
    return FGS_OK;
}
inline AdamHyper adam_hyper(int step, double lr, double beta1, double beta2, double eps) {   // adam.cu:52-54
    const double bc1_rcp = 1.0 / (1.0 - std::pow(beta1, step));
    const double bc2_sqrt_rcp = 1.0 / std::sqrt(1.0 - std::pow(beta2, step));
    AdamHyper h;
    h.step_size = static_cast<float>(lr * bc1_rcp);
    h.beta1 = static_cast<float>(beta1); h.beta2 = static_cast<float>(beta2); h.eps = static_cast<float>(eps);
    h.bc2_sqrt_rcp = static_cast<float>(bc2_sqrt_rcp);
    return h;
}

// The six parameter tensors of a Gaussian set (the backward passes do not read sh0)
struct GaussianParams {
    const float* means; const float* scales; const float* rotations; const float* opacities; const float* sh0; const float* sh_rest;
    bool complete(int total_sh_rest) const { return means && scales && rotations && opacities && sh0 && (total_sh_rest <= 0 || sh_rest); }
    void write(PreprocessArgs& pa) const { pa.means = means; pa.scales = scales; pa.rotations = rotations; pa.opacities = opacities; pa.sh0 = sh0; pa.sh_rest = sh_rest; }
};

// What every K12 / K13 launch shares: the parameters, the Gaussian count, the number of views and the SH layout. The callers add what differs:
// the views themselves (set_backward_view), gradient outputs or optimizer state, live_blocks, accumulation.
inline void fill_backward_args(PreprocessBackwardArgs& a, ShRestArgs& sh, const GaussianParams& p, uint32_t n, int n_views, const fgs_settings& s) {
    a.means = p.means; a.scales = p.scales; a.rotations = p.rotations; a.opacities = p.opacities; a.sh_rest = p.sh_rest;
    a.n = sh.n = n; a.n_views = sh.n_views = n_views;
    sh.total_sh_rest = s.total_sh_bases_rest; sh.active_sh_bases = s.active_sh_bases;
}
inline void set_backward_view(PreprocessBackwardArgs& a, ShRestArgs& sh, int k, const BackwardView& view) {
    a.view[k] = view; sh.view[k] = ShRestView{view.view_dir, view.n_touched, view.acc, view.slot};
}

// The optimizer state of the fused backward + Adam forms. API group order (Model.py:238-245): 0 means, 1 sh0, 2 sh_rest, 3 opacities, 4 scales, 5 rotations
struct FusedAdam {
    float* const* params; float* const* exp_avgs; float* const* exp_avg_sqs; int step; const double* lrs; double beta1, beta2, eps;
    bool valid() const { return params && exp_avgs && exp_avg_sqs && lrs && step >= 1; }
    GaussianParams gaussians() const { return {params[0], params[4], params[5], params[3], params[1], params[2]}; }
};
inline int check_adam_groups(const FusedAdam& o, int total_sh_rest) {
    for (int k = 0; k < 6; ++k)
        if (!o.params[k] || !o.exp_avgs[k] || !o.exp_avg_sqs[k]) {
            if (k == 2 && total_sh_rest == 0) continue;
            return fail(FGS_ERR_INVALID_ARGUMENT, "NULL tensor in group %d", k);
        }
    return FGS_OK;
}
inline void fill_fused_adam(PreprocessBackwardArgs& a, ShRestArgs& sh, const FusedAdam& o) {
    const int map[5] = {0, 1, 3, 4, 5};     // kernel group order: means, sh0, opacities, scales, rotations
    for (int k = 0; k < 5; ++k) {
        a.p[k] = o.params[map[k]]; a.m[k] = o.exp_avgs[map[k]]; a.v[k] = o.exp_avg_sqs[map[k]];
        a.h[k] = adam_hyper(o.step, o.lrs[map[k]], o.beta1, o.beta2, o.eps);
    }
    sh.p = o.params[2]; sh.m = o.exp_avgs[2]; sh.v = o.exp_avg_sqs[2]; sh.h = adam_hyper(o.step, o.lrs[2], o.beta1, o.beta2, o.eps);
}

// ---- the single-GPU pipeline (api.hip); the sharded renderer enters it behind K1 (forward_tail) and ahead of K12 (run_blend_backward) ----
enum ForwardMode { MODE_TRAINING, MODE_INFERENCE, MODE_SCORES };       // fgs_forward*, fgs_inference / fgs_inference_aux, fgs_pruning_scores
struct ForwardRequest {
    ForwardMode mode; GaussianParams params; int32_t n; const fgs_settings* settings;
    float* image; int to_chw, clamp_output;
    fgs_resize_fn resize; void* user; fgs_forward_state* state_out; hipStream_t stream;
    float* scores;                        // MODE_SCORES: the output, [N]
    int32_t instance_capacity;            // > 0: the host-synchronisation-free form (fgs_forward_async)
    // MODE_INFERENCE through fgs_inference_aux: per-pixel maps [H,W] written by the blend beside the image (each may be NULL, not all three);
    // MODE_TRAINING through fgs_forward_aux: alpha and expected depth (no median), plus the depth checkpoints a depth backward pass needs
    bool aux = false; float* aux_alpha = nullptr; float* aux_depth = nullptr; float* aux_median = nullptr;
};
// What K2..K10 know of the visible list. on_device: the two counts are BOUNDS (primitive count / caller's instance capacity) and the exact
// ones stay in the primitive blob's counters. depth_sel >= 0: the list is already depth-sorted and the sorted half is depth_sel.
struct ForwardCounts { uint32_t n_visible, n_instances; int depth_sel; bool on_device; };
int run_forward(const ForwardRequest& rq);
int forward_tail(const ForwardRequest& rq, PrimitiveBuffers& pb, const TileBuffers& tb, const Geometry& geo, ForwardCounts counts);

struct BackwardBlobs { void* primitive; void* tile; void* instance; void* bucket; void* scratch; };      // the forward pass's four blobs + the backward scratch
struct BackwardPlan {
    int32_t n; const fgs_settings* settings; const fgs_forward_state* state;
    Geometry geo; PrimitiveBuffers pb; TileBuffers tb; InstanceBuffers ib; BucketBuffers bb; BackwardScratch sc;
};
// with_depth: the scratch blob has the layout of fgs_backward_aux_scratch_bytes. The bucket blob is carved with ckpt_d whenever the state says it has one.
// with_abs: ... of fgs_backward_absgrad_scratch_bytes (the aux layout with the absolute sums behind it).
int plan_backward(BackwardPlan& P, const BackwardBlobs& blobs, int32_t n_primitives, const fgs_settings* settings, const fgs_forward_state* state, bool with_depth = false,
                  bool with_abs = false);
// staging pass + K11. cleared_by_preprocess: a K1 of this library filled the primitive blob and cleared the visible Gaussians' accumulator records
int run_blend_backward(const BackwardPlan& P, const float* grad_image, const float* image, hipStream_t stream, bool cleared_by_preprocess = true);
// the same with upstream gradients of accumulated opacity / expected depth (either may be NULL = zero; `depth` = the forward pass's map, read with grad_depth)
int run_blend_backward_aux(const BackwardPlan& P, const float* grad_image, const float* image, const float* grad_alpha, const float* grad_depth,
                           const float* depth, const float* means, hipStream_t stream);
// either of the two that also sums the absolute per-pixel shares of dL/dmean2d into P.sc.acc_abs (a plan made with_abs); with_maps: the second form
int run_blend_backward_abs(const BackwardPlan& P, const float* grad_image, const float* image, bool with_maps, const float* grad_alpha, const float* grad_depth,
                           const float* depth, const float* means, hipStream_t stream);
}  // namespace fgs

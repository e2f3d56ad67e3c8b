// C-ABI entry points of the operators around the rasterizer: the Adam step, the fused L1 + DSSIM loss, the reference's auxiliary operators
// (aux_ops.hip) and the maintenance of the Gaussian set on the device (densify.hip; Model.py:275-366, 459-463).
#include "fgs_host.h"

using namespace fgs;
namespace {
struct AdcScratch {
    uint32_t* plan; uint4* offsets; uint32_t* totals; char* scan_temp; size_t scan_temp_bytes;
    static AdcScratch carve(Carver& c, uint32_t n) {
        AdcScratch b;
        b.plan = c.take<uint32_t>("plan", n);
        b.offsets = c.take<uint4>("offsets", n);
        b.totals = c.take<uint32_t>("totals", 4);
        b.scan_temp_bytes = adc_scan_temp_bytes(n);
        b.scan_temp = c.take<char>("scan_temp", b.scan_temp_bytes);
        return b;
    }
};

// The loss scratch, in floats: three derivative maps [3,H,W] of plane3 each, then the forward kernel's partial sums -- one pair per wave, i.e. per
// strip of 64 columns and band of rows of a channel (l1_dssim_partials) -- on an 8-byte boundary (read as float2: 9 W H is odd for odd x odd images)
struct LossScratch {
    size_t plane3, partials_at;
    LossScratch(int width, int height) : plane3(3 * static_cast<size_t>(width) * static_cast<size_t>(height)), partials_at((3 * plane3 + 1) & ~static_cast<size_t>(1)) {}
    void point_maps(LossArgs& a, void* scratch) const { a.d_mu = static_cast<float*>(scratch); a.d_m11 = a.d_mu + plane3; a.d_m12 = a.d_m11 + plane3; }
    // the weighted loss appends the strip-bands' weight sums (one channel plane's worth) and their total S to the same layout
    void point_weighted(LossArgs& a, void* scratch, const float* weight, int width, int height) const {
        point_maps(a, scratch);
        a.weight = weight; a.partials = a.d_mu + partials_at; a.wpartials = a.partials + l1_dssim_partials(width, height);
        a.total_weight = a.wpartials + l1_dssim_weight_partials(width, height);
    }
};

const char* weighted_loss_refusal(const void* image, const void* target, const void* weight, const void* out, const void* scratch, int width, int height) {
    if (!weight) return "weight is NULL (the unweighted loss is fgs_l1_dssim_loss / fgs_l1_dssim_backward)";
    if (!image || !target || !out || !scratch) return "NULL image / target / output / scratch";
    if (width <= 0 || height <= 0) return "non-positive image size";
    if ((reinterpret_cast<uintptr_t>(scratch) & 7u) != 0) return "scratch must be 8-byte aligned";
    return nullptr;
}
}  // namespace

extern "C" {
#pragma GCC visibility push(default)
int32_t fgs_adam_step_multi_quiet(int32_t n_groups, const float* const* grads, float* const* params, float* const* exp_avgs,
                                  float* const* exp_avg_sqs, const int64_t* n_elements, const int32_t* steps, const double* lrs,
                                  double beta1, double beta2, double eps, const uint8_t* live_blocks, const int32_t* floats_per_gaussian,
                                  uint8_t* quiet_blocks, void* stream) {
    if (n_groups < 0 || n_groups > 8) return fail(FGS_ERR_INVALID_ARGUMENT, "n_groups %d (max 8)", n_groups);
    if ((live_blocks != nullptr || quiet_blocks != nullptr) && floats_per_gaussian == nullptr) return fail(FGS_ERR_INVALID_ARGUMENT, "live_blocks / quiet_blocks without floats_per_gaussian");
    AdamArgs a{};
    a.live_blocks = live_blocks;
    int64_t rows = -1;                  // quiet_blocks: the N all groups share
    // the skip rests on "adam_update with g = m = v = 0 is the identity", which holds for eps > 0 (as the float the kernel sees) and finite hyperparameters
    // only (0 / 0 and inf * 0 make the dense kernel write NaN, and the skip must not hide that); without live flags, or with a tensor beyond the kernel's
    // 32-bit row arithmetic, nothing says which blocks receive a gradient: the flags are not used then and every one of them is cleared below (the
    // moments become unknown)
    bool quiet_ok = quiet_blocks != nullptr && live_blocks != nullptr;
    for (int k = 0; k < n_groups; ++k) {
        if (n_elements[k] < 0 || steps[k] < 1) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: n_elements / step", k);
        if (n_elements[k] == 0) continue;
        if (!grads[k] || !params[k] || !exp_avgs[k] || !exp_avg_sqs[k]) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: NULL tensor", k);
        AdamGroup& g = a.g[a.n_groups++];
        g.grad = grads[k]; g.param = params[k]; g.exp_avg = exp_avgs[k]; g.exp_avg_sq = exp_avg_sqs[k]; g.n = n_elements[k];
        g.h = adam_hyper(steps[k], lrs[k], beta1, beta2, eps);
        g.row_len = 0;
        if (live_blocks != nullptr || quiet_blocks != nullptr) {
            if (floats_per_gaussian[k] < 1 || n_elements[k] % floats_per_gaussian[k] != 0) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: floats_per_gaussian", k);
            if (n_elements[k] < (int64_t{1} << 32)) g.row_len = static_cast<uint32_t>(floats_per_gaussian[k]);   // 32-bit index arithmetic in the kernel
            if (quiet_blocks != nullptr) {
                const int64_t n = n_elements[k] / floats_per_gaussian[k];
                if (rows >= 0 && n != rows) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: quiet_blocks needs one N for all groups (%lld vs %lld)", k, (long long)n, (long long)rows);
                rows = n;
            }
        }
        quiet_ok = quiet_ok && g.row_len != 0u && g.h.eps > 0.0f && std::isfinite(g.h.eps) && std::isfinite(g.h.step_size) && std::isfinite(g.h.beta1) &&
                   std::isfinite(g.h.beta2) && std::isfinite(g.h.bc2_sqrt_rcp);
    }
    if (quiet_ok) a.quiet_blocks = quiet_blocks;
    else if (quiet_blocks != nullptr && rows > 0) FGS_HIP(hipMemsetAsync(quiet_blocks, 0, static_cast<size_t>((rows + 63) / 64), static_cast<hipStream_t>(stream)));
    { StageScope t(ST_ADAM, static_cast<hipStream_t>(stream)); FGS_HIP(launch_adam(a, static_cast<hipStream_t>(stream))); }
    return FGS_OK;
}

int32_t fgs_adam_step_multi_live(int32_t n_groups, const float* const* grads, float* const* params, float* const* exp_avgs,
                                 float* const* exp_avg_sqs, const int64_t* n_elements, const int32_t* steps, const double* lrs,
                                 double beta1, double beta2, double eps, const uint8_t* live_blocks, const int32_t* floats_per_gaussian,
                                 void* stream) {
    return fgs_adam_step_multi_quiet(n_groups, grads, params, exp_avgs, exp_avg_sqs, n_elements, steps, lrs, beta1, beta2, eps, live_blocks,
                                     floats_per_gaussian, nullptr, stream);
}

int32_t fgs_adam_quiet_scan(int32_t n_groups, const float* const* exp_avgs, const float* const* exp_avg_sqs, const int64_t* n_elements,
                            const int32_t* floats_per_gaussian, uint8_t* quiet_out, void* stream) {
    if (n_groups < 0 || n_groups > 8) return fail(FGS_ERR_INVALID_ARGUMENT, "n_groups %d (max 8)", n_groups);
    if (n_groups > 0 && (!exp_avgs || !exp_avg_sqs || !n_elements || !floats_per_gaussian)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL argument");
    AdamQuietScanArgs a{};
    int64_t rows = -1;
    for (int k = 0; k < n_groups; ++k) {
        if (n_elements[k] < 0 || floats_per_gaussian[k] < 1 || n_elements[k] % floats_per_gaussian[k] != 0) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: n_elements / floats_per_gaussian", k);
        const int64_t n = n_elements[k] / floats_per_gaussian[k];
        if (rows >= 0 && n != rows) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: all groups must have the same N (%lld vs %lld)", k, (long long)n, (long long)rows);
        rows = n;
        if (n > 0x7fffffff || floats_per_gaussian[k] > (1 << 20)) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: N / floats_per_gaussian out of range", k);
        if (n == 0) continue;
        if (!exp_avgs[k] || !exp_avg_sqs[k]) return fail(FGS_ERR_INVALID_ARGUMENT, "group %d: NULL tensor", k);
        a.m[a.n_groups] = exp_avgs[k]; a.v[a.n_groups] = exp_avg_sqs[k]; a.row_len[a.n_groups] = static_cast<uint32_t>(floats_per_gaussian[k]);
        ++a.n_groups;
    }
    if (rows <= 0) return FGS_OK;
    if (!quiet_out) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL quiet_out");
    a.rows = static_cast<uint32_t>(rows); a.quiet_out = quiet_out;
    FGS_HIP(launch_adam_quiet_scan(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

int32_t fgs_adam_step_multi(int32_t n_groups, const float* const* grads, float* const* params, float* const* exp_avgs,
                            float* const* exp_avg_sqs, const int64_t* n_elements, const int32_t* steps, const double* lrs,
                            double beta1, double beta2, double eps, void* stream) {
    return fgs_adam_step_multi_live(n_groups, grads, params, exp_avgs, exp_avg_sqs, n_elements, steps, lrs, beta1, beta2, eps, nullptr, nullptr, stream);
}

int32_t fgs_adam_step(const float* grad, float* param, float* exp_avg, float* exp_avg_sq, int64_t n_elements,
                      int32_t step, double lr, double beta1, double beta2, double eps, void* stream) {
    return fgs_adam_step_multi(1, &grad, &param, &exp_avg, &exp_avg_sq, &n_elements, &step, &lr, beta1, beta2, eps, stream);
}

int32_t fgs_update_3d_filter(const float* positions, const float* w2c, float* filter_3d, uint8_t* visibility_mask, int32_t n_points,
                             int32_t width, int32_t height, float focal_x, float focal_y, float center_x, float center_y,
                             float near_plane, float clipping_tolerance, float distance2filter, void* stream) {
    if (n_points < 0 || (n_points > 0 && (!positions || !w2c || !filter_3d || !visibility_mask))) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    // host-side frustum bounds exactly as filter3d.cu:55-66
    const float bounds_factor = clipping_tolerance + 0.5f;
    const float width_f = static_cast<float>(width), height_f = static_cast<float>(height);
    const float max_x = bounds_factor * width_f, max_y = bounds_factor * height_f;
    const float off_x = center_x - 0.5f * width_f, off_y = center_y - 0.5f * height_f;
    const float left = (-max_x - off_x) / focal_x, right = (max_x - off_x) / focal_x;
    const float top = (-max_y - off_y) / focal_y, bottom = (max_y - off_y) / focal_y;
    FGS_HIP(launch_update_3d_filter(positions, w2c, filter_3d, visibility_mask, n_points, left, right, top, bottom, near_plane,
                                    distance2filter, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

int32_t fgs_relocation_table(float* table_host_2500) {
    if (!table_host_2500) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL table");
    relocation_coefficients(table_host_2500);
    return FGS_OK;
}

int32_t fgs_relocation_adjustment(const float* old_opacities, const float* old_scales, const int64_t* n_samples_per_primitive,
                                  const float* table_device, float* new_opacities, float* new_scales, int32_t n_primitives, void* stream) {
    if (n_primitives < 0 || (n_primitives > 0 && (!old_opacities || !old_scales || !n_samples_per_primitive || !table_device || !new_opacities || !new_scales)))
        return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    FGS_HIP(launch_relocation(old_opacities, old_scales, n_samples_per_primitive, table_device, new_opacities, new_scales,
                              static_cast<unsigned>(n_primitives), static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

int32_t fgs_add_noise(const float* raw_scales, const float* raw_rotations, const float* raw_opacities, const float* random_samples,
                      float* means, int32_t n_primitives, float current_lr, void* stream) {
    if (n_primitives < 0 || (n_primitives > 0 && (!raw_scales || !raw_rotations || !raw_opacities || !random_samples || !means)))
        return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    FGS_HIP(launch_add_noise(raw_scales, raw_rotations, raw_opacities, random_samples, means, static_cast<unsigned>(n_primitives), current_lr,
                             static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

size_t fgs_adc_scratch_bytes(int32_t n_primitives) {
    if (n_primitives < 0) return 0;
    Carver c(nullptr);
    AdcScratch::carve(c, static_cast<uint32_t>(n_primitives));
    return c.total();
}

int32_t fgs_adc_plan_thresholds(const float* densification_info, const float* scales, const float* rotations, const float* opacities, int32_t n_primitives,
                                float grad_threshold, float min_opacity_logit, int32_t prune_large_gaussians, float log_small, float log_large,
                                void* scratch, int32_t* counts_out, void* stream_) {
    if (n_primitives < 0 || !counts_out || !scratch) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    if (n_primitives > 0 && (!densification_info || !scales || !rotations || !opacities)) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL tensor");
    if (min_opacity_logit != min_opacity_logit || log_small != log_small || log_large != log_large) return fail(FGS_ERR_INVALID_ARGUMENT, "a threshold is NaN");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Carver c(scratch);
    const AdcScratch sc = AdcScratch::carve(c, static_cast<uint32_t>(n_primitives));
    AdcPlanArgs a{};
    a.densification_info = densification_info; a.scales = scales; a.rotations = rotations; a.opacities = opacities;
    a.n = static_cast<uint32_t>(n_primitives);
    a.grad_threshold = grad_threshold;
    a.min_opacity_logit = min_opacity_logit; a.log_small = log_small; a.log_large = log_large;
    a.prune_large = prune_large_gaussians ? 1 : 0;
    a.plan = sc.plan; a.offsets = sc.offsets; a.totals = sc.totals; a.scan_temp = sc.scan_temp; a.scan_temp_bytes = sc.scan_temp_bytes;
    FGS_HIP(launch_adc_plan(a, stream));
    uint32_t host[4] = {0, 0, 0, 0};
    FGS_HIP(hipMemcpyAsync(host, sc.totals, sizeof(host), hipMemcpyDeviceToHost, stream));     // the caller sizes the new tensors from these
    FGS_HIP(hipStreamSynchronize(stream));
    for (int k = 0; k < 4; ++k) counts_out[k] = static_cast<int32_t>(host[k]);
    return FGS_OK;
}

// The thresholds from float arguments: what a caller that holds float32 values gets. The reference forms them from Python doubles (0.01 is not
// float(0.01f)), which a float argument cannot carry: FasterGSCudaBackend goes through fgs_adc_plan_thresholds.
int32_t fgs_adc_plan(const float* densification_info, const float* scales, const float* rotations, const float* opacities, int32_t n_primitives,
                     float grad_threshold, float min_opacity, int32_t prune_large_gaussians, float percent_dense, float extent,
                     void* scratch, int32_t* counts_out, void* stream) {
    if (!(min_opacity > 0.0f && min_opacity < 1.0f) || !(percent_dense * extent > 0.0f)) return fail(FGS_ERR_INVALID_ARGUMENT, "min_opacity / percent_dense * extent out of range");
    const float min_opacity_logit = static_cast<float>(std::log(static_cast<double>(min_opacity) / (1.0 - static_cast<double>(min_opacity))));   // Model.py:360
    const float log_small = static_cast<float>(std::log(static_cast<double>(percent_dense) * static_cast<double>(extent)));                         // :315
    const float log_large = static_cast<float>(std::log(0.1 * static_cast<double>(extent)));                                                         // :363
    return fgs_adc_plan_thresholds(densification_info, scales, rotations, opacities, n_primitives, grad_threshold, min_opacity_logit, prune_large_gaussians,
                                   log_small, log_large, scratch, counts_out, stream);
}

int32_t fgs_adc_apply(const float* const* params, const float* const* exp_avgs, const float* const* exp_avg_sqs,
                      float* const* out_params, float* const* out_exp_avgs, float* const* out_exp_avg_sqs,
                      const float* noise, const void* scratch, int32_t n_primitives, int32_t total_sh_bases_rest, void* stream_) {
    if (n_primitives < 0 || !params || !out_params || !scratch || total_sh_bases_rest < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    if ((exp_avgs == nullptr) != (exp_avg_sqs == nullptr) || (exp_avgs && (!out_exp_avgs || !out_exp_avg_sqs))) return fail(FGS_ERR_INVALID_ARGUMENT, "moments: all four arrays or none");
    if (n_primitives == 0) return FGS_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    Carver c(const_cast<void*>(scratch));
    const AdcScratch sc = AdcScratch::carve(c, static_cast<uint32_t>(n_primitives));
    // optimizer-group order (Model.py:238-245): means, sh0, sh_rest, opacities, scales, rotations
    const uint32_t width[6] = {3u, 3u, 3u * static_cast<uint32_t>(total_sh_bases_rest), 1u, 3u, 4u};
    const int kind[6] = {1, 0, 0, 0, 2, 0};
    for (int k = 0; k < 6; ++k) {
        if (width[k] == 0) continue;
        if (!params[k] || !out_params[k]) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL tensor in group %d", k);
        AdcScatterArgs a{};
        a.in_p = params[k]; a.out_p = out_params[k];
        if (exp_avgs && exp_avgs[k]) {
            if (!exp_avg_sqs[k] || !out_exp_avgs[k] || !out_exp_avg_sqs[k]) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL moment tensor in group %d", k);
            a.in_m = exp_avgs[k]; a.in_v = exp_avg_sqs[k]; a.out_m = out_exp_avgs[k]; a.out_v = out_exp_avg_sqs[k];
        }
        a.scales = params[4]; a.rotations = params[5]; a.noise = noise;
        a.plan = sc.plan; a.offsets = sc.offsets; a.totals = sc.totals;
        a.n = static_cast<uint32_t>(n_primitives); a.width = width[k];
        FGS_HIP(launch_adc_scatter(kind[k], a, stream));
    }
    return FGS_OK;
}

int32_t fgs_gather_rows(int32_t n_tensors, const float* const* in, float* const* out, const int32_t* widths, const int64_t* index,
                        int32_t n_rows, void* stream) {
    if (n_tensors < 0 || n_tensors > kGatherTensors || n_rows < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "n_tensors %d (max %d) / n_rows %d", n_tensors, kGatherTensors, n_rows);
    if (n_rows == 0 || n_tensors == 0) return FGS_OK;
    if (!in || !out || !widths || !index) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL argument");
    GatherArgs a{};
    for (int k = 0; k < n_tensors; ++k) {
        if (widths[k] < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "tensor %d: width %d", k, widths[k]);
        if (widths[k] == 0) continue;
        if (!in[k] || !out[k]) return fail(FGS_ERR_INVALID_ARGUMENT, "tensor %d: NULL", k);
        GatherTensor& t = a.t[a.n_tensors++];
        t.in = in[k]; t.out = out[k]; t.width = static_cast<uint32_t>(widths[k]);
    }
    a.n_rows = static_cast<uint32_t>(n_rows); a.index = index;
    FGS_HIP(launch_gather_rows(a, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

size_t fgs_morton_order_temp_bytes(int32_t n_points) { return n_points < 0 ? 0 : morton_temp_bytes(static_cast<uint32_t>(n_points)); }

int32_t fgs_morton_order(const float* means, const float* lo, const float* hi, int64_t* order_out, int32_t n_points, void* temp, size_t temp_bytes,
                         void* stream) {
    if (n_points < 0) return fail(FGS_ERR_INVALID_ARGUMENT, "n_points %d", n_points);
    if (n_points == 0) return FGS_OK;
    if (!means || !lo || !hi || !order_out || !temp || temp_bytes < morton_temp_bytes(static_cast<uint32_t>(n_points))) return fail(FGS_ERR_INVALID_ARGUMENT, "NULL / short buffer");
    FGS_HIP(run_morton_order(means, lo, hi, order_out, static_cast<uint32_t>(n_points), temp, temp_bytes, static_cast<hipStream_t>(stream)));
    return FGS_OK;
}

size_t fgs_l1_dssim_scratch_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    return sizeof(float) * (LossScratch(width, height).partials_at + l1_dssim_partials(width, height));
}

int32_t fgs_l1_dssim_loss(const float* image, const float* target, int32_t width, int32_t height, float lambda_l1, float lambda_dssim,
                          float* sums, float* grad_image, void* scratch, void* stream_) {
    if (!image || !target || !sums || !scratch || width <= 0 || height <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LossArgs a{};
    a.image = image; a.target = target; a.sums = sums; a.grad = grad_image;
    const LossScratch layout(width, height);
    layout.point_maps(a, scratch); a.partials = a.d_mu + layout.partials_at;
    if ((reinterpret_cast<uintptr_t>(a.partials) & 7u) != 0) return fail(FGS_ERR_INVALID_ARGUMENT, "scratch must be 8-byte aligned");
    a.width = width; a.height = height; a.lambda_l1 = lambda_l1; a.lambda_dssim = lambda_dssim;
    { StageScope t(ST_LOSS, stream); FGS_HIP(launch_l1_dssim(a, stream)); }
    return FGS_OK;
}

int32_t fgs_l1_dssim_backward(const float* image, const float* target, int32_t width, int32_t height, float lambda_l1, float lambda_dssim,
                              const float* upstream, float* grad_image, const void* scratch, void* stream_) {
    if (!image || !target || !grad_image || !scratch || width <= 0 || height <= 0) return fail(FGS_ERR_INVALID_ARGUMENT, "bad argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LossArgs a{};
    a.image = image; a.target = target; a.grad = grad_image; a.upstream = upstream;
    LossScratch(width, height).point_maps(a, const_cast<void*>(scratch));      // the maps a forward launch left there
    a.width = width; a.height = height; a.lambda_l1 = lambda_l1; a.lambda_dssim = lambda_dssim;
    { StageScope t(ST_LOSS, stream); FGS_HIP(launch_l1_dssim_backward(a, stream)); }
    return FGS_OK;
}

size_t fgs_l1_dssim_weighted_scratch_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    return sizeof(float) * (LossScratch(width, height).partials_at + l1_dssim_partials(width, height) + l1_dssim_weight_partials(width, height) + 1);
}

int32_t fgs_l1_dssim_weighted_loss(const float* image, const float* target, const float* weight, int32_t width, int32_t height, float lambda_l1,
                                   float lambda_dssim, float* sums, float* grad_image, void* scratch, void* stream_) {
    if (const char* why = weighted_loss_refusal(image, target, weight, sums, scratch, width, height)) return fail(FGS_ERR_INVALID_ARGUMENT, "fgs_l1_dssim_weighted_loss: %s", why);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LossArgs a{};
    a.image = image; a.target = target; a.sums = sums; a.grad = grad_image;
    LossScratch(width, height).point_weighted(a, scratch, weight, width, height);
    a.width = width; a.height = height; a.lambda_l1 = lambda_l1; a.lambda_dssim = lambda_dssim;
    { StageScope t(ST_LOSS, stream); FGS_HIP(launch_l1_dssim(a, stream)); }
    return FGS_OK;
}

int32_t fgs_l1_dssim_weighted_backward(const float* image, const float* target, const float* weight, int32_t width, int32_t height, float lambda_l1,
                                       float lambda_dssim, const float* upstream, float* grad_image, const void* scratch, void* stream_) {
    if (const char* why = weighted_loss_refusal(image, target, weight, grad_image, scratch, width, height)) return fail(FGS_ERR_INVALID_ARGUMENT, "fgs_l1_dssim_weighted_backward: %s", why);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    LossArgs a{};
    a.image = image; a.target = target; a.grad = grad_image; a.upstream = upstream;
    LossScratch(width, height).point_weighted(a, const_cast<void*>(scratch), weight, width, height);   // the maps and S a forward launch left there
    a.width = width; a.height = height; a.lambda_l1 = lambda_l1; a.lambda_dssim = lambda_dssim;
    { StageScope t(ST_LOSS, stream); FGS_HIP(launch_l1_dssim_backward(a, stream)); }
    return FGS_OK;
}
#pragma GCC visibility pop
}  // extern "C"

// Host side of libsudokuvision_hip.so: context, weight loading, fp64 homography, argument checks.
// Everything exported here is declared in include/sudoku_vision_hip.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sv_augment_host.h"
#include "sv_dataset_rec.h"
#include "sv_synth_host.h"
#include "sv_internal.h"
#include "sv_philox.h"

// ---- errors ---------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

int sv_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *sv_last_error(void) { return g_err; }
extern "C" int sv_version(void) { return 2; }

// ---- context --------------------------------------------------------------------------------------
extern "C" int sv_ctx_create(int device, sv_ctx **out)
{
    if (!out) return sv_fail(SV_ERR_BAD_ARG, "sv_ctx_create: out is NULL");
    int count = 0;
    SV_HIP(hipGetDeviceCount(&count));
    if (device < 0 || device >= count) return sv_fail(SV_ERR_BAD_ARG, "sv_ctx_create: device %d of %d", device, count);
    SV_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    SV_HIP(hipGetDeviceProperties(&prop, device));
    sv_ctx *c = new sv_ctx();
    c->device = device;
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    *out = c;
    return SV_OK;
}

template <class W>   // sv_weights, sv_weights3 or sv_weights_light
static void free_weights(W &w)
{
    for (void *p : w.allocs) (void)hipFree(p);
    w = W();
}

extern "C" int sv_ctx_destroy(sv_ctx *ctx)
{
    if (!ctx) return SV_OK;
    (void)hipSetDevice(ctx->device);
    free_weights(ctx->w);
    free_weights(ctx->w3);
    free_weights(ctx->wl);
    free_weights(ctx->we);
    ctx->for_each_scratch([](sv_scratch &b) { b.release(); });
    for (auto &t : ctx->timeline) { (void)hipEventDestroy(t.t0); (void)hipEventDestroy(t.t1); }
    for (auto &e : ctx->event_pool) (void)hipEventDestroy(e);
    delete ctx;
    return SV_OK;
}

int sv_scratch::grow(sv_ctx *ctx, size_t bytes)
{
    if (bytes <= cap) return SV_OK;
    SV_HIP(hipSetDevice(ctx->device));
    if (p) SV_HIP(hipFree(p));
    p = nullptr;
    cap = 0;
    SV_HIP(hipMalloc(&p, bytes));
    cap = bytes;
    return SV_OK;
}

// features, cells and cells2 for `cells` cells: three allocations (kernels test their alignment)
int sv_ensure_scratch(sv_ctx *ctx, long cells)
{
    if (cells <= ctx->n_cells) return SV_OK;
    ctx->n_cells = 0;
    int rc;
    if ((rc = ctx->features.grow(ctx, sizeof(float) * 3136 * (size_t)cells))) return rc;
    if ((rc = ctx->cells.grow(ctx, (size_t)SV_CELL_PX * (size_t)cells))) return rc;
    if ((rc = ctx->cells2.grow(ctx, (size_t)SV_CELL_PX * (size_t)cells))) return rc;
    ctx->n_cells = cells;
    return SV_OK;
}

// the v3 forward's activation buffers for batches of `cells` cells (at most SV_V3_SUBBATCH of them are in flight)
static int sv_ensure_scratch_v3(sv_ctx *ctx, long cells)
{
    const long want = cells < SV_V3_SUBBATCH ? cells : SV_V3_SUBBATCH;
    if (want <= ctx->v3_cells) return SV_OK;
    ctx->v3_cells = 0;
    const int rc = ctx->v3_act.grow(ctx, svk_v3_scratch_bytes(want));
    if (rc) return rc;
    ctx->v3_cells = want;
    return SV_OK;
}

// the same with room for the MC forward, whose chunks fill all SV_V3_SUBBATCH cells whatever the batch, and its own scratch
static int sv_ensure_scratch_v3_mc(sv_ctx *ctx)
{
    const int rc = sv_ensure_scratch_v3(ctx, SV_V3_SUBBATCH);
    return rc ? rc : ctx->v3_mc.grow(ctx, svk_v3_mc_scratch_bytes());
}

extern "C" int sv_ctx_set_precision(sv_ctx *ctx, int precision)
{
    if (!ctx || (precision != SV_PREC_F32 && precision != SV_PREC_BF16)) return sv_fail(SV_ERR_BAD_ARG, "sv_ctx_set_precision: bad argument");
    ctx->precision = precision;
    return SV_OK;
}

extern "C" int sv_ctx_reserve(sv_ctx *ctx, long max_cells)
{
    if (!ctx || max_cells <= 0) return sv_fail(SV_ERR_BAD_ARG, "sv_ctx_reserve: bad argument");
    SV_HIP(hipSetDevice(ctx->device));
    int rc = ctx->range_flag.grow(ctx, 2 * sizeof(int));                  // sv_cnn_forward_f32's per-call range flag: no hipMalloc after reserve
    if (rc || (rc = sv_ensure_scratch(ctx, max_cells))) return rc;
    return ctx->w3.loaded ? sv_ensure_scratch_v3_mc(ctx) : SV_OK;            // v1-only contexts do not pay for the v3 activations
}

// ---- per-kernel timing -------------------------------------------------------------------------------
sv_time_scope::sv_time_scope(sv_ctx *c, int kernel, hipStream_t st) : ctx(c), s(st)
{
    if (!ctx || !ctx->timing) return;
    hipEvent_t e[2];
    for (auto &ev : e) {
        if (!ctx->event_pool.empty()) { ev = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
        else if (hipEventCreate(&ev) != hipSuccess) return;
    }
    (void)hipEventRecord(e[0], s);
    ctx->timeline.push_back({kernel, e[0], e[1]});
    idx = (int)ctx->timeline.size() - 1;
}

sv_time_scope::~sv_time_scope()
{
    if (idx >= 0) (void)hipEventRecord(ctx->timeline[idx].t1, s);
}

extern "C" int sv_timing_begin(sv_ctx *ctx)
{
    if (!ctx) return sv_fail(SV_ERR_BAD_ARG, "sv_timing_begin: NULL context");
    for (auto &t : ctx->timeline) { ctx->event_pool.push_back(t.t0); ctx->event_pool.push_back(t.t1); }
    ctx->timeline.clear();
    ctx->timing = true;
    return SV_OK;
}

extern "C" int sv_timing_end(sv_ctx *ctx, double *ms_total, long *launches, int n_kernels)
{
    if (!ctx || !ms_total || !launches || n_kernels < 0) return sv_fail(SV_ERR_BAD_ARG, "sv_timing_end: bad argument");
    ctx->timing = false;
    for (int k = 0; k < n_kernels; k++) { ms_total[k] = 0; launches[k] = 0; }
    for (auto &t : ctx->timeline) {
        SV_HIP(hipEventSynchronize(t.t1));
        float ms = 0;
        SV_HIP(hipEventElapsedTime(&ms, t.t0, t.t1));
        if (t.kernel < n_kernels) {                   // a caller built against an older header simply does not see the newer kernel ids
            ms_total[t.kernel] += ms;
            launches[t.kernel]++;
        }
        ctx->event_pool.push_back(t.t0);
        ctx->event_pool.push_back(t.t1);
    }
    ctx->timeline.clear();
    return SV_OK;
}

// ---- weights --------------------------------------------------------------------------------------
extern "C" int sv_load_weights_f32(sv_ctx *ctx, const float *blob)
{
    if (!ctx || !blob) return sv_fail(SV_ERR_BAD_ARG, "sv_load_weights_f32: NULL argument");
    SV_HIP(hipSetDevice(ctx->device));
    free_weights(ctx->w);
    const float *c1w = blob, *c1b = c1w + 288, *c2w = c1b + 32, *c2b = c2w + 18432, *f1w = c2b + 64,
                *f1b = f1w + 401408, *f2w = f1b + 128, *f2b = f2w + 1280;
    sv_weights &w = ctx->w;
    int rc;
    if ((rc = svk_pack_weights_h2(w, c1w, c1b, c2w, c2b, f1w))) return rc;
    if ((rc = svk_pack_weights_bf16(w, c2w, f1w))) return rc;
    if ((rc = svk_pack_weights_f32mfma(w, c2w, f1w))) return rc;
    if ((rc = sv_upload(w, &w.conv1_w, c1w, 288))) return rc;
    if ((rc = sv_upload(w, &w.conv1_b, c1b, 32))) return rc;
    if ((rc = sv_upload(w, &w.conv2_b, c2b, 64))) return rc;
    if ((rc = sv_upload(w, &w.fc1_b, f1b, 128))) return rc;
    if ((rc = sv_upload(w, &w.fc2_w, f2w, 1280))) return rc;
    if ((rc = sv_upload(w, &w.fc2_b, f2b, 10))) return rc;
    w.loaded = true;
    return SV_OK;
}

extern "C" int sv_load_weights_v3_f32(sv_ctx *ctx, const float *blob, long n_floats, int use_se)
{
    if (!ctx || !blob) return sv_fail(SV_ERR_BAD_ARG, "sv_load_weights_v3_f32: NULL argument");
    if (n_floats != svk_v3_blob_floats(use_se != 0))
        return sv_fail(SV_ERR_BAD_ARG, "sv_load_weights_v3_f32: %ld floats, DigitCNNv3(use_se=%s) has %ld", n_floats, use_se ? "True" : "False", svk_v3_blob_floats(use_se != 0));
    SV_HIP(hipSetDevice(ctx->device));
    SV_HIP(hipDeviceSynchronize());                  // a forward still running on the old images
    free_weights(ctx->w3);
    int rc = svk_pack_weights_v3(ctx->w3, blob, use_se != 0);
    if (rc) { free_weights(ctx->w3); return rc; }
    return ctx->n_cells > 0 ? sv_ensure_scratch_v3_mc(ctx) : SV_OK;
}

// the Light and Empty loads: `n_floats` against the model's count, then `pack` into the model's own slot
static int load_light_slot(const char *fn, sv_ctx *ctx, sv_weights_light sv_ctx::*slot, const float *blob, long n_floats, long want, int (*pack)(sv_weights_light &, const float *))
{
    if (!ctx || !blob) return sv_fail(SV_ERR_BAD_ARG, "%s: NULL argument", fn);
    sv_weights_light &w = ctx->*slot;
    if (n_floats != want) return sv_fail(SV_ERR_BAD_ARG, "%s: %ld floats, the model has %ld", fn, n_floats, want);
    SV_HIP(hipSetDevice(ctx->device));
    SV_HIP(hipDeviceSynchronize());                  // a forward still running on the old images
    free_weights(w);
    int rc = pack(w, blob);
    if (rc) free_weights(w);
    return rc;
}

extern "C" int sv_load_weights_v3_light_f32(sv_ctx *ctx, const float *blob, long n_floats)
{
    return load_light_slot("sv_load_weights_v3_light_f32", ctx, &sv_ctx::wl, blob, n_floats, SV_CNN3_LIGHT_PARAMS, svk_pack_weights_light);
}

extern "C" int sv_load_weights_empty_f32(sv_ctx *ctx, const float *blob, long n_floats)
{
    return load_light_slot("sv_load_weights_empty_f32", ctx, &sv_ctx::we, blob, n_floats, SV_EMPTY_PARAMS, svk_pack_weights_empty);
}

// ---- host math ------------------------------------------------------------------------------------
// cv2.getGaussianKernel(n, sigma<=0, CV_32F): fixed tables up to 7, else IEEE-double formula.
void sv_gaussian_taps_f32(int n, float *out)
{
    static const float t3[3] = {0.25f, 0.5f, 0.25f}, t5[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                       t7[7] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    if (n == 1) { out[0] = 1.f; return; }
    if (n == 3) { memcpy(out, t3, sizeof t3); return; }
    if (n == 5) { memcpy(out, t5, sizeof t5); return; }
    if (n == 7) { memcpy(out, t7, sizeof t7); return; }
    const double sigma = std::fma((double)n, 0.15, 0.35);
    const double scale2x = -0.125 / (sigma * sigma);
    const int half = (n - 1) / 2;
    std::vector<double> v(half);
    double sum = 0.0;
    for (int i = 0, x = 1 - n; i < half; i++, x += 2) {
        v[i] = std::exp((double)(x * x) * scale2x);
        sum += v[i];
    }
    sum *= 2.0;
    sum += 1.0;
    const double inv = 1.0 / sum;
    for (int i = 0; i < half; i++) out[i] = out[n - 1 - i] = (float)(v[i] * inv);
    out[half] = (float)inv;
}

namespace {

// order_points, cv/grid.py:74-91: TL = argmin(x+y), BR = argmax(x+y), TR = argmin(y-x), BL = argmax(y-x)
void order_points(const float *p, float *o)
{
    int lo_s = 0, hi_s = 0, lo_d = 0, hi_d = 0;
    float s[4], d[4];
    for (int i = 0; i < 4; i++) { s[i] = p[2 * i] + p[2 * i + 1]; d[i] = p[2 * i + 1] - p[2 * i]; }
    for (int i = 1; i < 4; i++) {
        if (s[i] < s[lo_s]) lo_s = i;
        if (s[i] > s[hi_s]) hi_s = i;
        if (d[i] < d[lo_d]) lo_d = i;
        if (d[i] > d[hi_d]) hi_d = i;
    }
    const int pick[4] = {lo_s, lo_d, hi_s, hi_d};
    for (int i = 0; i < 4; i++) { o[2 * i] = p[2 * pick[i]]; o[2 * i + 1] = p[2 * pick[i] + 1]; }
}

// cv2.getPerspectiveTransform: sv_augment_host.h (K22's builder solves the same system)
bool perspective_transform(const float *src, const float *dst, double *M) { return sv_perspective_transform(src, dst, M); }

// cv::invert for 3x3 doubles: cofactors scaled by 1/det
bool invert3(const double *S, double *D)
{
    double det = S[0] * (S[4] * S[8] - S[5] * S[7]) - S[1] * (S[3] * S[8] - S[5] * S[6]) + S[2] * (S[3] * S[7] - S[4] * S[6]);
    if (det == 0.) return false;
    det = 1. / det;
    D[0] = (S[4] * S[8] - S[5] * S[7]) * det;
    D[1] = (S[2] * S[7] - S[1] * S[8]) * det;
    D[2] = (S[1] * S[5] - S[2] * S[4]) * det;
    D[3] = (S[5] * S[6] - S[3] * S[8]) * det;
    D[4] = (S[0] * S[8] - S[2] * S[6]) * det;
    D[5] = (S[2] * S[3] - S[0] * S[5]) * det;
    D[6] = (S[3] * S[7] - S[4] * S[6]) * det;
    D[7] = (S[1] * S[6] - S[0] * S[7]) * det;
    D[8] = (S[0] * S[4] - S[1] * S[3]) * det;
    return true;
}

}  // namespace

// M = getPerspectiveTransform(ordered, inset corners -> the square), frame -> grid
static bool corners_to_m_one(const float *corners, int out_size, float inset_ratio, double *M)
{
    float o[8], in[8];
    order_points(corners, o);
    // float32 numpy arithmetic of cv/grid.py:113-121
    const float cx = (((o[0] + o[2]) + o[4]) + o[6]) / 4.f, cy = (((o[1] + o[3]) + o[5]) + o[7]) / 4.f;
    for (int i = 0; i < 4; i++) {
        const float dx = cx - o[2 * i], dy = cy - o[2 * i + 1];
        const float dist = std::sqrt(dx * dx + dy * dy);
        const float amt = dist * inset_ratio;
        in[2 * i] = o[2 * i] + (dx / dist) * amt;
        in[2 * i + 1] = o[2 * i + 1] + (dy / dist) * amt;
    }
    const float S = (float)(out_size - 1);
    const float dst[8] = {0, 0, S, 0, S, S, 0, S};
    return perspective_transform(in, dst, M);
}

static bool corners_to_minv_one(const float *corners, int out_size, float inset_ratio, double *minv)
{
    double M[9];
    return corners_to_m_one(corners, out_size, inset_ratio, M) && invert3(M, minv);
}

extern "C" int sv_corners_to_minv(const float *corners, int n, int out_size, float inset_ratio, double *minv)
{
    if (!corners || !minv || n <= 0 || out_size < 2) return sv_fail(SV_ERR_BAD_ARG, "sv_corners_to_minv: bad argument");
    for (int f = 0; f < n; f++)
        if (!corners_to_minv_one(corners + 8 * f, out_size, inset_ratio, minv + 9 * f))
            return sv_fail(SV_ERR_DEGENERATE, "sv_corners_to_minv: frame %d: corners do not define a homography", f);
    return SV_OK;
}

extern "C" int sv_corners_to_minv_batch(const float *corners, int n, int out_size, float inset_ratio, double *minv, uint8_t *ok)
{
    if (!corners || !minv || !ok || n <= 0 || out_size < 2) return sv_fail(SV_ERR_BAD_ARG, "sv_corners_to_minv_batch: bad argument");
    static const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int f = 0; f < n; f++) {
        ok[f] = corners_to_minv_one(corners + 8 * f, out_size, inset_ratio, minv + 9 * f) ? 1 : 0;
        if (!ok[f]) memcpy(minv + 9 * f, ident, sizeof ident);
    }
    return SV_OK;
}

extern "C" int sv_corners_to_m_batch(const float *corners, int n, int out_size, float inset_ratio, double *m, uint8_t *ok)
{
    if (!corners || !m || !ok || n <= 0 || out_size < 2) return sv_fail(SV_ERR_BAD_ARG, "sv_corners_to_m_batch: bad argument");
    static const double ident[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int f = 0; f < n; f++) {
        double minv[9];                      // the ok rule of sv_corners_to_minv_batch: M exists and can be inverted
        ok[f] = corners_to_m_one(corners + 8 * f, out_size, inset_ratio, m + 9 * f) && invert3(m + 9 * f, minv) ? 1 : 0;
        if (!ok[f]) memcpy(m + 9 * f, ident, sizeof ident);
    }
    return SV_OK;
}

// ---- argument checks + dispatch ---------------------------------------------------------------------
static inline hipStream_t S(void *s) { return (hipStream_t)s; }

extern "C" int sv_gray_u8(sv_ctx *ctx, const uint8_t *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint8_t *gray, void *stream)
{
    REQUIRE(ctx && bgr && gray, "NULL argument");
    REQUIRE_FRAMES();
    return svk_gray(bgr, n, H, W, pitch, img_stride, gray, S(stream));
}

extern "C" int sv_blur_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, int ksize, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE(n > 0 && H > 0 && W > 0, "bad shape");
    REQUIRE(ksize > 0 && (ksize & 1), "ksize must be odd and positive");
    if (ksize > 7) return sv_fail(SV_ERR_UNSUPPORTED, "sv_blur_u8: ksize %d (only 1,3,5,7 are restated bit-exactly)", ksize);
    return svk_blur(src, n, H, W, ksize, dst, S(stream));
}

extern "C" int sv_adaptive_threshold_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, int block, double c, int type_inv, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE(n > 0 && H > 0 && W > 0, "bad shape");
    REQUIRE(block > 1 && (block & 1), "block_size must be odd and > 1");
    if (block > 31) return sv_fail(SV_ERR_UNSUPPORTED, "sv_adaptive_threshold_u8: block_size %d > 31", block);
    float taps[31];
    sv_gaussian_taps_f32(block, taps);
    const int idelta = type_inv ? (int)std::floor(c) : (int)std::ceil(c);
    return svk_adaptive_threshold(src, n, H, W, block, taps, idelta, type_inv ? 1 : 0, dst, S(stream));
}

extern "C" int sv_preprocess_u8(sv_ctx *ctx, const uint8_t *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint8_t *binary, void *stream)
{
    REQUIRE(ctx && bgr && binary, "NULL argument");
    REQUIRE_FRAMES();
    return svk_preprocess(ctx, bgr, n, H, W, pitch, img_stride, binary, S(stream));
}

extern "C" int sv_preprocess_warp_cells_u8(sv_ctx *ctx, const uint8_t *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint8_t *binary,
                                           const double *minv, uint8_t *cells, void *stream)
{
    REQUIRE(ctx && bgr && binary && minv && cells, "NULL argument");
    REQUIRE_FRAMES();
    return svk_preprocess_warp_fused(ctx, bgr, n, H, W, pitch, img_stride, binary, minv, cells, S(stream));
}

extern "C" int sv_preprocess_bits_u8(sv_ctx *ctx, const uint8_t *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint32_t *bits, void *stream)
{
    REQUIRE(ctx && bgr && bits, "NULL argument");
    REQUIRE_FRAMES();
    REQUIRE(((uintptr_t)bits & 3) == 0, "bits must be 4-byte aligned");
    return svk_preprocess_bits(ctx, bgr, n, H, W, pitch, img_stride, bits, S(stream));
}

extern "C" int sv_despeckle_bits(sv_ctx *ctx, uint32_t *bits, int n, int H, int W, void *stream)
{
    REQUIRE(ctx && bits, "NULL argument");
    REQUIRE(n > 0 && H > 0 && W > 0 && W % 32 == 0, "bad shape (W must be a multiple of 32)");
    return svk_despeckle_bits(bits, n, H, W, S(stream));
}

extern "C" int sv_despeckle_u8(sv_ctx *ctx, const uint8_t *binary, int n, int H, int W, uint8_t *out, uint32_t *packed, void *stream)
{
    REQUIRE(ctx && binary && out, "NULL argument");
    REQUIRE(n > 0 && H > 0 && W > 0, "bad shape");
    REQUIRE(!packed || W % 32 == 0, "packed output needs W % 32 == 0");
    return svk_despeckle(binary, n, H, W, out, packed, S(stream));
}

// K11 (k11_components.hip).  The argument checks come before anything touches the context or the device.
static int component_filter_args(const void *ctx, const void *a, const void *b, int n, int H, int W, double min_area_ratio)
{
    REQUIRE(ctx && a && b, "NULL argument");
    REQUIRE(n >= 0 && H > 0 && W > 0, "bad shape");
    REQUIRE(min_area_ratio >= 0.0, "min_area_ratio must be a number >= 0");       // (false for NaN)
    return SV_OK;
}

extern "C" int sv_component_filter_bits(sv_ctx *ctx, uint32_t *bits, int n, int H, int W, double min_area_ratio, void *stream)
{
    int rc = component_filter_args(ctx, bits, bits, n, H, W, min_area_ratio);
    if (rc) return rc;
    if (W % 32) return sv_fail(SV_ERR_UNSUPPORTED, "sv_component_filter_bits: W must be a multiple of 32");
    if ((double)H * (double)W > 4e9) return sv_fail(SV_ERR_UNSUPPORTED, "sv_component_filter_bits: frames above 4e9 pixels are not supported");
    if (n == 0 || min_area_ratio == 0.0) return SV_OK;
    return svk_component_filter_bits(ctx, bits, n, H, W, min_area_ratio * ((double)H * (double)W), S(stream));
}

extern "C" int sv_component_filter_u8(sv_ctx *ctx, const uint8_t *binary, int n, int H, int W, double min_area_ratio, uint8_t *out, uint32_t *packed,
                                      void *stream)
{
    int rc = component_filter_args(ctx, binary, out, n, H, W, min_area_ratio);
    if (rc) return rc;
    REQUIRE(!packed || W % 32 == 0, "packed output needs W % 32 == 0");
    if ((double)H * (double)W > 4e9) return sv_fail(SV_ERR_UNSUPPORTED, "sv_component_filter_u8: frames above 4e9 pixels are not supported");
    if (n == 0) return SV_OK;
    return svk_component_filter(ctx, binary, n, H, W, min_area_ratio * ((double)H * (double)W), out, packed, S(stream));
}

extern "C" long sv_sparse_bits_record_bytes(int H, int W, long cap_values)
{
    if (H <= 0 || W <= 0 || (W & 31) || cap_values < 0) return -1;
    const long gpr = ((W >> 5) + 63) / 64;
    return (8 + 8 * gpr * H + 4 * cap_values + 15) / 16 * 16;
}

extern "C" int sv_pack_sparse_bits(sv_ctx *ctx, const uint32_t *bits, int n, int H, int W, uint8_t *records, long record_stride, void *stream)
{
    REQUIRE(ctx && bits && records, "NULL argument");
    REQUIRE(n > 0 && H > 0 && W > 0 && W % 32 == 0, "bad shape (W must be a multiple of 32)");
    const long G = (long)H * (((W >> 5) + 63) / 64);
    REQUIRE(G <= 16000, "frame too large for the sparse record (more than 16000 row groups)");
    REQUIRE(record_stride % 8 == 0 && record_stride >= 8 + 8 * G + 4 && ((uintptr_t)records & 7) == 0, "record stride must be a multiple of 8 with room for the masks");
    return svk_pack_sparse_bits(bits, n, H, W, records, record_stride, S(stream));
}

extern "C" int sv_copy_to_pinned_host(sv_ctx *ctx, const void *src, void *dst_host, size_t bytes, void *stream)
{
    REQUIRE(ctx && src && dst_host, "NULL argument");
    REQUIRE((((uintptr_t)src | (uintptr_t)dst_host) & 15) == 0, "source and destination must be 16-byte aligned");
    if (bytes == 0) return SV_OK;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, dst_host) != hipSuccess || attr.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return sv_fail(SV_ERR_BAD_ARG, "sv_copy_to_pinned_host: destination is not pinned (hipHostMalloc / hipHostRegister) host memory");
    }
    return svk_copy_to_host(src, dst_host, bytes, S(stream));
}

extern "C" int sv_warp_perspective_u8(sv_ctx *ctx, const uint8_t *img, int H, int W, ptrdiff_t pitch, int channels, const double *minv, int out_size, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && img && minv && dst, "NULL argument");
    REQUIRE(H > 0 && W > 0 && out_size > 0 && out_size < 32768, "bad shape");
    REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    REQUIRE(pitch >= (ptrdiff_t)W * channels, "pitch < row bytes");
    return svk_warp_perspective(img, H, W, pitch, channels, minv, out_size, dst, S(stream));
}

extern "C" int sv_extract_cells_u8(sv_ctx *ctx, const uint8_t *grid, int h, int w, ptrdiff_t pitch, int channels, int cell_size, int margin_h, int margin_w, uint8_t *cells, void *stream)
{
    REQUIRE(ctx && grid && cells, "NULL argument");
    REQUIRE(h >= 9 && w >= 9 && cell_size > 0, "bad shape");
    REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    REQUIRE(margin_h >= 0 && margin_w >= 0 && h / 9 - 2 * margin_h > 0 && w / 9 - 2 * margin_w > 0, "margin leaves an empty cell");
    return svk_extract_cells(grid, h, w, pitch, channels, cell_size, margin_h, margin_w, cells, S(stream));
}

extern "C" int sv_warp_cells_u8(sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv, uint8_t *cells, void *stream)
{
    REQUIRE(ctx && frames && minv && cells, "NULL argument");
    REQUIRE_FRAMES();
    return svk_warp_cells(ctx, frames, n, H, W, pitch, frame_stride, minv, cells, S(stream));
}

// the argument checks the two forwards share, reported under `fn`; `loaded`: the model's weights are there, else `loader` is what to call
static int cnn_args_ok(const char *fn, const sv_ctx *ctx, const void *x, long B, const float *logits, bool loaded, const char *loader)
{
    if (!ctx || !x || !logits) return sv_fail(SV_ERR_BAD_ARG, "%s: NULL argument", fn);
    if (B <= 0) return sv_fail(SV_ERR_BAD_ARG, "%s: B = %ld", fn, B);
    if (!loaded) return sv_fail(SV_ERR_NO_WEIGHTS, "%s: call %s first", fn, loader);
    return SV_OK;
}

static int glue_ok(const char *fn, int glue)
{
    return glue == SV_GLUE_NORMALIZE || glue == SV_GLUE_RUNPY ? SV_OK : sv_fail(SV_ERR_BAD_ARG, "%s: glue %d", fn, glue);
}

static int cnn_common(sv_ctx *ctx, const void *x, bool u8in, int glue, long B, float *logits, uint8_t *digits, float *conf, void *stream)
{
    int rc = cnn_args_ok("sv_cnn_forward", ctx, x, B, logits, ctx && ctx->w.loaded, "sv_load_weights_f32");
    if (rc) return rc;
    if ((rc = sv_ensure_scratch(ctx, B))) return rc;
    if ((rc = glue_ok("sv_cnn_forward", glue))) return rc;
    return svk_cnn_forward(ctx, x, u8in, glue, B, logits, digits, conf, S(stream));
}

extern "C" int sv_cnn_forward_f32(sv_ctx *ctx, const float *x, long B, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return cnn_common(ctx, x, false, SV_GLUE_NORMALIZE, B, logits, digits, conf, stream);
}

extern "C" int sv_cnn_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells, long B, int glue, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return cnn_common(ctx, cells, true, glue, B, logits, digits, conf, stream);
}

static int cnn3_common(sv_ctx *ctx, const void *x, bool u8in, int glue, long B, float *logits, float *features, uint8_t *digits, float *conf, void *stream)
{
    int rc = cnn_args_ok("sv_cnn3_forward", ctx, x, B, logits, ctx && ctx->w3.loaded, "sv_load_weights_v3_f32");
    if (rc) return rc;
    if (ctx->precision != SV_PREC_F32) return sv_fail(SV_ERR_UNSUPPORTED, "sv_cnn3_forward: the DigitCNNv3 forward has f32 arithmetic only (context is set to SV_PREC_BF16)");
    if ((rc = glue_ok("sv_cnn3_forward", glue))) return rc;
    if ((rc = sv_ensure_scratch_v3(ctx, B))) return rc;
    if (u8in && glue == SV_GLUE_RUNPY) {             // preprocess_cell as its own pass; its {0,255} output then takes the plain glue
        if ((rc = sv_ensure_scratch(ctx, B))) return rc;
        if ((rc = svk_preprocess_cells((const uint8_t *)x, B, ctx->cells2.as<u8>(), S(stream)))) return rc;
        x = ctx->cells2.p;
    }
    return svk_cnn3_forward(ctx, x, u8in, B, logits, features, digits, conf, S(stream));
}

extern "C" int sv_cnn3_forward_f32(sv_ctx *ctx, const float *x, long B, float *logits, float *features, uint8_t *digits, float *conf, void *stream)
{
    return cnn3_common(ctx, x, false, SV_GLUE_NORMALIZE, B, logits, features, digits, conf, stream);
}

extern "C" int sv_cnn3_forward_mc_f32(sv_ctx *ctx, const float *x, long B, int n_samples, float p_spatial, float p_fc, uint64_t seed, uint64_t offset,
                                      const uint8_t *keep1_in, const uint8_t *keep3_in, const uint8_t *keepf_in, float *mean, float *std, int64_t *predicted,
                                      float *logits_out, uint8_t *keep1_out, uint8_t *keep3_out, uint8_t *keepf_out, void *stream)
{
    REQUIRE(ctx && (x || B == 0), "NULL argument");
    REQUIRE(B >= 0, "B < 0");
    if (!ctx->w3.loaded) return sv_fail(SV_ERR_NO_WEIGHTS, "sv_cnn3_forward_mc_f32: call sv_load_weights_v3_f32 first");
    if (ctx->precision != SV_PREC_F32) return sv_fail(SV_ERR_UNSUPPORTED, "sv_cnn3_forward_mc_f32: the DigitCNNv3 forward has f32 arithmetic only (context is set to SV_PREC_BF16)");
    REQUIRE(p_spatial >= 0.f && p_spatial < 1.f, "p_spatial outside [0, 1)");
    REQUIRE(p_fc >= 0.f && p_fc <= 1.f, "p_fc outside [0, 1]");
    REQUIRE(n_samples >= 1 && n_samples <= SV_V3_SUBBATCH, "n_samples outside 1 .. SV_V3_SUBBATCH");
    REQUIRE((!keep1_in == !keep3_in) && (!keep1_in == !keepf_in), "keep_in: all three masks or none");
    if (B == 0) return SV_OK;
    const int rc = sv_ensure_scratch_v3_mc(ctx);
    if (rc) return rc;
    const uint8_t *const in[3] = {keep1_in, keep3_in, keepf_in};
    uint8_t *const out[3] = {keep1_out, keep3_out, keepf_out};
    return svk_cnn3_forward_mc(ctx, x, B, n_samples, p_spatial, p_fc, seed, offset, in, mean, std, (long long *)predicted, logits_out, out, S(stream));
}

extern "C" int sv_mc_dropout_masks_host(uint64_t seed, uint64_t offset, int n_samples, long B, float p_spatial, float p_fc, uint8_t *keep1, uint8_t *keep3,
                                        uint8_t *keepf)
{
    REQUIRE(n_samples >= 1 && B >= 0, "bad shape");
    REQUIRE(p_spatial >= 0.f && p_spatial < 1.f, "p_spatial outside [0, 1)");
    REQUIRE(p_fc >= 0.f && p_fc <= 1.f, "p_fc outside [0, 1]");
    sv_mc_masks_fill(seed, offset, n_samples, B, p_spatial, p_fc, keep1, keep3, keepf);
    return SV_OK;
}

extern "C" int sv_cnn3_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells, long B, int glue, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return cnn3_common(ctx, cells, true, glue, B, logits, nullptr, digits, conf, stream);
}

// what the Light and Empty forwards check and prepare, reported under `fn`: 1 = nothing to do (B == 0), 0 = go on with x (the cells
// after preprocess_cell where that glue was asked for), else the error
static int light_prepare(const char *fn, sv_ctx *ctx, const void *&x, bool u8in, int glue, long B, const void *out, const sv_weights_light *w, const char *loader, void *stream)
{
    if (ctx && B == 0) return w->loaded ? 1 : sv_fail(SV_ERR_NO_WEIGHTS, "%s: call %s first", fn, loader);
    int rc = cnn_args_ok(fn, ctx, x, B, (const float *)out, ctx && w->loaded, loader);
    if (rc) return rc;
    if (B > 0x7fffffffL) return sv_fail(SV_ERR_BAD_ARG, "%s: B = %ld", fn, B);
    if (ctx->precision != SV_PREC_F32) return sv_fail(SV_ERR_UNSUPPORTED, "%s: this forward has f32 arithmetic only (context is set to SV_PREC_BF16)", fn);
    if ((rc = glue_ok(fn, glue))) return rc;
    if (u8in && glue == SV_GLUE_RUNPY) {             // preprocess_cell as its own pass; its {0,255} output then takes the plain glue
        if ((rc = sv_ensure_scratch(ctx, B))) return rc;
        if ((rc = svk_preprocess_cells((const uint8_t *)x, B, ctx->cells2.as<u8>(), S(stream)))) return rc;
        x = ctx->cells2.p;
    }
    return SV_OK;
}

static int cnn3_light_common(sv_ctx *ctx, const void *x, bool u8in, int glue, long B, float *logits, float *features, uint8_t *digits, float *conf, void *stream)
{
    const int rc = light_prepare("sv_cnn3_light_forward", ctx, x, u8in, glue, B, logits, ctx ? &ctx->wl : nullptr, "sv_load_weights_v3_light_f32", stream);
    if (rc) return rc == 1 ? SV_OK : rc;
    return svk_cnn3_light_forward(ctx, x, u8in, B, logits, features, digits, conf, S(stream));
}

extern "C" int sv_cnn3_light_forward_f32(sv_ctx *ctx, const float *x, long B, float *logits, float *features, uint8_t *digits, float *conf, void *stream)
{
    return cnn3_light_common(ctx, x, false, SV_GLUE_NORMALIZE, B, logits, features, digits, conf, stream);
}

extern "C" int sv_cnn3_light_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells, long B, int glue, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return cnn3_light_common(ctx, cells, true, glue, B, logits, nullptr, digits, conf, stream);
}

static int empty_common(sv_ctx *ctx, const void *x, bool u8in, int glue, long B, float *logit, void *stream)
{
    const int rc = light_prepare("sv_empty_forward", ctx, x, u8in, glue, B, logit, ctx ? &ctx->we : nullptr, "sv_load_weights_empty_f32", stream);
    if (rc) return rc == 1 ? SV_OK : rc;
    return svk_empty_forward(ctx, x, u8in, B, logit, S(stream));
}

extern "C" int sv_empty_forward_f32(sv_ctx *ctx, const float *x, long B, float *logit, void *stream)
{
    return empty_common(ctx, x, false, SV_GLUE_NORMALIZE, B, logit, stream);
}

extern "C" int sv_empty_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells, long B, int glue, float *logit, void *stream)
{
    return empty_common(ctx, cells, true, glue, B, logit, stream);
}

extern "C" int sv_resize_linear_u8(sv_ctx *ctx, const uint8_t *src, int sh, int sw, ptrdiff_t pitch, uint8_t *dst, int dh, int dw, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE(sh > 0 && sw > 0 && dh > 0 && dw > 0 && dh < 65536 && pitch >= sw, "bad shape");
    return svk_resize_linear(src, sh, sw, pitch, dst, dh, dw, S(stream));
}

extern "C" int sv_cell_ink_ratio_u8(sv_ctx *ctx, const uint8_t *cells, long B, int cell_px, float *ratio, int *otsu, void *stream)
{
    REQUIRE(ctx && cells && ratio, "NULL argument");
    REQUIRE(B > 0 && B < 2147483647L && cell_px > 0, "bad shape");
    return svk_cell_ink_ratio(cells, B, cell_px, ratio, otsu, S(stream));
}

extern "C" int sv_preprocess_cells_u8(sv_ctx *ctx, const uint8_t *cells, long B, uint8_t *out, void *stream)
{
    REQUIRE(ctx && cells && out, "NULL argument");
    REQUIRE(B > 0, "B must be positive");
    return svk_preprocess_cells(cells, B, out, S(stream));
}

extern "C" int sv_softmax_topk_f32(sv_ctx *ctx, const float *logits, long B, int k, uint8_t *index, float *prob, void *stream)
{
    REQUIRE(ctx && logits && index && prob, "NULL argument");
    REQUIRE(B > 0 && k >= 1 && k <= SV_CLASSES, "need B > 0 and 1 <= k <= 10");
    return svk_softmax_topk(logits, B, k, index, prob, S(stream));
}

extern "C" int sv_eval_metrics(sv_ctx *ctx, const float *input, int input_is_prob, const void *labels, int labels_i64, long B, long index_base, float temperature,
                               const double *bin_edges, int n_bins, int accumulate, float *probs, uint8_t *pred, float *conf, float *true_prob, float *nll,
                               uint8_t *correct, sv_eval_stats *stats, sv_eval_failure *failures, long max_failures, void *stream)
{
    REQUIRE(ctx && stats && bin_edges, "NULL argument");
    REQUIRE(B >= 0 && B < (1l << 32), "need 0 <= B and B * 2^30 < 2^62");
    REQUIRE(B == 0 || (input && labels), "NULL argument");
    REQUIRE(index_base >= 0, "index_base must not be negative");
    REQUIRE(std::isfinite(temperature) && temperature > 0.f, "temperature must be finite and positive");
    REQUIRE(!input_is_prob || temperature == 1.f, "probabilities take no temperature");
    REQUIRE(n_bins >= 1 && n_bins <= SV_EVAL_MAX_BINS, "need 1 <= n_bins <= 64");
    for (int i = 0; i <= n_bins; i++) REQUIRE(bin_edges[i] == bin_edges[i] && (i == 0 || bin_edges[i] >= bin_edges[i - 1]), "bin_edges must be non-decreasing");
    REQUIRE(max_failures >= 0 && (failures || max_failures == 0), "max_failures needs a failures buffer");
    REQUIRE((((uintptr_t)stats | (uintptr_t)failures | (labels_i64 ? (uintptr_t)labels : 0)) & 7) == 0, "misaligned argument");
    REQUIRE((((uintptr_t)input | (uintptr_t)labels | (uintptr_t)probs | (uintptr_t)conf | (uintptr_t)true_prob | (uintptr_t)nll) & 3) == 0, "misaligned argument");
    return svk_eval_metrics(ctx, input, input_is_prob != 0, labels, labels_i64 != 0, B, index_base, temperature, bin_edges, n_bins, accumulate != 0, probs, pred, conf,
                            true_prob, nll, correct, stats, failures, max_failures, S(stream));
}

extern "C" int sv_eval_metrics_host(sv_ctx *ctx, const float *input, int input_is_prob, const void *labels, int labels_i64, long B, long index_base, float temperature,
                                    const double *bin_edges, int n_bins, int accumulate, float *probs, uint8_t *pred, float *conf, float *true_prob, float *nll,
                                    uint8_t *correct, sv_eval_stats *stats, sv_eval_failure *failures, long max_failures, sv_eval_stats *stats_host, void *stream)
{
    REQUIRE(stats_host, "NULL argument");
    const int rc = sv_eval_metrics(ctx, input, input_is_prob, labels, labels_i64, B, index_base, temperature, bin_edges, n_bins, accumulate, probs, pred, conf, true_prob,
                                   nll, correct, stats, failures, max_failures, stream);
    if (rc) return rc;
    SV_HIP(hipMemcpyAsync(stats_host, stats, sizeof(sv_eval_stats), hipMemcpyDeviceToHost, S(stream)));
    SV_HIP(hipStreamSynchronize(S(stream)));
    if (stats_host->bad_labels)
        return sv_fail(SV_ERR_BAD_ARG, "%s: %llu labels outside 0..9 (the other cells are counted)", __func__, (unsigned long long)stats_host->bad_labels);
    return SV_OK;
}

extern "C" int sv_resolve_conflicts(sv_ctx *ctx, const uint8_t *index, const float *prob, long n, int k, int beam_width, int max_corrections,
                                    double min_alt_conf, int acceptance_rule, uint8_t *digits, float *conf, uint8_t *index_out, float *prob_out, uint8_t *success,
                                    int32_t *num_conflicts_before, int32_t *num_conflicts_after, uint8_t *conflict_count, uint8_t *n_corrections,
                                    uint8_t *corr_cells, float *corr_conf, int32_t *paths_explored, double *score, void *stream)
{
    REQUIRE(ctx, "NULL argument");
    REQUIRE(n >= 0 && n < (1l << 31), "n out of range");
    if (!(k >= 1 && k <= 4 && beam_width >= 1 && beam_width <= 6 && max_corrections >= 0 && max_corrections <= 3))
        return sv_fail(SV_ERR_UNSUPPORTED, "%s: need 1 <= k <= 4, 1 <= beam_width <= 6, 0 <= max_corrections <= 3 (one wave searches one frame)", __func__);
    if (n == 0) return SV_OK;
    REQUIRE(index && prob, "NULL argument");
    REQUIRE((((uintptr_t)prob | (uintptr_t)conf | (uintptr_t)prob_out | (uintptr_t)num_conflicts_before | (uintptr_t)num_conflicts_after |
              (uintptr_t)corr_conf | (uintptr_t)paths_explored) & 3) == 0 && ((uintptr_t)score & 7) == 0, "misaligned argument");
    return svk_resolve_conflicts(index, prob, n, k, beam_width, max_corrections, min_alt_conf, acceptance_rule != 0, digits, conf, index_out, prob_out, success,
                                 num_conflicts_before, num_conflicts_after, conflict_count, n_corrections, corr_cells, corr_conf, paths_explored,
                                 score, S(stream));
}

extern "C" int sv_propagate_constraints(sv_ctx *ctx, const uint8_t *digits, const float *conf, long n, int max_iterations, uint8_t *grid, uint16_t *candidates,
                                        uint8_t *is_valid, int32_t *iterations, uint8_t *contradiction_cell, uint8_t *n_resolved, uint8_t *resolved,
                                        uint8_t *is_fixed, void *stream)
{
    REQUIRE(ctx, "NULL argument");
    REQUIRE(n >= 0 && n < (1l << 31), "n out of range");
    if (!(max_iterations >= 1 && max_iterations <= 100))
        return sv_fail(SV_ERR_UNSUPPORTED, "%s: need 1 <= max_iterations <= 100", __func__);
    if (n == 0) return SV_OK;
    REQUIRE(digits, "NULL argument");
    REQUIRE((((uintptr_t)conf | (uintptr_t)iterations) & 3) == 0 && ((uintptr_t)candidates & 1) == 0, "misaligned argument");
    return svk_propagate_constraints(digits, conf, n, max_iterations, grid, candidates, is_valid, iterations, contradiction_cell, n_resolved, resolved, is_fixed,
                                     S(stream));
}

extern "C" int sv_solve_sudoku_batch(sv_ctx *ctx, const uint8_t *grid, const uint8_t *active, int n, int max_nodes, uint8_t *solution, int8_t *result,
                                     int32_t *nodes, void *stream)
{
    REQUIRE(ctx, "NULL argument");
    REQUIRE(n >= 0, "n out of range");
    REQUIRE(max_nodes >= 1 && max_nodes <= SV_SOLVE_MAX_NODES, "need 1 <= max_nodes <= 65536");
    if (n == 0) return SV_OK;
    REQUIRE(grid, "NULL argument");
    REQUIRE(((uintptr_t)nodes & 3) == 0, "misaligned argument");
    return svk_solve_sudoku_batch(grid, active, n, max_nodes, solution, result, nodes, S(stream));
}

extern "C" int sv_motion_update_u8(sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, int channels, ptrdiff_t pitch, ptrdiff_t frame_stride,
                                   const uint8_t *prev_small, float threshold, uint8_t *small, int32_t *counts, int dh, int dw, void *stream)
{
    REQUIRE(ctx && frames && small && counts, "NULL argument");
    REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    REQUIRE(n > 0 && n < 65536 && H > 0 && W > 0 && pitch >= (ptrdiff_t)W * channels, "bad shape");
    REQUIRE(n == 1 || frame_stride >= pitch * (H - 1) + (ptrdiff_t)W * channels, "frames overlap (frame_stride too small)");
    REQUIRE(dh > 0 && dw > 0 && (long)dh * dw <= 0x7fffff00L, "bad target size");
    REQUIRE(((uintptr_t)counts & 3) == 0, "misaligned counts");
    const long small_bytes = (long)n * dh * dw;
    REQUIRE(!prev_small || prev_small + (long)dh * dw <= small || small + small_bytes <= prev_small, "prev_small overlaps small");
    return svk_motion_update(ctx, frames, n, H, W, channels, pitch, frame_stride, prev_small, threshold, small, counts, dh, dw, S(stream));
}

extern "C" int sv_set_overlay_glyphs(sv_ctx *ctx, const uint8_t *atlas)
{
    REQUIRE(atlas, "NULL argument");
    // the zero margin first: nothing is uploaded from an atlas that lacks it
    for (int g = 0; g < 9; g++)
        for (int i = 0; i < SV_OVERLAY_CELL; i++)
            for (int j = 0; j < SV_OVERLAY_CELL; j++) {
                const bool margin = i < SV_OVERLAY_MARGIN || i >= SV_OVERLAY_CELL - SV_OVERLAY_MARGIN || j < SV_OVERLAY_MARGIN || j >= SV_OVERLAY_CELL - SV_OVERLAY_MARGIN;
                if (margin && atlas[(g * SV_OVERLAY_CELL + i) * SV_OVERLAY_CELL + j])
                    return sv_fail(SV_ERR_BAD_ARG, "%s: glyph %d has a non-zero texel at row %d, column %d of its margin (rows and columns 0..2 and 47..49 must be zero)",
                                   __func__, g, i, j);
            }
    REQUIRE(ctx, "NULL argument");
    return svk_set_overlay_glyphs(ctx, atlas);
}

extern "C" int sv_render_overlay_u8(sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *m,
                                    const uint8_t *digits, const uint8_t *classes, const uint8_t *palette, int k, const uint8_t *active, int shadow,
                                    uint8_t *dst, ptrdiff_t dst_pitch, ptrdiff_t dst_stride, void *stream)
{
    REQUIRE(ctx && frames && m && digits && dst, "NULL argument");
    REQUIRE_FRAMES();
    REQUIRE(H <= 16 * 65535, "bad shape");
    REQUIRE(dst_pitch >= 3 * (ptrdiff_t)W, "bad shape");
    const ptrdiff_t row = 3 * (ptrdiff_t)W;
    REQUIRE(n == 1 || (img_stride >= pitch * (H - 1) + row && dst_stride >= dst_pitch * (H - 1) + row), "frames overlap (stride too small)");
    REQUIRE(!palette || (k >= 1 && k <= 256), "need 1 <= k <= 256");
    REQUIRE(((uintptr_t)m & 7) == 0, "misaligned m");
    if (!ctx->overlay_set) return sv_fail(SV_ERR_NO_WEIGHTS, "%s: no glyph atlas (sv_set_overlay_glyphs)", __func__);
    if (dst != frames) {
        const uint8_t *src_end = frames + img_stride * (n - 1) + pitch * (H - 1) + row, *dst_end = dst + dst_stride * (n - 1) + dst_pitch * (H - 1) + row;
        REQUIRE(dst_end <= frames || src_end <= dst, "dst overlaps frames (pass dst == frames to draw in place)");
        // the rest of the frame is a copy: all of it is copied, then the blocks the grid reaches are drawn in place
        if (n == 1 || (img_stride == pitch * H && dst_stride == dst_pitch * H))
            SV_HIP(hipMemcpy2DAsync(dst, (size_t)dst_pitch, frames, (size_t)pitch, (size_t)row, (size_t)n * H, hipMemcpyDeviceToDevice, S(stream)));
        else
            for (int f = 0; f < n; f++)
                SV_HIP(hipMemcpy2DAsync(dst + f * dst_stride, (size_t)dst_pitch, frames + f * img_stride, (size_t)pitch, (size_t)row, (size_t)H,
                                        hipMemcpyDeviceToDevice, S(stream)));
    } else {
        REQUIRE(dst_pitch == pitch && (n == 1 || dst_stride == img_stride), "in place: dst_pitch and dst_stride must equal pitch and img_stride");
    }
    return svk_render_overlay(ctx, dst, n, H, W, dst_pitch, dst_stride, m, digits, classes, palette, palette ? k : 3, active, shadow != 0, S(stream));
}

extern "C" int sv_frame_quality_stats_u8(sv_ctx *ctx, const uint8_t *img, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int channels,
                                         int64_t *lap_sum, int64_t *lap_sqsum, uint32_t *hist, void *stream)
{
    REQUIRE(ctx && img && lap_sum && lap_sqsum && hist, "NULL argument");
    REQUIRE(channels == 1 || channels == 3, "channels must be 1 or 3");
    REQUIRE(n > 0 && n < 65536 && H > 0 && W > 0 && pitch >= (ptrdiff_t)W * channels, "bad shape");
    REQUIRE(n == 1 || img_stride >= pitch * (H - 1) + (ptrdiff_t)W * channels, "frames overlap (img_stride too small)");
    REQUIRE((((uintptr_t)lap_sum | (uintptr_t)lap_sqsum) & 7) == 0 && ((uintptr_t)hist & 3) == 0, "misaligned output");
    return svk_frame_quality_stats(img, n, H, W, pitch, img_stride, channels, (long long *)lap_sum, (long long *)lap_sqsum, hist, S(stream));
}

extern "C" int sv_grid_line_coverage_u8(sv_ctx *ctx, const uint8_t *binary, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *minv,
                                        uint32_t *counts, void *stream)
{
    REQUIRE(ctx && binary && minv && counts, "NULL argument");
    REQUIRE(n > 0 && n < 65536 && H > 0 && W > 0 && pitch >= (ptrdiff_t)W, "bad shape");
    REQUIRE(((uintptr_t)minv & 7) == 0 && ((uintptr_t)counts & 3) == 0, "misaligned argument");
    return svk_grid_line_coverage(binary, false, n, H, W, pitch, img_stride, minv, counts, S(stream));
}

extern "C" int sv_grid_line_coverage_bits(sv_ctx *ctx, const uint32_t *bits, int n, int H, int W, const double *minv, uint32_t *counts, void *stream)
{
    REQUIRE(ctx && bits && minv && counts, "NULL argument");
    REQUIRE(n > 0 && n < 65536 && H > 0 && W > 0 && W % 32 == 0, "bad shape (W must be a multiple of 32)");
    REQUIRE((((uintptr_t)bits | (uintptr_t)counts) & 3) == 0 && ((uintptr_t)minv & 7) == 0, "misaligned argument");
    return svk_grid_line_coverage(bits, true, n, H, W, 0, 0, minv, counts, S(stream));
}

// ---- K7: cv/preprocess_v2.py ---------------------------------------------------------------------------
// one gray plane set: n frames of H x W, `pitch` bytes between rows, `img_stride` between frames; 65535 = the grid's y / z limit
#define REQUIRE_PLANES() \
    do { \
        REQUIRE(n > 0 && n < 65536 && H > 0 && H < 65536 && W > 0 && pitch >= (ptrdiff_t)W, "bad shape"); \
        REQUIRE(n == 1 || img_stride >= pitch * (H - 1) + (ptrdiff_t)W, "frames overlap (img_stride too small)"); \
    } while (0)

extern "C" int sv_morphology_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int op, int shape, int ksize,
                                uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(op >= SV_MORPH_DILATE && op <= SV_MORPH_OPEN, "op must be SV_MORPH_DILATE, _ERODE, _CLOSE or _OPEN");
    REQUIRE(shape == SV_SHAPE_RECT || shape == SV_SHAPE_ELLIPSE, "shape must be SV_SHAPE_RECT or SV_SHAPE_ELLIPSE");
    REQUIRE(ksize >= 1, "ksize must be positive");
    return svk_morphology(ctx, src, n, H, W, pitch, img_stride, op, shape, ksize, dst, S(stream));
}

extern "C" int sv_box_mean_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int ksize, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(ksize > 0 && (ksize & 1), "ksize must be odd and positive");
    return svk_box_mean(src, n, H, W, pitch, img_stride, ksize, dst, S(stream));
}

extern "C" int sv_gaussian_blur21_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE_PLANES();
    return svk_gaussian_blur21(src, n, H, W, pitch, img_stride, dst, S(stream));
}

extern "C" int sv_divide_normalize_u8(sv_ctx *ctx, const uint8_t *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const uint8_t *background,
                                      uint8_t *dst, void *stream)
{
    REQUIRE(ctx && gray && background && dst, "NULL argument");
    REQUIRE_PLANES();
    return svk_divide_normalize(gray, n, H, W, pitch, img_stride, background, dst, S(stream));
}

extern "C" int sv_clahe_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, double clip_limit, int tiles_x, int tiles_y,
                           uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(tiles_x > 0 && tiles_y > 0 && tiles_x * tiles_y <= 65535 && clip_limit == clip_limit, "bad tile grid or clip limit");
    return svk_clahe(ctx, src, n, H, W, pitch, img_stride, clip_limit, tiles_x, tiles_y, dst, S(stream));
}

extern "C" int sv_threshold_sauvola_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int window, double k,
                                       uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && dst, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(window > 0 && (window & 1), "window must be odd and positive");
    return svk_threshold_sauvola(src, n, H, W, pitch, img_stride, window, k, dst, S(stream));
}

extern "C" int sv_threshold_count_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int thresh, int type_inv,
                                     uint8_t *dst, uint32_t *counts, void *stream)
{
    REQUIRE(ctx && src && dst && counts, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(((uintptr_t)counts & 3) == 0, "misaligned counts");
    return svk_threshold_count(src, n, H, W, pitch, img_stride, thresh, type_inv ? 1 : 0, dst, counts, S(stream));
}

extern "C" int sv_shadow_mask_u8(sv_ctx *ctx, const uint8_t *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const uint8_t *local_mean, int delta,
                                 uint8_t *mask, uint32_t *counts, void *stream)
{
    REQUIRE(ctx && gray && local_mean && mask && counts, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(((uintptr_t)counts & 3) == 0, "misaligned counts");
    return svk_shadow_mask(gray, n, H, W, pitch, img_stride, local_mean, delta, mask, counts, S(stream));
}

extern "C" int sv_count_nonzero_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint32_t *counts, void *stream)
{
    REQUIRE(ctx && src && counts, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(((uintptr_t)counts & 3) == 0, "misaligned counts");
    return svk_count_nonzero(src, n, H, W, pitch, img_stride, counts, S(stream));
}

// ---- K13: cv/grid_v2.py ---------------------------------------------------------------------------------
extern "C" int sv_harris_corners_u8(sv_ctx *ctx, const uint8_t *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int max_corners,
                                    double quality_level, int min_distance, double k, int cand_capacity, float *corners, int *counts, float *response, void *stream)
{
    REQUIRE(ctx && gray && corners && counts, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(H >= 3 && W >= 3, "a frame must be at least 3x3");
    // with REQUIRE_PLANES' H < 65536: k_harris_select keeps a corner as x | y << 16, and the raster index y * W + x fits 32 bits
    REQUIRE(W < 65536, "W must be below 65536");
    REQUIRE(max_corners >= 1 && max_corners <= SV_HARRIS_MAX_CORNERS, "max_corners must be in 1..SV_HARRIS_MAX_CORNERS");
    REQUIRE(quality_level >= 0 && quality_level <= 1 && min_distance >= 0 && min_distance < 32768 && k == k, "bad quality_level, min_distance or k");
    REQUIRE(cand_capacity >= 1 && cand_capacity <= (1 << 24), "cand_capacity must be in 1..2^24");
    REQUIRE((((uintptr_t)corners | (uintptr_t)counts | (uintptr_t)response) & 3) == 0, "misaligned argument");
    return svk_harris_corners(ctx, gray, n, H, W, pitch, img_stride, max_corners, quality_level, min_distance, k, cand_capacity, corners, counts, response, S(stream));
}

extern "C" int sv_warp_affine_u8(sv_ctx *ctx, const uint8_t *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *M, int dst_h, int dst_w,
                                 int border_value, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && M && dst, "NULL argument");
    REQUIRE_PLANES();
    REQUIRE(W < 32768 && H < 32768, "source larger than cv2's 16-bit coordinates");
    REQUIRE(dst_h > 0 && dst_h < 65536 && dst_w > 0 && dst_w < 65536, "bad destination size");
    REQUIRE(border_value >= 0 && border_value <= 255, "border_value must be in 0..255");
    REQUIRE(((uintptr_t)M & 7) == 0, "misaligned matrices");
    return svk_warp_affine(ctx, src, n, H, W, pitch, img_stride, M, dst_h, dst_w, border_value, dst, S(stream));
}

static int jpeg_info_ok(const sv_jpeg_info *info, ptrdiff_t pitch, const char *fn, int denom, int channels = 3)
{
    const char *what = nullptr;
    const bool swap = info->orientation >= 5;
    if (!(info->width > 0 && info->height > 0 && info->width < 65536 && info->height < 65536)) what = "bad image size";
    else if (!(info->components == 1 || info->components == 3)) what = "components must be 1 or 3";
    else if (!((info->h_samp == 1 && info->v_samp == 1) || (info->h_samp == 2 && (info->v_samp == 1 || info->v_samp == 2)))) what = "sampling must be 1x1, 2x1 or 2x2";
    else if (!(info->orientation >= 1 && info->orientation <= 8)) what = "orientation must be 1..8";
    else if (!(info->out_width == (swap ? info->height : info->width) && info->out_height == (swap ? info->width : info->height))) what = "out_width/out_height do not match the orientation";
    else if (pitch < channels * (ptrdiff_t)((info->out_width + denom - 1) / denom)) what = "pitch smaller than a row";
    return what ? sv_fail(SV_ERR_BAD_ARG, "%s: %s", fn, what) : SV_OK;
}

static bool jpeg_scale_ok(int d) { return d == 1 || d == 2 || d == 4 || d == 8; }

extern "C" int sv_jpeg_scaled_size(const sv_jpeg_info *info, int scale_denom, int *out_width, int *out_height)
{
    REQUIRE(jpeg_scale_ok(scale_denom), "scale_denom must be 1, 2, 4 or 8");
    REQUIRE(info && out_width && out_height, "NULL argument");
    *out_width = (info->out_width + scale_denom - 1) / scale_denom;
    *out_height = (info->out_height + scale_denom - 1) / scale_denom;
    return SV_OK;
}

// The four reconstruct entries.  dense: coef, else masks, offsets and values.  Only a scaled entry can come with a bad scale_denom; at
// scale_denom 1 a scaled entry is the unscaled one, and reports its errors under that name.
static int jpeg_reconstruct(bool dense, sv_ctx *ctx, const sv_jpeg_info *info, const int16_t *coef, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                            const uint16_t *quant, uint8_t *bgr, ptrdiff_t pitch, void *stream, int scale_denom)
{
    static const char *const entry[2][2] = {{"sv_jpeg_reconstruct_sparse_bgr_u8", "sv_jpeg_reconstruct_sparse_scaled_bgr_u8"},
                                            {"sv_jpeg_reconstruct_bgr_u8", "sv_jpeg_reconstruct_scaled_bgr_u8"}};
    REQUIRE_AS(entry[dense][1], jpeg_scale_ok(scale_denom), "scale_denom must be 1, 2, 4 or 8");
    const char *fn = entry[dense][scale_denom != 1];
    REQUIRE_AS(fn, ctx && info && (dense ? coef != nullptr : masks && offsets && values) && quant && bgr, "NULL argument");
    const int rc = jpeg_info_ok(info, pitch, fn, scale_denom);
    if (rc) return rc;
    if (dense) REQUIRE_AS(fn, ((uintptr_t)coef & 15) == 0 && ((uintptr_t)quant & 15) == 0, "coef and quant must be 16-byte aligned");
    else REQUIRE_AS(fn, ((uintptr_t)masks & 7) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)values & 1) == 0 && ((uintptr_t)quant & 15) == 0, "misaligned argument");
    return svk_jpeg_reconstruct(ctx, info, scale_denom, coef, masks, offsets, values, quant, bgr, pitch, S(stream), fn);
}

extern "C" int sv_jpeg_reconstruct_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const int16_t *coef, const uint16_t *quant, uint8_t *bgr, ptrdiff_t pitch, void *stream)
{
    return jpeg_reconstruct(true, ctx, info, coef, nullptr, nullptr, nullptr, quant, bgr, pitch, stream, 1);
}

extern "C" int sv_jpeg_reconstruct_sparse_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                                                 const uint16_t *quant, uint8_t *bgr, ptrdiff_t pitch, void *stream)
{
    return jpeg_reconstruct(false, ctx, info, nullptr, masks, offsets, values, quant, bgr, pitch, stream, 1);
}

extern "C" int sv_jpeg_reconstruct_scaled_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const int16_t *coef, const uint16_t *quant, uint8_t *bgr, ptrdiff_t pitch, void *stream,
                                                 int scale_denom)
{
    return jpeg_reconstruct(true, ctx, info, coef, nullptr, nullptr, nullptr, quant, bgr, pitch, stream, scale_denom);
}

extern "C" int sv_jpeg_reconstruct_sparse_scaled_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                                                        const uint16_t *quant, uint8_t *bgr, ptrdiff_t pitch, void *stream, int scale_denom)
{
    return jpeg_reconstruct(false, ctx, info, nullptr, masks, offsets, values, quant, bgr, pitch, stream, scale_denom);
}

// The two luma-only reconstruct entries (cv2.IMREAD_GRAYSCALE, IMREAD_REDUCED_GRAYSCALE_*).  info: sv_jpeg_parse_luma's
static int jpeg_reconstruct_gray(bool dense, const sv_jpeg_info *info, const int16_t *coef, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                                 const uint16_t *quant, uint8_t *gray, ptrdiff_t pitch, void *stream, int scale_denom)
{
    const char *fn = dense ? "sv_jpeg_reconstruct_gray_u8" : "sv_jpeg_reconstruct_sparse_gray_u8";
    REQUIRE_AS(fn, jpeg_scale_ok(scale_denom), "scale_denom must be 1, 2, 4 or 8");
    REQUIRE_AS(fn, info && (dense ? coef != nullptr : masks && offsets && values) && quant && gray, "NULL argument");
    const int rc = jpeg_info_ok(info, pitch, fn, scale_denom, 1);
    if (rc) return rc;
    if (dense) REQUIRE_AS(fn, ((uintptr_t)coef & 15) == 0 && ((uintptr_t)quant & 15) == 0, "coef and quant must be 16-byte aligned");
    else REQUIRE_AS(fn, ((uintptr_t)masks & 7) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)values & 1) == 0 && ((uintptr_t)quant & 15) == 0, "misaligned argument");
    return svk_jpeg_reconstruct_gray(info, scale_denom, coef, masks, offsets, values, quant, gray, pitch, S(stream), fn);
}

extern "C" int sv_jpeg_reconstruct_gray_u8(sv_ctx *ctx, const sv_jpeg_info *info, const int16_t *coef, const uint16_t *quant, uint8_t *gray, ptrdiff_t pitch, void *stream,
                                           int scale_denom)
{
    REQUIRE(ctx, "NULL argument");
    return jpeg_reconstruct_gray(true, info, coef, nullptr, nullptr, nullptr, quant, gray, pitch, stream, scale_denom);
}

extern "C" int sv_jpeg_reconstruct_sparse_gray_u8(sv_ctx *ctx, const sv_jpeg_info *info, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                                                  const uint16_t *quant, uint8_t *gray, ptrdiff_t pitch, void *stream, int scale_denom)
{
    REQUIRE(ctx, "NULL argument");
    return jpeg_reconstruct_gray(false, info, nullptr, masks, offsets, values, quant, gray, pitch, stream, scale_denom);
}

// The two forward entries of the encoder; channels 3 (BGR) or 1 (gray)
static int jpeg_forward(const char *fn, int channels, sv_ctx *ctx, const sv_jpeg_enc *plan, const uint8_t *src, int n, ptrdiff_t pitch, ptrdiff_t img_stride, int16_t *coef,
                        uint64_t *masks, uint32_t *offsets, int16_t *values, uint32_t *counts, void *stream)
{
    REQUIRE_AS(fn, ctx && plan && src, "NULL argument");
    const bool any = masks || offsets || values || counts, all = masks && offsets && values && counts;
    REQUIRE_AS(fn, any == all, "masks, offsets, values and counts come together");
    REQUIRE_AS(fn, coef || all, "no output asked for");
    REQUIRE_AS(fn, n > 0 && n < 65536, "n must be in 1..65535");
    const sv_jpeg_info &info = plan->info;
    sv_jpeg_enc want;                                               // a plan is only ever what sv_jpeg_encode_plan made of its six arguments
    const int sampling = info.h_samp == 1 ? SV_JPEG_444 : info.v_samp == 1 ? SV_JPEG_422 : SV_JPEG_420;
    if (sv_jpeg_encode_plan(info.width, info.height, info.components, sampling, plan->quality, info.restart_interval, &want) != SV_OK ||
        memcmp(want.quant, plan->quant, sizeof want.quant) != 0 || memcmp(want.recip, plan->recip, sizeof want.recip) != 0 || want.out_bound != plan->out_bound ||
        want.info.h_samp != info.h_samp || want.info.v_samp != info.v_samp ||      // the kernels size their tiles by these: v_samp 3 must not reach them
        want.info.coef_count != info.coef_count || want.info.sparse_capacity != info.sparse_capacity || want.info.orientation != info.orientation ||
        want.info.out_width != info.out_width || want.info.out_height != info.out_height)
        return sv_fail(SV_ERR_BAD_ARG, "%s: the plan was not made by sv_jpeg_encode_plan", fn);
    REQUIRE_AS(fn, info.components == channels, channels == 3 ? "a BGR frame needs a plan of 3 components" : "a gray frame needs a plan of 1 component");
    REQUIRE_AS(fn, pitch >= (ptrdiff_t)channels * info.width, "pitch smaller than a row");
    REQUIRE_AS(fn, n == 1 || img_stride >= pitch * (ptrdiff_t)(info.height - 1) + (ptrdiff_t)channels * info.width, "frames overlap");
    REQUIRE_AS(fn, ((uintptr_t)coef & 15) == 0 && ((uintptr_t)masks & 7) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)values & 1) == 0 && ((uintptr_t)counts & 3) == 0,
               "misaligned output");
    return svk_jpeg_forward(ctx, plan, src, channels, n, pitch, img_stride, coef, masks, offsets, values, counts, S(stream));
}

extern "C" int sv_jpeg_forward_bgr_u8(sv_ctx *ctx, const sv_jpeg_enc *plan, const uint8_t *bgr, int n, ptrdiff_t pitch, ptrdiff_t img_stride, int16_t *coef, uint64_t *masks,
                                      uint32_t *offsets, int16_t *values, uint32_t *counts, void *stream)
{
    return jpeg_forward("sv_jpeg_forward_bgr_u8", 3, ctx, plan, bgr, n, pitch, img_stride, coef, masks, offsets, values, counts, stream);
}

extern "C" int sv_jpeg_forward_gray_u8(sv_ctx *ctx, const sv_jpeg_enc *plan, const uint8_t *gray, int n, ptrdiff_t pitch, ptrdiff_t img_stride, int16_t *coef, uint64_t *masks,
                                       uint32_t *offsets, int16_t *values, uint32_t *counts, void *stream)
{
    return jpeg_forward("sv_jpeg_forward_gray_u8", 1, ctx, plan, gray, n, pitch, img_stride, coef, masks, offsets, values, counts, stream);
}

// The two deflate entries of the PNG encoder; channels 3 (BGR) or 1 (gray)
static int png_deflate(const char *fn, int channels, sv_ctx *ctx, const sv_png_enc *plan, const uint8_t *src, int n, ptrdiff_t pitch, ptrdiff_t frame_stride, uint8_t *stream_out,
                       uint32_t *band_len, uint32_t *adler, uint32_t *status, void *stream)
{
    REQUIRE_AS(fn, ctx && plan && src && stream_out && band_len && adler && status, "NULL argument");
    REQUIRE_AS(fn, n > 0 && n < 65536, "n must be in 1..65535");
    sv_png_enc want;                                                // a plan is only ever what sv_png_encode_plan made of its six arguments
    if (sv_png_encode_plan(plan->width, plan->height, plan->channels, plan->filter, plan->strategy, plan->band_rows, &want) != SV_OK || want.band_rows != plan->band_rows ||
        want.bands != plan->bands || want.row_bytes != plan->row_bytes || want.filtered_bytes != plan->filtered_bytes || want.slot_bytes != plan->slot_bytes ||
        want.stream_bound != plan->stream_bound || want.out_bound != plan->out_bound)
        return sv_fail(SV_ERR_BAD_ARG, "%s: the plan was not made by sv_png_encode_plan", fn);
    REQUIRE_AS(fn, plan->channels == channels, channels == 3 ? "a BGR frame needs a plan of 3 channels" : "a gray frame needs a plan of 1 channel");
    REQUIRE_AS(fn, pitch >= (ptrdiff_t)channels * plan->width, "pitch smaller than a row");
    REQUIRE_AS(fn, n == 1 || frame_stride >= pitch * (ptrdiff_t)(plan->height - 1) + (ptrdiff_t)channels * plan->width, "frames overlap");
    REQUIRE_AS(fn, ((uintptr_t)band_len & 3) == 0 && ((uintptr_t)adler & 3) == 0 && ((uintptr_t)status & 3) == 0, "misaligned output");
    return svk_png_deflate(ctx, plan, src, n, pitch, frame_stride, stream_out, band_len, adler, status, S(stream));
}

extern "C" int sv_png_deflate_bgr_u8(sv_ctx *ctx, const sv_png_enc *plan, const uint8_t *bgr, int n, ptrdiff_t pitch, ptrdiff_t frame_stride, uint8_t *stream_out,
                                     uint32_t *band_len, uint32_t *adler, uint32_t *status, void *stream)
{
    return png_deflate("sv_png_deflate_bgr_u8", 3, ctx, plan, bgr, n, pitch, frame_stride, stream_out, band_len, adler, status, stream);
}

extern "C" int sv_png_deflate_gray_u8(sv_ctx *ctx, const sv_png_enc *plan, const uint8_t *gray, int n, ptrdiff_t pitch, ptrdiff_t frame_stride, uint8_t *stream_out,
                                      uint32_t *band_len, uint32_t *adler, uint32_t *status, void *stream)
{
    return png_deflate("sv_png_deflate_gray_u8", 1, ctx, plan, gray, n, pitch, frame_stride, stream_out, band_len, adler, status, stream);
}

// The PNG decoder's device half; channels 3 (BGR) or 1 (gray).  Only the geometry of the info is used, and only one sv_png_parse could have produced.
static int png_reconstruct(const char *fn, int channels, sv_ctx *ctx, const sv_png_info *info, const uint8_t *filtered, const uint8_t *row_filter, const uint8_t *palette, int n,
                           uint8_t *out, ptrdiff_t pitch, ptrdiff_t frame_stride, uint32_t *status, void *stream)
{
    REQUIRE_AS(fn, ctx && info && filtered && row_filter && out && status, "NULL argument");
    REQUIRE_AS(fn, n > 0 && n < 65536, "n must be in 1..65535");
    REQUIRE_AS(fn, sv_png_geometry_ok(info), "the info was not made by sv_png_parse");
    const int type = info->color_type;
    REQUIRE_AS(fn, type != 3 || palette, "colour type 3 needs a palette");
    REQUIRE_AS(fn, pitch >= channels * (ptrdiff_t)info->width, "pitch smaller than a row");
    REQUIRE_AS(fn, n == 1 || frame_stride >= pitch * (ptrdiff_t)(info->height - 1) + channels * (ptrdiff_t)info->width, "frames overlap");
    REQUIRE_AS(fn, ((uintptr_t)status & 3) == 0 && ((uintptr_t)palette & 3) == 0, "misaligned status or palette");
    return svk_png_reconstruct(ctx, info, filtered, row_filter, type == 3 ? palette : nullptr, n, out, pitch, frame_stride, status, channels == 1, S(stream));
}

extern "C" int sv_png_reconstruct_bgr_u8(sv_ctx *ctx, const sv_png_info *info, const uint8_t *filtered, const uint8_t *row_filter, const uint8_t *palette, int n, uint8_t *out,
                                         ptrdiff_t pitch, ptrdiff_t frame_stride, uint32_t *status, void *stream)
{
    return png_reconstruct("sv_png_reconstruct_bgr_u8", 3, ctx, info, filtered, row_filter, palette, n, out, pitch, frame_stride, status, stream);
}

extern "C" int sv_png_reconstruct_gray_u8(sv_ctx *ctx, const sv_png_info *info, const uint8_t *filtered, const uint8_t *row_filter, const uint8_t *palette, int n, uint8_t *out,
                                          ptrdiff_t pitch, ptrdiff_t frame_stride, uint32_t *status, void *stream)
{
    return png_reconstruct("sv_png_reconstruct_gray_u8", 1, ctx, info, filtered, row_filter, palette, n, out, pitch, frame_stride, status, stream);
}

// ---- K24: PNG cell data sets to model input (k24_dataset_cells.hip; the record rules live in sv_dataset_rec.h) ----
extern "C" int sv_dataset_cells(sv_ctx *ctx, const uint8_t *filtered, size_t filtered_size, const sv_dataset_record *records, long n, const uint8_t *palettes, int n_palettes,
                                int mode, uint8_t *out_u8, float *out_f32, uint32_t *status, void *stream)
{
    REQUIRE(ctx && filtered && records && status, "NULL argument");
    REQUIRE(out_u8 || out_f32, "at least one of out_u8 and out_f32 is needed");
    REQUIRE(n >= 1 && n <= 0x7fffffffL / 784, "n must be at least 1 and n * 784 below 2^31");
    REQUIRE(mode == SV_CELLS_GRAY || mode == SV_CELLS_DATASET, "mode must be SV_CELLS_GRAY or SV_CELLS_DATASET");
    REQUIRE(n_palettes >= 0 && n_palettes < SV_CELLS_NO_PALETTE && (n_palettes == 0 || palettes), "n_palettes must be 0 .. 65534, with palettes when above 0");
    REQUIRE((uintptr_t)records % 8 == 0 && (uintptr_t)status % 4 == 0 && (uintptr_t)out_f32 % 4 == 0 && (uintptr_t)palettes % 4 == 0, "misaligned records, status, out_f32 or palettes");
    return svk_dataset_cells(ctx, filtered, filtered_size, records, n, n_palettes ? palettes : nullptr, n_palettes, mode, out_u8, out_f32, status, S(stream));
}

extern "C" int sv_dataset_check_records(const sv_dataset_record *records, long n, size_t filtered_size, int n_palettes)
{
    REQUIRE(records && n >= 1, "NULL records or n below 1");
    for (long i = 0; i < n; i++) {
        svds::Geom g;
        const char *why = svds::refuse(records[i], filtered_size, n_palettes, g);
        if (why) return sv_fail(SV_ERR_BAD_ARG, "sv_dataset_check_records: record %ld: %s", i, why);
    }
    return SV_OK;
}

// K2 into the caller's cells (or the context's), then the forward `model` selects: 0 DigitCNN, 1 DigitCNNv3, 2 DigitCNNv3Light
static int frames_to_digits(const char *fn, int model, sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv,
                            int glue, uint8_t *cells, float *logits, uint8_t *digits, float *conf, void *stream)
{
    REQUIRE_AS(fn, ctx && frames && minv && logits && digits, "NULL argument");
    REQUIRE_AS(fn, frames_ok(n, H, W, pitch), "bad shape");
    static const char *const loader[3] = {"sv_load_weights_f32", "sv_load_weights_v3_f32", "sv_load_weights_v3_light_f32"};
    if (!(model == 2 ? ctx->wl.loaded : model == 1 ? ctx->w3.loaded : ctx->w.loaded)) return sv_fail(SV_ERR_NO_WEIGHTS, "%s: call %s first", fn, loader[model]);
    const long B = (long)n * SV_CELLS;
    int rc = sv_ensure_scratch(ctx, B);
    if (rc) return rc;
    uint8_t *c = cells ? cells : ctx->cells.as<u8>();
    if ((rc = svk_warp_cells(ctx, frames, n, H, W, pitch, frame_stride, minv, c, S(stream)))) return rc;
    if (model == 2) return cnn3_light_common(ctx, c, true, glue, B, logits, nullptr, digits, conf, stream);
    return model == 1 ? cnn3_common(ctx, c, true, glue, B, logits, nullptr, digits, conf, stream) : cnn_common(ctx, c, true, glue, B, logits, digits, conf, stream);
}

extern "C" int sv_frames_to_digits(sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv, int glue, uint8_t *cells, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return frames_to_digits("sv_frames_to_digits", 0, ctx, frames, n, H, W, pitch, frame_stride, minv, glue, cells, logits, digits, conf, stream);
}

extern "C" int sv_frames_to_digits_v3(sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv, int glue, uint8_t *cells, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return frames_to_digits("sv_frames_to_digits_v3", 1, ctx, frames, n, H, W, pitch, frame_stride, minv, glue, cells, logits, digits, conf, stream);
}

extern "C" int sv_frames_to_digits_v3_light(sv_ctx *ctx, const uint8_t *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv, int glue, uint8_t *cells, float *logits, uint8_t *digits, float *conf, void *stream)
{
    return frames_to_digits("sv_frames_to_digits_v3_light", 2, ctx, frames, n, H, W, pitch, frame_stride, minv, glue, cells, logits, digits, conf, stream);
}

// ---- K22: data augmentation (k22_augment.hip; the host rules live in sv_augment_host.h) ----
extern "C" int sv_augment_u8(sv_ctx *ctx, const uint8_t *src, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const sv_aug_step *steps,
                             const int32_t *n_steps, const int32_t *src_index, long n_out, uint64_t seed, long index_base, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && src && steps && n_steps && src_index && dst, "NULL argument");
    REQUIRE(n_src >= 1 && n_out >= 1 && n_out <= 0x7fffffffL, "n_src and n_out must be at least 1 (n_out below 2^31)");
    REQUIRE(H >= 4 && W >= 4 && H <= SV_AUG_MAX_SIDE && W <= SV_AUG_MAX_SIDE, "sides must be 4 .. SV_AUG_MAX_SIDE");
    REQUIRE(pitch >= W && (n_src == 1 || img_stride >= pitch * (H - 1) + W), "bad pitch or image stride");
    REQUIRE(index_base >= 0 && index_base < (1L << 56) - n_out, "index_base + n_out must stay below 2^56");
    REQUIRE((uintptr_t)steps % 8 == 0, "steps must be 8-byte aligned");
    return svk_augment(ctx, src, n_src, H, W, pitch, img_stride, steps, n_steps, src_index, n_out, seed, index_base, dst, S(stream));
}

extern "C" int sv_augment_check_program(const sv_aug_step *steps, const int32_t *n_steps, const int32_t *src_index, long n_out, int n_src, int H, int W)
{
    char msg[256];
    const int rc = sv_aug_check_program(steps, n_steps, src_index, n_out, n_src, H, W, msg, sizeof msg);
    return rc ? sv_fail(rc, "sv_augment_check_program: %s", msg) : SV_OK;
}

extern "C" int sv_augment_rotation_matrix(double cx, double cy, double angle_deg, double scale, double *m)
{
    REQUIRE(m, "NULL argument");
    sv_aug_rotation_matrix(cx, cy, angle_deg, scale, m);
    return SV_OK;
}

extern "C" int sv_augment_perspective_matrix(const float *src, const float *dst, double *m)
{
    REQUIRE(src && dst && m, "NULL argument");
    if (!sv_perspective_transform(src, dst, m)) return sv_fail(SV_ERR_DEGENERATE, "sv_augment_perspective_matrix: the points define no homography");
    return SV_OK;
}

extern "C" int sv_augment_elastic_taps(double sigma, float *taps, int cap, int *radius)
{
    REQUIRE(taps && radius, "NULL argument");
    const int r = sv_aug_elastic_radius(sigma);
    REQUIRE(r >= 0, "sigma must be positive and finite");
    *radius = r;
    if (cap < r + 1) return sv_fail(SV_ERR_BUFFER, "sv_augment_elastic_taps: sigma %g needs %d taps, room for %d", sigma, r + 1, cap);
    sv_aug_elastic_taps(sigma, r, taps);
    return SV_OK;
}

extern "C" int sv_augment_field_host(uint64_t seed, long index, int slot, uint32_t salt, int H, int W, uint32_t *words)
{
    REQUIRE(words, "NULL argument");
    REQUIRE(H >= 1 && W >= 1 && H <= SV_AUG_MAX_SIDE && W <= SV_AUG_MAX_SIDE, "sides must be 1 .. SV_AUG_MAX_SIDE");
    REQUIRE(index >= 0 && index < (1L << 56) && slot >= 0 && slot < 256, "index or slot outside the counter layout");
    for (int p = 0; p < H * W; p++) {
        const sv_philox4 w = sv_aug_draw(seed, (uint64_t)index, slot, salt, (uint32_t)p);
        for (int k = 0; k < 4; k++) words[4 * p + k] = w.v[k];
    }
    return SV_OK;
}

// ---- K23: synthetic digit cells (k23_synth_cells.hip; the host rules live in sv_synth_host.h) ----
extern "C" int sv_synth_cells_u8(sv_ctx *ctx, const sv_syn_cell *cells, const sv_aug_step *steps, const int32_t *n_steps, long n_out, int size, const uint8_t *atlas,
                                 const int32_t *atlas_dims, int n_slots, uint64_t seed, long index_base, uint8_t *dst, void *stream)
{
    REQUIRE(ctx && cells && steps && n_steps && dst, "NULL argument");
    REQUIRE(n_out >= 1 && n_out <= 0x7fffffffL, "n_out must be at least 1 and below 2^31");
    REQUIRE(size >= 4 && size <= SV_AUG_MAX_SIDE, "size must be 4 .. SV_AUG_MAX_SIDE");
    REQUIRE(n_slots >= 0 && n_slots <= (1 << 20) && (n_slots == 0 || (atlas && atlas_dims)), "n_slots must be 0 .. 2^20, with an atlas and its dims when above 0");
    REQUIRE(index_base >= 0 && index_base < (1L << 56) - n_out, "index_base + n_out must stay below 2^56");
    REQUIRE((uintptr_t)steps % 8 == 0 && (uintptr_t)cells % 8 == 0, "cells and steps must be 8-byte aligned");
    return svk_synth_cells(ctx, cells, steps, n_steps, n_out, size, atlas, atlas_dims, n_slots, seed, index_base, dst, S(stream));
}

extern "C" int sv_synth_check_program(const sv_syn_cell *cells, const sv_aug_step *steps, const int32_t *n_steps, long n_out, int size, const int32_t *atlas_dims, int n_slots)
{
    char msg[256];
    const int rc = sv_syn_check_program(cells, steps, n_steps, n_out, size, atlas_dims, n_slots, msg, sizeof msg);
    return rc ? sv_fail(rc, "sv_synth_check_program: %s", msg) : SV_OK;
}

extern "C" int sv_synth_gaussian_taps_q8(int k, double sigma, int32_t *taps)
{
    REQUIRE(taps, "NULL argument");
    REQUIRE(sv_syn_gaussian_taps_q8(k, sigma, taps), "k must be 3 or 5 and sigma positive and finite");
    return SV_OK;
}

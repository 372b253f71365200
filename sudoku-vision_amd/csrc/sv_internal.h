// Internal declarations shared by the translation units of libsudokuvision_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/sudoku_vision_hip.h"

typedef uint8_t u8;

// Packed DigitCNN weights as the kernels consume them (each family's packer, next to its kernels, has the layouts).
struct sv_weights {
    float *conv1_w = nullptr;   // [32][9]
    float *conv1_b = nullptr;   // [32]
    float *conv2_wreg = nullptr;// [2 np][2 t][72 ks][64 lane]  MFMA B-operand register image
    float *conv2_wino = nullptr;// [4 nt][16 xi][8 ks][64 lane]  Winograd U = G g G^T as MFMA B-operand image (x_cnn_round1.hip; null in the product)
    float *conv2_b = nullptr;   // [64]
    float *fc1_wreg = nullptr;  // [196 chunk][8 t][64 lane][4 e] MFMA B-operand register image
    float *fc1_b = nullptr;     // [128]
    unsigned short *conv2_wsplit = nullptr; // [4 nt][16 xi][3 parts][64 lane][8] U split into three bf16 parts (x_cnn_round1.hip k_conv_features_wsplit; null in the product)
    unsigned short *conv2_bf16 = nullptr; // [9 tap][4 t][64 lane][8] bf16 MFMA B image (bf16 configuration)
    unsigned short *fc1_bf16 = nullptr;   // [98 step][8 t][64 lane][8] bf16
    // k3_cnn_h2.hip: weights x 2^e split into f16 hi + lo (w * 2^e = hi + lo to 22 bits); scale_inv = 2^-e
    unsigned short *conv2_h2 = nullptr;   // [9 tap][2 np][2 t][2 part][64 lane][8] f16: oc = 32np + 2*(lane&15) + t, ic = 8*(lane>>4) + j
    unsigned short *fc1_h2 = nullptr;     // [98 step][8 t][2 part][64 lane][8] f16: n = 16t + (lane&15), feature = 64*(step/2) + 16*(lane>>4) + 8*(step%2) + j
    unsigned short *conv1_h2 = nullptr;   // [2 chalf][4 pos][2 mfma][64 lane][8] f16: conv1 as a GEMM over the 4x4 patch of a pooling window (k3_cnn_h2.hip)
    float conv1_h2_scale_inv = 1.f, conv2_h2_scale_inv = 1.f, fc1_h2_scale_inv = 1.f;
    // the f16-pair kernels carry conv1's activations and the features times powers of two (1 unless a layer's worst-case bound is below 1,
    // svk_pack_weights_h2); the scale_inv factors above fold them in, and these are the biases of conv1 and conv2 with the same factors
    float *conv1_b_h2 = nullptr;          // [32]
    float *conv2_b_h2 = nullptr;          // [64]
    // range of the f16-pair kernels for THESE weights (svk_pack_weights_h2): with inputs in [-1, 1] (8-bit cells after the glue) every activation
    // stays below the f16 range iff h2_in_range; an f32 input batch is inside it iff h2_x_lo <= max|x| <= h2_x_hi (0 > hi: never)
    bool h2_in_range = true;
    float h2_x_lo = 0.f, h2_x_hi = 0.f;
    float *fc2_w = nullptr;     // [10][128]
    float *fc2_b = nullptr;     // [10]
    bool loaded = false;
    std::vector<void *> allocs; // every device buffer above (sv_upload), freed together
};

// Packed DigitCNNv3 weights (k8_cnn_v3.hip: svk_pack_weights_v3 has the layouts), BatchNorm folded into every conv
struct sv_conv3 { float *w = nullptr, *b = nullptr; };   // MFMA B-operand image [cout/16][cin/4][taps][64 lane], folded bias [cout]
struct sv_weights3 {
    sv_conv3 stem, conv1[5], conv2[5], shortcut[5];      // shortcut: layers 2 and 4 only (1x1, stride 2)
    float *se1[5] = {}, *se2[5] = {};                    // se.excite.0.weight [C/4][C], se.excite.2.weight [C][C/4]; NULL without SE
    float *fc_w = nullptr, *fc_b = nullptr;              // [10][128], [10]
    float temperature = 1.f;
    bool use_se = true, loaded = false;
    std::vector<void *> allocs;
};

// Packed DigitCNNv3Light or EmptyClassifier weights (k12_cnn_v3_light.hip: svk_pack_weights_light / _empty have the layouts)
struct sv_weights_light {
    sv_conv3 conv[3];                                    // Light: 1->24, 24->48, 48->96 (BatchNorm folded); Empty: 1->16, 16->32 (own bias)
    float *fc1_w = nullptr, *fc1_b = nullptr;            // Light: fc [10][128] (zero-padded from 96), [10]; Empty: classifier.1 [8][49][32][4], [32]
    float *fc2_w = nullptr, *fc2_b = nullptr;            // Empty: classifier.4 [32], [1]
    float temperature = 1.f;
    bool loaded = false;
    std::vector<void *> allocs;
};

struct sv_ctx;

// One device buffer that a context owns and only ever grows.  The kernels' files say what lives inside each (layout comments there).
struct sv_scratch {
    void *p = nullptr;
    size_t cap = 0;             // bytes
    // At least `bytes`: nothing to do while they fit (the hot path: one compare), else free and allocate anew -- the contents are not
    // kept, and hipFree synchronises the device.  A failed allocation leaves p == nullptr, cap == 0.
    int grow(sv_ctx *ctx, size_t bytes);
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return (T *)p; }
};

struct sv_ctx {
    int device = 0;
    int num_cus = 256;
    sv_weights w;
    sv_weights3 w3;
    sv_weights_light wl, we;    // DigitCNNv3Light, EmptyClassifier
    // grow-only scratch; for_each_scratch below lists every one of them
    sv_scratch v3_act;          // k8_cnn_v3.hip: three activation buffers of [v3_cells][32*784] floats
    long v3_cells = 0;          // at most SV_V3_SUBBATCH
    sv_scratch v3_mc;           // k8_cnn_v3.hip: the MC forward's layer1 outputs, probabilities and keep bytes of one chunk (svk_v3_mc_scratch_bytes)
    sv_scratch features;        // float [cells][49][64] pooled conv2 output
    sv_scratch cells;           // u8 [cells][784]
    sv_scratch cells2;          // u8 [cells][784] preprocess_cell output (SV_GLUE_RUNPY)
    long n_cells = 0;           // what features, cells and cells2 hold (sv_ensure_scratch); nonzero only while all three are allocated
    sv_scratch jpeg_planes;     // decoded component planes (MCU-padded) between the IDCT and the colour kernel
    sv_scratch jpeg_enc;        // k17_jpeg_encode.hip: the dense coefficient blocks of a sparse-only encode, int16 [n][coef_count]
    sv_scratch png_enc;         // k18_png_encode.hip: the per-band slots of a deflate call, u8 [n][bands][slot_bytes]
    sv_scratch png_dec;         // k19_png_decode.hip: the unfiltered samples u8 [n][H][row_bytes], then the segment job list
    sv_scratch pp2;             // k7_preprocess_v2.hip: element rows + doubling planes + the close/open intermediate, or CLAHE's tile histograms + LUTs
    sv_scratch cc;              // k11_components.hip: run numbering, union-find parents and bounding boxes (layout at the top of that file)
    sv_scratch grid2;           // k13_grid_v2.hip: the Harris response, tile and frame maxima, candidate counts and sort keys
    sv_scratch k1_list;         // k1_threshold_mm.hip: optional diagnostic counter (pixels decided by the exact evaluation), sv_preprocess_stats; 16 bytes
    sv_scratch range_flag;      // int [2]: the per-call kernel choice for f32 inputs (k3_cnn.hip k_input_range)
    sv_scratch overlay;         // k16_overlay.hip: the glyph atlas u8 [9][50][50], then the default palette u8 [3][3]
    sv_scratch eval;            // k21_eval.hip: the failure list's base, per-workgroup wrong counts and per-cell wrong flags (layout at the top of that file)
    bool overlay_set = false;   // sv_set_overlay_glyphs has filled `overlay`
    // sv_ctx_destroy frees through this and nothing else: a new buffer goes in here
    template <class F> void for_each_scratch(F f)
    {
        for (sv_scratch *b : {&v3_act, &v3_mc, &features, &cells, &cells2, &jpeg_planes, &jpeg_enc, &png_enc, &png_dec, &pp2, &cc, &grid2, &k1_list, &range_flag, &overlay, &eval}) f(*b);
    }
    int precision = 0;          // SV_PREC_F32 / SV_PREC_BF16 (sv_ctx_set_precision)
    int cnn_kernels = 0;        // SV_CNN_AUTO / _F16PAIR / _F32MFMA (sv_ctx_set_cnn_kernels)
    bool x_fc_frame = false;    // x_cnn_round1.hip (svx_ctx_set_fc_frame_kernel): k_fc_head_frame for large batches; never set in the product
    int x_motion_shape = 0;     // k15_motion.hip: 1 = the two-launch shape (x_motion.cpp, svx_ctx_set_motion_shape); never set in the product
#ifdef SV_DEV
    int dev_ablate = 0;         // k3_cnn_h2.hip: the ablation / stamp bits of k_conv_features_h2 (sv_dev_set_h2_ablate, svk_cnn_forward_h2)
#endif
    // optional per-kernel timing (sv_timing_begin/sv_timing_end): hipEvents on the launch stream
    bool timing = false;
    struct timed { int kernel; hipEvent_t t0, t1; };
    std::vector<timed> timeline;
    std::vector<hipEvent_t> event_pool;
};

enum sv_kernel_id { SVK_PREPROCESS = 0, SVK_WARP_CELLS = 1, SVK_CONV_FEATURES = 2, SVK_FC_HEAD = 3, SVK_FUSED12 = 4, SVK_HARRIS = 5, SVK_WARP_AFFINE = 6, SVK_COUNT = 7 };

// RAII bracket: records an event before and after a launch when ctx->timing is on
struct sv_time_scope {
    sv_ctx *ctx; hipStream_t s; int idx = -1;
    sv_time_scope(sv_ctx *c, int kernel, hipStream_t st);
    ~sv_time_scope();
};

int sv_fail(int code, const char *fmt, ...);

#define SV_HIP(expr)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return sv_fail(SV_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

#define SV_LAUNCH_CHECK(name)                                                                \
    do {                                                                                     \
        hipError_t e_ = hipGetLastError();                                                   \
        if (e_ != hipSuccess) return sv_fail(SV_ERR_HIP, "launch %s: %s", name, hipGetErrorString(e_)); \
    } while (0)

// argument checks of the entry points: SV_ERR_BAD_ARG with "<entry point>: <what>"
#define REQUIRE_AS(fn, cond, what) \
    do { if (!(cond)) return sv_fail(SV_ERR_BAD_ARG, "%s: %s", fn, what); } while (0)
#define REQUIRE(cond, what) REQUIRE_AS(__func__, cond, what)
// one BGR frame batch: n frames of H x W pixels, `pitch` bytes between rows; 65535 = the grid's z limit
static inline bool frames_ok(int n, int H, int W, ptrdiff_t pitch) { return n > 0 && n < 65536 && H > 0 && W > 0 && pitch >= 3 * (ptrdiff_t)W; }
#define REQUIRE_FRAMES() REQUIRE(frames_ok(n, H, W, pitch), "bad shape")

int sv_ensure_scratch(sv_ctx *ctx, long cells);

// n elements of src -> a new device buffer *dst, recorded in w.allocs (w: any of the weight structs above)
template <class W, class T>
int sv_upload(W &w, T **dst, const T *src, size_t n)
{
    SV_HIP(hipMalloc((void **)dst, n * sizeof(T)));
    w.allocs.push_back(*dst);
    SV_HIP(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return SV_OK;
}

// The conv/fc kernel family of an SV_PREC_F32 forward (svk_cnn_forward).  The values are ABI: sv_conv_kernel_info reports them.
enum sv_cnn_algo { SV_ALGO_F32MFMA = 0, SV_ALGO_X_WINOGRAD = 2, SV_ALGO_X_WSPLIT = 3, SV_ALGO_F16PAIR = 4 };

// The one seam between the product and the cross-check kernels of the test-only libsudokuvision_xcheck.so: x_cnn_round1.hip defines
// sv_xcheck, the product links x_none.cpp, where it is null (SV_CNN_X_WINOGRAD / _WSPLIT are then unknown selections and x_fc_frame stays
// false).  Hidden: the tests load both libraries into one process, and each must see its own whichever was loaded first.
struct sv_xcheck_ops {
    bool (*select_conv)(int which, sv_cnn_algo *algo);      // a further selection of sv_ctx_set_cnn_kernels (SV_CNN_X_*) -> its kernel family
    int (*pack_weights)(sv_weights &w, const float *c2w);   // conv2_wino and conv2_wsplit, after svk_pack_weights_f32mfma's own images
    // the launches alone: svk_cnn_forward keeps the timing scope and the launch check
    void (*launch_conv)(sv_ctx *ctx, sv_cnn_algo algo, const void *x, bool x_is_u8, long B, hipStream_t s);   // SV_ALGO_X_WINOGRAD / _X_WSPLIT -> ctx->features
    void (*launch_fc_frame)(sv_ctx *ctx, long B, float *logits, u8 *digits, float *conf, const int *run_if_set, hipStream_t s);   // k_fc_head_frame
};
extern __attribute__((visibility("hidden"))) const sv_xcheck_ops *const sv_xcheck;

// kernel launchers (one per .hip file)
int svk_gray(const u8 *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, u8 *gray, hipStream_t s);
int svk_blur(const u8 *src, int n, int H, int W, int ksize, u8 *dst, hipStream_t s);
int svk_adaptive_threshold(const u8 *src, int n, int H, int W, int block, const float *taps, int idelta, int type_inv,
                           u8 *dst, hipStream_t s);
int svk_preprocess(sv_ctx *ctx, const u8 *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, u8 *binary, hipStream_t s);
int svk_preprocess_bits(sv_ctx *ctx, const u8 *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint32_t *bits, hipStream_t s);
int svk_despeckle_bits(uint32_t *bits, int n, int H, int W, hipStream_t s);
int svk_preprocess_warp_fused(sv_ctx *ctx, const u8 *bgr, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, u8 *binary, const double *minv, u8 *cells,
                              hipStream_t s);
int svk_warp_perspective(const u8 *img, int H, int W, ptrdiff_t pitch, int channels, const double *minv, int out_size,
                         u8 *dst, hipStream_t s);
int svk_extract_cells(const u8 *grid, int h, int w, ptrdiff_t pitch, int channels, int cell_size, int margin_h,
                      int margin_w, u8 *cells, hipStream_t s);
int svk_warp_cells(sv_ctx *ctx, const u8 *frames, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv,
                   u8 *cells, hipStream_t s);
int svk_cnn_forward(sv_ctx *ctx, const void *x, bool x_is_u8, int glue, long B, float *logits, u8 *digits, float *conf,
                    hipStream_t s);
// weight images of one kernel family from the PyTorch-layout tensors of the blob (sv_load_weights_f32), uploaded into w
int svk_pack_weights_f32mfma(sv_weights &w, const float *c2w, const float *f1w);
int svk_pack_weights_bf16(sv_weights &w, const float *c2w, const float *f1w);
int svk_pack_weights_h2(sv_weights &w, const float *c1w, const float *c1b, const float *c2w, const float *c2b, const float *f1w);

int svk_despeckle(const u8 *src, int n, int H, int W, u8 *dst, unsigned *packed, hipStream_t s);
int svk_pack_sparse_bits(const uint32_t *bits, int n, int H, int W, u8 *records, long stride, hipStream_t s);
int svk_copy_to_host(const void *src, void *dst_host, size_t bytes, hipStream_t s);
int svk_resize_linear(const u8 *src, int sh, int sw, ptrdiff_t pitch, u8 *dst, int dh, int dw, hipStream_t s);
// Which fc head serves a batch of B cells (svk_cnn_forward_h2, svk_cnn_forward_bf16): a CU's share of the cells, at least one M tile.  While it
// fits one pass of the per-CU head (sv_fc_head.h: 6 M tiles of 16 cells) that head runs, one workgroup per `share` cells; beyond that the share
// would take a second full pass over the weight image for a few cells, and the wave-tile head, two co-resident 64-cell workgroups per CU, does better.
constexpr int SV_FC_PERCU_CELLS = 16 * 6;
inline long sv_fc_percu_share(const sv_ctx *ctx, long B)
{
    const long per = (B + ctx->num_cus - 1) / ctx->num_cus;
    return per > 16 ? per : 16;
}
int svk_cnn_forward_bf16(sv_ctx *ctx, const u8 *cells, long B, float *logits, u8 *digits, float *conf, hipStream_t s);
int svk_cnn_forward_h2(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logits, u8 *digits, float *conf, const int *run_if_clear, hipStream_t s);
int svk_cell_ink_ratio(const u8 *cells, long B, int npx, float *ratio, int *otsu, hipStream_t s);
int svk_preprocess_cells(const u8 *cells, long B, u8 *out, hipStream_t s);
// denom: libjpeg's scale_denom, 1, 2, 4 or 8; dense when coef != nullptr, else sparse; fn: the entry point that was called, for error texts
int svk_jpeg_reconstruct(sv_ctx *ctx, const sv_jpeg_info *info, int denom, const int16_t *coef, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                         const uint16_t *quant, u8 *bgr, ptrdiff_t pitch, hipStream_t s, const char *fn);
// k20_jpeg_gray.hip (info: sv_jpeg_parse_luma's; the image goes straight into `gray`, no scratch)
int svk_jpeg_reconstruct_gray(const sv_jpeg_info *info, int denom, const int16_t *coef, const uint64_t *masks, const uint32_t *offsets, const int16_t *values,
                              const uint16_t *quant, u8 *gray, ptrdiff_t pitch, hipStream_t s, const char *fn);
int svk_softmax_topk(const float *logits, long B, int k, u8 *index, float *prob, hipStream_t s);
int svk_frame_quality_stats(const u8 *img, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int C, long long *lap_sum, long long *lap_sqsum,
                            uint32_t *hist, hipStream_t s);
int svk_grid_line_coverage(const void *src, bool bits, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *minv, uint32_t *counts,
                           hipStream_t s);
// k7_preprocess_v2.hip
int svk_morphology(sv_ctx *ctx, const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int op, int shape, int k, u8 *dst, hipStream_t s);
int svk_box_mean(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int k, u8 *dst, hipStream_t s);
int svk_threshold_sauvola(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int window, double k, u8 *dst, hipStream_t s);
int svk_gaussian_blur21(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, u8 *dst, hipStream_t s);
int svk_clahe(sv_ctx *ctx, const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, double clip, int tiles_x, int tiles_y, u8 *dst, hipStream_t s);
int svk_divide_normalize(const u8 *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const u8 *background, u8 *dst, hipStream_t s);
int svk_threshold_count(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int thresh, int type_inv, u8 *dst, uint32_t *counts, hipStream_t s);
int svk_shadow_mask(const u8 *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const u8 *local_mean, int delta, u8 *mask, uint32_t *counts, hipStream_t s);
int svk_count_nonzero(const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, uint32_t *counts, hipStream_t s);

// k8_cnn_v3.hip
int svk_pack_weights_v3(sv_weights3 &w, const float *blob, bool use_se);
long svk_v3_blob_floats(bool use_se);
size_t svk_v3_scratch_bytes(long cells);
int svk_cnn3_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logits, float *features, u8 *digits, float *conf, hipStream_t s);
size_t svk_v3_mc_scratch_bytes();
int svk_cnn3_forward_mc(sv_ctx *ctx, const float *x, long B, int S, float p_spatial, float p_fc, uint64_t seed, uint64_t offset, const u8 *const keep_in[3],
                        float *mean, float *std, long long *predicted, float *logits_out, u8 *const keep_out[3], hipStream_t s);

// k12_cnn_v3_light.hip
int svk_pack_weights_light(sv_weights_light &w, const float *blob);
int svk_pack_weights_empty(sv_weights_light &w, const float *blob);
int svk_cnn3_light_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logits, float *features, u8 *digits, float *conf, hipStream_t s);
int svk_empty_forward(sv_ctx *ctx, const void *x, bool x_is_u8, long B, float *logit, hipStream_t s);

// k9_resolve.hip
int svk_resolve_conflicts(const u8 *index, const float *prob, long n, int k, int beam_width, int max_corrections, double min_alt_conf, int accept, u8 *digits,
                          float *conf, u8 *index_out, float *prob_out, u8 *success, int *before, int *after, u8 *conflict_count, u8 *ncorr,
                          u8 *corr_cells, float *corr_conf, int *explored, double *score, hipStream_t s);

// k10_propagate.hip
int svk_propagate_constraints(const u8 *digits, const float *conf, long n, int max_iterations, u8 *grid, uint16_t *candidates, u8 *is_valid, int *iterations,
                              u8 *contradiction_cell, u8 *n_resolved, u8 *resolved, u8 *is_fixed, hipStream_t s);

// k11_components.hip (min_area: the floor itself, min_area_ratio * H * W of the true frame size)
int svk_component_filter_bits(sv_ctx *ctx, uint32_t *bits, int n, int H, int W, double min_area, hipStream_t s);
int svk_component_filter(sv_ctx *ctx, const u8 *binary, int n, int H, int W, double min_area, u8 *out, uint32_t *packed, hipStream_t s);

// k13_grid_v2.hip
int svk_harris_corners(sv_ctx *ctx, const u8 *gray, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int max_corners, double quality_level,
                       int min_distance, double k, int cand_capacity, float *corners, int *counts, float *response, hipStream_t s);
int svk_warp_affine(sv_ctx *ctx, const u8 *src, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *fwd, int dh, int dw, int border, u8 *dst,
                    hipStream_t s);

// k14_solve.hip
int svk_solve_sudoku_batch(const u8 *grid, const u8 *active, int n, int max_nodes, u8 *solution, int8_t *result, int *nodes, hipStream_t s);

// k15_motion.hip
int svk_motion_update(sv_ctx *ctx, const u8 *frames, int n, int H, int W, int C, ptrdiff_t pitch, ptrdiff_t frame_stride, const u8 *prev_small,
                      float threshold, u8 *small, int32_t *counts, int dh, int dw, hipStream_t s);

// k16_overlay.hip
int svk_set_overlay_glyphs(sv_ctx *ctx, const u8 *atlas);
int svk_render_overlay(sv_ctx *ctx, u8 *img, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const double *m, const u8 *digits, const u8 *classes,
                       const u8 *palette, int k, const u8 *active, bool shadow, hipStream_t s);

// k17_jpeg_encode.hip (channels 3: BGR, 1: gray; coef nullptr: dense blocks in ctx->jpeg_enc; masks nullptr: dense output only)
int svk_jpeg_forward(sv_ctx *ctx, const sv_jpeg_enc *plan, const u8 *src, int channels, int n, ptrdiff_t pitch, ptrdiff_t img_stride, int16_t *coef, uint64_t *masks,
                     uint32_t *offsets, int16_t *values, uint32_t *counts, hipStream_t s);

// k18_png_encode.hip (the plan's channels say BGR or gray; the slots live in ctx->png_enc)
int svk_png_deflate(sv_ctx *ctx, const sv_png_enc *plan, const u8 *src, int n, ptrdiff_t pitch, ptrdiff_t frame_stride, u8 *stream, uint32_t *band_len, uint32_t *adler,
                    uint32_t *status, hipStream_t s);

// k19_png_decode.hip (the unfiltered samples and the job list live in ctx->png_dec)
int svk_png_reconstruct(sv_ctx *ctx, const sv_png_info *info, const u8 *filtered, const u8 *row_filter, const u8 *palette, int n, u8 *out, ptrdiff_t pitch,
                        ptrdiff_t frame_stride, uint32_t *status, bool gray, hipStream_t s);

// k24_dataset_cells.hip (no scratch: the whole cell lives in LDS)
int svk_dataset_cells(sv_ctx *ctx, const u8 *filtered, size_t filtered_size, const sv_dataset_record *records, long n, const u8 *palettes, int n_palettes, int mode,
                      u8 *out_u8, float *out_f32, uint32_t *status, hipStream_t s);

// k21_eval.hip (the failure list's scratch lives in ctx->eval)
int svk_eval_metrics(sv_ctx *ctx, const float *input, bool prob, const void *labels, bool i64, long B, long index_base, float T, const double *bin_edges, int n_bins,
                     bool accumulate, float *probs, u8 *pred, float *conf, float *true_prob, float *nll, u8 *correct, sv_eval_stats *stats,
                     sv_eval_failure *failures, long max_failures, hipStream_t s);

// k22_augment.hip (no scratch: the program and the images are the caller's)
int svk_augment(sv_ctx *ctx, const u8 *src, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const sv_aug_step *steps, const int32_t *n_steps,
                const int32_t *src_index, long n_out, uint64_t seed, long index_base, u8 *dst, hipStream_t s);
// k23_synth_cells.hip (no scratch: the records, the atlas and the output are the caller's)
int svk_synth_cells(sv_ctx *ctx, const sv_syn_cell *cells, const sv_aug_step *steps, const int32_t *n_steps, long n_out, int size, const u8 *atlas, const int32_t *dims,
                    int n_slots, uint64_t seed, long index_base, u8 *dst, hipStream_t s);

// host_png.cpp: whether an sv_png_info's geometry is one sv_png_parse produces (format table, limits, derived fields)
bool sv_png_geometry_ok(const sv_png_info *info);

// host helpers
void sv_gaussian_taps_f32(int n, float *out);

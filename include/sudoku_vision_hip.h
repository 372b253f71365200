/*
 * sudoku_vision_hip.h -- C ABI of libsudokuvision_hip.so, the MI355X (gfx950) implementation of the
 * sudoku-vision frame -> digits hot path.
 *
 * The reference (HueCodes/sudoku-vision) has no FFI: its boundary for this path is a set of Python
 * call signatures (cv/preprocess.py, cv/grid.py, cv/extract.py, ml/model.py) over cv2 / torch.
 * Each entry point below names the reference function (file:line under /root/reference) whose
 * arithmetic it replaces; sudoku-vision_amd/{cv,ml}/ re-expose them under the reference's names
 * through ctypes.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Pointers marked [dev] are device (HBM) addresses valid on the
 *     context's device; [host] are host addresses.  The library never allocates or frees
 *     caller-visible memory; scratch and packed weights live inside the opaque context.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Every [dev] call is
 *     asynchronous on that stream; nothing synchronises the device.
 *   - Return value: SV_OK (0) or a negative sv_status.  sv_last_error() gives the message of the last
 *     failure on the calling thread.  No C++ exception crosses this boundary.
 *   - Images are 8-bit, row-major, `pitch` bytes between rows, BGR interleaved when 3-channel
 *     (what cv2.imread hands the reference, pipeline/run.py:250).
 *   - A context is bound to one device and is not thread-safe; use one per host thread/stream.
 */
#ifndef SUDOKU_VISION_HIP_H
#define SUDOKU_VISION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sv_ctx sv_ctx;

typedef enum sv_status {
    SV_OK = 0,
    SV_ERR_BAD_ARG = -1,      /* null pointer, non-positive size, even kernel size, ... */
    SV_ERR_HIP = -2,          /* a HIP runtime call failed (message holds hipGetErrorString) */
    SV_ERR_NO_WEIGHTS = -3,   /* CNN entry point called before sv_load_weights_f32 */
    SV_ERR_UNSUPPORTED = -4,  /* parameter outside what this build restates (e.g. blur ksize 9) */
    SV_ERR_DEGENERATE = -5,   /* corners do not define a homography (singular system) */
    SV_ERR_BUFFER = -6        /* caller-provided output buffer too small (required sizes are reported) */
} sv_status;

#define SV_CNN_PARAMS 421642        /* ml/model.py: count_parameters(DigitCNN()) */
#define SV_CELLS 81
#define SV_CELL_PX 784              /* 28*28 */
#define SV_CLASSES 10

/* ---- library / context ------------------------------------------------------------------------ */

int sv_version(void);                               /* ABI version, currently 2 (2: sv_timing_end takes the array length; sv_ctx_set_cnn_kernels).  Entries added
                                                     * since, the JPEG encoder's among them, are additions within version 2: nothing that existed changed */
const char *sv_last_error(void);                    /* thread-local, never NULL */

/* Creates a context on HIP device `device` (replaces nothing: the reference keeps no state except
 * the model object of pipeline/run.py:98-111). */
int sv_ctx_create(int device, sv_ctx **out);
int sv_ctx_destroy(sv_ctx *ctx);

/* Arithmetic of the CNN's conv2/fc1 (BASELINE.json configs[1] vs configs[4]).  SV_PREC_F32 (default): f32-grade results, logits
 * within 1e-4 of the PyTorch-CPU model (which kernels deliver them: sv_ctx_set_cnn_kernels below).  SV_PREC_BF16: bf16 operands, f32
 * accumulation (v_mfma_f32_16x16x32_bf16); parity target = predicted digit indices.  Applies to sv_cnn_forward_cells_u8 and
 * sv_frames_to_digits. */
#define SV_PREC_F32 0
#define SV_PREC_BF16 1
int sv_ctx_set_precision(sv_ctx *ctx, int precision);

/* Which kernels compute the SV_PREC_F32 forward.  Nothing in the process environment influences this.
 *   SV_CNN_AUTO (default)  csrc/k3_cnn_h2.hip -- every f32 operand as a pair of f16 halves (22 significant bits) on the f16 matrix pipe,
 *                          f32 accumulation -- whenever that is safe, else csrc/k3_cnn.hip's f32-MFMA kernels.  "Safe" = inputs, conv1
 *                          activations and features stay inside f16's range (|v| < 65,504): sv_load_weights_f32 bounds the activations
 *                          from the weights (worst case over inputs in [-1, 1], which is what 8-bit cells become; weights are carried times
 *                          a power of two, as are activations whose bound is below 1), and an f32 input batch (sv_cnn_forward_f32) is
 *                          range-checked on the device per call -- out of range, NaN/Inf or all below 2^-3 (where an unscaled pair loses
 *                          bits), it takes the f32 kernels, with no host synchronisation either way.  So the entry points accept what
 *                          ml/model.py:34-42 accepts: any finite f32 weights and inputs.  Accuracy, either way: the logits are as close
 *                          to an exact (float64) evaluation of the model as PyTorch-CPU's own f32 forward is, within a small factor
 *                          (tests/test_gpu_cnn_accuracy.py states the bound and the measured ratios), at any scale of weights and inputs.
 *   SV_CNN_F16PAIR         the f16-pair kernels unconditionally (inputs/activations beyond 65,504 then overflow to inf)
 *   SV_CNN_F32MFMA         the f32-MFMA kernels unconditionally (true f32 throughout; about 4x slower) */
#define SV_CNN_AUTO 0
#define SV_CNN_F16PAIR 1
#define SV_CNN_F32MFMA 2
int sv_ctx_set_cnn_kernels(sv_ctx *ctx, int which);

/* Pre-sizes the context's scratch for batches of up to `max_cells` cells so that later calls do
 * no hipMalloc (needed before hipGraph capture). */
int sv_ctx_reserve(sv_ctx *ctx, long max_cells);

/* Measurement aid (no reference counterpart; pipeline/run.py:247-352 uses time.time()).  Between
 * sv_timing_begin and sv_timing_end every launch of the hot kernels is bracketed by hipEvents on
 * the stream it is launched on.  sv_timing_end waits for those events and returns, per kernel id
 * 0 = preprocess, 1 = warp_cells, 2 = conv_features, 3 = fc_head, 4 = the fused preprocess + warp_cells launch: total
 * milliseconds and launches. */
#define SV_TIMED_KERNELS 5
int sv_timing_begin(sv_ctx *ctx);
/* n_kernels = the length of the caller's two arrays (SV_TIMED_KERNELS of the header it was built against): ids >= n_kernels are not reported. */
int sv_timing_end(sv_ctx *ctx, double *ms_total /*host, n_kernels*/, long *launches /*host, n_kernels*/, int n_kernels);

/* Measurement aid: which conv/fc kernels sv_cnn_forward_cells_u8 / sv_frames_to_digits launch on this context with the weights
 * loaded (4 = f16 hi/lo operand pairs on the f16 matrix pipe, csrc/k3_cnn_h2.hip; 0 = f32 MFMA, csrc/k3_cnn.hip) and the matrix
 * instructions they issue per 28x28 cell: v_mfma_f32_16x16x4_f32 (2048 FLOP each) for conv2 and conv1 (0 = conv1 on the VALU) of the f32-MFMA
 * kernels, or v_mfma_f32_16x16x32_f16 (16384 FLOP each) for the conv kernel and the fc kernel of the default pair.  bench.py prices
 * a kernel's roofline fraction on the work it issues against the peak of the pipe it issues it on. */
int sv_conv_kernel_info(sv_ctx *ctx, int *algo, int *mfma_f32_conv2_per_cell, int *mfma_f32_conv1_per_cell,
                        int *mfma_f16_conv_per_cell, int *mfma_f16_fc_per_cell);

/* Loads DigitCNN weights: `blob` [host] is the state_dict flattened in key order
 * conv1.weight[32,1,3,3] conv1.bias[32] conv2.weight[64,32,3,3] conv2.bias[64] fc1.weight[128,3136]
 * fc1.bias[128] fc2.weight[10,128] fc2.bias[10] = SV_CNN_PARAMS floats.
 * Replaces model.load_state_dict(...) + model.to(device), pipeline/run.py:101-108.
 * Synchronous (packs on the host, copies, waits). */
int sv_load_weights_f32(sv_ctx *ctx, const float *blob);

/* ---- K1: preprocessing (cv/preprocess.py) ----------------------------------------------------- */

/* grayscale(), cv/preprocess.py:15-19 (cv2.cvtColor BGR2GRAY).  n images, `img_stride` bytes apart. */
int sv_gray_u8(sv_ctx *ctx, const uint8_t *bgr /*dev*/, int n, int H, int W, ptrdiff_t pitch,
               ptrdiff_t img_stride, uint8_t *gray /*dev, n*H*W*/, void *stream);

/* blur(), cv/preprocess.py:22-29 (cv2.GaussianBlur (k,k), sigma 0).  ksize in {1,3,5,7}. */
int sv_blur_u8(sv_ctx *ctx, const uint8_t *src /*dev, n*H*W*/, int n, int H, int W, int ksize,
               uint8_t *dst /*dev*/, void *stream);

/* threshold(), cv/preprocess.py:32-54 (cv2.adaptiveThreshold 255, GAUSSIAN_C).  block odd, 3..31.
 * type_inv: 1 = THRESH_BINARY_INV (preprocess.py:51), 0 = THRESH_BINARY (pipeline/run.py:91-93). */
int sv_adaptive_threshold_u8(sv_ctx *ctx, const uint8_t *src /*dev, n*H*W*/, int n, int H, int W,
                             int block, double c, int type_inv, uint8_t *dst /*dev*/, void *stream);

/* preprocess_for_grid_detection(), cv/preprocess.py:57-65: gray -> blur 5 -> threshold(11, 2, INV),
 * fused in one kernel.  n frames. */
int sv_preprocess_u8(sv_ctx *ctx, const uint8_t *bgr /*dev*/, int n, int H, int W, ptrdiff_t pitch,
                     ptrdiff_t img_stride, uint8_t *binary /*dev, n*H*W*/, void *stream);

/* BASELINE configs[4], "fused threshold/warp" for the device-only mode: preprocess_for_grid_detection (cv/preprocess.py:57-65) and
 * warp_perspective + extract_cells (cv/grid.py:94-133, cv/extract.py:13-56) of the same frames in ONE launch, for callers that know the
 * corners before thresholding (a tracker, the benchmark's generator corners).  Same outputs as sv_preprocess_u8 + sv_warp_cells_u8.
 * The grid places everything that reads frame f on the same XCD at the same time, so the two stages share the frame's bytes in L2.
 * Needs H, W >= 16, W % 4 == 0 and 4-byte aligned frames / binary: SV_ERR_UNSUPPORTED otherwise. */
int sv_preprocess_warp_cells_u8(sv_ctx *ctx, const uint8_t *bgr /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                uint8_t *binary /*dev, n*H*W*/, const double *minv /*dev, n*9*/, uint8_t *cells /*dev, n*81*784*/, void *stream);

/* preprocess_for_grid_detection() with the binary written as 1 bit per pixel (bit = pixel != 0, LSB = leftmost, W/32
 * words per row, rows dense): the form the host corner search reads (sv_find_grid_corners_bits_batch) when nothing
 * else consumes the byte image.  Same pixels as sv_preprocess_u8.  Needs H, W >= 16, W % 32 == 0 and a 4-byte aligned
 * frame layout (pitch, img_stride, bgr), else SV_ERR_UNSUPPORTED -- use sv_preprocess_u8 + sv_despeckle_u8(packed). */
int sv_preprocess_bits_u8(sv_ctx *ctx, const uint8_t *bgr /*dev*/, int n, int H, int W, ptrdiff_t pitch,
                          ptrdiff_t img_stride, uint32_t *bits /*dev, n*H*W/32*/, void *stream);

/* sv_despeckle_u8 on a bit image, in place (same filter, same precondition, same result as its `packed` output). */
int sv_despeckle_bits(sv_ctx *ctx, uint32_t *bits /*dev, n*H*W/32*/, int n, int H, int W, void *stream);

/* Accelerator for the host corner search, not a reference stage: erases connected components of a {0,255}
 * image that lie strictly inside a 64x64 tile (two passes, the second with the tile grid offset by (32,32)).  Such
 * components can neither be nor influence the result of find_grid_contour (argument in csrc/k4_despeckle.hip), so
 * sv_find_grid_corners_u8(despeckled) == sv_find_grid_corners_u8(binary).  out may equal binary.
 * A pass erases every such component of a tile unless the tile's flood fill has not settled within its iteration cap
 * (MAX_IT = 96 in csrc/k4_despeckle.hip; thin diagonal paths that wind through a tile need more, natural images come
 * close: DESIGN.md, K4): that tile is left exactly as it is for that pass.  So the filter erases a subset of the
 * strictly-inside components, always whole ones; the equality above holds for any subset.
 * packed (optional, needs W % 32 == 0): the result as 1 bit per pixel (LSB = leftmost, W/32 words per row) for a
 * cheap D2H copy -- when given, `out` is scratch (first pass only) and `packed` holds the result; feed it to
 * sv_find_grid_corners_bits_batch.
 * PRECONDITION for the equality above: min_area_ratio * H * W > 61 * 61 (an erased component's bounding box is at most
 * 62x62 px, so its contour area is at most 61*61; with a smaller area floor, e.g. frames under ~193x193 at the default
 * ratio 0.1, the grid itself could be erased).  The library cannot check it (min_area_ratio belongs to the search);
 * callers must (sudoku-vision_amd/pipeline.py does). */
int sv_despeckle_u8(sv_ctx *ctx, const uint8_t *binary /*dev, n*H*W*/, int n, int H, int W,
                    uint8_t *out /*dev, n*H*W*/, uint32_t *packed /*dev, n*H*W/32, or NULL*/, void *stream);

/* K11, a second accelerator for the host corner search, behind sv_despeckle_*; opt-in, not a reference stage.  An exact connected-
 * component filter (csrc/k11_components.hip): with min_area = min_area_ratio * ((double)H * (double)W), every 8-connected component of
 * foreground (pixel != 0) whose pixel bounding box x0..x1, y0..y1 (inclusive) has (double)(x1 - x0) * (double)(y1 - y0) < min_area is
 * erased, and every other pixel is unchanged.  That is the comparison by which find_grid_contour skips a contour, and a contour's area
 * never exceeds the product, so
 *     sv_find_grid_corners_*(filtered with ratio r, searched with r') == sv_find_grid_corners_*(binary, r')   for every r' >= r
 * (argument at the top of the kernel file).  There is no iteration cap and no input that is left as it is; a 1-pixel-high or -wide
 * component always goes when min_area > 0; min_area_ratio == 0 erases nothing.  Results do not depend on the order the kernels' atomics
 * land in.  Batched over n frames, stream-ordered, no host synchronisation; n == 0 is a no-op.
 * Shapes: any H, W >= 1 with H * W <= 4e9 for the byte form (out may equal binary; packed, optional, needs W % 32 == 0 and receives
 * the result as 1 bit per pixel as well); W % 32 == 0 for the bit form (in place), else SV_ERR_UNSUPPORTED.
 * NULL pointers, negative sizes, a negative or NaN ratio: SV_ERR_BAD_ARG.
 * Scratch in the context, grow-only (nothing is allocated by a call at a shape no larger than an earlier one): 8.25 bytes per pixel of
 * a frame padded to W % 32 == 0 (one word per possible run start for the union-find parent and three box limits, a word per 32 pixels
 * for the run numbering, the byte form's bit image), for at most as many frames of a batch as fit in 1 GiB (one frame at least); a
 * longer batch is worked off in groups on the stream. */
int sv_component_filter_bits(sv_ctx *ctx, uint32_t *bits /*dev, n*H*W/32, in place*/, int n, int H, int W, double min_area_ratio, void *stream);
int sv_component_filter_u8(sv_ctx *ctx, const uint8_t *binary /*dev, n*H*W*/, int n, int H, int W, double min_area_ratio,
                           uint8_t *out /*dev, n*H*W, may equal binary*/, uint32_t *packed /*dev, n*H*W/32, or NULL*/, void *stream);

/* Sparse form of sv_despeckle_u8's packed output for the D2H copy (a despeckled frame is mostly zero words: the hand-over to
 * the host search shrinks 3-4x).  Record of one frame, little endian:
 *   u32 n_values, u32 cap_values, u64 mask[H * gpr], u32 value[cap_values]        gpr = ceil(W/32/64)
 * mask[y * gpr + g] bit k = word 64g + k of row y is non-zero; the non-zero words follow in raster order.  n_values >
 * cap_values: the frame did not fit (values truncated) -- use the dense image for it.  cap_values is what fits in
 * record_stride (a multiple of 8; sv_sparse_bits_record_bytes gives the stride for a wanted capacity).
 * sv_find_grid_corners_sparse_batch / sv_sparse_bits_expand read records on the host. */
long sv_sparse_bits_record_bytes(int H, int W, long cap_values);
int sv_pack_sparse_bits(sv_ctx *ctx, const uint32_t *bits /*dev, n*H*W/32*/, int n, int H, int W,
                        uint8_t *records /*dev, n*record_stride*/, long record_stride, void *stream);

/* Device -> pinned host copy done by a kernel (16-byte stores into mapped host memory) instead of the DMA engine: the
 * hand-over of the binary to the host corner search (the reference hands cv2.findContours a numpy array, cv/grid.py:18;
 * here the array has to cross PCIe first).  ~55 GB/s against 22-30 for hipMemcpyAsync on the MI355X boxes measured
 * (tools/ubench_d2h.hip).  dst_host must be pinned host memory (hipHostMalloc, hipHostRegister, torch pin_memory) --
 * SV_ERR_BAD_ARG otherwise; both pointers 16-byte aligned.  Stream-ordered like a hipMemcpyAsync. */
int sv_copy_to_pinned_host(sv_ctx *ctx, const void *src /*dev*/, void *dst_host /*pinned host*/, size_t bytes, void *stream);

/* ---- host corner search (cv/grid.py:16-71; stays on the CPU, no context, no GPU) ----------------- */

/* find_grid_contour(binary, min_area_ratio), cv/grid.py:37-71, with approximate_polygon's
 * epsilon_ratio (:24-34): external contours (cv2.findContours RETR_EXTERNAL/CHAIN_APPROX_SIMPLE), largest
 * first, the first one >= min_area_ratio*H*W whose cv2.approxPolyDP(epsilon_ratio*perimeter) has 4
 * vertices.  binary [host].  Returns 1 and corners[8] = (x,y)*4 in approxPolyDP order, 0 if none
 * (the reference returns None), or a negative sv_status. */
int sv_find_grid_corners_u8(const uint8_t *binary /*host*/, int H, int W, ptrdiff_t pitch,
                            double min_area_ratio, double epsilon_ratio, int *corners /*host, 8*/);

/* The same for n images on `threads` host threads; found[i] = 1/0. */
int sv_find_grid_corners_batch_u8(const uint8_t *binary /*host*/, int n, int H, int W, ptrdiff_t pitch,
                                  ptrdiff_t img_stride, double min_area_ratio, double epsilon_ratio,
                                  int *corners /*host, n*8*/, uint8_t *found /*host, n*/, int threads);

/* detect_grid_contour(binary, min_area_ratio), cv/grid_v2.py:102-128: sv_find_grid_corners_u8's search with run_v2's loop.
 * Contours by area, largest first (ties in cv2's order); the loop ends at the first contour below min_area_ratio*H*W; a
 * 4-vertex approximation is taken only if is_valid_quadrilateral (cv/grid_v2.py:64-95) holds for its float32 corners, in
 * float32 arithmetic: for every vertex, with v1 = p[i] - p[i+1] and v2 = p[i+2] - p[i+1],
 * acos(clip(dot(v1,v2) / (|v1|*|v2| + 1e-6f), -1, 1)) * (180/pi) lies in [45, 135]; and the longest side is <= 2 * the
 * shortest.  Otherwise the search goes on with the next contour.  Returns 1 / 0 / a negative sv_status like the v1 entry. */
int sv_find_grid_corners_v2_u8(const uint8_t *binary /*host*/, int H, int W, ptrdiff_t pitch,
                               double min_area_ratio, double epsilon_ratio, int *corners /*host, 8*/);

/* The same for n images on `threads` host threads; found[i] = 1/0. */
int sv_find_grid_corners_v2_batch_u8(const uint8_t *binary /*host*/, int n, int H, int W, ptrdiff_t pitch,
                                     ptrdiff_t img_stride, double min_area_ratio, double epsilon_ratio,
                                     int *corners /*host, n*8*/, uint8_t *found /*host, n*/, int threads);

/* detect_lines, cv/grid_v2.py:135-149 = cv2.HoughLinesP(binary, rho, theta, threshold, minLineLength, maxLineGap): the
 * progressive probabilistic Hough transform (csrc/host_hough.cpp; host code, it is sequential).  rho and theta are rounded
 * to float as cv2 takes them.  numangle = round(pi/theta), numrho = round(((W+H)*2+1)/rho); trig table float:
 * cos(n*theta)/rho, sin(n*theta)/rho computed in double, rounded once.  The non-zero points are collected in raster order
 * and drawn with cv::RNG's generator, state = (uint32)state*4164903690 + (state>>32) from state 2^64-1, idx = low 32 bits %
 * remaining, the drawn point replaced by the last; a point whose mask is already clear is skipped.  A point votes at every
 * angle n in bin round(x*cos[n] + y*sin[n]) + (numrho-1)/2 (float products and sum, round half to even); the first
 * maximum above threshold-1 names the line.  From the point the line is walked both ways in 16-bit fixed point (major
 * axis +-1, minor axis round(b*65536/|a|) in float, start offset by half a unit) to the image border or until more than
 * max_line_gap pixels in a row are clear; the last set pixel of each side is an end.  The line is good if |dx| or |dy| of
 * the ends is >= min_line_length.  A second walk up to the ends clears the mask and, for a good line, takes the cleared
 * pixels' votes back.  Good lines are written as (x0, y0, x1, y1) in the order they are found.  *count = lines found;
 * SV_ERR_BUFFER (with *count set) when cap is too small. */
int sv_hough_lines_p_u8(const uint8_t *binary /*host*/, int H, int W, ptrdiff_t pitch, double rho, double theta, int threshold,
                        int min_line_length, int max_line_gap, int *lines /*host, cap*4*/, int cap, int *count);

/* sv_find_grid_corners_batch_u8 on bit-packed images (layout of sv_despeckle_u8's `packed`). */
int sv_find_grid_corners_bits_batch(const uint32_t *bits /*host, n*H*W/32*/, int n, int H, int W,
                                    double min_area_ratio, double epsilon_ratio,
                                    int *corners /*host, n*8*/, uint8_t *found /*host, n*/, int threads);

/* Restrict the library's host worker threads (the batch searches above, the JPEG entropy decoder) to the given CPUs --
 * normally the CPUs of the NUMA node the GPU's pinned buffers live on: on a two-socket MI355X host the search runs 10-20 %
 * slower and with 40-ms outliers when its threads wander to the other socket.  n = 0: no restriction for workers started
 * later.  The thread that calls a batch function works too and keeps its own mask. */
int sv_host_pool_set_affinity(const int *cpus /*host, n*/, int n);

/* The same on sparse records (sv_pack_sparse_bits).  found[i] = 2: record i overflowed, search its dense image instead. */
int sv_find_grid_corners_sparse_batch(const uint8_t *records /*host, n*record_stride*/, long record_stride, int n, int H, int W,
                                      double min_area_ratio, double epsilon_ratio,
                                      int *corners /*host, n*8*/, uint8_t *found /*host, n*/, int threads);

/* One sparse record -> the dense bit image (H*W/32 words).  SV_ERR_BUFFER if the record overflowed. */
int sv_sparse_bits_expand(const uint8_t *record /*host*/, int H, int W, uint32_t *bits /*host, H*W/32*/);

/* find_contours(), cv/grid.py:16-21.  Contours in cv2's order, concatenated: points = (x,y) pairs,
 * sizes[i] = vertices of contour i.  If a buffer is too small (or NULL) returns SV_ERR_BUFFER with
 * the required counts in n_points / n_contours. */
int sv_find_contours_u8(const uint8_t *binary /*host*/, int H, int W, ptrdiff_t pitch,
                        int *points /*host, cap_points*2*/, long cap_points, int *sizes /*host*/,
                        int cap_contours, long *n_points, int *n_contours);

/* The same on a bit-packed image (1 bit per pixel, LSB = leftmost, W/32 words per row -- sv_despeckle_u8's packed output; W % 32 == 0):
 * the scanner sv_find_grid_corners_bits_batch uses, which never expands the image to bytes.  Same contours, same order. */
int sv_find_contours_bits(const uint32_t *bits /*host*/, int H, int W, int *points, long cap_points, int *sizes, int cap_contours,
                          long *n_points, int *n_contours);

/* cv2.contourArea / cv2.arcLength / cv2.approxPolyDP on int32 (x,y) vertices (cv/grid.py:31-33,58,61). */
int sv_contour_area_i32(const int *xy /*host*/, int n, double *area);
int sv_arc_length_i32(const int *xy /*host*/, int n, int closed, double *length);
int sv_approx_poly_dp_i32(const int *xy /*host*/, int n, double epsilon, int closed,
                          int *out /*host, n*2*/, int *n_out);

/* ---- solver (host; scope row N4) -------------------------------------------------------------------- */

/* solve_sudoku(), solver/src/sudoku.c:72-81, as an in-process call instead of pipeline/run.py:163-202's
 * subprocess + /tmp files.  grid/solution: 81 digits row-major, 0 = empty.  *result: 1 solved, 0 no solution,
 * -1 invalid input (solver/include/sudoku.h:13-16); solution = grid unless solved. */
int sv_solve_sudoku(const uint8_t *grid /*host, 81*/, uint8_t *solution /*host, 81*/, int *result);

/* ---- K14: the solver for n grids in one launch (pipeline/run_v2.py:393-407, run_solver) ---------------- */

/* Result codes of the batch entries on top of the reference's 1 / 0 / -1 (solver/include/sudoku.h:13-16). */
#define SV_SOLVE_BUDGET 2           /* max_nodes search nodes were entered and another one was due: the frame is undecided */
#define SV_SOLVE_SKIPPED 3          /* active[f] == 0: the caller did not want this frame solved */
#define SV_SOLVE_MAX_NODES 65536    /* the largest budget a launch takes */

/* solver/src/sudoku.c for n grids, one wave per grid: validate_grid (:413-467); init_candidates (:226-247); propagate (:287-401):
 * naked singles row-major, each placed before the next cell is looked at, then hidden singles by row, by column, by box, digits
 * ascending, repeated while anything was placed; solve_with_candidates (:6-59): branch on the first cell with the fewest candidates,
 * digits ascending.  The same decision order as sv_solve_sudoku, so the same grid also where a puzzle has several solutions.
 * A node is one entry into solve_with_candidates (one call of propagate); the root is node 1.  When a node would be entered
 * with max_nodes already entered, the frame ends with SV_SOLVE_BUDGET.
 *   grid [n*81]      0 = empty, 1..9; a byte above 9 or a duplicate in a unit: result -1
 *   active [n]       or NULL (all): frames with 0 are not solved (SV_SOLVE_SKIPPED)
 * Outputs, each may be NULL:
 *   solution [n*81]  = grid unless result is 1; may be grid itself
 *   result [n]       1, 0, -1, SV_SOLVE_BUDGET, SV_SOLVE_SKIPPED
 *   nodes [n]        nodes entered; 0 for results -1 and SV_SOLVE_SKIPPED
 * Asynchronous on `stream`; a frame's result does not depend on the rest of the batch.  1 <= max_nodes <= SV_SOLVE_MAX_NODES,
 * otherwise SV_ERR_BAD_ARG; n == 0 is SV_OK. */
int sv_solve_sudoku_batch(sv_ctx *ctx, const uint8_t *grid /*dev, n*81*/, const uint8_t *active /*dev, n, or NULL*/, int n, int max_nodes,
                          uint8_t *solution /*dev, n*81*/, int8_t *result /*dev, n*/, int32_t *nodes /*dev, n, or NULL*/, void *stream);

/* The same on the host over `threads` threads, all pointers host memory: same codes, same solutions, same node counts.
 * max_nodes == 0: no budget (then SV_SOLVE_BUDGET never occurs; nodes saturates at INT32_MAX); max_nodes < 0: SV_ERR_BAD_ARG. */
int sv_solve_sudoku_batch_host(const uint8_t *grid, const uint8_t *active /*or NULL*/, int n, int max_nodes, uint8_t *solution,
                               int8_t *result, int32_t *nodes /*or NULL*/, int threads);

/* ---- K2: perspective warp + cell extraction (cv/grid.py, cv/extract.py) ------------------------- */

/* Host, fp64.  order_points + inset + cv2.getPerspectiveTransform to (0,0)..(S-1,S-1) + the inverse
 * warpPerspective takes, cv/grid.py:74-91,111-130.  corners: n*8 floats (x,y)*4 in any order;
 * minv: n*9 doubles (destination -> source). */
int sv_corners_to_minv(const float *corners /*host*/, int n, int out_size, float inset_ratio,
                       double *minv /*host*/);

/* The same for a batch in which single frames may be degenerate (order_points picks one point twice for a quad rotated
 * near 45 degrees, cv/grid.py:79-91: the 8x8 system is then singular): ok[f] = 1 and minv[f] filled, or ok[f] = 0 and
 * minv[f] = identity.  Never returns SV_ERR_DEGENERATE; the caller masks the frames with ok[f] = 0. */
int sv_corners_to_minv_batch(const float *corners /*host*/, int n, int out_size, float inset_ratio,
                             double *minv /*host*/, uint8_t *ok /*host, n*/);

/* cv2.warpPerspective(image, M, (S,S)), cv/grid.py:131: bilinear, 1/32-px coordinates, 15-bit
 * weights, constant-0 border.  channels 1 or 3.  One image. */
int sv_warp_perspective_u8(sv_ctx *ctx, const uint8_t *img /*dev*/, int H, int W, ptrdiff_t pitch,
                           int channels, const double *minv /*dev, 9*/, int out_size,
                           uint8_t *dst /*dev, S*S*channels*/, void *stream);

/* extract_cells(), cv/extract.py:13-56: 9x9 split, margin crop, BGR2GRAY, cv2.resize to
 * cell_size^2.  margin_h/margin_w are the caller's int(cell_h*margin_ratio), int(cell_w*...). */
int sv_extract_cells_u8(sv_ctx *ctx, const uint8_t *grid /*dev*/, int h, int w, ptrdiff_t pitch,
                        int channels, int cell_size, int margin_h, int margin_w,
                        uint8_t *cells /*dev, 81*cell_size^2*/, void *stream);

/* Fused warp_perspective(frame, corners) -> extract_cells(warped) with the reference defaults
 * (450, inset 0, 28, 0.1): only the 81 40x40 crops are ever warped.  n frames; minv n*9 doubles. */
int sv_warp_cells_u8(sv_ctx *ctx, const uint8_t *frames /*dev*/, int n, int H, int W, ptrdiff_t pitch,
                     ptrdiff_t frame_stride, const double *minv /*dev, n*9*/,
                     uint8_t *cells /*dev, n*81*784*/, void *stream);

/* ---- K3: DigitCNN forward (ml/model.py) --------------------------------------------------------- */

/* DigitCNN.forward, ml/model.py:34-42 (eval mode): x f32 [B,1,28,28] -> logits f32 [B,10].
 * digits (argmax, pipeline/run.py:142) and conf (softmax[argmax], :141-143) may be NULL.
 * Any finite f32 input is accepted: a batch outside the range the default kernels carry exactly is computed by the f32-MFMA kernels
 * (sv_ctx_set_cnn_kernels).  A cell holding NaN/Inf does not disturb the other cells of its batch; its own logits are unspecified (the
 * reference yields NaN there; ReLU and max-pool here are IEEE maxNum, which drops a NaN). */
int sv_cnn_forward_f32(sv_ctx *ctx, const float *x /*dev*/, long B, float *logits /*dev, B*10*/,
                       uint8_t *digits /*dev, B, or NULL*/, float *conf /*dev, B, or NULL*/,
                       void *stream);

/* The glue pipeline/run.py:122-136 puts between extract_cells and the model, fused into the CNN's input stage. */
typedef enum sv_glue {
    SV_GLUE_NORMALIZE = 0,  /* x = ((255 - cell)/255 - 0.5)/0.5                      (run.py:126-135 without preprocess_cell) */
    SV_GLUE_RUNPY = 1       /* preprocess_cell first: CLAHE(2.0,(4,4)) + adaptiveThreshold(GAUSSIAN_C, BINARY, 11, 2),
                               run.py:73-95, then the same invert + normalise -- exactly what run.py feeds the model */
} sv_glue;

/* cv2.resize(img, (dw, dh)), default INTER_LINEAR, on an 8-bit gray image (cv/extract.py:52 and :93). */
int sv_resize_linear_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int sh, int sw, ptrdiff_t pitch,
                        uint8_t *dst /*dev, dh*dw*/, int dh, int dw, void *stream);

/* is_cell_empty(), cv/extract.py:59-79, batched: per cell the Otsu threshold (cv2.threshold THRESH_OTSU) and
 * ratio = countNonZero(BINARY_INV image) / pixels; the caller compares ratio < threshold (default 0.02).
 * cells: B images of cell_px pixels each.  otsu may be NULL. */
int sv_cell_ink_ratio_u8(sv_ctx *ctx, const uint8_t *cells /*dev, B*cell_px*/, long B, int cell_px,
                         float *ratio /*dev, B*/, int *otsu /*dev, B, or NULL*/, void *stream);

/* preprocess_cell(), pipeline/run.py:73-95, on B 28x28 gray cells: CLAHE(2.0,(4,4)) then
 * adaptiveThreshold(GAUSSIAN_C, THRESH_BINARY, 11, 2).  out: u8 {0,255}, B*784. */
int sv_preprocess_cells_u8(sv_ctx *ctx, const uint8_t *cells /*dev, B*784*/, long B,
                           uint8_t *out /*dev, B*784*/, void *stream);

/* DigitCNN.forward on 8-bit cells with the glue fused in. */
int sv_cnn_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells /*dev, B*784*/, long B, int glue,
                            float *logits /*dev*/, uint8_t *digits /*dev or NULL*/,
                            float *conf /*dev or NULL*/, void *stream);

/* ---- K8: DigitCNNv3 forward (ml/model_v3.py), the model pipeline/run_v2.py:95-128 loads ------------------------------------------ */

/* Floats in the weight blob of sv_load_weights_v3_f32: DigitCNNv3(use_se=True) and DigitCNNv3(use_se=False). */
#define SV_CNN3_PARAMS_SE 700587
#define SV_CNN3_PARAMS_NOSE 679595
#define SV_CNN3_FEATURES 128
/* The v3 forward keeps its activations in context scratch, 3 * 32*28*28 floats (301,056 bytes) per cell, for at most this many cells: a
 * larger batch runs as consecutive sub-batches, so the scratch never exceeds SV_V3_SUBBATCH * 301,056 bytes = 147 MiB.  sv_ctx_reserve
 * sizes it for all SV_V3_SUBBATCH cells whatever max_cells is: sv_cnn3_forward_mc_f32 fills them at any batch size. */
#define SV_V3_SUBBATCH 512

/* blob: the state_dict of DigitCNNv3 (ml/model_v3.py:113-149) flattened in key order, the int64 num_batches_tracked entries skipped:
 * temperature[1] stem.0.weight[32,1,3,3] stem.1.{weight,bias,running_mean,running_var}[32], then per layer1..5
 * conv1.weight bn1.{...} conv2.weight bn2.{...} [se.excite.0.weight se.excite.2.weight] [shortcut.0.weight shortcut.1.{...}],
 * fc.weight[10,128] fc.bias[10].  n_floats must be SV_CNN3_PARAMS_SE (use_se != 0) or SV_CNN3_PARAMS_NOSE, else SV_ERR_BAD_ARG.
 * Every BatchNorm is folded into its convolution here, in double, with eps = 1e-5.
 * Replaces DigitCNNv3() + load_state_dict + model.to(device), pipeline/run_v2.py:99-121.  Synchronous.  Independent of
 * sv_load_weights_f32: a context may hold both models.  If sv_ctx_reserve was called before, the v3 scratch is sized here. */
int sv_load_weights_v3_f32(sv_ctx *ctx, const float *blob /*host*/, long n_floats, int use_se);

/* DigitCNNv3.forward, ml/model_v3.py:163-184 (eval mode), in true f32 on v_mfma_f32_16x16x4_f32: x f32 [B,1,28,28] -> logits f32 [B,10].
 * features: what forward(x, return_features=True) returns (:175-178).  digits: argmax of the logits.  conf: softmax(logits / temperature)
 * at that digit, get_confidence (:216-225).  Each may be NULL.  A cell's results do not depend on the rest of the batch, and a cell
 * holding NaN/Inf does not disturb the others (its own logits are unspecified: ReLU here is IEEE maxNum, which drops a NaN).
 * SV_ERR_NO_WEIGHTS before sv_load_weights_v3_f32; SV_ERR_UNSUPPORTED on a context set to SV_PREC_BF16 (f32 is the only arithmetic).
 * After sv_ctx_reserve (with the v3 weights loaded, in either order) no v3 entry allocates, so they can be captured in a hipGraph. */
int sv_cnn3_forward_f32(sv_ctx *ctx, const float *x /*dev, B*784*/, long B, float *logits /*dev, B*10*/,
                        float *features /*dev, B*128, or NULL*/, uint8_t *digits /*dev, B, or NULL*/, float *conf /*dev, B, or NULL*/,
                        void *stream);

/* The same on 8-bit cells with the glue of pipeline/run_v2.py:131-146 + :161-163 fused in: SV_GLUE_RUNPY is exactly what run_v2 feeds
 * the model (its preprocess_cell is run.py's), SV_GLUE_NORMALIZE the invert + normalise alone. */
int sv_cnn3_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells /*dev, B*784*/, long B, int glue, float *logits /*dev, B*10*/,
                             uint8_t *digits /*dev or NULL*/, float *conf /*dev or NULL*/, void *stream);

/* MC dropout: DigitCNNv3.forward_with_uncertainty, ml/model_v3.py:186-214.  For each of n_samples samples s and each cell b the forward
 * runs with the network's three dropouts active -- spatial dropout (:80-92, whole channels, x * keep / (1 - p_spatial)) on layer1's 32 and
 * layer3's 64 output channels (:167, :170), nn.Dropout(p_fc) on the 128 pooled features (:181) -- and probs = softmax(logits /
 * temperature).  mean f32 [B,10]: the mean over the samples; std f32 [B,10]: their unbiased standard deviation (divisor n_samples - 1; NaN
 * for one sample, as torch.std); predicted int64 [B]: the first maximum of mean.  logits_out f32 [n_samples,B,10]: the per-sample logits.
 * keep*_out u8 [n_samples,B,32], [n_samples,B,64], [n_samples,B,128]: the masks that were used, 1 = keep.  Every output may be NULL.
 *
 * DEVIATION, deliberate: BatchNorm keeps its running statistics.  The reference enables dropout with self.train() (:200), which also
 * switches its eleven BatchNorms to batch statistics and overwrites their running buffers on every sample, so its result depends on
 * what else is in the batch and every later eval forward changes.  Here nothing of the model is written, a cell's results do not depend
 * on the rest of the batch, and with both rates 0 every sample's logits are sv_cnn3_forward_f32's bit for bit (std exactly 0).
 *
 * Masks.  keep*_in (all three, or all NULL): the caller's masks in the shapes of keep*_out, nonzero = keep; they replace the generator.
 * Otherwise a keep bit is a pure function of (seed, offset, s, b, site, channel) -- not of B, n_samples or how the work is chunked --
 * drawn by Philox4x32-10 (csrc/sv_philox.h):
 *     key     = (seed & 0xffffffff, seed >> 32)
 *     counter = (b, s, site * 64 + channel / 4 + ((offset >> 32 & 0xffffff) << 8), offset & 0xffffffff)
 *     the four output words serve channels 4g .. 4g + 3; site 0 = layer1, 1 = layer3, 2 = the features
 *     keep    = (uint64)word < llrint((1.0 - (double)p) * 4294967296.0)           always at p = 0, never at p = 1
 * PyTorch's own draw order is not reproduced (it differs between its CPU and GPU backends anyway).  sv_mc_dropout_masks_host is the
 * same generator on the host.
 *
 * Stem and layer1 run once per cell, layers 2..5 per (sample, cell), in chunks of SV_V3_SUBBATCH / n_samples whole cells; results repeat
 * bit for bit.  Scratch: the forward's activations for SV_V3_SUBBATCH cells plus 49 MiB of the entry's own, constant, sized by
 * sv_ctx_reserve / sv_load_weights_v3_f32 like the forward's: after sv_ctx_reserve the entry allocates nothing and can be captured in a
 * hipGraph.  seed, offset and the mask pointers are launch arguments: a replay repeats the captured masks.  Asynchronous on `stream`.
 * SV_ERR_NO_WEIGHTS and SV_ERR_UNSUPPORTED as sv_cnn3_forward_f32; SV_ERR_BAD_ARG for p_spatial outside [0, 1), p_fc outside [0, 1],
 * n_samples < 1 or > SV_V3_SUBBATCH, or some but not all of keep*_in.  B = 0 is SV_OK. */
int sv_cnn3_forward_mc_f32(sv_ctx *ctx, const float *x /*dev, B*784*/, long B, int n_samples, float p_spatial, float p_fc, uint64_t seed, uint64_t offset,
                           const uint8_t *keep1_in /*dev or NULL*/, const uint8_t *keep3_in /*dev or NULL*/, const uint8_t *keepf_in /*dev or NULL*/,
                           float *mean /*dev, B*10, or NULL*/, float *std /*dev, B*10, or NULL*/, int64_t *predicted /*dev, B, or NULL*/,
                           float *logits_out /*dev, n_samples*B*10, or NULL*/, uint8_t *keep1_out /*dev or NULL*/, uint8_t *keep3_out /*dev or NULL*/,
                           uint8_t *keepf_out /*dev or NULL*/, void *stream);

/* The masks sv_cnn3_forward_mc_f32 draws at (seed, offset) with keep*_in NULL, on the host: keep1 u8 [n_samples,B,32], keep3
 * [n_samples,B,64], keepf [n_samples,B,128], each or NULL.  Needs no context and no GPU.  SV_ERR_BAD_ARG for the rates as above,
 * n_samples < 1 or B < 0. */
int sv_mc_dropout_masks_host(uint64_t seed, uint64_t offset, int n_samples, long B, float p_spatial, float p_fc, uint8_t *keep1 /*host*/,
                             uint8_t *keep3 /*host*/, uint8_t *keepf /*host*/);

/* sv_frames_to_digits with the v3 model: K2, then sv_cnn3_forward_cells_u8 (pipeline/run_v2.py:149-163 after the warp). */
int sv_frames_to_digits_v3(sv_ctx *ctx, const uint8_t *frames /*dev*/, int n, int H, int W,
                           ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv /*dev, n*9*/, int glue,
                           uint8_t *cells /*dev n*81*784 or NULL*/, float *logits /*dev, n*81*10*/,
                           uint8_t *digits /*dev, n*81*/, float *conf /*dev n*81 or NULL*/, void *stream);

/* ---- K12: DigitCNNv3Light and EmptyClassifier forwards (ml/model_v3.py:232-320) -------------------------------------------------- */

/* Floats in the weight blobs of sv_load_weights_v3_light_f32 and sv_load_weights_empty_f32. */
#define SV_CNN3_LIGHT_PARAMS 53699
#define SV_CNN3_LIGHT_FEATURES 96
#define SV_EMPTY_PARAMS 55041

/* blob: the state_dict of DigitCNNv3Light (ml/model_v3.py:245-270) flattened in key order, the int64 num_batches_tracked entries skipped:
 * temperature[1] features.0.weight[24,1,3,3] features.1.{weight,bias,running_mean,running_var}[24] features.4.weight[48,24,3,3]
 * features.5.{...}[48] features.8.weight[96,48,3,3] features.9.{...}[96] fc.weight[10,96] fc.bias[10].  n_floats must be
 * SV_CNN3_LIGHT_PARAMS, else SV_ERR_BAD_ARG.  Every BatchNorm is folded into its convolution here, in double, with eps = 1e-5.
 * Synchronous.  The model has a weight slot of its own: a context may hold the DigitCNN, DigitCNNv3, DigitCNNv3Light and EmptyClassifier
 * weights at once, and loading one leaves the others as they are.  The Light and Empty forwards need no scratch of their own. */
int sv_load_weights_v3_light_f32(sv_ctx *ctx, const float *blob /*host*/, long n_floats);

/* DigitCNNv3Light.forward, ml/model_v3.py:272-276 (eval mode), in true f32 on v_mfma_f32_16x16x4_f32, one launch, activations in LDS:
 * x f32 [B,1,28,28] -> logits f32 [B,10].  features: the 96 pooled values the fc layer reads (:274).  digits: argmax of the logits.
 * conf: softmax(logits / temperature) at that digit, get_confidence (:278-282).  Each may be NULL.  A cell's results do not depend on
 * the rest of the batch, and a cell holding NaN/Inf does not disturb the others (its own logits are unspecified).  B = 0 is SV_OK.
 * SV_ERR_NO_WEIGHTS before sv_load_weights_v3_light_f32; SV_ERR_UNSUPPORTED on a context set to SV_PREC_BF16.
 * After sv_ctx_reserve no Light or Empty entry allocates, so they can be captured in a hipGraph. */
int sv_cnn3_light_forward_f32(sv_ctx *ctx, const float *x /*dev, B*784*/, long B, float *logits /*dev, B*10*/,
                              float *features /*dev, B*96, or NULL*/, uint8_t *digits /*dev, B, or NULL*/, float *conf /*dev, B, or NULL*/,
                              void *stream);

/* The same on 8-bit cells with the glue fused in, as sv_cnn3_forward_cells_u8. */
int sv_cnn3_light_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells /*dev, B*784*/, long B, int glue, float *logits /*dev, B*10*/,
                                   uint8_t *digits /*dev or NULL*/, float *conf /*dev or NULL*/, void *stream);

/* sv_frames_to_digits with the Light model: K2, then sv_cnn3_light_forward_cells_u8. */
int sv_frames_to_digits_v3_light(sv_ctx *ctx, const uint8_t *frames /*dev*/, int n, int H, int W,
                                 ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv /*dev, n*9*/, int glue,
                                 uint8_t *cells /*dev n*81*784 or NULL*/, float *logits /*dev, n*81*10*/,
                                 uint8_t *digits /*dev, n*81*/, float *conf /*dev n*81 or NULL*/, void *stream);

/* blob: the state_dict of EmptyClassifier (ml/model_v3.py:292-311) flattened in key order: features.0.weight[16,1,3,3] features.0.bias[16]
 * features.3.weight[32,16,3,3] features.3.bias[32] classifier.1.weight[32,1568] classifier.1.bias[32] classifier.4.weight[1,32]
 * classifier.4.bias[1].  n_floats must be SV_EMPTY_PARAMS, else SV_ERR_BAD_ARG.  Synchronous; a weight slot of its own. */
int sv_load_weights_empty_f32(sv_ctx *ctx, const float *blob /*host*/, long n_floats);

/* EmptyClassifier.forward, ml/model_v3.py:313-315 (eval mode), true f32, one launch: x f32 [B,1,28,28] -> logit f32 [B,1].  The sigmoid
 * and threshold of is_empty (:317-320) are the caller's.  Batch independence, NaN isolation, B = 0 and the error codes as
 * sv_cnn3_light_forward_f32, with sv_load_weights_empty_f32 as the load. */
int sv_empty_forward_f32(sv_ctx *ctx, const float *x /*dev, B*784*/, long B, float *logit /*dev, B*/, void *stream);

/* The same on 8-bit cells with the glue fused in. */
int sv_empty_forward_cells_u8(sv_ctx *ctx, const uint8_t *cells /*dev, B*784*/, long B, int glue, float *logit /*dev, B*/, void *stream);

/* F.softmax(output, dim=1) then probs.topk(top_k), pipeline/run_v2.py:165-178 (predict_cells_with_alternatives):
 * per cell the k most probable classes, most probable first (index[.,0] = the predicted digit, prob[.,0] = its
 * confidence, the rest = run_v2's `alternatives`).  1 <= k <= 10.
 * Ties: equal probabilities come lower class index first (bit-equal logits always tie; so do the classes of a confident cell whose
 * exponentials underflow to 0.0).  sv_resolve_conflicts' slot order relies on it.
 * Rows that are not finite: a NaN or +inf logit, or ten -inf, make the row's denominator NaN; every prob of that row is then NaN and
 * its k indices are still distinct classes (the finite exponentials by value, the rest by class index); other rows are unaffected.
 * -inf beside finite logits is an ordinary probability of 0. */
int sv_softmax_topk_f32(sv_ctx *ctx, const float *logits /*dev, B*10*/, long B, int k,
                        uint8_t *index /*dev, B*k*/, float *prob /*dev, B*k*/, void *stream);

/* ---- K21: model evaluation metrics (ml/evaluate_v2.py:67-220 evaluate_dataset / compute_calibration / find_failures,
 * ml/train.py:157-190 evaluate) -- the bookkeeping the reference does on the host, one cell and one class at a time, in one pass
 * over the logits on the device (csrc/k21_eval.hip). */
#define SV_EVAL_MAX_BINS 64
#define SV_EVAL_CONF_ONE 1073741824ull   /* 2^30: the unit of the fixed-point confidence sums */

/* The aggregates, one small device block, every field an integer.  A cell is VALID when its ten inputs are finite and its label is
 * 0..9; only valid cells enter confusion, n, n_correct, n_wrong, the bins and the totals.  A cell with a NaN or Inf input counts in
 * `nonfinite` and nowhere else; a finite cell whose label is outside 0..9 counts in `bad_labels` and nowhere else.
 * Confidence sums are sums of (uint64_t)(conf * 2^30).  conf is the largest of ten f32 probabilities that sum to about 1, so
 * conf >= 0.1 > 2^-7: an f32 that large is a whole multiple of 2^-30, so the product is an integer below 2^31, exact, and so is the
 * conversion: the sum is the exact sum of the f32 confidences (times 2^30) while B * 2^30 < 2^62, whatever the launch shape and whatever order the atomics land in.  (In probability-input mode
 * that holds for rows that are probabilities; a largest entry below 2^-7 is truncated to a multiple of 2^-30.) */
typedef struct sv_eval_stats {
    uint64_t confusion[10][10];                 /* [label][pred] */
    uint64_t n, n_correct, n_wrong;             /* valid cells; pred == label; pred != label */
    uint64_t bad_labels, nonfinite;
    uint64_t bin_count[SV_EVAL_MAX_BINS];       /* reliability bins (ml/evaluate_v2.py:162-168): cells, correct cells, sum of conf */
    uint64_t bin_correct[SV_EVAL_MAX_BINS];
    uint64_t bin_conf[SV_EVAL_MAX_BINS];
    uint64_t tot_count[3], tot_correct[3], tot_conf[3];   /* the same three sums over [0] all valid, [1] correct, [2] wrong cells */
} sv_eval_stats;

/* One misclassified cell (ml/evaluate_v2.py:208-217): index = index_base + its position in the call, top3 = its three most probable
 * classes, most probable first, equal probabilities lowest class first (the selection of sv_softmax_topk_f32). */
typedef struct sv_eval_failure {
    int64_t index;
    int32_t label, pred;
    float conf, true_prob;
    int32_t top3_index[3];
    float top3_prob[3];
} sv_eval_failure;

/* input f32 [B,10], contiguous: logits (input_is_prob == 0) or probabilities (!= 0: compute_calibration's argument, temperature
 * must be 1).  labels [B]: int64 (labels_i64 != 0) or int32.  Per cell, in f32:
 *   p = softmax(input / temperature) by k_softmax_topk's sequence of operations -- z = input / T, m = max z, e = expf(z - m),
 *   den = e0 + ... + e9 in class order, p = e / den -- so probs is bit-identical to what sv_softmax_topk_f32 returns for the same
 *   logits at T = 1; in probability mode p = input;
 *   pred = argmax of the input, ties to the lowest class, a NaN entry counting as the largest and the first NaN winning (np.argmax,
 *   torch.argmax); conf = p[pred]; true_prob = p[label];
 *   nll = logsumexp(z) - z[label] = logf(den) - (z[label] - m)   (probability mode: -logf(p[label]));  correct = pred == label.
 * Per-cell outputs, each [dev] and each may be NULL: probs [B*10], pred [B], conf [B], true_prob [B], nll [B], correct [B].  A cell
 * that is not finite gets whatever the arithmetic gives (NaN probabilities) and correct 0; a bad label gets true_prob = nll = NaN.
 * In probability mode a row whose largest entry is outside [0, 1] counts as not finite.
 * Bins: bin_edges [host, n_bins + 1] non-decreasing doubles, 1 <= n_bins <= SV_EVAL_MAX_BINS (they travel as a kernel argument: the
 * pointer is not kept).  A cell is in bin i when (double)conf > bin_edges[i] && (double)conf <= bin_edges[i + 1]
 * (ml/evaluate_v2.py:163); a cell in no bin is in no bin.
 * stats [dev, 8-byte aligned]: cleared first by a launch on the stream unless accumulate != 0, then added to -- counts per workgroup in
 * LDS and one integer atomic per non-zero entry and workgroup, no float atomic anywhere -- so one call over B cells and any split of
 * them into accumulating calls leave the same bytes.
 * failures [dev, max_failures records, or NULL with max_failures 0]: record r is the r-th wrong valid cell in sample order counted
 * from the last clear of stats (ml/evaluate_v2.py:203-206: the list stops at max_failures); its place comes from a prefix sum over
 * the wrong flags (per workgroup counts, one scan launch), not from an atomic append.  stats->n_wrong is the total whatever
 * max_failures is.  Records past min(n_wrong, max_failures) are not written.  Every accumulating call's wrong cells take their places,
 * whatever its own max_failures: a call with max_failures 0 between two others writes nothing, the later call's records start behind
 * the places of its wrong cells, and the records of those places stay unwritten.
 * Asynchronous on `stream`; reads nothing back.  Scratch (only with max_failures > 0) lives in the context and only grows: a first
 * call at a larger B allocates, so warm up before capturing into a graph.
 * SV_ERR_BAD_ARG: NULL ctx / input / labels / stats / bin_edges, B < 0 or B * 2^30 >= 2^62, index_base < 0, temperature not finite
 * or <= 0, bad n_bins or edges, max_failures < 0.  B == 0 is SV_OK (stats is still cleared unless accumulate). */
int sv_eval_metrics(sv_ctx *ctx, const float *input /*dev, B*10*/, int input_is_prob, const void *labels /*dev, B*/, int labels_i64, long B,
                    long index_base, float temperature, const double *bin_edges /*host, n_bins+1*/, int n_bins, int accumulate,
                    float *probs /*dev*/, uint8_t *pred /*dev*/, float *conf /*dev*/, float *true_prob /*dev*/, float *nll /*dev*/,
                    uint8_t *correct /*dev*/, sv_eval_stats *stats /*dev*/, sv_eval_failure *failures /*dev*/, long max_failures, void *stream);

/* sv_eval_metrics, then *stats_host = *stats: that copy and the wait for it are the one synchronisation.  SV_ERR_BAD_ARG (after the
 * copy: stats_host is filled in and the other cells are counted) when stats_host->bad_labels > 0. */
int sv_eval_metrics_host(sv_ctx *ctx, const float *input /*dev, B*10*/, int input_is_prob, const void *labels /*dev, B*/, int labels_i64, long B,
                         long index_base, float temperature, const double *bin_edges /*host, n_bins+1*/, int n_bins, int accumulate,
                         float *probs /*dev*/, uint8_t *pred /*dev*/, float *conf /*dev*/, float *true_prob /*dev*/, float *nll /*dev*/,
                         uint8_t *correct /*dev*/, sv_eval_stats *stats /*dev*/, sv_eval_failure *failures /*dev*/, long max_failures,
                         sv_eval_stats *stats_host /*host*/, void *stream);

/* The validation and correction stage of pipeline/run_v2.py:344-371 for n frames in one launch: validate_predictions
 * (pipeline/validator.py:69-159) on the 81 cells of each frame and, where they break the sudoku rules, ConflictResolver.resolve
 * (pipeline/conflict_resolver.py:58-286): a beam search over the cells' alternatives for the cheapest <= max_corrections corrections.
 * Exact: every output equals the reference's; the f64 score equals it to the bit whenever no confidence of a filled cell or of a
 * qualifying alternative is below 2^-18 (then the sum of 81 of them is exact in a double in any order; softmax top-1 values and
 * alternatives that passed min_alt_conf = 0.1 always are), and is otherwise within rounding of it.  That is the domain in which
 * "to the bit" is defined: every confidence that can enter a path's sum (top-1 of a filled cell, any qualifying alternative) is 0 or
 * >= 2^-18.  A min_alt_conf below 2^-18 leaves it; outside it even CPython's own sum() depends on its version (compensated from 3.12).
 * index, prob: the output of sv_softmax_topk_f32 over n*81 cells; per cell digit = index[.,0] (0 = empty), confidence = prob[.,0],
 * alternatives = slots 1..k-1.  Classes are 0..9 (any other value is read as an empty cell / no alternative), probabilities finite
 * and >= 0.  run_v2 passes beam_width 5, max_corrections 3, and min_alt_conf is ConflictResolver's default 0.1 (:65).
 * acceptance_rule != 0 applies pipeline/run_v2.py:365 on the device: a repair that neither succeeded nor left fewer conflicts than
 * the input had is dropped, and digits, conf, index_out, prob_out, num_conflicts_after, conflict_count, n_corrections, corr_cells and
 * corr_conf then describe the input (no corrections); success, paths_explored and score stay what the search reported.
 * Outputs, each may be NULL; index_out / prob_out may be index / prob themselves:
 *   digits, conf [n*81]              the resulting cells: corrected when success, else the best attempt, or the input when no
 *                                    alternative qualified (ResolutionResult.cells); callers apply run_v2.py:365 to accept them
 *   index_out, prob_out [n*81*k]     the same cells with their alternatives as _apply_correction (:225-244) leaves them: the old digit
 *                                    first, then the others; a slot the correction emptied holds index 255, prob 0
 *   success [n]                      ResolutionResult.success
 *   num_conflicts_before/_after [n]  ValidationResult.num_conflicts of the input and of the resulting cells
 *   conflict_count [n*81]            how many conflicts of the resulting cells name each cell (0-3); != 0: cells_in_conflict
 *   n_corrections [n], corr_cells [n*3*3] = (cell, old digit, new digit), corr_conf [n*3*2] = (old confidence, alternative's
 *                                    confidence): corrections_made in order; unused entries are 0
 *   paths_explored [n], score [n]    as the reference reports them (score 0 unless a correction made the frame valid)
 * One wave per frame; a frame's result does not depend on the rest of the batch.  1 <= k <= 4, 1 <= beam_width <= 6,
 * 0 <= max_corrections <= 3, otherwise SV_ERR_UNSUPPORTED; n == 0 is SV_OK. */
int sv_resolve_conflicts(sv_ctx *ctx, const uint8_t *index /*dev, n*81*k*/, const float *prob /*dev, n*81*k*/, long n, int k,
                         int beam_width, int max_corrections, double min_alt_conf, int acceptance_rule, uint8_t *digits /*dev*/, float *conf /*dev*/,
                         uint8_t *index_out /*dev*/, float *prob_out /*dev*/, uint8_t *success /*dev*/,
                         int32_t *num_conflicts_before /*dev*/, int32_t *num_conflicts_after /*dev*/, uint8_t *conflict_count /*dev*/,
                         uint8_t *n_corrections /*dev*/, uint8_t *corr_cells /*dev*/, float *corr_conf /*dev*/,
                         int32_t *paths_explored /*dev*/, double *score /*dev*/, void *stream);

/* The last stage of pipeline/run_v2.py before the solver (:373-391), resolve_with_constraints(recognized_grid, confidences), for n
 * frames in one launch: ConstraintResolver.__init__ + propagate (pipeline/constraint_resolver.py:48-267): naked and hidden singles
 * until nothing moves, a contradiction, or max_iterations passes.  Every output equals the reference's, on contradictory grids too,
 * where the result depends on the order in which CPython's list(set(...)) hands back the hidden singles of a pass (:200): the
 * kernel replays that set (CPython 3.8+: the tuple hash of (row, col, digit) and Objects/setobject.c's table).
 * digits: 0 = empty, 1..9; conf: the cells' confidences, or NULL for the reference's default 1.0 everywhere.
 * Outputs, each may be NULL; grid may be digits itself:
 *   grid [n*81]               PropagationResult.grid
 *   candidates [n*81]         Cell.candidates as a mask, bit d (1..9) set = d still possible; a placed cell holds its digit alone, a
 *                             cell that came filled holds its digit unless a peer showed the same one (then nothing)
 *   is_valid [n]              0 when a contradiction was found (run_v2 then reports the frame `invalid`)
 *   iterations [n]            passes run, the one that found no progress included
 *   contradiction_cell [n]    9 * row + col, 255 = none
 *   n_resolved [n], resolved [n*81*2] = (cell, digit): cells_resolved in order; unused entries are 255
 *   is_fixed [n*81]           Cell.is_fixed: digit > 0 and (double)conf > 0.9
 * A frame holding a byte above 9 is no grid: is_valid 0, iterations 0, contradiction_cell 255, grid = digits, candidates 0,
 * n_resolved 0; nothing is indexed with such a byte.  One wave per frame; a frame's result does not depend on the rest of the batch.
 * 1 <= max_iterations <= 100 (the reference's default), otherwise SV_ERR_UNSUPPORTED; n == 0 is SV_OK. */
int sv_propagate_constraints(sv_ctx *ctx, const uint8_t *digits /*dev, n*81*/, const float *conf /*dev, n*81, or NULL*/, long n,
                             int max_iterations, uint8_t *grid /*dev*/, uint16_t *candidates /*dev*/, uint8_t *is_valid /*dev*/,
                             int32_t *iterations /*dev*/, uint8_t *contradiction_cell /*dev*/, uint8_t *n_resolved /*dev*/,
                             uint8_t *resolved /*dev*/, uint8_t *is_fixed /*dev*/, void *stream);

/* ---- N4: JPEG front end -- what cv2.imread does before the path starts (pipeline/run.py:250, pipeline/run_v2.py:267,
 * tests/test_integration.py:126).  Baseline / extended-sequential Huffman JPEG, 8-bit, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0,
 * restart intervals, EXIF orientation applied as imread applies it.  The serial Huffman bit stream is decoded on the host
 * (threads: restart intervals of one image, or images of a batch); dequantisation, the inverse DCT (libjpeg's JDCT_ISLOW),
 * "fancy" chroma up-sampling, YCbCr -> BGR and the orientation run on the GPU, so the frame is born in HBM where K1 and K2
 * read it.  Progressive, arithmetic-coded, 12-bit, CMYK files: SV_ERR_UNSUPPORTED. */
typedef struct sv_jpeg_info {
    int width, height;              /* as stored */
    int out_width, out_height;      /* after the EXIF orientation: the shape imread returns */
    int components;                 /* 1 (gray) or 3 (YCbCr) */
    int h_samp, v_samp;             /* luma sampling factors: 1x1, 2x1 or 2x2 */
    int orientation;                /* EXIF tag 0x0112, 1..8 (1 when absent) */
    int restart_interval;           /* MCUs, 0 = none */
    long coef_count;                /* int16 values sv_jpeg_entropy_decode writes (64 per block) */
    long sparse_capacity;           /* values sv_jpeg_entropy_decode_sparse may need room for (bound from the file size) */
} sv_jpeg_info;

int sv_jpeg_parse(const uint8_t *data /*host*/, size_t size, sv_jpeg_info *info);

/* Huffman decoding -> coefficient blocks: per component, blocks row-major over the MCU-padded block grid, 64 values per
 * block in natural (row-major, de-zigzagged) order; quant: 3 x 64 quantiser steps, natural order, per component. */
int sv_jpeg_entropy_decode(const uint8_t *data /*host*/, size_t size, int16_t *coef /*host, coef_count*/,
                           uint16_t *quant /*host, 192*/, int threads);
/* The same in the compact form that crosses PCIe: per block (same block order) a 64-bit mask over ZIGZAG positions and the
 * index of the block's first value; `values` receives the non-zero coefficients, zigzag order, block after block.  A q90
 * 1080p frame is ~2 MB this way instead of 6.3 MB.  values_used: every index the masks/offsets refer to is below it (copy
 * that prefix).  SV_ERR_BUFFER when values_cap < info.sparse_capacity turns out too small. */
int sv_jpeg_entropy_decode_sparse(const uint8_t *data /*host*/, size_t size, uint64_t *masks /*host, coef_count/64*/,
                                  uint32_t *offsets /*host, coef_count/64*/, int16_t *values /*host, values_cap*/,
                                  long values_cap, long *values_used, uint16_t *quant /*host, 192*/, int threads);

/* A batch of files over `threads` host threads.  Dense output when coefs != NULL (masks..values_used ignored), sparse output
 * otherwise.  status[i] = per-image sv_status; returns the first failure. */
int sv_jpeg_entropy_decode_batch(const uint8_t *const *datas, const size_t *sizes, int n, int16_t *const *coefs /*host or NULL*/,
                                 uint64_t *const *masks, uint32_t *const *offsets, int16_t *const *values,
                                 const long *values_cap, long *values_used, uint16_t *quants /*host, n*192*/,
                                 int threads, int *status /*n*/);

/* Device half: coefficients -> BGR frame (out_height x out_width x 3, row pitch `pitch` bytes), asynchronous on `stream`. */
int sv_jpeg_reconstruct_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const int16_t *coef /*dev*/,
                               const uint16_t *quant /*dev, 192*/, uint8_t *bgr /*dev*/, ptrdiff_t pitch, void *stream);
int sv_jpeg_reconstruct_sparse_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const uint64_t *masks /*dev*/,
                                      const uint32_t *offsets /*dev*/, const int16_t *values /*dev*/,
                                      const uint16_t *quant /*dev, 192*/, uint8_t *bgr /*dev*/, ptrdiff_t pitch, void *stream);

/* Reduced-size decode: libjpeg's scale_denom, what cv2.imread(path, cv2.IMREAD_REDUCED_COLOR_2 / _4 / _8) asks for.  The entropy
 * stage is the one above (every coefficient is still decoded); the device half runs libjpeg's 4x4 / 2x2 / 1x1 inverse DCTs
 * (jidctred.c), decodes 4:2:0 chroma at twice the luma block size instead of up-sampling it (jdmaster.c), and never produces
 * the full-size image.  Bit-identical to libjpeg-turbo at the same scale.  scale_denom is 1, 2, 4 or 8 (1: the entries above,
 * unchanged); anything else is SV_ERR_BAD_ARG.  The frame is ceil(out_height / d) x ceil(out_width / d) x 3: */
int sv_jpeg_scaled_size(const sv_jpeg_info *info, int scale_denom, int *out_width, int *out_height);
int sv_jpeg_reconstruct_scaled_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const int16_t *coef /*dev*/,
                                      const uint16_t *quant /*dev, 192*/, uint8_t *bgr /*dev*/, ptrdiff_t pitch, void *stream,
                                      int scale_denom);
int sv_jpeg_reconstruct_sparse_scaled_bgr_u8(sv_ctx *ctx, const sv_jpeg_info *info, const uint64_t *masks /*dev*/,
                                             const uint32_t *offsets /*dev*/, const int16_t *values /*dev*/,
                                             const uint16_t *quant /*dev, 192*/, uint8_t *bgr /*dev*/, ptrdiff_t pitch,
                                             void *stream, int scale_denom);

/* Grayscale read: cv2.imread(path, cv2.IMREAD_GRAYSCALE) and IMREAD_REDUCED_GRAYSCALE_2 / _4 / _8 of a JPEG file (ml/datasets.py:81,153,
 * ml/evaluate.py:67, tools/augment_data.py:328,361, tools/dataset_stats.py:211,245, tools/label_cells.py:42).  OpenCV asks libjpeg for
 * JCS_GRAYSCALE, and libjpeg then returns the inverse DCT of the Y component and never decodes Cb or Cr -- not the gray conversion of the colour
 * image.  So does this: the luma mode of the entropy decoder parses the chroma blocks of an interleaved scan (to stay in step with the bit
 * stream) and stores Y's alone; the device half transforms them straight into the caller's [H, W] image.  Bit-identical to libjpeg-turbo's
 * JCS_GRAYSCALE output at scale_denom 1, 2, 4 and 8; the EXIF orientation is applied as imread applies it.  Every file the colour entries refuse
 * is refused here with the same status.
 *
 * sv_jpeg_parse_luma fills sv_jpeg_info as sv_jpeg_parse does, except coef_count and sparse_capacity: they count Y's blocks (64 values each)
 * and the room Y's values may need.  Size staging from them, and hand this info to the reconstruct entries below.
 * Y's blocks lie in scan order: MCU after MCU (row-major), the h_samp x v_samp blocks of an MCU row-major; so the block at raster position
 * (bx, by) is record ((by / v_samp) * mcu_cols + bx / h_samp) * h_samp * v_samp + (by % v_samp) * h_samp + bx % h_samp, with
 * mcu_cols = ceil(width / (8 * h_samp)).  For a single-component file this is sv_jpeg_entropy_decode's layout.  quant: Y's 64 steps alone. */
int sv_jpeg_parse_luma(const uint8_t *data /*host*/, size_t size, sv_jpeg_info *info);
int sv_jpeg_entropy_decode_luma(const uint8_t *data /*host*/, size_t size, int16_t *coef /*host, coef_count*/,
                                uint16_t *quant /*host, 64*/, int threads);
int sv_jpeg_entropy_decode_luma_sparse(const uint8_t *data /*host*/, size_t size, uint64_t *masks /*host, coef_count/64*/,
                                       uint32_t *offsets /*host, coef_count/64*/, int16_t *values /*host, values_cap*/,
                                       long values_cap, long *values_used, uint16_t *quant /*host, 64*/, int threads);
int sv_jpeg_entropy_decode_luma_batch(const uint8_t *const *datas, const size_t *sizes, int n, int16_t *const *coefs /*host or NULL*/,
                                      uint64_t *const *masks, uint32_t *const *offsets, int16_t *const *values,
                                      const long *values_cap, long *values_used, uint16_t *quants /*host, n*64*/,
                                      int threads, int *status /*n*/);
/* Device half: Y records -> gray image, ceil(out_height / scale_denom) x ceil(out_width / scale_denom) bytes, row pitch `pitch` bytes (any
 * alignment), asynchronous on `stream`.  No scratch memory.  Status codes are those of the BGR entries. */
int sv_jpeg_reconstruct_gray_u8(sv_ctx *ctx, const sv_jpeg_info *info /*sv_jpeg_parse_luma's*/, const int16_t *coef /*dev*/,
                                const uint16_t *quant /*dev, 64*/, uint8_t *gray /*dev*/, ptrdiff_t pitch, void *stream,
                                int scale_denom);
int sv_jpeg_reconstruct_sparse_gray_u8(sv_ctx *ctx, const sv_jpeg_info *info /*sv_jpeg_parse_luma's*/, const uint64_t *masks /*dev*/,
                                       const uint32_t *offsets /*dev*/, const int16_t *values /*dev*/,
                                       const uint16_t *quant /*dev, 64*/, uint8_t *gray /*dev*/, ptrdiff_t pitch,
                                       void *stream, int scale_denom);

/* ---- JPEG encoder -- what cv2.imwrite does after the path ends (pipeline/run.py:431: cv2.imwrite(args.output, overlay)).  Baseline JPEG, 8-bit,
 * gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0, optional restart interval.  The mirror image of the decoder above: colour conversion, down-sampling, edge
 * replication, the forward DCT (libjpeg's JDCT_ISLOW) and quantisation run on the GPU and leave the coefficients in the decoder's own layouts
 * (dense, or the compact mask + values form that crosses PCIe); the serial Huffman bit packing runs on the host (threads: restart intervals of
 * one image, or images of a batch).  The file is the one libjpeg-turbo writes with its defaults -- Annex K Huffman tables, no optimize_coding,
 * baseline-forced quantiser tables, JFIF 1.01 header, density 1:1 -- byte for byte.  Progressive, optimised tables, arithmetic coding, 12-bit
 * samples, EXIF: not written. */
#define SV_JPEG_444 0
#define SV_JPEG_422 1
#define SV_JPEG_420 2
typedef struct sv_jpeg_enc {
    sv_jpeg_info info;              /* the geometry in the decoder's terms (orientation 1, out size = size); coef_count as above */
    int quality;                    /* 1..100 */
    uint16_t quant[192];            /* quantiser steps, natural order, per component (chroma twice) */
    uint32_t recip[192];            /* ceil(2^32 / (8 * quant)): the device quantiser's multipliers */
    long out_bound;                 /* bytes that hold the file whatever the image */
} sv_jpeg_enc;

/* components 1 (gray; sampling ignored) or 3; sampling SV_JPEG_444 / _422 / _420; quality 1..100 (jpeg_set_quality, force_baseline);
 * restart: MCUs per restart interval, 0..65535 (0 = none).  Anything else, or a non-positive size, or a side above 65535: SV_ERR_BAD_ARG. */
int sv_jpeg_encode_plan(int width, int height, int components, int sampling, int quality, int restart, sv_jpeg_enc *plan);
/* Bytes that hold the file of an image whose sparse form has values_count values (far below plan->out_bound for real images) */
long sv_jpeg_encode_bound(const sv_jpeg_enc *plan, long values_count);

/* Device half, n frames of plan's size (BGR: plan of 3 components; gray: of 1), row pitch `pitch` >= row bytes and frame stride img_stride
 * in bytes, any alignment; asynchronous on `stream`.  Dense output: coef != NULL receives n * coef_count values in sv_jpeg_entropy_decode's
 * layout (16-byte aligned).  Sparse output: masks, offsets (n * coef_count / 64 each), values (n * coef_count: frame f's values start at
 * f * coef_count; offsets are relative to that) and counts (n: values of each frame, so the host copies only that prefix) -- all four or none;
 * exactly what sv_jpeg_entropy_decode_sparse produces for the file, so sv_jpeg_reconstruct_sparse_bgr_u8 takes a frame's records as they are.
 * With coef == NULL the dense blocks live in the context's scratch.  SV_ERR_BAD_ARG: NULL frames, no output at all, n outside 1..65535,
 * pitch < row bytes, a plan whose component count does not match the entry. */
int sv_jpeg_forward_bgr_u8(sv_ctx *ctx, const sv_jpeg_enc *plan, const uint8_t *bgr /*dev*/, int n, ptrdiff_t pitch, ptrdiff_t img_stride,
                           int16_t *coef /*dev or NULL*/, uint64_t *masks /*dev or NULL*/, uint32_t *offsets /*dev*/, int16_t *values /*dev*/,
                           uint32_t *counts /*dev*/, void *stream);
int sv_jpeg_forward_gray_u8(sv_ctx *ctx, const sv_jpeg_enc *plan, const uint8_t *gray /*dev*/, int n, ptrdiff_t pitch, ptrdiff_t img_stride,
                            int16_t *coef /*dev or NULL*/, uint64_t *masks /*dev or NULL*/, uint32_t *offsets /*dev*/, int16_t *values /*dev*/,
                            uint32_t *counts /*dev*/, void *stream);

/* Host half: one frame's sparse records -> the file.  values_count: the frame's count; records that refer beyond it, a zero value under a set
 * mask bit or a value no baseline code exists for are SV_ERR_BAD_ARG.  *out_size bytes are written; SV_ERR_BUFFER (with *out_size = what is
 * needed) when out_cap is too small.  threads > 1 work on restart intervals; the bytes do not depend on threads. */
int sv_jpeg_entropy_encode(const sv_jpeg_enc *plan, const uint64_t *masks /*host*/, const uint32_t *offsets /*host*/, const int16_t *values /*host*/,
                           long values_count, uint8_t *out /*host*/, size_t out_cap, size_t *out_size, int threads);
/* n frames of one plan over `threads` host threads.  status[i] = per-image sv_status; returns the first failure. */
int sv_jpeg_entropy_encode_batch(const sv_jpeg_enc *plan, int n, const uint64_t *const *masks, const uint32_t *const *offsets,
                                 const int16_t *const *values, const long *values_count, uint8_t *const *outs, const size_t *out_caps,
                                 size_t *out_sizes, int threads, int *status /*n*/);

/* ---- PNG encoder -- the lossless way out of HBM (pipeline/run.py --output solved.png, tools/extract_cells.py's warped_grid.png and cell_r_c.png).
 * 8 bits per sample, non-interlaced, colour type 2 (RGB, from BGR frames) or 0 (gray); chunks IHDR, one IDAT, IEND.  The IDAT payload is a zlib
 * stream: 78 01, the bands' deflate streams in order, the final empty block 03 00, the Adler-32 of the filtered bytes.  A band is band_rows whole
 * rows, filtered from original neighbours and compressed on its own (distance-1 matches only, Z_RLE; one dynamic Huffman block, or one stored block
 * when that is no larger), ended on a byte boundary by an empty stored block: the GPU writes every band in parallel (csrc/k18_png_encode.hip), the host
 * adds the container and the checksums (csrc/host_png.cpp).  No libz, no libpng.  16-bit samples, alpha, palettes, interlacing: not written. */
#define SV_PNG_FILTER_NONE 0
#define SV_PNG_FILTER_SUB 1             /* cv2's default when no compression parameter is given */
#define SV_PNG_FILTER_UP 2
#define SV_PNG_FILTER_AVERAGE 3
#define SV_PNG_FILTER_PAETH 4
#define SV_PNG_FILTER_ADAPTIVE 5        /* per row the filter with the smallest sum of abs((int8) byte); the lowest number on a tie */
#define SV_PNG_RLE 0                    /* literals and distance-1 matches of 3..258 bytes */
#define SV_PNG_HUFFMAN_ONLY 1           /* literals only */
#define SV_PNG_STORED 2                 /* stored blocks only */
typedef struct sv_png_enc {
    int width, height, channels;        /* channels 1 (gray) or 3 (BGR in, RGB in the file) */
    int filter, strategy;
    int band_rows, bands;               /* rows of a band (the last band has the rest), bands of a frame */
    long row_bytes;                     /* 1 + width * channels: filter-type byte and samples */
    long filtered_bytes;                /* height * row_bytes */
    long slot_bytes;                    /* device scratch of one band */
    long stream_bound;                  /* bytes that hold a frame's bands whatever the image: filtered_bytes + 10 * bands */
    long out_bound;                     /* bytes that hold the file whatever the image */
} sv_png_enc;

/* channels 1 or 3; filter SV_PNG_FILTER_*; strategy SV_PNG_*; band_rows 0 = automatic (about 32 KB of filtered bytes, at most 512 rows), else
 * 1..512 rows with band_rows * row_bytes <= 65535.  Anything else, a NULL plan, or a side outside 1..65535: SV_ERR_BAD_ARG.  A row of more than
 * 65,535 filtered bytes (width above 21,844 BGR pixels): SV_ERR_UNSUPPORTED. */
int sv_png_encode_plan(int width, int height, int channels, int filter, int strategy, int band_rows, sv_png_enc *plan);

/* Device half, n frames of plan's size (BGR: a plan of 3 channels; gray: of 1), row pitch `pitch` >= row bytes and frame stride frame_stride in
 * bytes, any alignment; asynchronous on `stream`.  stream_out receives frame f's bands, contiguous and in order, at f * plan->stream_bound;
 * band_len, adler and status (n * plan->bands each, 4-byte aligned) the length of every band's piece, the Adler-32 of its filtered bytes and 0 (a
 * status other than 0 means the band did not fit its slot: its length is 0 and the frame's stream is not a PNG's; the bound makes that
 * impossible).  The per-band slots live in the context's scratch.  SV_ERR_BAD_ARG: NULL arguments, n outside 1..65535, pitch < row bytes, frames
 * that overlap, a plan sv_png_encode_plan did not make or of the other entry's channel count, misaligned outputs. */
int sv_png_deflate_bgr_u8(sv_ctx *ctx, const sv_png_enc *plan, const uint8_t *bgr /*dev*/, int n, ptrdiff_t pitch, ptrdiff_t frame_stride,
                          uint8_t *stream_out /*dev*/, uint32_t *band_len /*dev*/, uint32_t *adler /*dev*/, uint32_t *status /*dev*/, void *stream);
int sv_png_deflate_gray_u8(sv_ctx *ctx, const sv_png_enc *plan, const uint8_t *gray /*dev*/, int n, ptrdiff_t pitch, ptrdiff_t frame_stride,
                           uint8_t *stream_out /*dev*/, uint32_t *band_len /*dev*/, uint32_t *adler /*dev*/, uint32_t *status /*dev*/, void *stream);

/* Host half: one frame's bands (their bytes back to back, band_len[plan->bands], adler[plan->bands]) -> the file.  Each band's bytes must be a
 * deflate stream of that band's filtered bytes that ends on a byte boundary without a final block, adler[] the Adler-32 of those filtered bytes.
 * A length above the band's share of stream_bound is SV_ERR_BAD_ARG.  *out_size bytes are written; SV_ERR_BUFFER (with *out_size = what is
 * needed) when out_cap is too small. */
int sv_png_assemble(const sv_png_enc *plan, const uint8_t *stream /*host*/, const uint32_t *band_len /*host*/, const uint32_t *adler /*host*/,
                    uint8_t *out /*host*/, size_t out_cap, size_t *out_size);
/* n frames of one plan over `threads` host threads.  status[i] = per-image sv_status; returns the first failure. */
int sv_png_assemble_batch(const sv_png_enc *plan, int n, const uint8_t *const *streams, const uint32_t *const *band_len, const uint32_t *const *adler,
                          uint8_t *const *outs, const size_t *out_caps, size_t *out_sizes, int threads, int *status /*n*/);

/* ---- PNG decoder -- cv2.imread(path) for a .png (pipeline/run.py:250, pipeline/run_v2.py, tools/extract_cells.py reading back warped_grid.png
 * and cell_r_c.png).  Split as the JPEG decoder is: the serial entropy stage (inflate) runs on host threads (csrc/host_png.cpp, no libz, no
 * libpng), the unfilter and the expansion to BGR on the GPU (csrc/k19_png_decode.hip).  Colour types 0, 2, 3, 4, 6 at every bit depth the
 * specification allows, non-interlaced.  The frame is what cv2.imread(path, IMREAD_COLOR) returns: 16-bit samples keep their high byte, gray
 * samples below 8 bits are scaled by bit replication, palette indices go through PLTE, alpha is dropped (not composited), gray is replicated
 * and RGB becomes BGR; tRNS, gAMA and every other ancillary chunk are ignored.  Adam7, IMREAD_UNCHANGED / _GRAYSCALE / _ANYDEPTH: not decoded. */
#define SV_PNG_MAX_FILTERED_BYTES (1L << 29)  /* 512 MiB of filtered bytes per image; a larger file is SV_ERR_UNSUPPORTED */
#define SV_PNG_MAX_SIDE 65535                 /* as for the encoder; a larger side is SV_ERR_UNSUPPORTED */
#define SV_PNG_PALETTE_STRIDE 1024            /* device palette of one image: 256 RGB entries, then the entry count as a uint32 at byte 768 */
typedef struct sv_png_info {
    int width, height;
    int bit_depth;                      /* 1, 2, 4, 8, 16 */
    int color_type;                     /* 0 gray, 2 RGB, 3 palette, 4 gray + alpha, 6 RGB + alpha */
    int interlace;                      /* 0 (a file with 1, Adam7, is refused) */
    int channels;                       /* samples per pixel in the file: 1, 3, 1, 2, 4 */
    int bpp;                            /* the filters' left distance: max(1, channels * bit_depth / 8) */
    int palette_entries;                /* 0 without PLTE */
    long row_bytes;                     /* ceil(width * channels * bit_depth / 8) */
    long filtered_bytes;                /* height * (1 + row_bytes): what the zlib stream must inflate to, exactly */
    long idat_offset;                   /* the first IDAT chunk's offset in the file */
    uint8_t palette[768];               /* PLTE's RGB entries, zero beyond palette_entries */
} sv_png_info;

/* Signature, chunk walk, the CRC-32 of every critical chunk, IHDR, PLTE (pipeline/run.py:250: what cv2.imread checks before it decodes).
 * SV_ERR_UNSUPPORTED: an Adam7 file, filtered_bytes above SV_PNG_MAX_FILTERED_BYTES, a side above SV_PNG_MAX_SIDE.  SV_ERR_BAD_ARG: anything
 * malformed -- a bad signature or CRC, a missing IHDR, IDAT or IEND, chunks out of order, IDATs that are not consecutive, colour type 3 without
 * PLTE, an unknown critical chunk, a (colour type, depth) pair the specification does not have, a side of 0.  Ancillary chunks are skipped unread. */
int sv_png_parse(const uint8_t *data /*host*/, size_t size, sv_png_info *info);

/* The IDAT payloads, taken as one zlib stream without copying them together (a block, a code or the header may straddle chunks), inflated into
 * filtered[0 .. info->filtered_bytes) (pipeline/run.py:250: the serial half of cv2.imread).  cap < filtered_bytes is SV_ERR_BUFFER; nothing past
 * filtered_bytes is ever written and inflation stops the moment the stream would produce more.  row_filter (height bytes, may be NULL) receives
 * each row's filter byte.  SV_ERR_BAD_ARG for every malformed stream: a bad zlib header (CM != 8, window > 32 K, FDICT, FCHECK), truncated
 * input, stored LEN != ~NLEN, block type 3, an over-subscribed code, an incomplete code (but a single code of one bit, which zlib accepts), a
 * code-length repeat without a previous length or past HLIT + HDIST, no end-of-block code, a distance before the start of the output, a wrong
 * Adler-32, fewer or more than filtered_bytes bytes, a filter byte above 4. */
int sv_png_inflate(const uint8_t *data /*host*/, size_t size, const sv_png_info *info, uint8_t *filtered /*host*/, size_t cap, uint8_t *row_filter /*host or NULL*/);
/* n files over `threads` host threads.  status[i] = per-image sv_status; returns the first failure. */
int sv_png_inflate_batch(const uint8_t *const *datas, const size_t *sizes, const sv_png_info *infos, int n, uint8_t *const *filtered, const size_t *caps,
                         uint8_t *const *row_filters /*or NULL*/, int threads, int *status /*n*/);

/* Device half (pipeline/run.py:250: the rest of cv2.imread, the frame left in HBM for K1/K2): n images of info's geometry, image i's filtered
 * bytes at filtered + i * info->filtered_bytes, -> BGR frames, row pitch `pitch` >= 3 * width, frame i at out + i * frame_stride; asynchronous on
 * `stream`, never synchronises with the host; the unfiltered samples live in the context's scratch.  row_filter: n * height filter bytes on the
 * device (what sv_png_inflate copied out); the kernels find the segments of rows from them, and a value above 4 is taken as 0 (None).  palette:
 * n * SV_PNG_PALETTE_STRIDE bytes for colour type 3, else NULL.  status (n uint32, 4-byte aligned) is zeroed on the stream, then bit 0 of
 * status[i] is set when image i held a palette index past its palette's end (that pixel is black; cv2 fails on such a file).  Only the
 * geometry fields of info are read.  SV_ERR_BAD_ARG: NULL arguments, n outside 1..65535, pitch < 3 * width, frames that overlap, an info
 * sv_png_parse would not have produced. */
int sv_png_reconstruct_bgr_u8(sv_ctx *ctx, const sv_png_info *info, const uint8_t *filtered /*dev*/, const uint8_t *row_filter /*dev*/,
                              const uint8_t *palette /*dev or NULL*/, int n, uint8_t *out /*dev*/, ptrdiff_t pitch, ptrdiff_t frame_stride,
                              uint32_t *status /*dev*/, void *stream);
/* The same under the same contract, but the frame is what cv2.imread(path, IMREAD_GRAYSCALE) returns (ml/datasets.py:81, :153, ml/evaluate.py:67):
 * one gray byte a pixel, pitch >= width.  Colour types 0 and 4: the sample (the high byte of 16 bits; 1, 2, 4 bits replicated), alpha dropped;
 * exact.  Colour types 2, 3, 6: the BGR pixel of the entry above through sv_gray_u8's arithmetic, i.e. cv2.cvtColor(cv2.imread(path),
 * COLOR_BGR2GRAY); cv2's own gray read of a colour file lets libpng convert, whose rounding is argued, not measured, here: it may differ by one
 * level on colour files. */
int sv_png_reconstruct_gray_u8(sv_ctx *ctx, const sv_png_info *info, const uint8_t *filtered /*dev*/, const uint8_t *row_filter /*dev*/,
                               const uint8_t *palette /*dev or NULL*/, int n, uint8_t *out /*dev*/, ptrdiff_t pitch, ptrdiff_t frame_stride,
                               uint32_t *status /*dev*/, void *stream);

/* ---- K24: a data set of PNG cells -> model input (ml/datasets.py:18-46 preprocess_cell, :69-92 SyntheticDataset.__getitem__, :141-164
 * RealDataset.__getitem__; ml/evaluate.py:67 for the plain gray read).  One launch takes the FILTERED bytes of n small PNG files (what
 * sv_png_inflate wrote), each with a geometry of its own, to n cells of 28 x 28: unfilter, the gray read of sv_png_reconstruct_gray_u8,
 * cv2.resize(img, (28, 28)) when the file is not 28 x 28 (sv_resize_linear_u8's arithmetic), then the mode; the cell never leaves the chip
 * in between (csrc/k24_dataset_cells.hip). */
#define SV_CELLS_GRAY 0                 /* stop after the resize: cv2.imread(path, IMREAD_GRAYSCALE) at 28 x 28 */
#define SV_CELLS_DATASET 1              /* then datasets.preprocess_cell: CLAHE(2.0, (4,4)), adaptiveThreshold(GAUSSIAN_C, BINARY, 11, 2), 255 - x */
#define SV_CELLS_MAX_SIDE 64            /* a cell's sides are 1 .. 64 */
#define SV_CELLS_MAX_ROW_BYTES 512      /* 64 pixels of RGBA at 16 bits */
#define SV_CELLS_NO_PALETTE 0xffff      /* sv_dataset_record.palette of a cell without one */
#define SV_CELLS_STATUS_PALETTE 1u      /* status bit 0, as for sv_png_reconstruct_bgr_u8: a palette index past the palette's end (that pixel is 0) */
#define SV_CELLS_STATUS_REFUSED 2u      /* status bit 1: the kernel refused the record; the cell's outputs are zeros */
typedef struct sv_dataset_record {      /* 16 bytes, 8-byte aligned */
    uint64_t offset;                    /* where the cell's filtered stream, height * (1 + row_bytes) bytes, starts inside `filtered` */
    uint16_t width, height;             /* 1 .. SV_CELLS_MAX_SIDE */
    uint8_t color_type, bit_depth;      /* a pair of the PNG specification; the stream is non-interlaced */
    uint16_t palette;                   /* which of the n_palettes palettes (colour type 3), else SV_CELLS_NO_PALETTE */
} sv_dataset_record;

/* filtered (filtered_size bytes), records (n of them) and palettes (n_palettes * SV_PNG_PALETTE_STRIDE bytes, or NULL with n_palettes 0) are on
 * the device.  out_u8 (n * 784 bytes) and out_f32 (n * 784 floats, float(u8) / 255.0f by a true division: torch.from_numpy(img).float() / 255.0
 * to the bit) are on the device; either may be NULL, not both.  status (n uint32) is written by the kernel itself for every cell, 0 or SV_CELLS_STATUS_*.
 * The kernel trusts no byte of a record: one that sv_dataset_check_records would refuse is refused there too (SV_CELLS_STATUS_REFUSED, outputs
 * zero), a filter byte above 4 is None, and nothing outside filtered[0 .. filtered_size) and the palettes is ever read.  Asynchronous on
 * `stream`; never allocates or synchronises, so it can be captured in a graph.  SV_ERR_BAD_ARG: NULL or misaligned arguments, n outside
 * 1 .. (2^31 - 1) / 784, another mode, n_palettes outside 0 .. 65534. */
int sv_dataset_cells(sv_ctx *ctx, const uint8_t *filtered /*dev*/, size_t filtered_size, const sv_dataset_record *records /*dev*/, long n,
                     const uint8_t *palettes /*dev or NULL*/, int n_palettes, int mode, uint8_t *out_u8 /*dev or NULL*/, float *out_f32 /*dev or NULL*/,
                     uint32_t *status /*dev*/, void *stream);
/* The same rules on the host, no GPU: SV_OK, or SV_ERR_BAD_ARG with the first malformed record in sv_last_error (a side outside 1 .. 64, a
 * (colour type, depth) pair the specification does not have, a stream that does not lie inside filtered_size, a palette index at or past
 * n_palettes, colour type 3 without one). */
int sv_dataset_check_records(const sv_dataset_record *records /*host*/, long n, size_t filtered_size, int n_palettes);

/* ---- quality gate: the per-pixel statistics of cv/grid_quality.py (pipeline/run_v2.py:299-311) ------------------------- */

/* The integer sums behind compute_sharpness (cv/grid_quality.py:48-62) and compute_contrast (:65-87) for n frames:
 * gray = cv2.cvtColor(BGR2GRAY) (channels 3; channels 1: the frame is the gray image), L = cv2.Laplacian(gray, CV_64F)
 * (3x3 [0 1 0; 1 -4 1; 0 1 0], BORDER_REFLECT_101; on a 1-pixel axis the neighbour is the pixel itself).
 * Per frame: lap_sum = sum(L), lap_sqsum = sum(L^2) (|L| <= 1020), hist[256] = cv2.calcHist of gray.  Any H, W >= 1, any
 * pitch >= W*channels and frame stride img_stride.  Integer accumulation only: the result does not depend on the order of
 * the partial sums.  The outputs are zeroed on `stream` first. */
int sv_frame_quality_stats_u8(sv_ctx *ctx, const uint8_t *img /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                              int channels, int64_t *lap_sum /*dev, n*/, int64_t *lap_sqsum /*dev, n*/, uint32_t *hist /*dev, n*256*/,
                              void *stream);

/* compute_completeness (cv/grid_quality.py:90-149) without the 450x450 warp: per frame and band, how many warped pixels of
 * the band are > 0.  Band 2i = warped rows, band 2i+1 = warped columns [max(0,c-2), min(450,c+3)), c = min(50i, 449),
 * i = 0..9 (the order of the reference's line_scores); every band spans all 450 pixels the other way (41,400 warped pixels
 * per frame).  Each warped pixel is cv2.warpPerspective's (INTER_LINEAR, 1/32-px coordinates, 15-bit weights, constant-0
 * border), minv = sv_corners_to_minv_batch(corners, 450, 0) (the same getPerspectiveTransform as compute_completeness).
 * binary: n 8-bit images (pitch, img_stride). */
int sv_grid_line_coverage_u8(sv_ctx *ctx, const uint8_t *binary /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                             const double *minv /*dev, n*9*/, uint32_t *counts /*dev, n*20*/, void *stream);

/* The same on bit images (sv_preprocess_bits_u8's layout: 1 bit per pixel, LSB = leftmost, W/32 words per row, rows and
 * frames dense; a set bit is 255).  W % 32 == 0. */
int sv_grid_line_coverage_bits(sv_ctx *ctx, const uint32_t *bits /*dev, n*H*W/32*/, int n, int H, int W,
                               const double *minv /*dev, n*9*/, uint32_t *counts /*dev, n*20*/, void *stream);

/* ---- K7: run_v2's preprocessing, cv/preprocess_v2.py (pipeline/run_v2.py:278-280) -------------------------------------
 * Every entry takes n gray frames of H x W (any `pitch` >= W, `img_stride` bytes between frames, any alignment) and writes
 * dense [n][H][W] outputs that must not overlap the inputs.  cv2 is not available to pin these against: the arithmetic
 * stated here is the contract (tests/preprocess_v2_ref.py restates it in numpy), parity with OpenCV is unpinned as for K1/K2.
 * Stages with intermediates keep them in the context's grow-on-demand scratch. */

/* cv2.dilate / cv2.erode / cv2.morphologyEx(MORPH_CLOSE | MORPH_OPEN) with cv2.getStructuringElement(shape, (k, k)),
 * cv/preprocess_v2.py:52-53, 108-109, 190-200.  ELLIPSE: r = c = k/2, row i (dy = i - r) covers columns
 * [max(c-dx,0), min(c+dx+1,k)), dx = round_half_even(c * sqrt((r*r - dy*dy) * (1/(r*r)))) in double; RECT: all ones.  Anchor
 * (k/2, k/2).  dst = max | min of src over the element's ones placed unreflected on the pixel; pixels outside the image do
 * not take part.  CLOSE = dilate then erode, OPEN = erode then dilate.  1 <= ksize <= 4095 (larger than the image included). */
#define SV_MORPH_DILATE 0
#define SV_MORPH_ERODE 1
#define SV_MORPH_CLOSE 2
#define SV_MORPH_OPEN 3
#define SV_SHAPE_RECT 0
#define SV_SHAPE_ELLIPSE 1
int sv_morphology_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int op, int shape,
                     int ksize, uint8_t *dst /*dev, n*H*W*/, void *stream);

/* cv2.blur(gray, (k, k)) on u8, cv/preprocess_v2.py:93: S = the integer sum over the k x k window (BORDER_REFLECT_101,
 * reflected repeatedly when the window is larger than the image), dst = (2*S + k*k) / (2*k*k): the mean rounded to nearest
 * (k*k is odd: no ties).  ksize odd, <= 1023. */
int sv_box_mean_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int ksize,
                   uint8_t *dst /*dev, n*H*W*/, void *stream);

/* cv2.GaussianBlur(img, (21, 21), 0) on u8, cv/preprocess_v2.py:112 (sv_blur_u8 stops at 7): sigma 3.5, taps in 8 fractional
 * bits 0 2 2 4 6 11 15 20 25 28 30 28 25 20 15 11 6 4 2 2 0 (sum 256), horizontal pass exact, vertical pass (sum + 2^15) >> 16,
 * BORDER_REFLECT_101. */
int sv_gaussian_blur21_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                          uint8_t *dst /*dev, n*H*W*/, void *stream);

/* (gray.astype(float32) / maximum(background, 1).astype(float32) * 255).clip(0, 255).astype(uint8), cv/preprocess_v2.py:56-60
 * and :115-119: one IEEE float32 division, one float32 multiplication, truncation. */
int sv_divide_normalize_u8(sv_ctx *ctx, const uint8_t *gray /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                           const uint8_t *background /*dev, n*H*W dense*/, uint8_t *dst /*dev, n*H*W*/, void *stream);

/* cv2.createCLAHE(clip_limit, (tiles_x, tiles_y)).apply(gray), cv/preprocess_v2.py:128-129 and :325-326, any size: when H or W
 * does not divide by the grid the image is extended at the bottom / right by tiles - size % tiles pixels (BORDER_REFLECT_101) and
 * tile size, histograms, LUTs and blend weights come from the extended size.  Per tile: histogram, clip at
 * max(1, int(clip * area / 256)), clipped mass spread evenly (+1 every max(256 / residual, 1) bins for the residual),
 * LUT[i] = round_half_even(cumsum[i] * (255.f / area)); per pixel the float32 bilinear blend of the four nearest tiles' LUTs,
 * one rounding per operation, round_half_even.  sv_preprocess_cells_u8 remains the fused 28x28 special case. */
int sv_clahe_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, double clip_limit,
                int tiles_x, int tiles_y, uint8_t *dst /*dev, n*H*W*/, void *stream);

/* threshold_sauvola(gray, window, k), cv/preprocess_v2.py:152-175: S1, S2 = the window sums of g and g*g as integers
 * (BORDER_REFLECT_101); mean = float32(double(S1) * (1.0 / w^2)), sq likewise from S2; then float32, one rounding each:
 * var = max(sq - mean*mean, 0), sd = sqrt(var), t = mean * (1 + float32(k) * (sd / 128 - 1)); dst = float32(g) < t ? 255 : 0.
 * window odd, <= 1023. */
int sv_threshold_sauvola_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int window,
                            double k, uint8_t *dst /*dev, n*H*W*/, void *stream);

/* A fixed threshold and the count of the pixels it sets: dst = g > thresh ? 255 : 0 (type_inv 0: detect_glare's mask,
 * cv/preprocess_v2.py:73) or g > thresh ? 0 : 255 (type_inv 1: THRESH_BINARY_INV at the Otsu threshold, :148, which the caller
 * computes from sv_frame_quality_stats_u8's histogram); counts[f] = pixels of frame f set to 255. */
int sv_threshold_count_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, int thresh,
                          int type_inv, uint8_t *dst /*dev, n*H*W*/, uint32_t *counts /*dev, n*/, void *stream);

/* detect_shadow's mask, cv/preprocess_v2.py:96: mask = int(gray) - int(local_mean) < delta ? 255 : 0 (delta = -30), and its count. */
int sv_shadow_mask_u8(sv_ctx *ctx, const uint8_t *gray /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                      const uint8_t *local_mean /*dev, n*H*W dense*/, int delta, uint8_t *mask /*dev, n*H*W*/, uint32_t *counts /*dev, n*/,
                      void *stream);

/* counts[f] = pixels != 0 of frame f: what score_binary's np.mean(b) / 255 needs of a {0,255} image, cv/preprocess_v2.py:285-290. */
int sv_count_nonzero_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                        uint32_t *counts /*dev, n*/, void *stream);

/* ---- K13: run_v2's grid detection fallbacks, cv/grid_v2.py (pipeline/run_v2.py:287) ------------------------------------
 * n gray frames of H x W (any `pitch` >= W, `img_stride` bytes between frames).  cv2 is not available to pin these against:
 * the arithmetic stated here is the contract (tests/grid_v2_ref.py restates it in numpy); parity with OpenCV is unpinned. */

/* detect_corners_harris, cv/grid_v2.py:272-290 = cv2.goodFeaturesToTrack(gray, max_corners, quality_level, min_distance,
 * blockSize=3, useHarrisDetector=True, k).  All borders BORDER_REFLECT_101; IEEE float32 operations in this order, none fused:
 *   ks = [f32(s), f32(2s), f32(s)], s = 1/(4*3*255) in double
 *   Dx: rows p[x+1] - p[x-1], then columns ks[1]*S[y] + ks[0]*(S[y-1] + S[y+1])
 *   Dy: rows ks[1]*p[x] + ks[0]*(p[x-1] + p[x+1]), then columns S[y+1] - S[y-1]
 *   a, b, c = the 3x3 sums of Dx*Dx, Dx*Dy, Dy*Dy (float32 products; summed in double, each row left to right, then the
 *   rows top to bottom; rounded to float32 once; the product images are reflected at the border)
 *   response = a*c - b*b - (k*(a+c))*(a+c), the subtractions left to right
 * Selection per frame: max = the largest response; nothing if max <= 0; a response below quality_level*max (product in
 * double) counts as 0; candidates are the non-zero pixels equal to the maximum of their 3x3 neighbourhood, the outermost
 * one-pixel frame excluded; ordered by response descending, ties in raster order; a candidate is kept unless a kept corner
 * lies at squared distance < min_distance^2 (integers); at most max_corners (1..SV_HARRIS_MAX_CORNERS) are kept.
 * corners[f][i] = (x, y) as float, counts[f] = corners of frame f.  cand_capacity: room for candidates per frame in the
 * context's scratch; a frame with more fails the call with SV_ERR_BUFFER (the message names the count) -- never a shorter
 * list.  response: NULL, or where to leave the response images (else they live in the context's scratch).
 * 3 <= H, W <= 65535, SV_ERR_BAD_ARG otherwise: the selection keeps a corner as two 16-bit coordinates and a candidate's
 * raster index y*W + x in 32 bits, and H*W < 2^32 follows from the two limits (nothing else bounds the product).
 * The call waits for `stream` (the status depends on the candidate counts). */
#define SV_HARRIS_MAX_CORNERS 4096
int sv_harris_corners_u8(sv_ctx *ctx, const uint8_t *gray /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                         int max_corners, double quality_level, int min_distance, double k, int cand_capacity,
                         float *corners /*dev, n*max_corners*2*/, int *counts /*dev, n*/, float *response /*dev n*H*W or NULL*/,
                         void *stream);

/* rotate_image's warp, cv/grid_v2.py:371-394 = cv2.warpAffine(src, M, (dst_w, dst_h), INTER_LINEAR, BORDER_CONSTANT,
 * border_value) on single-channel u8.  M: per frame the FORWARD 2x3 matrix, inverted in double as cv2 does:
 * D = M0*M4 - M1*M3; D = D ? 1/D : 0; A11 = M4*D; A22 = M0*D; M1 *= -D; M3 *= -D; b1 = -A11*M2 - M1*M5;
 * b2 = -M3*M2 - A22*M5.  Destination (x, y) reads the source at X = (sat((M1*y + b1)*1024) + 16 + sat(A11*x*1024)) >> 5,
 * Y likewise from M3, A22, b2 (sat: round half to even, saturated to int32); cell (X >> 5, Y >> 5) saturated to int16,
 * fractions (X & 31, Y & 31) / 32; bilinear with cv2's 15-bit weight table (weights sum to 32768), (sum + 16384) >> 15, a tap
 * outside the source is border_value.  H, W < 32768. */
int sv_warp_affine_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                      const double *M /*dev, n*6*/, int dst_h, int dst_w, int border_value, uint8_t *dst /*dev, n*dst_h*dst_w*/,
                      void *stream);

/* ---- K15: the motion gate of a camera feed, cv/stabilizer.py (MotionDetector) ----------------------------------------- */

/* MotionDetector.update, cv/stabilizer.py:264-291, called for n consecutive frames of one feed, in one launch:
 *   small[i]  = cv2.resize(gray(frames[i]), (dw, dh)) (:273-277; the detector's size is dw, dh = 160, 120); gray = cv2.cvtColor(BGR2GRAY)
 *               for channels 3, the frame itself for channels 1
 *   counts[i] = the pixels with |small[i] - small[i-1]| > threshold (:284-285), small[-1] = prev_small; counts[0] = 0 when
 *               prev_small is NULL (the detector's first frame, :279-281)
 * The caller compares counts[i] / (dh*dw) with min_area_ratio (:287-291) and keeps small[n-1] as the next call's prev_small.
 * The comparison is the reference's float comparison, exact: a difference d is an integer, so d > threshold <=> d > floor(threshold);
 * a NaN threshold counts nothing.
 * Resize: cv2's 8-bit INTER_LINEAR as sv_resize_linear_u8 states it (11-bit coefficients from the float32 source coordinate, edge taps
 * clamped with weights 2048 / 0, (((b0*(t0>>4))>>16) + ((b1*(t1>>4))>>16) + 2) >> 2), upscaling included; a frame that already is
 * dh x dw is copied; and a frame of exactly 2*dh x 2*dw takes the 2x2 mean (s00 + s01 + s10 + s11 + 2) >> 2, because cv2.resize
 * replaces INTER_LINEAR by INTER_AREA at an exact factor of two on both axes (OpenCV's resize.cpp; cv2 is not available to pin it
 * against).  sv_resize_linear_u8 does not have that last case.  Only the taps are read and converted to gray: no full-size gray
 * image exists.
 * Any H, W, dh, dw >= 1 (dh*dw < 2^31 - 256), any pitch >= W*channels, frame_stride bytes between frames, any alignment.  prev_small
 * must not overlap small.  No allocation, no host synchronisation: a memset of counts and one kernel launch on `stream`. */
int sv_motion_update_u8(sv_ctx *ctx, const uint8_t *frames /*dev*/, int n, int H, int W, int channels /*1 or 3 (BGR)*/,
                        ptrdiff_t pitch, ptrdiff_t frame_stride, const uint8_t *prev_small /*dev, dh*dw, or NULL*/, float threshold,
                        uint8_t *small /*dev, n*dh*dw*/, int32_t *counts /*dev, n*/, int dh, int dw, void *stream);

/* ---- K16: the solution drawn into the camera frame ------------------------------------------------------------------------ */

#define SV_OVERLAY_GRID 450    /* the solution layer: 9 x 9 cells of SV_OVERLAY_CELL texels (pipeline/overlay.py:27) */
#define SV_OVERLAY_CELL 50
#define SV_OVERLAY_MARGIN 3    /* rows and columns 0..2 and 47..49 of every glyph are zero */

/* The 8-bit coverage atlas of the digits 1..9, [9][50][50] (glyph d-1 draws digit d, one texel per pixel of the 450 x 450 layer),
 * copied into the context together with the default palette.  Rows and columns 0..2 and 47..49 of every glyph must be zero:
 * SV_ERR_BAD_ARG otherwise, checked before anything is uploaded.  Synchronous, like the weight loaders. */
int sv_set_overlay_glyphs(sv_ctx *ctx, const uint8_t *atlas /*host, 9*50*50*/);

/* The forward homography of sv_corners_to_minv_batch: M = cv2.getPerspectiveTransform(ordered, inset corners -> (0,0)..(S-1,S-1)),
 * frame -> grid, the matrix that function inverts.  Same arguments and the same ok rule (ok[f] = 0 exactly where it is 0 there);
 * a degenerate quad gives ok[f] = 0 and m[f] = identity. */
int sv_corners_to_m_batch(const float *corners /*host*/, int n, int out_size, float inset_ratio,
                          double *m /*host*/, uint8_t *ok /*host, n*/);

/* Draws 81 digits per frame into n BGR frames, in one launch.  The result is defined by three steps.
 *   Layers (450 x 450, never materialised): A[i][j] = atlas[d-1][i%50][j%50] with d = digits[f][(i/50)*9 + j/50], 0 where d == 0,
 *     d > 9 or the cell's class >= k; B[i][j] = A[i-2][j-2] >> 1 for i, j >= 2, else 0 (the drop shadow); both 0 outside [0,450).
 *   Warp: a = cv2.warpPerspective(A, M, (W,H), INTER_LINEAR | WARP_INVERSE_MAP, BORDER_CONSTANT 0) and s likewise from B, in the
 *     arithmetic of sv_warp_perspective_u8 with the W x H frame as the destination: blocks of bh = min(16,H) rows by
 *     bw = min(1024/bh, W) columns counted from the frame's origin, the homography m[f] (frame -> grid, sv_corners_to_m_batch)
 *     evaluated in double at the block origin and stepped by M0*x1, W = 32/W (0 where W is 0), clamped to int32, rounded half to
 *     even, >> 5 saturated to int16, five fraction bits, four taps with 15-bit weights, (sum + 2^14) >> 15.
 *   Blend, per channel c, in integers: t = shadow ? (f*(255-s) + 127)/255 : f;  out = (t*(255-a) + palette[cls][c]*a + 127)/255,
 *     cls = the class of the cell that holds the top-left tap, (clamp(Y>>5,0,449)/50, clamp(X>>5,0,449)/50).
 * classes NULL: class 0 everywhere.  palette NULL: the default, k = 3: BGR (255,100,0) solved, (0,0,0) original, (0,0,255) low
 * confidence (pipeline/overlay.py:63-71).  active NULL: every frame; a frame with active[f] == 0 is copied unchanged.
 * dst == frames (then dst_pitch, dst_stride must equal pitch, img_stride) draws in place and touches only the 64 x 16 blocks that
 * the grid's square can reach; otherwise dst must not overlap frames: it receives a device copy of the frames and is then drawn
 * into.  Any H, W >= 1 (H <= 16*65535), pitch >= 3*W, any alignment; n < 65536, 1 <= k <= 256: SV_ERR_BAD_ARG otherwise;
 * SV_ERR_NO_WEIGHTS before sv_set_overlay_glyphs.  No allocation, no host synchronisation. */
int sv_render_overlay_u8(sv_ctx *ctx, const uint8_t *frames /*dev*/, int n, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                         const double *m /*dev, n*9*/, const uint8_t *digits /*dev, n*81*/, const uint8_t *classes /*dev, n*81, or NULL*/,
                         const uint8_t *palette /*dev, k*3 BGR, or NULL*/, int k, const uint8_t *active /*dev, n, or NULL*/,
                         int shadow, uint8_t *dst /*dev; may equal frames*/, ptrdiff_t dst_pitch, ptrdiff_t dst_stride, void *stream);

/* ---- K22: batched data augmentation, tools/augment_data.py ------------------------------------------------------------------ */

/* One launch turns n_src gray images into n_out augmented copies: output i loads src[clamp(src_index[i], 0, n_src-1)], runs
 * steps[i][0 .. clamp(n_steps[i], 0, SV_AUG_MAX_STEPS)) on chip and is stored once.  Between two steps the image is u8, as each of
 * the reference's functions returns u8.  cv2 is not available, so the arithmetic stated here is the contract; parity with OpenCV
 * itself is unpinned (as for K13).
 *
 * A step record is 96 bytes, 8-byte aligned: int32 op; int32 i[5]; then 72 bytes read as double d[9] or as float f[18].
 *   SV_AUG_NONE, or any op the kernel does not know: the identity.
 *   SV_AUG_AFFINE (rotate, translate): d[0..5] the FORWARD 2x3 matrix.  cv2.warpAffine(INTER_LINEAR, BORDER_REPLICATE) in the
 *     arithmetic of sv_warp_affine_u8 above (the inversion, 1/1024 fixed point, + 16, >> 5, int16 cells, 15-bit weights
 *     (32-a)(32-b)*32 .. ab*32, (sum + 16384) >> 15), but a tap outside the image reads the nearest pixel (both tap
 *     coordinates clamped into the image), not a constant.
 *   SV_AUG_PERSPECTIVE (perspective_warp): d[0..8] the FORWARD 3x3 matrix.  Inverted in double by cofactors times 1/det, every
 *     product and difference rounded separately (a zero determinant gives the zero matrix, as cv::invert leaves it); then
 *     sv_warp_perspective_u8's coordinates with the image as one block (width <= 64): X0 = (0 + M1*y) + M2, W = W0 + M6*x,
 *     W = W ? 32/W : 0, saturated, rounded half to even, >> 5 saturated to int16, five fraction bits; same weights, taps clamped.
 *   SV_AUG_BRIGHTNESS (adjust_brightness): d[0] = delta.  float32(p) + float32(delta), clipped to [0, 255], truncated.
 *   SV_AUG_CONTRAST (adjust_contrast): d[0] = factor.  mean = (double)(integer sum of the pixels) / (double)(H*W); then
 *     ((double)p - mean) * factor + mean in double, each operation rounded, clipped to [0, 255], truncated.  This is what the
 *     reference computes under NumPy >= 2, where np.mean's float64 scalar promotes the float32 image to float64 (under NumPy 1 the
 *     same line stayed in float32).
 *   SV_AUG_BLUR (gaussian_blur): i[0] = k in {1, 3, 5}.  Integer taps [1,2,1] / [1,4,6,4,1] on rows and columns, BORDER_REFLECT_101,
 *     (S + 8) >> 4 resp. (S + 128) >> 8 of the exact 2-D sum S: sv_blur_u8's rounding.  k = 1 is the identity.
 *   SV_AUG_SCALE (scale): i[0] = new_w, i[1] = new_h, i[2] = 1 to crop (factor > 1), 0 to pad.  cv2.resize to (new_w, new_h) in
 *     sv_resize_linear_u8's arithmetic (the same device function, csrc/sv_device.h's sv_resize_px); crop: the H x W window at ((new_h-H)/2, (new_w-W)/2); pad: the scaled image at
 *     ((H-new_h)/2, (W-new_w)/2) of a plane of 128 (floor divisions).  The scaled image is never materialised.
 *   SV_AUG_FILL_RECT (random_erasing): columns i[0] .. i[0]+i[2]-1 of rows i[1] .. i[1]+i[3]-1 become i[4].
 *   SV_AUG_ELASTIC (elastic_transform): i[0] = radius r <= SV_AUG_MAX_RADIUS, i[4] = salt, f[0] = float32(alpha), f[1 + j] = the
 *     Gaussian tap at distance j = 0..r (sv_augment_elastic_taps).  Per pixel the fields ux, uy = (word >> 8) * 2^-23 - 1 in float32
 *     (exact) from words 0 and 1 of the pixel's random block; each field is filtered along rows, then along columns, with
 *     BORDER_REFLECT_101: acc = t[-r]*v[-r]; acc = acc + t[j]*v[j] for j = -r+1 .. r, every product and sum a float32 rounding.
 *     Then dx = ux' * f[0], map_x = float32(x) + dx (likewise y); cv2.remap(INTER_LINEAR, BORDER_REPLICATE): X = sat(rint(map_x*32)),
 *     cell X >> 5 saturated to int16, fraction X & 31, the weights above, taps clamped.
 *   SV_AUG_NOISE_GAUSS (add_noise "gaussian"): d[0] = sigma = intensity*255, i[4] = salt.  From words w0, w1 of the pixel's block, in
 *     double: u1 = (w0 + 1) * 2^-32, u2 = w1 * 2^-32, z = sqrt(-2 * ln(u1)) * cos(6.283185307179586 * u2); (double)p + sigma*z,
 *     clipped to [0, 255], truncated.  ln and cos are the platform's double functions (a few ulp apart between libraries).
 *   SV_AUG_NOISE_SP (add_noise "salt_pepper"): d[0] = intensity/2, i[4] = salt.  255 where w0 * 2^-32 < d[0]; then 0 where
 *     w1 * 2^-32 < d[0] (pepper over salt, the reference's order).
 * The random block of a pixel is Philox4x32-10 (csrc/sv_philox.h) with key (seed low, seed high) and counter
 *   (y*W + x,  g low 32 bits,  (g >> 32) << 8 | step slot,  salt),  g = index_base + i, the output's global index:
 * a pure function of (seed, g, slot, salt, pixel), never of n_out, the launch shape or how a job is split into calls.  The bits are
 * not NumPy's: the reference's np.random fields are not reproduced, only their distributions.
 * 4 <= H, W <= SV_AUG_MAX_SIDE, pitch >= W, n_src, n_out >= 1, 0 <= index_base, index_base + n_out < 2^56: SV_ERR_BAD_ARG otherwise.
 * Nothing a caller uploads can make the kernel read or write outside its buffers; sv_augment_check_program is what tells a caller
 * that a program is malformed.  Asynchronous on `stream`, graph-capturable; no allocation, no host synchronisation. */
#define SV_AUG_MAX_STEPS 10
#define SV_AUG_MAX_SIDE 64
#define SV_AUG_MAX_RADIUS 16
typedef enum sv_aug_op {
    SV_AUG_NONE = 0, SV_AUG_AFFINE = 1, SV_AUG_PERSPECTIVE = 2, SV_AUG_BRIGHTNESS = 3, SV_AUG_CONTRAST = 4, SV_AUG_BLUR = 5,
    SV_AUG_SCALE = 6, SV_AUG_FILL_RECT = 7, SV_AUG_ELASTIC = 8, SV_AUG_NOISE_GAUSS = 9, SV_AUG_NOISE_SP = 10
} sv_aug_op;
typedef struct sv_aug_step {
    int32_t op;
    int32_t i[5];
    union { double d[9]; float f[18]; };
} sv_aug_step;
int sv_augment_u8(sv_ctx *ctx, const uint8_t *src /*dev*/, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                  const sv_aug_step *steps /*dev, n_out*SV_AUG_MAX_STEPS*/, const int32_t *n_steps /*dev, n_out*/,
                  const int32_t *src_index /*dev, n_out*/, long n_out, uint64_t seed, long index_base,
                  uint8_t *dst /*dev, n_out*H*W*/, void *stream);

/* What the kernel cannot check, on the host copies of a program: a known op in every used slot, 0 <= n_steps <= SV_AUG_MAX_STEPS,
 * 0 <= src_index < n_src, finite matrices and scalars, k in {1,3,5}, a scale size of 1 .. 2*side that agrees with its crop / pad flag,
 * a rectangle inside the image with a value 0..255, an elastic radius <= SV_AUG_MAX_RADIUS and < min(H, W) (REFLECT_101 reflects
 * once) with finite taps.  SV_ERR_BAD_ARG with a message that names the output and the step.  Needs no context and no GPU. */
int sv_augment_check_program(const sv_aug_step *steps /*host*/, const int32_t *n_steps /*host*/, const int32_t *src_index /*host*/,
                             long n_out, int n_src, int H, int W);

/* Host helpers of the program builder, in the library's double arithmetic.
 * cv2.getRotationMatrix2D((cx, cy), angle_deg, scale): a = angle * (pi/180), alpha = cos(a)*scale, beta = sin(a)*scale,
 * m = [alpha, beta, (1-alpha)*cx - beta*cy; -beta, alpha, beta*cx + (1-alpha)*cy]. */
int sv_augment_rotation_matrix(double cx, double cy, double angle_deg, double scale, double *m /*host, 6*/);
/* cv2.getPerspectiveTransform(src, dst) on four float32 point pairs: the 8x8 elimination of sv_corners_to_m_batch.
 * SV_ERR_DEGENERATE when the points define no homography. */
int sv_augment_perspective_matrix(const float *src /*host, 8*/, const float *dst /*host, 8*/, double *m /*host, 9*/);
/* The float32 taps of cv2.GaussianBlur((0,0), sigma) on a float32 image: radius r = (round(8*sigma + 1) | 1) / 2; in double
 * v[j] = exp((2j)^2 * (-0.125 / sigma^2)), sum = 2*(v[r] + .. + v[1]) + 1 (added in that order), taps[j] = float(v[j] * (1/sum)),
 * taps[0] = float(1/sum).  cap < r + 1: SV_ERR_BUFFER with *radius set; sigma not positive and finite: SV_ERR_BAD_ARG. */
int sv_augment_elastic_taps(double sigma, float *taps /*host, cap*/, int cap, int *radius);
/* The random words of one output's step slot on the host, the kernel's own generator: words[(y*W + x)*4 + k], k = 0..3. */
int sv_augment_field_host(uint64_t seed, long index, int slot, uint32_t salt, int H, int W, uint32_t *words /*host, H*W*4*/);

/* ---- K23: synthetic digit cells, ml/generate_synthetic_v2.py --------------------------------------------------------------- */

/* One launch draws n_out square gray cells of `size` x `size`: output i builds its base image from cells[i] (phase A), runs
 * steps[i][0 .. clamp(n_steps[i], 0, SV_AUG_MAX_STEPS)) on it on chip (phase B) and is stored once.  cv2 is not available, so for the
 * cv2 calls the arithmetic stated here is the contract and parity with OpenCV itself is unpinned (as for K13 and K22); the numpy and
 * Pillow arithmetic of the reference is reproduced bit for bit.
 *
 * A cell record (sv_syn_cell) is 96 bytes, 8-byte aligned: 18 int32, then double bg_d[3].
 * Phase A, per pixel (x, y), in this order:
 *   background (generate_paper_background, ml/generate_synthetic_v2.py:128-174), bg_kind:
 *     SV_SYN_BG_PLAIN (:132-135)     p = bg_value.
 *     SV_SYN_BG_TEXTURED (:137-146)  p = trunc(clip((double)bg_value + bg_d[0] * z, 0, 255)), z the pixel's normal (below).  Then, when
 *                                    grain_stride is 2..4, every row y = k * grain_stride gets max(p - d_k, 0), d_k = bits 2k, 2k+1 of
 *                                    the 64 bits grain_d[0] | grain_d[1] << 32 (k < 32: a side of 64 at stride 2 has 32 such rows).
 *     SV_SYN_BG_GRADIENT (:148-167)  grad_dir 0 (horizontal, i = x) or 1 (vertical, i = y): t = i * bg_d[1] + bg_d[0], two double roundings,
 *                                    but t = bg_d[2] at i = size - 1: np.linspace's own terms (start, step, stop);
 *                                    p = trunc(clip((double)bg_value + t, 0, 255)).  grad_dir 2 (radial): c = size / 2 (integer),
 *                                    t = (sqrt((double)((x-c)^2 + (y-c)^2)) / ((double)size / 2)) * bg_d[0], IEEE sqrt and division;
 *                                    p = trunc(clip((double)bg_value - t, 0, 255)).
 *     SV_SYN_BG_NOISY (:169-172)     as textured, without grain.
 *     SV_SYN_BG_KEEP                 p = what dst[i] holds at (x, y) when the kernel starts: the way an existing image enters (the
 *                                    single-image add_grid_artifacts and apply_augmentation).  A workgroup reads its own output alone.
 *   grid-line artefacts (add_grid_artifacts, :177-206): art_edges bit 0 top, 1 bottom, 2 left, 3 right; on the band of art_width
 *     (1..2) rows or columns at that edge p = min(p, art_dark).
 *   smudge (generate_empty_cell, :261-270): smudge = (x, y, side, darkness); side 0 is none, else p = min(p, darkness) on the square.
 *   glyph (generate_digit, :223-247): glyph_slot -1 is none.  m = atlas[slot][y - glyph_y][x - glyph_x] inside the slot's (w, h) mask,
 *     0 outside it; (glyph_x, glyph_y) is the signed top-left corner of Pillow's coverage mask (font.getmask2(text, "L")) in cell
 *     coordinates, so a mask partly or wholly outside the cell is clipped -- what the reference's padded canvas and crop do.
 *     t = ink * m + 255 * (255 - m) + 128;  digit = (t + (t >> 8)) >> 8      (Pillow's blend of ink over white, ImageDraw.text)
 *     p = trunc(float32(p) * float32(digit) / 255), two float32 roundings    (the multiply blend, :247)
 * The normal of a pixel: words w0, w1 of the Philox block (K22's layout above) of (seed, g = index_base + i, slot SV_SYN_BG_SLOT, salt
 * bg_salt, pixel y*size + x), through K22's Box-Muller.  No step has slot SV_SYN_BG_SLOT.  sv_augment_field_host gives the words.
 *
 * Phase B runs sv_aug_step records: every K22 op above with K22's arithmetic (the random block of step `slot` as above), and
 *   SV_SYN_AFFINE_CONST (apply_augmentation :284-288): SV_AUG_AFFINE, but a tap outside the image reads i[0] (BORDER_CONSTANT,
 *     borderValue; the reference passes 255).  d[0..5] the forward matrix.
 *   SV_SYN_PERSPECTIVE_CONST (:331-341): SV_AUG_PERSPECTIVE with the same border rule, border i[0].  d[0..8] the forward matrix.
 *   SV_SYN_SCALE_PAD (:291-305): SV_AUG_SCALE with the pad value in i[3] (the reference pads with 255): i[0] = new_w, i[1] = new_h
 *     (down to 1), i[2] = 1 to crop, 0 to pad; the same floor-division offsets and sv_resize_linear_u8 arithmetic.
 *   SV_SYN_GAUSS_BLUR (:308-311, cv2.GaussianBlur(img, (k, k), sigma)): i[0] = k in {3, 5}; i[1], i[2], i[3] the taps at distance 0, 1, 2
 *     as integers in Q8.8 with i[1] + 2*i[2] + 2*i[3] = 256 (i[3] = 0 at k = 3): sv_synth_gaussian_taps_q8.  Rows are accumulated
 *     unrounded, R(x, y) = sum_i t|i| * p(x+i, y); columns then give (sum_j t|j| * R(x, y+j) + 2^15) >> 16.  BORDER_REFLECT_101.
 *   SV_SYN_ERODE, SV_SYN_DILATE (:344-349, a 2 x 2 kernel of ones, anchor (1, 1)): the minimum resp. maximum over (x-1..x, y-1..y), taps
 *     outside the image ignored.
 * An op that is neither is the identity.  These ops are valid only here: sv_augment_u8 and sv_augment_check_program keep their set.
 *
 * The atlas is u8 [n_slots][SV_SYN_GLYPH_SIDE][SV_SYN_GLYPH_SIDE], a slot's mask in its top-left corner, row pitch SV_SYN_GLYPH_SIDE;
 * atlas_dims is int32 [n_slots][2] = (w, h).  Glyph rasterisation is the host's (Pillow / FreeType, once per font, size and digit).
 * Nothing a caller uploads can make the kernel touch memory outside its buffers: a slot outside 0 .. n_slots-1 draws nothing, (w, h)
 * are clamped to the slot, offsets, rectangles, widths, strides, taps and counts are clamped or clipped, values are clamped to 0..255.
 * 4 <= size <= SV_AUG_MAX_SIDE, n_out >= 1, n_slots >= 0 (atlas and atlas_dims may be NULL at 0), 0 <= index_base,
 * index_base + n_out < 2^56: SV_ERR_BAD_ARG otherwise.  Asynchronous on `stream`, graph-capturable; no allocation, no host sync. */
#define SV_SYN_GLYPH_SIDE 32
#define SV_SYN_BG_SLOT 255
typedef enum sv_syn_bg { SV_SYN_BG_PLAIN = 0, SV_SYN_BG_TEXTURED = 1, SV_SYN_BG_GRADIENT = 2, SV_SYN_BG_NOISY = 3, SV_SYN_BG_KEEP = 4 } sv_syn_bg;
typedef enum sv_syn_op {
    SV_SYN_AFFINE_CONST = 32, SV_SYN_PERSPECTIVE_CONST = 33, SV_SYN_SCALE_PAD = 34, SV_SYN_GAUSS_BLUR = 35, SV_SYN_ERODE = 36, SV_SYN_DILATE = 37
} sv_syn_op;
typedef struct sv_syn_cell {
    int32_t bg_kind;       /* sv_syn_bg */
    int32_t bg_value;      /* the plain value, or the base */
    int32_t bg_salt;       /* the 32 bits of the field's salt */
    int32_t grad_dir;      /* 0 horizontal, 1 vertical, 2 radial */
    int32_t grain_stride;  /* 0: no grain; else 2..4 */
    uint32_t grain_d[2];   /* 2 bits per grain row */
    int32_t art_edges, art_width, art_dark;
    int32_t smudge[4];     /* x, y, side (0: none), darkness */
    int32_t glyph_slot;    /* -1: none */
    int32_t glyph_x, glyph_y, glyph_ink;
    double bg_d[3];        /* textured, noisy: sigma;  gradient h / v: start, step, stop;  radial: strength */
} sv_syn_cell;
int sv_synth_cells_u8(sv_ctx *ctx, const sv_syn_cell *cells /*dev, n_out*/, const sv_aug_step *steps /*dev, n_out*SV_AUG_MAX_STEPS*/,
                      const int32_t *n_steps /*dev, n_out*/, long n_out, int size, const uint8_t *atlas /*dev*/,
                      const int32_t *atlas_dims /*dev, n_slots*2*/, int n_slots, uint64_t seed, long index_base,
                      uint8_t *dst /*dev, n_out*size*size*/, void *stream);

/* What the kernel cannot report, on host copies: a known background kind and gradient direction, base, value, darkness and ink in
 * 0..255, a finite sigma, strength and linspace terms, a grain stride of 0 or 2..4 with every used d in 1..3, artefact edges in 0..15
 * with a width of 1..2, a smudge inside the cell, a glyph slot of -1 .. n_slots-1 whose mask is 1..SV_SYN_GLYPH_SIDE on both sides;
 * 0 <= n_steps <= SV_AUG_MAX_STEPS; a K22 op that sv_augment_check_program accepts or a K23 op with a border / pad value in 0..255, finite
 * matrices, a scale size of 1 .. 2*size that agrees with its flag, k in {3, 5} with taps >= 0 summing to 256.  SV_ERR_BAD_ARG with
 * a message that names the output and the field or step.  Needs no context and no GPU. */
int sv_synth_check_program(const sv_syn_cell *cells /*host*/, const sv_aug_step *steps /*host*/, const int32_t *n_steps /*host*/, long n_out,
                           int size, const int32_t *atlas_dims /*host, may be NULL at n_slots 0*/, int n_slots);
/* The Q8.8 taps of SV_SYN_GAUSS_BLUR at distance 0, 1, 2: in double v[j] = exp(-(j*j) / (2*sigma*sigma)), j = 0 .. k/2,
 * sum = v[0] + 2*v[1] (+ 2*v[2]); taps[j] = rint(v[j] / sum * 256) for j >= 1 and taps[0] = 256 - 2*taps[1] - 2*taps[2], so that they sum to
 * 256 exactly; taps[2] = 0 at k = 3.  k not 3 or 5, or a sigma that is not positive and finite: SV_ERR_BAD_ARG. */
int sv_synth_gaussian_taps_q8(int k, double sigma, int32_t *taps /*host, 3*/);

/* ---- the whole device-resident path ----------------------------------------------------------- */

/* frames + homographies -> 81 digits per frame: K2 then K3 on `stream`, no host sync.
 * cells may be NULL (then context scratch is used). */
int sv_frames_to_digits(sv_ctx *ctx, const uint8_t *frames /*dev*/, int n, int H, int W,
                        ptrdiff_t pitch, ptrdiff_t frame_stride, const double *minv /*dev, n*9*/, int glue,
                        uint8_t *cells /*dev n*81*784 or NULL*/, float *logits /*dev, n*81*10*/,
                        uint8_t *digits /*dev, n*81*/, float *conf /*dev n*81 or NULL*/, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SUDOKU_VISION_HIP_H */

// What the DigitCNN kernels of the product (k3_cnn.hip, k3_cnn_h2.hip, k3_cnn_bf16.hip) and the round-1 cross-check kernels of the
// test-only library (x_cnn_round1.hip) all use on the device: the vector types, the input tile, the feature row and the 8-bit input
// glue.  One definition each; the fc heads' shared code is in sv_fc_head.h, its leaf functions in sv_device.h.
#pragma once
#include "sv_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int IN_W = 30, IN_CELL = 900;  // zero-padded 30x30 input
constexpr int FEAT = 3136;
// the f32 kernels' conv1 output in the LDS (k3_cnn.hip, x_cnn_round1.hip)
constexpr int PLANE = 257;               // 16x16 plane + 1 float of bank skew
constexpr int C1_CELL = 32 * PLANE;      // conv1 output of one cell

__device__ __forceinline__ float glue_norm(u8 c) { return sv_glue_norm(c); }     // sv_device.h: shared with k8_cnn_v3.hip

}  // namespace

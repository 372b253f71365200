// What the f32 DigitCNN kernels of the product (k3_cnn.hip) and the round-1 cross-check kernels of the test-only library
// (x_cnn_round1.hip) both use on the device: the LDS geometry of a cell, the feature row, and the 8-bit input glue.  One definition each;
// the fc heads' shared epilogue is in sv_device.h.
#pragma once
#include "sv_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int PLANE = 257;               // 16x16 plane + 1 float of bank skew
constexpr int C1_CELL = 32 * PLANE;      // conv1 output of one cell
constexpr int IN_W = 30, IN_CELL = 900;  // zero-padded 30x30 input
constexpr int FEAT = 3136;

__device__ __forceinline__ float glue_norm(u8 c) { return sv_glue_norm(c); }     // sv_device.h: shared with k8_cnn_v3.hip

}  // namespace

// Test-only (libsudokuvision_xcheck.so): selects K15's two-launch shape, so that tests and tools/time_motion.py can hold the two launch
// shapes of csrc/k15_motion.hip against each other.  Both are the product's own kernels; only this setter is not shipped.
#include "../../include/sudoku_vision_xcheck.h"
#include "sv_internal.h"

extern "C" int svx_ctx_set_motion_shape(sv_ctx *ctx, int shape)
{
    if (!ctx || (shape != SVX_MOTION_ONE_LAUNCH && shape != SVX_MOTION_TWO_PASS)) return sv_fail(SV_ERR_BAD_ARG, "svx_ctx_set_motion_shape: bad argument");
    ctx->x_motion_shape = shape;
    return SV_OK;
}

// The product's side of the seam to the cross-check kernels (sv_internal.h): libsudokuvision_hip.so has none.
#include "sv_internal.h"

const sv_xcheck_ops *const sv_xcheck = nullptr;

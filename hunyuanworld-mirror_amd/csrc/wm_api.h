// What the C-ABI entry files (wm_api_ops.cpp, wm_api_scene.cpp) share: the public header, the launcher interface and the status mapping.
#pragma once
#include "../../include/wm_hip.h"
#include "wm_kernels.h"

// For entries whose launcher checks sizes itself and answers hipErrorInvalidValue: that is the caller's mistake, not a HIP failure.
// Entries that report every launcher error as WM_ERR_HIP write `== hipSuccess ? WM_OK : WM_ERR_HIP` out and do not come through here.
static inline wm_status wm_status_of(hipError_t e) { return e == hipSuccess ? WM_OK : e == hipErrorInvalidValue ? WM_ERR_INVALID : WM_ERR_HIP; }

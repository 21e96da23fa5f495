// sbm_capi.hip — host side of libsbm_hip.so: the C ABI of include/sbm.h on top
// of the kernels in sbm_kernels.h.  gfx950 only; there is no CPU fallback: every
// entry point fails with SBM_ERR_HIP when no GPU is usable.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <dlfcn.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sbm.h"
#include "sbm_kernels.h"
#include "sbm_call_record.h"
#include "sbm_quantize_stream.h"
#include "sbm_quantize_rows_plan.h"
#include "sbm_source_lines.h"
#include "sbm_frame_ptrs_plan.h"
#include "sbm_frame_planes_plan.h"
#include "sbm_frame_source.h"
#include "sbm_train_kernels.h"
#include "sbm_rotate_kernels.h"
#include "sbm_nms_kernels.h"
#include "sbm_verify_kernels.h"
#include "sbm_install_kernels.h"

using namespace sbm;

// Round 3: the host side is one translation unit in four parts.
#include "sbm_capi_ctx.inc"     // sbm_ctx, buffers, launch helpers
#include "sbm_capi_match.inc"   // the match entry points of include/sbm.h
#include "sbm_capi_stages.inc"  // stage entry points, profiling
#include "sbm_capi_multi.inc"   // RCCL, sharded / banded steps, sbm_match_sharded
#include "sbm_capi_nms.inc"     // match epilogue + NMS on the device
#include "sbm_capi_train.inc"   // batched template training on the device
#include "sbm_capi_install.inc" // device-trained families as the template set
#include "sbm_capi_verify.inc"  // normalised correlation per kept match on the device

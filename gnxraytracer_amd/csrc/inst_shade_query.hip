// inst_shade_query.hip -- explicit instantiations of the shading-query kernels (shade_query_kernel.hip.h); api.hip sees them as `extern template`
#include <hip/hip_runtime.h>

#include "host_scene.h"
#include "shade_query_kernel.hip.h"
using namespace gnxr;
template GX_BSDF_QUERY_SIGNATURE(LM_ALL)
template GX_LIGHT_SAMPLE_QUERY_SIGNATURE(LT_ALL)
template GX_LIGHT_LE_QUERY_SIGNATURE(LT_ALL)
template GX_TRACE_CLOSEST_CODE_SIGNATURE(32)
template GX_TRACE_CLOSEST_CODE_SIGNATURE(64)

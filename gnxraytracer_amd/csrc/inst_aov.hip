// inst_aov.hip -- explicit instantiations of the feature-buffer resolve kernel (aov_kernel.hip.h); api.hip sees them as `extern template`
#include <hip/hip_runtime.h>

#include "host_scene.h"
#include "aov_kernel.hip.h"
using namespace gnxr;
#define X(M) template GX_AOV_RESOLVE_SIGNATURE(M)
GX_AOV_INSTANCES(X)
#undef X

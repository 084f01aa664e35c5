// inst_shade_kinds.hip -- explicit instantiations of k_shade for the kinds of glossy material (conductor, rough dielectric), see kernel_instances.h
#include "kernel_instances.h"
using namespace gnxr;
#define X(M, L) template GX_SHADE_KIND_SIGNATURE(M, L)
GX_SHADE_KIND_INSTANCES(X)
#undef X

// inst_shade_kinds.hip -- explicit instantiations of k_shade for the kinds of glossy material (conductor, rough dielectric) and for the reordered MIS half
// (SM_DIR_FIRST, SM_DEFER), see kernel_instances.h
#include "kernel_instances.h"
using namespace gnxr;
#define X(M, L) template GX_SHADE_KIND_SIGNATURE(M, L)
GX_SHADE_KIND_INSTANCES(X)
#undef X
#define X(M, L, S) template GX_SHADE_MIS_SIGNATURE(M, L, S)
GX_SHADE_MIS_INSTANCES(X)
#undef X

// material_kernel.hip.h -- gnxr_scene_update_materials / gnxr_scene_set_triangle_materials on the device: the per-triangle share of the
// material tables, which is held in LEAF order (DTri::material, tri_class[]), rewritten from tables held in AUTHORING order.  After
// gnxr_scene_rebuild_bvh the leaf order exists only on the device, so the way from one order to the other is DTri::prim, read here.
//
//   k_material_tris     every leaf-order triangle: material word and key byte (shade class | kind << kClassKeyKindShift) from its authored
//                       material and its own-attributes byte
//   k_material_gather   the inverse (test hook): per authored triangle the authored material it shows and its shade class
//
// The arithmetic is triangle_material's (scene_compile.cpp), which gnxr_scene_create applies on the host.
#pragma once
#include <hip/hip_runtime.h>

#include "gnxr_device_types.h"
#include "refit_kernel.hip.h"

namespace gnxr {
namespace matedit {

// tri_material / own_attr: per authored triangle; mat_map: per authored material (internal index or -1, attribute copy or -1, shade class, kind).
// Writes 4 bytes of the triangle's second row and one byte of tri_class: plain stores, every element by one lane.  The ids in tri_material
// were validated on the host ([-1, n_materials)), so mat_map is indexed without a further test.
static __global__ void __launch_bounds__(refit::kB) k_material_tris(DTri *__restrict__ tris, unsigned char *__restrict__ tri_class, int n_tris,
                                                                    const int *__restrict__ tri_material, const unsigned char *__restrict__ own_attr,
                                                                    const int4 *__restrict__ mat_map) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const int prim = tris[li].prim;
        if ((unsigned)prim >= (unsigned)n_tris) continue;   // bounds guard: prim indexes two tables here; a damaged triangle table must not become a wild read
        const int authored = tri_material[prim];
        int material = authored, cls = 0;
        if (authored >= 0) {
            const int4 e = mat_map[authored];
            const bool own = own_attr[prim] != 0;
            material = e.x < 0 ? -1 : (own ? e.y : e.x);
            cls = e.x < 0 ? 0 : (own ? 3 : (e.z | (e.w << kClassKeyKindShift)));
        }
        tris[li].material = material;
        tri_class[li] = (unsigned char)cls;
    }
}

// authored: per internal material (the attribute copies included) the authored index (CompiledScene::material_authored)
static __global__ void __launch_bounds__(refit::kB) k_material_gather(const DTri *__restrict__ tris, const unsigned char *__restrict__ tri_class, int n_tris,
                                                                      const int *__restrict__ authored, int *__restrict__ material_out,
                                                                      unsigned char *__restrict__ class_out) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const int prim = tris[li].prim;
        if ((unsigned)prim >= (unsigned)n_tris) continue;   // bounds guard: prim is a store index here
        const int m = tris[li].material;
        material_out[prim] = m >= 0 ? authored[m] : -1;
        class_out[prim] = tri_class[li] & kClassKeyClassMask;
    }
}

}  // namespace matedit
}  // namespace gnxr

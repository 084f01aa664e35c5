// lights_kernel.hip.h -- gnxr_scene_set_lights on the device: which light a triangle is (DTri::light) is held in LEAF order, a light's
// triangle (gnxr_light::tri) is given in AUTHORING order.  After gnxr_scene_rebuild_bvh / gnxr_scene_set_geometry the leaf order exists
// only on the device, so the way from one order to the other is DTri::prim, read here (as material_kernel.hip.h does for the materials).
//
//   k_lights_scatter   one lane per light record: light_of_prim[tri] = its index, for the AREA_TRI records (the table is -1 on entry)
//   k_lights_bind      one lane per leaf-order triangle: DTri::light from light_of_prim[prim], and the light's tri_leaf the other way
//   k_lights_gather    the inverse (test hook): DTri::light per triangle in authoring order
//
// Corners, area, inv_area and normal of the bound records are k_refit_lights' (refit_kernel.hip.h), which runs after k_lights_bind.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/gnxr.h"
#include "gnxr_device_types.h"
#include "refit_kernel.hip.h"

namespace gnxr {
namespace lightedit {

// The records arrive with tri_leaf holding the AUTHORED triangle of an AREA_TRI light (-1 for every other type).  The host has refused
// ranges outside [0, n_tris) and triangles named twice, so every word has one writer; the range is tested again because it is a store index.
static __global__ void __launch_bounds__(refit::kB) k_lights_scatter(const DLight *__restrict__ lights, int n_lights, int *__restrict__ light_of_prim, int n_tris) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_lights; i += gridDim.x * blockDim.x) {
        if (lights[i].type != GNXR_LIGHT_AREA_TRI) continue;
        const int prim = lights[i].tri_leaf;
        if ((unsigned)prim < (unsigned)n_tris) light_of_prim[prim] = i;
    }
}

// Writes 4 bytes of the triangle's third row (plain stores, every element by one lane) and, for an emissive triangle, the tri_leaf word of
// its record in `lights` (null: the triangles only -- how a failed call puts the old values back).  tri_n / tri_s: the scene's per-corner
// normals and tangents in leaf order (12 floats per triangle, zeros == none) or null; a triangle that has either and becomes emissive
// raises *flag, as gnxr_scene_create refuses it (a byte-wise test: -0 counts as a value, as there).
static __global__ void __launch_bounds__(refit::kB) k_lights_bind(DTri *__restrict__ tris, int n_tris, const int *__restrict__ light_of_prim, DLight *__restrict__ lights,
                                                                 int n_lights, const float *__restrict__ tri_n, const float *__restrict__ tri_s, int *__restrict__ flag) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const int prim = tris[li].prim;
        if ((unsigned)prim >= (unsigned)n_tris) continue;   // bounds guard: prim indexes a table here; a damaged triangle table must not become a wild read
        const int l = light_of_prim[prim];
        tris[li].light = l;
        if (l < 0 || l >= n_lights || !lights) continue;
        lights[l].tri_leaf = li;
        unsigned int any = 0;
        if (tri_n) for (int k = 0; k < 9; ++k) any |= __float_as_uint(tri_n[(size_t)li * 12 + k]);
        if (tri_s) for (int k = 0; k < 9; ++k) any |= __float_as_uint(tri_s[(size_t)li * 12 + k]);
        if (any) *flag = 1;
    }
}

static __global__ void __launch_bounds__(refit::kB) k_lights_gather(const DTri *__restrict__ tris, int n_tris, int *__restrict__ light_out) {
    for (int li = blockIdx.x * blockDim.x + threadIdx.x; li < n_tris; li += gridDim.x * blockDim.x) {
        const int prim = tris[li].prim;
        if ((unsigned)prim >= (unsigned)n_tris) continue;   // bounds guard: prim is a store index here
        light_out[prim] = tris[li].light;
    }
}

}  // namespace lightedit
}  // namespace gnxr

// hot_leaves_table.cpp -- dev tool (host compiler only): which leaves do the first 64 breadth-first 4-wide nodes of a scene reference, and what
// do they take of k_trace4's hot-leaf region (trace4_kernel.hip.h: 48 B per triangle, 32 B per leaf box, kHotBytes = 768)?
// Compiles a mesh with the library's own scene compiler (scene_compile.cpp + scene_builder.cpp), as tests/wide_collapse_check.cpp does.
// usage: hot_leaves_table mesh.bin      mesh.bin = int32 n_vertices, int32 n_triangles, float32 xyz[n_vertices][3], int32 idx[n_triangles][3]
//        (python tools/hot_leaves_table.py writes it for the benchmark's scenes and runs this)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gnxr.h"
#include "host_scene.h"

using namespace gnxr;

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: %s mesh.bin\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    int32_t nv = 0, nt = 0;
    if (std::fread(&nv, 4, 1, f) != 1 || std::fread(&nt, 4, 1, f) != 1 || nv <= 0 || nt <= 0) return 2;
    std::vector<float> v(3 * (size_t)nv);
    std::vector<int32_t> idx(3 * (size_t)nt), mat(nt, -1), light(nt, -1);
    if (std::fread(v.data(), 4, v.size(), f) != v.size() || std::fread(idx.data(), 4, idx.size(), f) != idx.size()) return 2;
    std::fclose(f);
    gnxr_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.abi_version = GNXR_ABI_VERSION;
    d.n_vertices = nv; d.n_triangles = nt;
    d.vertices = v.data(); d.indices = idx.data(); d.tri_material = mat.data(); d.tri_light = light.data();
    d.camera_medium = -1;
    d.bvh_split_method = GNXR_BVH_SAH;
    CompiledScene cs;
    if (!compile_scene(&d, &cs)) { std::printf("compile_scene failed\n"); return 1; }
    const int kTop = 64, kHotBytes = 768;
    std::printf("%d triangles, %zu DNode4, root4 %d, leaf1_from_verts %d\n", nt, cs.nodes4.size(), cs.root4, cs.leaf1_from_verts);
    std::printf("node slot  first  tris  box  bytes  sum  admitted\n");
    int sum = 0, leaves = 0, hot = 0;
    for (int n = 0; n < kTop && n < (int)cs.nodes4.size() && cs.root4 >= 0; ++n)
        for (int s = 0; s < 4; ++s) {
            const int32_t ref = cs.nodes4[n].child[s];
            if (ref >= -1) continue;   // interior, or kNode4Empty
            const int lr = ~ref, first = lr & 0xffffff, cnt = (lr >> 24) & 0x7f;
            const int box = (cnt > 1 || !cs.leaf1_from_verts) ? 1 : 0;
            const int bytes = 48 * cnt + 32 * box;
            sum += bytes; ++leaves;
            const bool ok = sum <= kHotBytes;   // thread order, a prefix sum: as the kernel's prologue admits them
            hot += ok;
            std::printf("%4d %4d %6d %5d %4d %6d %4d  %s\n", n, s, first, cnt, box, bytes, sum, ok ? "yes" : "no");
        }
    std::printf("%d leaves under the first %d nodes, %d B; %d admitted\n", leaves, kTop, sum, hot);
    return 0;
}

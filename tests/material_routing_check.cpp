// material_routing_check.cpp -- stand-alone host program behind tests/test_material_grid.py::test_compile_material_routing: the material
// compiler (compile_materials, scene_compile.cpp) on the gnxr_material records of a file, host compiler only, no device.  For every record
// one line: its index, the number of lobes with allowMultipleLobes (Path / VolPath / DirectLighting), the number without (Whitted), the
// shade class and the material kind -- what routes a hit to one of the k_shade instances.  "OK" at the end; exits 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gnxr.h"
#include "host_scene.h"

using namespace gnxr;

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: material_routing_check <file of gnxr_material records>\n"); return 1; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 1; }
    std::vector<gnxr_material> mats;
    gnxr_material m;
    while (std::fread(&m, sizeof(m), 1, f) == 1) mats.push_back(m);
    std::fclose(f);
    if (mats.empty()) { std::printf("no records\n"); return 1; }
    MaterialTables mt;
    const std::vector<int32_t> no_spheres;
    if (!compile_materials(mats.data(), (int)mats.size(), 0, no_spheres, nullptr, nullptr, 0, nullptr, &mt)) { std::printf("FAILED %s\n", get_error()); return 1; }
    for (size_t i = 0; i < mats.size(); ++i) {
        const int32_t *map = &mt.mat_map[4 * i];   // internal index (-1: no BSDF), attribute copy, shade class, kind
        int lobes = 0, lobes_single = 0;
        if (map[0] >= 0) {
            const DMaterial &d = mt.materials[map[0]], &s = mt.materials_single[map[0]];
            lobes = d.n_lobes; lobes_single = s.n_lobes;
            if (d.shade_class != map[2] || material_kind(d) != map[3]) { std::printf("FAILED mat_map of record %zu disagrees with its compiled material\n", i); return 1; }
        }
        std::printf("%zu %d %d %d %d\n", i, lobes, lobes_single, map[2], map[3]);
    }
    std::printf("OK\n");
    return 0;
}

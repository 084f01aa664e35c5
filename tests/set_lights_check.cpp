// set_lights_check.cpp -- stand-alone host program behind tests/test_set_lights.py::test_light_list_validation_host: the host part of
// gnxr_scene_set_lights (compile_light_list, scene_compile.cpp) on a scene compiled by the library's own scene compiler (host compiler
// only, no device).  Every rule of the call that is decided on the host is asked here: ranges, duplicates, unknown types, the INFINITE
// rules, and that a refusal or an acceptance leaves the compiled scene as it was.  Prints one line per case and "OK" at the end; exits 1
// at the first failed check.  (Also the program to build with -fsanitize=address,undefined when the validation changes.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gnxr.h"
#include "host_scene.h"

using namespace gnxr;

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static gnxr_light light(int type, int tri = -1) {
    gnxr_light l;
    std::memset(&l, 0, sizeof(l));
    l.type = type; l.tri = tri; l.n_samples = 1;
    l.le[0] = l.le[1] = l.le[2] = 1.f;
    for (int k = 0; k < 4; ++k) l.light_to_world[5 * k] = 1.f;
    l.center[2] = 1.f; l.radius = 30.f; l.falloff_start = 20.f;
    return l;
}

// kNt triangles in a row; lights: AREA on triangle 1, then (with_env) a SKYBOX if sky_first, the INFINITE light, a POINT light
static const int kNt = 7;
static bool compile(bool with_env, bool sky_first, CompiledScene *cs, std::vector<gnxr_light> *lights) {
    static std::vector<float> verts;
    static std::vector<int32_t> idx, mat, tl;
    static std::vector<float> env;
    verts.clear(); idx.clear();
    for (int i = 0; i < kNt; ++i) {
        const float p[9] = {(float)i, 0, 0, i + 0.8f, 0, 0.1f * i, (float)i, 1, 0};
        verts.insert(verts.end(), p, p + 9);
        for (int k = 0; k < 3; ++k) idx.push_back(3 * i + k);
    }
    mat.assign(kNt, -1); tl.assign(kNt, -1);
    lights->clear();
    lights->push_back(light(GNXR_LIGHT_AREA_TRI, 1));
    tl[1] = 0;
    if (with_env) {
        if (sky_first) lights->push_back(light(GNXR_LIGHT_SKYBOX));
        lights->push_back(light(GNXR_LIGHT_INFINITE));
    }
    lights->push_back(light(GNXR_LIGHT_POINT));
    env.assign(8 * 4 * 3, 0.5f);
    gnxr_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.abi_version = GNXR_ABI_VERSION;
    d.n_vertices = 3 * kNt; d.n_triangles = kNt;
    d.vertices = verts.data(); d.indices = idx.data(); d.tri_material = mat.data(); d.tri_light = tl.data();
    d.lights = lights->data(); d.n_lights = (int)lights->size();
    if (with_env) { d.env_rgb = env.data(); d.env_width = 8; d.env_height = 4; }
    d.camera_medium = -1;
    d.bvh_split_method = GNXR_BVH_SAH;
    return compile_scene(&d, cs);
}

struct Out { std::vector<DLight> recs; std::vector<int32_t> inf, lop; };
static int run(const CompiledScene &cs, const std::vector<gnxr_light> &ls, Out *o, const char *what, int want) {
    const std::vector<DLight> lights0 = cs.lights;
    const std::vector<gnxr_light> desc0 = cs.desc_lights;
    const std::vector<int32_t> inf0 = cs.infinite_lights;
    const int rc = compile_light_list(cs, ls.empty() ? nullptr : ls.data(), (int)ls.size(), &o->recs, &o->inf, &o->lop);
    std::printf("%-58s -> %d%s%s\n", what, rc, rc ? "  " : "", rc ? get_error() : "");
    CHECK(rc == want, "%s: expected %d", what, want);
    CHECK(lights0.size() == cs.lights.size() && std::memcmp(lights0.data(), cs.lights.data(), lights0.size() * sizeof(DLight)) == 0, "%s: cs.lights changed", what);
    CHECK(desc0.size() == cs.desc_lights.size() && (desc0.empty() || std::memcmp(desc0.data(), cs.desc_lights.data(), desc0.size() * sizeof(gnxr_light)) == 0), "%s: cs.desc_lights changed", what);
    CHECK(inf0 == cs.infinite_lights, "%s: cs.infinite_lights changed", what);
    if (rc == GNXR_ERR_UNSUPPORTED) CHECK(std::strstr(get_error(), "gnxr_scene_update_environment") != nullptr, "%s: the message does not name gnxr_scene_update_environment", what);
    return rc;
}

int main() {
    Out o;
    {   // a scene without an INFINITE light
        CompiledScene cs;
        std::vector<gnxr_light> ls;
        CHECK(compile(false, false, &cs, &ls), "%s", get_error());
        run(cs, {}, &o, "no env: empty list", GNXR_OK);
        CHECK(o.recs.size() == 1 && o.inf.empty() && (int)o.lop.size() == kNt, "sizes of the empty list");
        for (int v : o.lop) CHECK(v == -1, "light_of_prim of the empty list");
        std::vector<gnxr_light> many;
        for (int t = kNt - 1; t >= 0; --t) many.push_back(light(GNXR_LIGHT_AREA_TRI, t));
        many.push_back(light(GNXR_LIGHT_SKYBOX));
        many.push_back(light(GNXR_LIGHT_SPOT));
        many.push_back(light(GNXR_LIGHT_DISTANT));
        run(cs, many, &o, "no env: every triangle emissive + sky + spot + distant", GNXR_OK);
        CHECK((int)o.recs.size() == kNt + 3 && o.inf.size() == 1 && o.inf[0] == kNt, "sizes");
        for (int t = 0; t < kNt; ++t) {
            CHECK(o.lop[t] == kNt - 1 - t, "light_of_prim[%d] = %d", t, o.lop[t]);
            CHECK(o.recs[kNt - 1 - t].type == GNXR_LIGHT_AREA_TRI && o.recs[kNt - 1 - t].tri_leaf == t, "the record carries its authored triangle");
        }
        CHECK(o.recs[kNt].tri_leaf == -1 && o.recs[kNt + 1].tri_leaf == -1, "tri_leaf of the other types");
        std::vector<gnxr_light> bad = many;
        bad[2].tri = kNt;
        run(cs, bad, &o, "no env: tri == n_triangles", GNXR_ERR_INVALID);
        bad[2].tri = -1;
        run(cs, bad, &o, "no env: tri == -1", GNXR_ERR_INVALID);
        bad[2].tri = 0x7fffffff;
        run(cs, bad, &o, "no env: tri == INT_MAX", GNXR_ERR_INVALID);
        bad = many;
        bad[kNt - 1].tri = bad[0].tri;
        run(cs, bad, &o, "no env: a triangle named twice", GNXR_ERR_INVALID);
        bad = many;
        bad.back().type = 77;
        run(cs, bad, &o, "no env: unknown type after good records", GNXR_ERR_INVALID);
        bad.back().type = 0;
        run(cs, bad, &o, "no env: type 0", GNXR_ERR_INVALID);
        bad = many;
        bad.push_back(light(GNXR_LIGHT_INFINITE));
        run(cs, bad, &o, "no env: an INFINITE record", GNXR_ERR_UNSUPPORTED);
    }
    for (int sky_first = 0; sky_first < 2; ++sky_first) {
        CompiledScene cs;
        std::vector<gnxr_light> ls;
        CHECK(compile(true, sky_first != 0, &cs, &ls), "%s", get_error());
        const gnxr_light env = ls[sky_first ? 2 : 1], sky = light(GNXR_LIGHT_SKYBOX);
        run(cs, ls, &o, sky_first ? "sky + env: the list it has" : "env: the list it has", GNXR_OK);
        CHECK(o.inf == cs.infinite_lights, "infinite indices of the unchanged list");
        std::vector<gnxr_light> l2;
        if (sky_first) l2 = {sky, light(GNXR_LIGHT_POINT), env}; else l2 = {env, light(GNXR_LIGHT_AREA_TRI, 5), sky};
        run(cs, l2, &o, "env moved to another index, its side of the sky box kept", GNXR_OK);
        CHECK(o.inf.size() == 2, "two infinite indices");
        if (sky_first) l2 = {env, sky}; else l2 = {sky, env};
        run(cs, l2, &o, "env moved across a SKYBOX record", GNXR_ERR_UNSUPPORTED);
        if (sky_first) l2 = {sky, env, env}; else l2 = {env, env};
        run(cs, l2, &o, "a second INFINITE record", GNXR_ERR_UNSUPPORTED);
        if (sky_first) l2 = {sky, light(GNXR_LIGHT_AREA_TRI, 0)}; else l2 = {light(GNXR_LIGHT_AREA_TRI, 0)};
        run(cs, l2, &o, "the INFINITE record dropped", GNXR_ERR_UNSUPPORTED);
        run(cs, {}, &o, "the empty list on a scene with an INFINITE light", GNXR_ERR_UNSUPPORTED);
        gnxr_light changed = env;
        changed.n_samples = 4;
        if (sky_first) l2 = {sky, changed}; else l2 = {changed};
        run(cs, l2, &o, "the INFINITE record with another n_samples", GNXR_ERR_UNSUPPORTED);
        if (!sky_first) {   // dropping the sky box that FOLLOWED the environment light is fine: flip_y looks at what precedes it
            l2 = {env};
            run(cs, l2, &o, "only the INFINITE record", GNXR_OK);
        }
    }
    std::printf("OK\n");
    return 0;
}

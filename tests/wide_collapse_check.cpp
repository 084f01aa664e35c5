// wide_collapse_check.cpp -- stand-alone host program behind tests/test_wide_collapse.py: compiles seeded triangle soups with the
// library's own scene compiler (scene_compile.cpp + scene_builder.cpp, host compiler only) and checks the 4-wide tree against the binary
// tree it was collapsed from.  Everything the checks compare against is computed here by recursion on the binary tree, not with the
// functions of wide_collapse.h.  Prints one line per soup and "OK" at the end; exits 1 at the first failed check.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "gnxr.h"
#include "host_scene.h"

using namespace gnxr;

#define CHECK(c, ...) do { if (!(c)) { std::printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static bool compile(const std::vector<float> &verts, CompiledScene *cs) {
    const int n = (int)verts.size() / 9;
    std::vector<int32_t> idx(3 * (size_t)n), mat(n, -1), light(n, -1);
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int32_t)i;
    gnxr_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.abi_version = GNXR_ABI_VERSION;
    d.n_vertices = 3 * n; d.n_triangles = n;
    d.vertices = verts.data(); d.indices = idx.data(); d.tri_material = mat.data(); d.tri_light = light.data();
    d.camera_medium = -1;
    d.bvh_split_method = GNXR_BVH_SAH;
    return compile_scene(&d, cs);
}

static std::vector<float> soup(int n, uint32_t seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(0.f, 1.f);
    std::vector<float> v;
    for (int i = 0; i < n; ++i) {
        const float c[3] = {u(rng), u(rng), u(rng)};
        const float s = 0.02f + 0.2f * u(rng) * u(rng);
        for (int k = 0; k < 9; ++k) v.push_back(c[k % 3] + s * (u(rng) - .5f));
    }
    return v;
}
// triangle i sits at 3^i on the x axis and is 3^i large: every SAH split peels the smallest ones off one end, the cuts become chains
static std::vector<float> growing_soup(int n) {
    std::vector<float> v;
    float x = 1.f;
    for (int i = 0; i < n; ++i, x *= 3.f) {
        const float p[9] = {x, 0.f, 0.f, x * 1.5f, x * 0.5f, 0.f, x, 0.f, x * 0.5f};
        v.insert(v.end(), p, p + 9);
    }
    return v;
}

struct Tree {
    const CompiledScene &cs;
    const std::vector<DNode> &bn;
    explicit Tree(const CompiledScene &c) : cs(c), bn(c.nodes) {}
    bool leaf(int x) const { return (bn[x].meta & 0xffffu) != 0; }
    int A(int x) const { return x + 1; }
    int B(int x) const { return bn[x].offset; }
    int axis(int x) const { return (int)(bn[x].meta >> 16); }
    double area(int x) const {
        const double dx = (double)bn[x].hi0 - bn[x].lo[0], dy = (double)bn[x].hi1 - bn[x].lo[1], dz = (double)bn[x].hi2 - bn[x].lo[2];
        return 2. * (dx * dy + dy * dz + dz * dx);
    }
    int32_t leaf_ref(int x) const { return ~(int32_t)((uint32_t)bn[x].offset | ((bn[x].meta & 0x7fu) << 24)); }
};

struct Tally { long cut2 = 0, cut3 = 0, balanced4 = 0, chain4 = 0; };

// slots of the cut in the order BVHAccel::Intersect reaches them for a ray of octant `oct`: near child first at every binary node
static void near_first(const Tree &t, int x, const int slot_of[], const int src[4], int oct, std::vector<int> *out, int depth) {
    for (int k = 0; k < 4; ++k) if (src[k] == x) { out->push_back(k); return; }
    CHECK(!t.leaf(x) && depth < 3, "binary node %d lies under no slot", x);
    const int neg = (oct >> t.axis(x)) & 1;
    near_first(t, neg ? t.B(x) : t.A(x), slot_of, src, oct, out, depth + 1);
    near_first(t, neg ? t.A(x) : t.B(x), slot_of, src, oct, out, depth + 1);
}
// the four slots a 4-bit code stands for, nearest first (the table of the DNode4 layout, restated)
static void decode(unsigned code, int o[4]) {
    const int d2 = (code >> 2) & 1, d1 = (code >> 1) & 1, d0 = code & 1;
    if (!(code & 8u)) {
        const int first = d2 ? 2 : 0, second = 2 - first;
        o[0] = first + d1; o[1] = first + 1 - d1; o[2] = second + d0; o[3] = second + 1 - d0;
    } else {
        std::vector<int> pair = d0 ? std::vector<int>{3, 2} : std::vector<int>{2, 3}, rest, all;
        if (d1) { rest = pair; rest.push_back(1); } else { rest = {1}; rest.insert(rest.end(), pair.begin(), pair.end()); }
        if (d2) { all = rest; all.push_back(0); } else { all = {0}; all.insert(all.end(), rest.begin(), rest.end()); }
        for (int i = 0; i < 4; ++i) o[i] = all[i];
    }
}

// walks the 4-wide tree from DNode4 `i`, whose children must be a cut under binary node `R`
static void walk(const Tree &t, int i, int R, int below_in, std::vector<int> *tri_seen, std::vector<char> *node_seen, int *need, double *root_area, Tally *tally) {
    const CompiledScene &cs = t.cs;
    CHECK(i >= 0 && (size_t)i < cs.nodes4.size() && !(*node_seen)[i], "DNode4 %d out of range or reached twice", i);
    (*node_seen)[i] = 1;
    CHECK(!t.leaf(R), "DNode4 %d is rooted at a leaf", i);
    const DNode4 &d = cs.nodes4[i];
    const int32_t *src = &cs.node4_src[4 * (size_t)i];
    *root_area += t.area(R);
    int n = 0;
    for (int k = 0; k < 4; ++k) {
        if (src[k] < 0) {
            CHECK(d.child[k] == kNode4Empty && d.lox[k] > d.hix[k] && d.loy[k] > d.hiy[k] && d.loz[k] > d.hiz[k], "empty slot %d of node %d is not inverted", k, i);
            continue;
        }
        ++n;
        const DNode &g = t.bn[src[k]];
        const float have[6] = {d.lox[k], d.loy[k], d.loz[k], d.hix[k], d.hiy[k], d.hiz[k]}, want[6] = {g.lo[0], g.lo[1], g.lo[2], g.hi0, g.hi1, g.hi2};
        CHECK(std::memcmp(have, want, sizeof(have)) == 0, "slot %d of node %d does not hold the box of binary node %d", k, i, src[k]);
        for (int j = 0; j < k; ++j) CHECK(src[j] != src[k], "binary node %d fills two slots", src[k]);
    }
    CHECK(n >= 2 && n <= 4, "node %d has %d children", i, n);
    bool chain = false;
    for (int oct = 0; oct < 8; ++oct) {
        std::vector<int> want;
        near_first(t, R, nullptr, src, oct, &want, 0);   // also: every leaf under R lies under exactly one slot
        CHECK((int)want.size() == n, "the slots of node %d are no cut", i);
        const unsigned byte = ((oct < 4 ? d.order_lo : d.order_hi) >> (8 * (oct & 3))) & 255u, code = (d.codes >> (4 * oct)) & 15u;
        int by_code[4];
        decode(code, by_code);
        std::vector<int> got_byte, got_code;
        unsigned seen = 0;
        for (int j = 0; j < 4; ++j) {
            const int s = (byte >> (2 * j)) & 3;
            seen |= 1u << s;
            if (src[s] >= 0) got_byte.push_back(s);
            if (src[by_code[j]] >= 0) got_code.push_back(by_code[j]);
        }
        CHECK(seen == 15u, "order byte %02x of node %d is no permutation", byte, i);
        CHECK(got_byte == want, "order byte of node %d, octant %d", i, oct);
        CHECK(got_code == want, "order code of node %d, octant %d", i, oct);
        chain = chain || (code & 8u);
    }
    if (n == 2) tally->cut2++; else if (n == 3) tally->cut3++; else if (chain) tally->chain4++; else tally->balanced4++;
    if (chain) CHECK(n == 4, "node %d: a chain of %d", i, n);
    const int below = below_in + n - 1;   // references the node leaves on the stack while its first child is walked
    *need = std::max(*need, below + 1);
    for (int k = 0; k < 4; ++k) {
        if (src[k] < 0) continue;
        if (t.leaf(src[k])) {
            CHECK(d.child[k] == t.leaf_ref(src[k]), "slot %d of node %d: leaf reference", k, i);
            const DNode &g = t.bn[src[k]];
            for (int j = 0; j < (int)(g.meta & 0xffffu); ++j) (*tri_seen)[g.offset + j]++;
        } else {
            CHECK(d.child[k] >= 0 && d.child[k] != kNode4Empty, "slot %d of node %d: interior reference", k, i);
            walk(t, d.child[k], src[k], below, tri_seen, node_seen, need, root_area, tally);
        }
    }
}

// summed area of the DNode4 roots under the two-level rule: every interior node at even depth
static double two_level(const Tree &t, int x, int depth) {
    if (t.leaf(x)) return 0.;
    return ((depth & 1) == 0 ? t.area(x) : 0.) + two_level(t, t.A(x), depth + 1) + two_level(t, t.B(x), depth + 1);
}
// exhaustive: every cut of up to four nodes under x, as lists of nodes
static std::vector<std::vector<int>> cuts(const Tree &t, int x) {
    std::vector<std::vector<int>> r{{x}};
    if (t.leaf(x)) return r;
    const auto a = cuts(t, t.A(x)), b = cuts(t, t.B(x));
    for (const auto &ca : a) for (const auto &cb : b) if (ca.size() + cb.size() <= 4) { auto c = ca; c.insert(c.end(), cb.begin(), cb.end()); r.push_back(c); }
    return r;
}
static double best(const Tree &t, int x) {
    if (t.leaf(x)) return 0.;
    double m = std::numeric_limits<double>::infinity();
    for (const auto &c : cuts(t, x)) {
        if (c.size() < 2) continue;
        double s = 0.;
        for (int y : c) s += best(t, y);
        m = std::min(m, s);
    }
    return t.area(x) + m;
}

static void check_soup(const char *name, const std::vector<float> &verts, Tally *tally) {
    CompiledScene cs;
    CHECK(compile(verts, &cs), "%s: %s", name, get_error());
    const Tree t(cs);
    const int n = (int)verts.size() / 9;
    CHECK(cs.node4_src.size() == 4 * cs.nodes4.size(), "node4_src size");
    if (cs.root4 < 0) {   // a one-leaf scene
        CHECK(cs.nodes.size() == 1 && cs.root4 == t.leaf_ref(0) && cs.nodes4.size() == 1 && cs.stack4_need == 1, "%s: one-leaf scene", name);
        std::printf("%-12s %6d triangles: one leaf\n", name, n);
        return;
    }
    std::vector<int> tri_seen(n, 0);
    std::vector<char> node_seen(cs.nodes4.size(), 0);
    int need = 1;
    double area = 0.;
    Tally local;
    walk(t, cs.root4, 0, 0, &tri_seen, &node_seen, &need, &area, &local);
    for (int i = 0; i < n; ++i) CHECK(tri_seen[i] == 1, "%s: triangle %d reached %d times", name, i, tri_seen[i]);
    for (size_t i = 0; i < node_seen.size(); ++i) CHECK(node_seen[i], "%s: DNode4 %zu is not reachable", name, i);
    CHECK(need == cs.stack4_need, "%s: stack4_need %d, the longest root path needs %d", name, cs.stack4_need, need);
    // fp32 sums of up to 2 log2(n) terms decide the cuts; the areas here are summed in double
    const double tol = 1e-5;
    const double two = two_level(t, 0, 0);
    CHECK(area <= two * (1. + tol), "%s: root area %.9g above the two-level rule's %.9g", name, area, two);
    double opt = -1.;
    if (n <= 13) {
        opt = best(t, 0);
        CHECK(std::fabs(area - opt) <= tol * opt, "%s: root area %.9g, exhaustive search %.9g", name, area, opt);
    }
    std::printf("%-12s %6d triangles: %6zu DNode4  cuts 2/3/4b/4c %ld/%ld/%ld/%ld  stack %d  area %.6g (two-level %.6g%s)\n", name, n, cs.nodes4.size(), local.cut2, local.cut3,
                local.balanced4, local.chain4, need, area, two, opt >= 0. ? ", exhaustive: equal" : "");
    tally->cut2 += local.cut2; tally->cut3 += local.cut3; tally->balanced4 += local.balanced4; tally->chain4 += local.chain4;
}

int main() {
    Tally tally;
    const int sizes[] = {1, 2, 3, 4, 5, 7, 8, 13, 64, 2049};
    for (int n : sizes) {
        char name[32];
        std::snprintf(name, sizeof(name), "soup%d", n);
        check_soup(name, soup(n, 1000u + (uint32_t)n), &tally);
    }
    check_soup("growing12", growing_soup(12), &tally);
    CHECK(tally.cut2 > 0 && tally.cut3 > 0 && tally.balanced4 > 0 && tally.chain4 > 0, "cuts 2/3/4b/4c seen: %ld/%ld/%ld/%ld", tally.cut2, tally.cut3, tally.balanced4, tally.chain4);
    {   // 65 536 triangles on one centroid: one leaf that LinearBVHNode cannot count -- the checked error, no crash
        std::vector<float> v;
        const float p[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
        for (int i = 0; i < 65536; ++i) v.insert(v.end(), p, p + 9);
        CompiledScene cs;
        CHECK(!compile(v, &cs) && std::strstr(get_error(), "16-bit primitive count"), "65 536 coincident triangles: %s", get_error());
        std::printf("coincident65536: refused (%s)\n", get_error());
    }
    std::printf("OK\n");
    return 0;
}

"""gnxr_scene_set_geometry: the triangle mesh of a live scene replaced, tree and tables built on the device (csrc/geometry_kernel.hip.h,
csrc/api_geometry.hip.h in front of the rebuild of csrc/api_rebuild.hip.h).

The reference of every GPU case is a FRESH scene: the same materials, lights, media, textures, spheres and camera, the target mesh and
set_bvh_split_method("hlbvh") -- code the existing suites pin to the compiled reference.  The small soups are also compared with the numpy
restatement (tests/hlbvh_reference.py).  There are no tolerances: trees, 4-wide node tables, hit records, images, ray counts, feature
buffers and light-selection tables are compared bit for bit (binary bounds up to the sign of a zero, the rule of test_hlbvh_build.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before libgnxr.so is loaded, as in test_scene_update.py)

import hlbvh_reference as hr
import scenes
import test_hlbvh_build as thb
import test_scene_rebuild as tsr
import test_scene_update as tsu

ERR_INVALID = -1
W, H, SPP = 48, 40, 4
PER_TRIANGLE = ("indices", "tri_material", "tri_light", "medium_inside", "medium_outside", "uv", "normals", "tangents")


# ---------------------------------------------------------------- helpers
def geometry_of(b):
    """the geometry fields of a builder's description as the keyword arguments of Scene.set_geometry (numpy copies; absent arrays None)"""
    d = b.desc()
    nv, nt = d.n_vertices, d.n_triangles

    def arr(p, shape):
        return np.ctypeslib.as_array(p, shape=shape).copy() if p else None

    return dict(vertices=arr(d.vertices, (nv, 3)), indices=arr(d.indices, (nt, 3)), tri_material=arr(d.tri_material, (nt,)), tri_light=arr(d.tri_light, (nt,)),
                medium_inside=arr(d.tri_medium_inside, (nt,)), medium_outside=arr(d.tri_medium_outside, (nt,)), uv=arr(d.tri_uv, (nt, 6)), normals=arr(d.tri_n, (nt, 9)),
                tangents=arr(d.tri_s, (nt, 9)))


class ReGeom:
    """The builder's description with its geometry fields replaced by `geom` (kept alive here), gnxr_light::tri taken from tri_light and
    the given split method: what Scene.set_geometry(**geom) must be indistinguishable from (with "hlbvh"), and how a scene with the
    builder's materials, lights, media and textures starts on another mesh."""

    def __init__(self, builder, geom, split="hlbvh"):
        self.builder, self.split = builder, {"sah": 0, "hlbvh": 1}[split]
        self.geom = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in geom.items()}
        self.lights = None

    def desc(self):
        d, g = self.builder.desc(), self.geom
        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))
        d.n_vertices, d.n_triangles = len(g["vertices"]), len(g["indices"])
        d.vertices, d.indices, d.tri_material = fp(g["vertices"]), ip(g["indices"]), ip(g["tri_material"])
        if g["tri_light"] is None:
            g["tri_light"] = np.full(d.n_triangles, -1, np.int32)
        d.tri_light, d.tri_medium_inside, d.tri_medium_outside = ip(g["tri_light"]), ip(g["medium_inside"]), ip(g["medium_outside"])
        d.tri_uv, d.tri_n, d.tri_s = fp(g["uv"]), fp(g["normals"]), fp(g["tangents"])
        import gnxraytracer_amd as gx
        self.lights = (gx.Light * max(d.n_lights, 1))()
        if d.n_lights:
            C.memmove(self.lights, d.lights, d.n_lights * C.sizeof(gx.Light))
        for l in range(d.n_lights):
            if self.lights[l].type == gx._abi.LIGHT_AREA_TRI:
                at = np.flatnonzero(g["tri_light"] == l)
                assert len(at) == 1, (l, at)
                self.lights[l].tri = int(at[0])
        d.lights = C.cast(self.lights, C.POINTER(gx.Light))
        d.bvh_split_method = self.split
        d.keep_alive = self   # the arrays live as long as the description (a Scene keeps the description it was created from)
        return d


def start_geometry(target, drop=3):
    """Another mesh for a scene with `target`'s tables: the Cornell box and the 2 k-triangle model (every drop-th model triangle left out),
    every material of the target in turn, its area lights on the first triangles, no media and no per-corner arrays."""
    src = scenes.cornell()
    src.AddModel(tsu.MESH2K, 0)
    g = geometry_of(src)
    nt = len(g["indices"])
    keep = np.ones(nt, bool)
    keep[np.arange(12, nt)[::drop]] = False
    d = target.desc()
    out = dict(vertices=g["vertices"], indices=g["indices"][keep].copy())
    n = len(out["indices"])
    out["tri_material"] = (np.arange(n) % d.n_materials).astype(np.int32)
    out["tri_light"] = np.full(n, -1, np.int32)
    import gnxraytracer_amd as gx
    area = [l for l in range(d.n_lights) if d.lights[l].type == gx._abi.LIGHT_AREA_TRI]
    out["tri_light"][:len(area)] = area
    out.update(medium_inside=None, medium_outside=None, uv=None, normals=None, tangents=None)
    return out


def on_device(g, device=0):
    return {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(f"cuda:{device}")) for k, v in g.items()}


def permuted(g, seed):
    """the same triangles in another order of the list"""
    p = np.random.default_rng(seed).permutation(len(g["indices"]))
    return {k: (v if v is None or k not in PER_TRIANGLE else np.ascontiguousarray(v[p])) for k, v in g.items()}


def same_light_tables(a, b):
    for strategy in ("spatial", "uniform", "power"):
        ta, tb = a.light_grid_table(strategy), b.light_grid_table(strategy)
        assert ta.shape == tb.shape and ta.tobytes() == tb.tobytes(), strategy


def light_copy(gx, rec):
    l = gx.Light()
    C.memmove(C.byref(l), C.byref(rec), C.sizeof(gx.Light))
    return l


def empty_scene(gx):
    s = object.__new__(gx.Scene)
    s._h, s.device, s.n_vertices, s.n_triangles = None, 0, 8, 4
    return s


def record(gx, g, **over):
    """a gnxr_geometry over numpy arrays or tensors (the caller keeps them alive); `over` replaces fields"""
    rec = gx._abi.Geometry()
    rec.struct_size = C.sizeof(gx._abi.Geometry)
    rec.n_vertices, rec.n_triangles = len(g["vertices"]), len(g["indices"])
    for field, key in (("vertices", "vertices"), ("indices", "indices"), ("tri_material", "tri_material"), ("tri_light", "tri_light"), ("tri_medium_inside", "medium_inside"),
                       ("tri_medium_outside", "medium_outside"), ("tri_uv", "uv"), ("tri_n", "normals"), ("tri_s", "tangents")):
        x = g.get(key)
        setattr(rec, field, None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr()))
    for k, v in over.items():
        setattr(rec, k, v)
    return rec


# ---------------------------------------------------------------- CPU
def test_set_geometry_exported_with_a_prototype(gx):
    lib = C.CDLL(gx.LIB_PATH)
    assert hasattr(lib, "gnxr_scene_set_geometry")
    assert "gnxr_scene_set_geometry" in gx._abi.PROTOTYPES


def test_set_geometry_rejects_null_arguments_before_the_device(gx):
    """GNXR_ERR_INVALID without a GPU: a null scene, with and without a record"""
    v, i = thb.make_case("tiny3")
    g = dict(vertices=v, indices=i, tri_material=np.zeros(len(i), np.int32))
    rec = record(gx, g)
    assert gx.lib().gnxr_scene_set_geometry(None, C.byref(rec), None) == ERR_INVALID
    assert gx.lib().gnxr_scene_set_geometry(None, None, None) == ERR_INVALID


def test_geometry_record_layout(gx):
    """the header's layout on this ABI: four int32 and nine pointers, 4 * 4 + 9 * 8 = 88 bytes (the pointers alone are 72), no padding"""
    G = gx._abi.Geometry
    assert C.sizeof(G) == 4 * 4 + 9 * C.sizeof(C.c_void_p) == 88
    assert [getattr(G, f).offset for f, _ in G._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80][:len(G._fields_)]
    assert gx.lib().gnxr_abi_sizeof(14) == -1   # the index list did not grow: the record carries struct_size instead


def test_set_geometry_rejects_malformed_arguments_before_the_library(gx):
    """Wrong types, shapes, dtypes, devices and mixed kinds raise ValueError, a bad stream TypeError / ValueError; the handle here is empty,
    so a library call would fail differently (GnxrError)."""
    s = empty_scene(gx)
    v, i = thb.make_case("tiny4")
    m = np.zeros(len(i), np.int32)
    n = len(i)
    bad_calls = [
        dict(vertices=v.tolist()), dict(vertices="mesh"), dict(vertices=v.astype(np.float64)), dict(vertices=v.reshape(-1)), dict(vertices=v[:, :2]), dict(vertices=v[:0]),
        dict(indices=i.astype(np.int64)), dict(indices=i.reshape(-1)), dict(indices=i[:0]), dict(indices=i.tolist()),
        dict(tri_material=m.astype(np.int64)), dict(tri_material=m[:-1]), dict(tri_material=m.reshape(-1, 1)), dict(tri_material=None), dict(tri_material=1.5), dict(tri_material=True),
        dict(tri_light=m[:-1]), dict(tri_light=m.astype(np.float32)),
        dict(medium_inside=m), dict(medium_outside=m), dict(medium_inside=m, medium_outside=m[:-1]),
        dict(uv=np.zeros((n, 5), np.float32)), dict(uv=np.zeros((n, 6), np.float64)), dict(uv=np.zeros((n - 1, 6), np.float32)),
        dict(normals=np.zeros((n, 3), np.float32)), dict(tangents=np.zeros((n, 9), np.float64)), dict(tangents=np.zeros(9 * n, np.float32)),
        # mixed kinds, and tensors that are not on the scene's device
        dict(vertices=torch.from_numpy(v)), dict(indices=torch.from_numpy(i)), dict(tri_material=torch.from_numpy(m)),
        dict(vertices=torch.from_numpy(v), indices=torch.from_numpy(i), tri_material=torch.from_numpy(m)),
    ]
    for over in bad_calls:
        kw = dict(vertices=v, indices=i, tri_material=m)
        kw.update(over)
        with pytest.raises(ValueError):
            s.set_geometry(**kw)
    for bad, exc in (("stream", TypeError), (1.5, TypeError), (True, TypeError), ([0], TypeError), (object(), TypeError), (-1, ValueError), (np.int64(-3), ValueError)):
        with pytest.raises(exc):
            s.set_geometry(v, i, m, stream=bad)
    assert (s.n_vertices, s.n_triangles) == (8, 4)
    # well-formed arguments reach the library, which refuses the empty handle
    with pytest.raises(gx.GnxrError):
        s.set_geometry(v, i, 0)


# ---------------------------------------------------------------- GPU: tree equality
@functools.lru_cache(maxsize=None)
def soup(name):
    return thb.make_case(name)


@functools.lru_cache(maxsize=None)
def reference_tree(name):
    """computed once and shared (read-only) by the host and the device run of a case"""
    return hr.hlbvh_reference(*soup(name))


def same_rays(a, b, device, seed):
    rays = torch.from_numpy(scenes.random_rays(20000, seed=seed, inside=2.2)).to(f"cuda:{device}")
    ha, hb = a.intersect(rays), b.intersect(rays)
    assert torch.equal(ha.hits.view(torch.int32), hb.hits.view(torch.int32))
    assert torch.equal(a.occluded(rays), b.occluded(rays))
    return int((ha.prim >= 0).sum())


TREE_STEPS = [("tiny1", "tiny5"), ("uniform2049", "tiny3"), ("tiny4", "uniform6000"), ("tiny3", "tiny3shared")]


@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["numpy", "torch"])
@pytest.mark.parametrize("start,target", TREE_STEPS)
def test_set_geometry_tree_equals_fresh_scene(gpu, start, target, memory):
    """growing and shrinking: a leaf root -> two levels of DNode4; across the sort tile edge -> one partial node; -> past 1024 4-wide nodes;
    -> a multi-primitive leaf.  Tree, 4-wide table, info and 20 000 rays of a fresh HLBVH scene, and the numpy reference's tree."""
    v0, i0 = soup(start)
    v1, i1 = soup(target)
    s = gpu.Scene(tsr.soup_builder(gpu, v0, i0, "sah"))
    if memory == "numpy":
        s.set_geometry(v1, i1, 0)
    else:
        g = on_device(dict(vertices=v1, indices=i1), s.device)
        s.set_geometry(g["vertices"], g["indices"], 0)
    assert (s.n_vertices, s.n_triangles) == (len(v1), len(i1))
    fresh = gpu.Scene(tsr.soup_builder(gpu, v1, i1, "hlbvh"))
    tsr.same_scene_tables(s, fresh)
    nodes4, root4, need = s.bvh4()
    n = len(i1)
    if target == "tiny3shared":
        assert root4 == ~(0 | (n << 24)) and nodes4.shape == (1, 32) and not nodes4.any() and need == 1
    else:
        assert root4 == 0
    if target == "tiny5":
        assert len(nodes4) >= 2
    if target == "uniform6000":
        assert len(nodes4) > 1024
    hits = same_rays(s, fresh, s.device, seed=23)
    if n >= 1000:
        assert hits > 0
    tsr.same_tree(s.bvh(), reference_tree(target))
    mat, cls = s.triangle_materials()
    fm, fc = fresh.triangle_materials()
    assert np.array_equal(mat, fm) and np.array_equal(cls, fc) and len(mat) == n


# ---------------------------------------------------------------- GPU: results with every leaf-order table
def moved_emissive_scene():
    """test_scene_rebuild.emissive_scene's tables; its triangles in another order, its emissive meshes elsewhere in space"""
    b = tsr.emissive_scene()
    g = geometry_of(b)
    ev = np.unique(g["indices"][g["tri_light"] >= 0])
    g["vertices"][ev] += np.array([0.07, -0.05, 0.04], np.float32)
    return b, permuted(g, seed=61)


def target_case(kind):
    """(builder that carries the tables, target geometry, integrators that apply)"""
    if kind == "emissive":
        b, g = moved_emissive_scene()
        return b, g, ("path", "whitted", "direct", "volpath")
    b = {"attributes": tsr.attr_scene, "medium": scenes.volume_cornell, "spheres": lambda: scenes.cornell_sphere("glass")}[kind]()
    return b, geometry_of(b), ("path", "volpath") if kind == "medium" else ("path", "whitted", "direct", "volpath")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["attributes", "medium", "spheres", "emissive"])
def test_set_geometry_results_with_other_leaf_order_tables(gpu, kind):
    """Created with SAH on the Cornell box and the 2 k-triangle model, then given: per-corner uvs, normals and tangents under an image
    texture; triangles that bound media, under VolPath; a scene with a sphere (its primitive id, the ids buffer); emissive triangles at
    other places of the list and of space."""
    b, g, names = target_case(kind)
    s = gpu.Scene(ReGeom(b, start_geometry(b), "sah").desc())
    s.set_geometry(**g)
    fresh = gpu.Scene(ReGeom(b, g, "hlbvh").desc())
    tsr.same_scene_tables(s, fresh)
    tsr.same_results(gpu, s, fresh, names=names)
    same_light_tables(s, fresh)
    if kind == "spheres":
        rays = torch.from_numpy(scenes.random_rays(20000, seed=21)).to(f"cuda:{s.device}")
        assert int(s.intersect(rays).prim.max()) == len(g["indices"])   # the sphere: n_triangles + 0


@pytest.mark.gpu
def test_set_geometry_tables_appear_and_vanish(gpu):
    """uvs, normals, tangents and media on a scene that had none, then a plain mesh again: both states equal their fresh scenes"""
    b = tsr.attr_scene()
    g = geometry_of(b)
    plain = start_geometry(b)
    s = gpu.Scene(ReGeom(b, plain, "sah").desc())
    s.set_geometry(**on_device(g, s.device))
    fresh = gpu.Scene(ReGeom(b, g, "hlbvh").desc())
    tsr.same_scene_tables(s, fresh)
    tsr.same_results(gpu, s, fresh, names=("path", "whitted"))
    plain2 = start_geometry(b, drop=2)
    s.set_geometry(**plain2)
    fresh2 = gpu.Scene(ReGeom(b, plain2, "hlbvh").desc())
    tsr.same_scene_tables(s, fresh2)
    tsr.same_results(gpu, s, fresh2, names=("path", "whitted"))
    same_light_tables(s, fresh2)


# ---------------------------------------------------------------- GPU: later edits
@pytest.mark.gpu
def test_later_edits_work_on_the_new_mesh(gpu):
    """update_vertices (a refit over the new corner table), set_triangle_materials, update_lights, rebuild_bvh and a second set_geometry
    back to the first mesh: each state equals the fresh scene given the same edits; the reserved path state does not grow"""
    b, nv = tsu.dragon(gpu)
    g = geometry_of(b)
    first = start_geometry(b)
    it = gpu.PathIntegrator(5, 1.0, "spatial")
    s = gpu.Scene(ReGeom(b, first, "sah").desc())
    it.Reserve(s, W, H, SPP)
    _, st0 = it.Render(s, W, H, SPP)
    s.set_geometry(**on_device(g, s.device))
    b.set_bvh_split_method("hlbvh")
    fresh = gpu.Scene(b)
    tsr.same_scene_tables(s, fresh)
    _, st1 = it.Render(s, W, H, SPP)
    assert st1["state_bytes"] == st0["state_bytes"] > 0
    # a refit
    v2 = tsu.deform(g["vertices"], nv, seed=71, amount=0.05)
    for x in (s, fresh):
        x.update_vertices(v2[:nv])
    tsr.same_scene_tables(s, fresh)
    tsu.same_render(gpu, it, s, fresh, W, H, SPP)
    # materials per triangle
    ids = np.random.default_rng(72).integers(0, b.desc().n_materials, 500).astype(np.int32)
    for x in (s, fresh):
        x.set_triangle_materials(ids, first_triangle=100)
    (ma, ca), (mb, cb) = s.triangle_materials(), fresh.triangle_materials()
    assert np.array_equal(ma, mb) and np.array_equal(ca, cb) and np.array_equal(ma[100:600], ids)
    tsu.same_render(gpu, it, s, fresh, W, H, SPP)
    # an area light's radiance: the record names the triangle the new mesh gives the light
    rec = light_copy(gpu, b.desc().lights[0])
    assert g["tri_light"][rec.tri] == 0 and int(np.flatnonzero(first["tri_light"] == 0)[0]) != rec.tri
    rec.le[0], rec.le[1], rec.le[2] = 3.0 * rec.le[0], 0.5 * rec.le[1], 2.0 * rec.le[2]
    for x in (s, fresh):
        x.update_lights([rec], 0)
    tsu.same_render(gpu, it, s, fresh, W, H, SPP)
    # a rebuild over the refitted vertices
    for x in (s, fresh):
        x.rebuild_bvh()
    tsr.same_scene_tables(s, fresh)
    tsu.same_render(gpu, it, s, fresh, W, H, SPP)
    # back to the first mesh (the light keeps its edited radiance)
    s.set_geometry(**first)
    back = ReGeom(b, first, "hlbvh")
    fresh2 = gpu.Scene(back.desc())
    rec2 = light_copy(gpu, back.lights[0])
    rec2.le[0], rec2.le[1], rec2.le[2] = rec.le[0], rec.le[1], rec.le[2]
    fresh2.update_lights([rec2], 0)
    tsr.same_scene_tables(s, fresh2)
    tsr.same_results(gpu, s, fresh2, names=("path", "direct"))
    _, st2 = it.Render(s, W, H, SPP)
    assert st2["state_bytes"] == st0["state_bytes"]


# ---------------------------------------------------------------- GPU: refusals
def refusal_scene(gx):
    """the Cornell box (triangles 10 and 11 are area lights 0 and 1; light 2 is the sky box) and a soup of 300 triangles; no media"""
    b = scenes.cornell(sky=True)
    v, i = thb.uniform(300, 5)
    b.add_mesh(v, i, 0)
    return b


def bad_geometries(g, k, n_materials, n_lights):
    """(name, geometry with one bad record at triangle k) for every per-triangle GNXR_ERR_INVALID case"""
    nt, nv = len(g["indices"]), len(g["vertices"])

    def edit(**changes):
        out = {key: (None if val is None else val.copy()) for key, val in g.items()}
        for key, fn in changes.items():
            if out[key] is None:
                out[key] = {"medium_inside": np.full(nt, -1, np.int32), "medium_outside": np.full(nt, -1, np.int32), "normals": np.zeros((nt, 9), np.float32),
                            "tangents": np.zeros((nt, 9), np.float32)}[key]
            fn(out[key])
        return out

    def at(row, value, col=None):
        def fn(a):
            if col is None:
                a[row] = value
            else:
                a[row, col] = value
        return fn

    corner = int(g["indices"][k, 0])
    yield "index == n_vertices", edit(indices=at(k, nv, 1))
    yield "index -1", edit(indices=at(k, -1, 2))
    yield "index far outside", edit(indices=at(k, 2 ** 31 - 1, 0))
    yield "material == n_materials", edit(tri_material=at(k, n_materials))
    yield "material -2", edit(tri_material=at(k, -2))
    yield "medium 0 of none", edit(medium_inside=at(0, -1), medium_outside=at(k, 0))
    yield "medium -2", edit(medium_inside=at(k, -2), medium_outside=at(0, -1))
    yield "light == n_lights", edit(tri_light=at(k, n_lights))
    yield "light -2", edit(tri_light=at(k, -2))
    yield "a light that is no AREA_TRI light", edit(tri_light=at(k, 2))
    yield "a light named twice", edit(tri_light=at(k, 0))
    yield "a light not named", edit(tri_light=at(11, -1))
    yield "normals on an emissive triangle", edit(tri_light=lambda a: (at(10, -1)(a), at(k, 0)(a)), normals=at(k, 1.0, 4))
    yield "tangents on an emissive triangle", edit(tri_light=lambda a: (at(11, -1)(a), at(k, 1)(a)), tangents=at(k, -0.0, 8))
    yield "a NaN vertex", edit(vertices=at(corner, np.nan, 1))
    yield "an infinite vertex", edit(vertices=at(corner, np.inf, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["numpy", "torch"])
def test_refusals_leave_the_scene_untouched(gpu, memory):
    """every GNXR_ERR_INVALID case, one bad record in an otherwise good mesh, in the middle of the list and in its last triangle: the
    error comes back, bvh4() and a small render are bit-identical to before"""
    b = refusal_scene(gpu)
    g = geometry_of(b)
    d = b.desc()
    nt = len(g["indices"])
    s = gpu.Scene(b)
    it = gpu.PathIntegrator(3, 1.0, "spatial")
    wide0 = s.bvh4()
    img0, _ = it.Render(s, 16, 12, 1)

    def unchanged():
        wide = s.bvh4()
        assert wide[0].tobytes() == wide0[0].tobytes() and wide[1:] == wide0[1:]
        img, _ = it.Render(s, 16, 12, 1)
        assert tsu.biteq(img0, img)
        assert (s.n_vertices, s.n_triangles) == (len(g["vertices"]), nt)

    put = (lambda x: on_device(x, s.device)) if memory == "torch" else (lambda x: x)
    for k in (nt // 2, nt - 1):
        for name, bad in bad_geometries(g, k, d.n_materials, d.n_lights):
            with pytest.raises(gpu.GnxrError) as e:
                s.set_geometry(**put(bad))
            assert f"error {ERR_INVALID}" in str(e.value), (name, k, str(e.value))
            unchanged()
    # what the binding refuses itself is refused by the library too
    arrays = put(g)
    call = lambda rec: gpu.lib().gnxr_scene_set_geometry(s._h, None if rec is None else C.byref(rec), None)
    rec_cases = [None, record(gpu, arrays, struct_size=64), record(gpu, arrays, struct_size=0), record(gpu, arrays, n_vertices=0), record(gpu, arrays, n_triangles=0),
                 record(gpu, arrays, n_triangles=-5), record(gpu, arrays, vertices=None), record(gpu, arrays, indices=None), record(gpu, arrays, tri_material=None),
                 record(gpu, arrays, tri_light=None), record(gpu, arrays, tri_medium_inside=None), record(gpu, arrays, tri_medium_outside=None)]
    other = on_device(g, s.device) if memory == "numpy" else g   # one array from the other side
    rec_cases.append(record(gpu, arrays, vertices=(other["vertices"].data_ptr() if memory == "numpy" else other["vertices"].ctypes.data)))
    rec_cases.append(record(gpu, arrays, tri_light=(other["tri_light"].data_ptr() if memory == "numpy" else other["tri_light"].ctypes.data)))
    for n_case, rec in enumerate(rec_cases):
        assert call(rec) == ERR_INVALID, n_case
        unchanged()
    # and the good mesh is accepted afterwards
    s.set_geometry(**arrays)
    b.set_bvh_split_method("hlbvh")
    tsr.same_scene_tables(s, gpu.Scene(b))


@pytest.mark.gpu
def test_oversized_morton_run_is_refused(gpu):
    """65 536 triangles on one Morton code (the input check of the build itself, no fault): refused, the scene gives the bits it gave before"""
    v_bad, i_bad = thb.make_case("oversized")
    v, i = soup("tiny5")
    s = gpu.Scene(tsr.soup_builder(gpu, v, i, "sah"))
    tree0, wide0 = s.bvh(), s.bvh4()
    with pytest.raises(gpu.GnxrError, match="a leaf exceeds 65535 primitives") as e:
        s.set_geometry(v_bad, i_bad, 0)
    assert f"error {ERR_INVALID}" in str(e.value)
    tree1, wide1 = s.bvh(), s.bvh4()
    for x, y in zip(tree0, tree1):
        assert x.tobytes() == y.tobytes()
    assert wide0[0].tobytes() == wide1[0].tobytes() and wide0[1:] == wide1[1:]
    assert (s.n_vertices, s.n_triangles) == (len(v), len(i))


# ---------------------------------------------------------------- GPU: stream ordering
@pytest.mark.gpu
def test_set_geometry_reads_after_the_work_queued_on_its_stream(gpu):
    """the tensors are written by kernels queued on a side stream immediately before the call on that stream, with no synchronisation from
    the caller in between"""
    b, _ = tsu.dragon(gpu)
    g = geometry_of(b)
    s = gpu.Scene(ReGeom(b, start_geometry(b), "sah").desc())
    dev = f"cuda:{s.device}"
    base = on_device(g, s.device)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        busy = torch.randn(2048, 2048, device=dev)
        for _ in range(8):
            busy = busy @ busy * 1e-3                      # keeps the stream busy while the host runs ahead
        t = {k: (None if x is None else torch.zeros_like(x)) for k, x in base.items()}
        for k, x in base.items():
            if x is not None:
                t[k].add_(x)                               # a kernel on st fills every array
        s.set_geometry(**t)                                # reads on the current stream: st
    b.set_bvh_split_method("hlbvh")
    fresh = gpu.Scene(b)
    tsr.same_scene_tables(s, fresh)
    tsu.same_render(gpu, gpu.PathIntegrator(5, 1.0, "spatial"), s, fresh, W, H, SPP)
    # and with the stream passed explicitly while another one is current
    t2 = permuted(g, seed=81)
    with torch.cuda.stream(st):
        d2 = {k: (None if x is None else torch.from_numpy(x).pin_memory().to(dev, non_blocking=True)) for k, x in t2.items()}
    s.set_geometry(**d2, stream=st)
    tsr.same_scene_tables(s, gpu.Scene(ReGeom(b, t2, "hlbvh").desc()))


# ---------------------------------------------------------------- GPU: replicas
@pytest.mark.gpu
@pytest.mark.parametrize("memory", ["numpy", "torch"])
def test_set_geometry_on_replicas(gpu, memory):
    """Device 0 listed twice, the way test_scene_rebuild.test_rebuild_on_replicas runs it: both copies take the new mesh (the second one
    through the host), and a refusal leaves both alone"""
    b = tsr.attr_scene()
    g = geometry_of(b)
    it = gpu.PathIntegrator(5, 1.0, "spatial")
    single = gpu.Scene(ReGeom(b, g, "hlbvh").desc())
    try:
        gpu.init_devices([0, 0])
        multi = gpu.Scene(ReGeom(b, start_geometry(b), "sah").desc())
        img0, _ = it.Render(multi, 16, 12, 1)
        bad = dict(g)
        bad["indices"] = g["indices"].copy()
        bad["indices"][-1, 2] = len(g["vertices"])
        with pytest.raises(gpu.GnxrError):
            multi.set_geometry(**(on_device(bad, multi.device) if memory == "torch" else bad))
        img1, _ = it.Render(multi, 16, 12, 1)
        assert tsu.biteq(img0, img1)
        multi.set_geometry(**(on_device(g, multi.device) if memory == "torch" else g))
        tsu.same_render(gpu, it, multi, single, W, H, SPP)
        tsr.same_scene_tables(multi, single)
    finally:
        gpu.init(0)

"""numpy float32 restatement of the deformation calls of include/gnxr.h: gnxr_skin_vertices_device (skin), gnxr_scene_recompute_normals
(recompute_normals) and gnxr_scene_update_attributes (update_attributes, a row replacement with the call's refusals).

Every arithmetic step is one rounded float32 operation -- numpy's elementwise multiply, add, subtract, divide and sqrt on float32 arrays are
exactly that, and no expression here lets numpy fuse two of them -- and every sum runs in the order the header states, so the device's
results are compared with these on bits.  Vectorised over vertices where the definition is per vertex; the vertex sums of the normals,
whose order across triangles is part of the definition, are a plain loop."""
import numpy as np

f32 = np.float32
UV_DEFAULT = np.array([0, 0, 1, 0, 1, 1], f32)


def _f(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == f32, a.dtype
    return a


def skin(rest, bone_index, bone_weight, bones, morph_delta=None, morph_weight=None):
    """(V, 3) float32 positions.  rest (V, 3), bone_index (V, 4) int32, bone_weight (V, 4), bones (B, 3, 4) or (B, 12), morph_delta
    (M, V, 3), morph_weight (M,).  Raises ValueError for a bone index outside [0, B) in a slot with a non-zero weight."""
    rest, bone_weight = _f(rest), _f(bone_weight)
    bones = _f(bones).reshape(-1, 3, 4)
    q = rest.copy()
    if morph_delta is not None:
        morph_delta, morph_weight = _f(morph_delta), _f(morph_weight)
        for m in range(len(morph_delta)):
            q = q + morph_weight[m] * morph_delta[m]          # one multiply, one add per component
    P = np.zeros_like(q)
    for k in range(4):
        w = bone_weight[:, k]
        used = w != 0                                          # a slot whose weight is exactly 0 (either sign) is skipped, its index not looked at
        b = bone_index[used, k]
        if ((b < 0) | (b >= len(bones))).any():
            raise ValueError("bone index out of range in a used slot")
        m, x = bones[b], q[used]
        T = ((m[:, :, 0] * x[:, 0:1] + m[:, :, 1] * x[:, 1:2]) + m[:, :, 2] * x[:, 2:3]) + m[:, :, 3]
        P[used] = P[used] + w[used, None] * T
    assert P.dtype == f32
    return P


def smooth_rows(tri_n):
    """which triangles are smooth: a bit set anywhere in the nine floats of the row (-0 counts)"""
    return (_f(tri_n).reshape(-1, 9).view(np.uint32) != 0).any(axis=1)


def recompute_normals(vertices, indices, tri_n, flip=False):
    """(new tri_n (T, 9), number of corners of smooth triangles that kept their old normal).  vertices (V, 3): what the scene holds;
    indices (T, 3) int32; tri_n (T, 9): the rows the scene holds (zero rows: flat triangles)."""
    v, tri_n = _f(vertices), _f(tri_n).reshape(-1, 9)
    idx = np.asarray(indices).reshape(-1, 3)
    S = smooth_rows(tri_n)
    p0, p1, p2 = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    a, b = p1 - p0, p2 - p0
    F = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)
    assert F.dtype == f32
    if flip:
        F = -F
    N = np.zeros((len(v), 3), f32)                             # every sum starts from +0
    with np.errstate(over="ignore", invalid="ignore"):
        for t in np.flatnonzero(S):                            # ascending authoring triangle ...
            for k in range(3):                                 # ... then ascending corner
                N[idx[t, k]] = N[idx[t, k]] + F[t]
        out, kept = tri_n.copy(), 0
        for t in np.flatnonzero(S):
            for k in range(3):
                n = N[idx[t, k]]
                l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
                if np.isfinite(l2) and l2 > 0:
                    out[t, 3 * k:3 * k + 3] = n / np.sqrt(l2)  # three divisions by the one rounded root
                else:
                    kept += 1
    assert out.dtype == f32
    return out, kept


def own_attributes(tri_uv, tri_n, tri_s, n_triangles):
    """the own-attribute byte per triangle: uvs that differ in a bit from the defaults, or a bit set in the normal or tangent row"""
    own = np.zeros(n_triangles, bool)
    if tri_uv is not None:
        own |= (_f(tri_uv).reshape(-1, 6).view(np.uint32) != UV_DEFAULT.view(np.uint32)).any(axis=1)
    for a in (tri_n, tri_s):
        if a is not None:
            own |= smooth_rows(a)
    return own


def update_attributes(tables, tri_light, first, uv=None, normals=None, tangents=None):
    """tables = (tri_uv, tri_n, tri_s) of the scene (None: no such table) -> the tables after the edit.  Raises ValueError("invalid") /
    ValueError("unsupported") where the call refuses; tri_light (T,) int32: >= 0 marks an emissive triangle."""
    rows = (uv, normals, tangents)
    nt = len(tri_light)
    given = [r for r in rows if r is not None]
    n = len(given[0]) if given else 0
    if first < 0 or first + n > nt or (not given):
        raise ValueError("invalid")
    if any(r is not None and t is None for r, t in zip(rows, tables)):
        raise ValueError("unsupported")
    new = [None if t is None else _f(t).copy() for t in tables]
    for r, t in zip(rows, new):
        if r is not None:
            t[first:first + n] = _f(r)
    if (own_attributes(*new, nt) != own_attributes(*tables, nt)).any():
        raise ValueError("unsupported")
    emissive = np.asarray(tri_light)[first:first + n] >= 0
    for r in rows[1:]:
        if r is not None and (smooth_rows(r) & emissive).any():
            raise ValueError("unsupported")
    return tuple(new)


def icosphere(subdivisions=2, radius=1.0):
    """An icosahedron subdivided `subdivisions` times with shared vertices (2: 162 vertices, 320 triangles), counter-clockwise seen from
    outside: (vertices (V, 3) float32, indices (T, 3) int32)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in tris:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = out
    return (np.asarray(v) * radius).astype(f32), np.asarray(tris, np.int32)

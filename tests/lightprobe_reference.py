"""numpy restatement of the light probes (include/gnxr.h, "Light probes"): the probe rays, the projection on the nine real spherical
harmonics of bands 0 to 2 with its butterfly sums, the bake's scaling and the irradiance, each operation a single fp32 operation in the
written order.  The device results are compared with these on bits."""
import numpy as np

f32 = np.float32
PI = f32(3.14159265358979323846)
FOUR_PI = f32(12.566370614359172)
A0, A1, A2 = f32(3.14159265), f32(2.09439510), f32(0.78539816)
A = [A0, A1, A1, A1, A2, A2, A2, A2, A2]
BLOCK = 64


def biteq(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------- the basis
def basis(d):
    """d: (..., 3) float32 -> (..., 9) float32"""
    d = np.asarray(d, f32)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    Y = np.empty(d.shape[:-1] + (9,), f32)
    Y[..., 0] = f32(0.282095)
    Y[..., 1] = f32(0.488603) * y
    Y[..., 2] = f32(0.488603) * z
    Y[..., 3] = f32(0.488603) * x
    Y[..., 4] = f32(1.092548) * (x * y)
    Y[..., 5] = f32(1.092548) * (y * z)
    Y[..., 6] = f32(0.315392) * ((f32(3) * (z * z)) - f32(1))
    Y[..., 7] = f32(1.092548) * (x * z)
    Y[..., 8] = f32(0.546274) * ((x * x) - (y * y))
    return Y


# ---------------------------------------------------------------- probe rays
def probe_directions(u, sincos):
    """UniformSampleSphere (core/Sampling.cpp:72-77).  u: (n, 2) = Halton dimensions 3 and 4; sincos(theta) -> (sin, cos) with the
    library's bits.  Returns d (n, 3)."""
    u = np.asarray(u, f32)
    z = f32(1) - f32(2) * u[:, 0]
    r = np.sqrt(np.maximum(f32(0), f32(1) - z * z))
    phi = (f32(2) * PI) * u[:, 1]
    s, c = sincos(phi.astype(f32))
    return np.stack([r * c, r * s, z], axis=1).astype(f32)


def probe_rays(pos, px, py, s, u, W, H, medium, sincos):
    """(rays [n, 8], samples [n, 4], valid [n]) of gnxr_lightprobe_rays_device; u: (n, 2) Halton dimensions 3 and 4 of the records (anything
    where a record is invalid)"""
    pos = np.asarray(pos, f32)
    n = len(pos)
    valid = np.isfinite(pos).all(axis=1) & (px >= 0) & (px < W) & (py >= 0) & (py < H) & (s >= 0)
    d = probe_directions(np.where(valid[:, None], u, f32(0.5)), sincos)
    rays, samples = np.zeros((n, 8), f32), np.zeros((n, 4), np.int32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = pos, f32(np.inf), d
    samples[:] = np.stack([px, py, s, np.full(n, medium, np.int32)], axis=1)
    rays[~valid] = 0
    samples[~valid] = 0
    return rays, samples, valid


# ---------------------------------------------------------------- the projection
def butterfly(v):
    """v: (..., 64) float32, lane l on the last axis.  For m = 32 .. 1 every lane becomes v[l] + v[l ^ m]; returns lane 0."""
    v = np.array(v, f32)
    assert v.shape[-1] == BLOCK
    lanes = np.arange(BLOCK)
    with np.errstate(all="ignore"):
        for m in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lanes ^ m]
    return v[..., 0]


def project(d, L, n_probes, start=None):
    """d: (n_probes * n_samples, 3) directions, L: (n_probes * n_samples, 3+) radiance, probe-major.  Returns the sums (n_probes, 9, 4);
    start: the sums to continue from (GNXR_SH_CONTINUE), else 0."""
    d, L = np.asarray(d, f32).reshape(n_probes, -1, 3), np.asarray(L, f32).reshape(n_probes, -1, np.shape(L)[-1])[..., :3]
    n_samples = d.shape[1]
    out = np.zeros((n_probes, 9, 4), f32)
    acc = np.zeros((n_probes, 9, 3), f32) if start is None else np.array(np.asarray(start, f32)[..., :3], f32)
    with np.errstate(all="ignore"):
        terms = L[:, :, None, :] * basis(d)[:, :, :, None]          # (probe, sample, slot, channel)
        for b0 in range(0, n_samples, BLOCK):
            block = np.zeros((n_probes, BLOCK, 9, 3), f32)              # a lane past n_samples holds +0.0f
            block[:, :min(BLOCK, n_samples - b0)] = terms[:, b0:b0 + BLOCK]
            acc = acc + butterfly(np.moveaxis(block, 1, -1))
    out[..., :3] = acc
    return out


def bake_scale(sums, spp):
    """sums (n_probes, 9, 4) over all spp samples -> coefficients: rgb = (sum * 4 pi) / spp, w = 0"""
    out = np.zeros_like(np.asarray(sums, f32))
    out[..., :3] = (np.asarray(sums, f32)[..., :3] * FOUR_PI) / f32(spp)
    return out


# ---------------------------------------------------------------- evaluation
def irradiance(sh, probe, normals):
    """sh: (n_probes, 9, 4), probe: (n,) int, normals: (n, 3).  Returns (E [n, 4], valid [n])."""
    sh, normals, probe = np.asarray(sh, f32), np.asarray(normals, f32), np.asarray(probe)
    valid = (probe >= 0) & (probe < len(sh))
    c = sh[np.where(valid, probe, 0)][..., :3] if len(sh) else np.zeros((len(probe), 9, 3), f32)    # (n, 9, 3)
    Y = basis(normals)                                              # (n, 9)
    with np.errstate(all="ignore"):
        e = A[0] * (c[:, 0] * Y[:, 0, None])
        for j in range(1, 9):
            e = e + A[j] * (c[:, j] * Y[:, j, None])
    E = np.concatenate([e.astype(f32), np.ones((len(probe), 1), f32)], axis=1)
    E[~valid] = 0
    return E, valid

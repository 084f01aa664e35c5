"""Temporal accumulation (include/gnxr.h, "Temporal accumulation") restated in numpy: the pixel-centre camera ray, the reprojection of
gnxr_motion_device and the validate / gather / blend of gnxr_temporal_accumulate_device.  Every array is float32 and every operation
one numpy operation, so each is rounded on its own in the written order, as the kernels' are.  WorldToRaster comes from
gx.camera_matrices, its single definition.

TEST INFRASTRUCTURE: imported only from tests/."""
import numpy as np

f32 = np.float32
INF = f32(np.inf)
EPS = f32(2.0 ** -24)
GAMMA3 = (f32(3) * EPS) / (f32(1) - f32(3) * EPS)


def biteq(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())


def lum(r, g, b):
    return (f32(0.212671) * r + f32(0.715160) * g) + f32(0.072169) * b


def finite(x):
    return (np.ascontiguousarray(x, f32).view(np.uint32) & 0x7f800000) != 0x7f800000


# ---------------------------------------------------------------- the camera ray (camera_ray of kernels.hip.h for a pinhole)
def camera_ray(r2c, c2w, ortho, pfx, pfy):
    """(o, d), each (n, 3), of the film positions (pfx, pfy) = pixel + film sample: camera_ray's operations with lens_radius == 0"""
    with np.errstate(all="ignore"):
        r, m = np.asarray(r2c, f32).reshape(16), np.asarray(c2w, f32).reshape(16)
        pfx, pfy = np.asarray(pfx, f32), np.asarray(pfy, f32)
        zero = np.zeros_like(pfx)

        def point(k):   # xform_point: left to right
            return ((r[4 * k] * pfx + r[4 * k + 1] * pfy) + r[4 * k + 2] * zero) + r[4 * k + 3]

        xp, yp, zp, wp = point(0), point(1), point(2), point(3)
        inv = f32(1) / wp
        one = wp == 1
        pc = [np.where(one, xp, inv * xp), np.where(one, yp, inv * yp), np.where(one, zp, inv * zp)]
        if ortho:
            oc, dc = pc, [zero, zero, zero + f32(1)]
        else:
            il = f32(1) / np.sqrt((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2])
            oc, dc = [zero, zero, zero], [pc[0] * il, pc[1] * il, pc[2] * il]
        x, y, z = oc

        def row(k):
            return (m[4 * k] * x + m[4 * k + 1] * y) + (m[4 * k + 2] * z + m[4 * k + 3])

        def row_abs(k):
            return ((np.abs(m[4 * k] * x) + np.abs(m[4 * k + 1] * y)) + np.abs(m[4 * k + 2] * z)) + np.abs(m[4 * k + 3])

        xw, yw, zw, ww = row(0), row(1), row(2), row(3)
        err = [GAMMA3 * row_abs(0), GAMMA3 * row_abs(1), GAMMA3 * row_abs(2)]
        iw = f32(1) / ww
        onew = ww == 1
        ow = [np.where(onew, xw, iw * xw), np.where(onew, yw, iw * yw), np.where(onew, zw, iw * zw)]
        dw = [(m[4 * k] * dc[0] + m[4 * k + 1] * dc[1]) + m[4 * k + 2] * dc[2] for k in range(3)]
        l2 = (dw[0] * dw[0] + dw[1] * dw[1]) + dw[2] * dw[2]
        dt = ((np.abs(dw[0]) * err[0] + np.abs(dw[1]) * err[1]) + np.abs(dw[2]) * err[2]) / l2
        pos = l2 > 0
        ow = [np.where(pos, ow[k] + dw[k] * dt, ow[k]) for k in range(3)]
        return np.stack(ow, -1).astype(f32), np.stack(dw, -1).astype(f32)


def centre_rays(gx, camera, W, H):
    """the (H * W, 8) gnxr_ray records of the rays through the pixel centres, row-major: (o, +inf, d, 0)"""
    m = gx.camera_matrices(camera, W, H)
    py, px = np.mgrid[0:H, 0:W]
    o, d = camera_ray(m["r2c"], m["c2w"], bool(camera.orthographic), px.reshape(-1).astype(f32) + f32(0.5), py.reshape(-1).astype(f32) + f32(0.5))
    return gx.make_rays(o, d, np.inf)


# ---------------------------------------------------------------- gnxr_motion_device after the hit
def reproject(gx, rays, hits, camera, prev_camera, W, H, prev_corners=None):
    """motion (n, 4), guide (n, 4), prim (n,) from the centre rays and their gnxr_hit records (gx.HIT_DTYPE).  prev_corners: None, or
    (n, 3, 3) float32, the previous positions of the three corners of each ray's hit triangle (rows of other rays are not read) together
    with a mask: a pair (corners, is_triangle)."""
    with np.errstate(all="ignore"):
        n = len(rays)
        o, d = rays[:, 0:3], rays[:, 4:7]
        prim, t = hits["prim"], hits["t"]
        miss = prim < 0
        guide = np.concatenate([hits["n"], t[:, None]], 1).astype(f32)
        guide[miss] = 0
        pm = gx.camera_matrices(prev_camera, W, H)
        m, c2w = pm["w2r"].reshape(16), pm["c2w"].reshape(16)
        eye = [c2w[3], c2w[7], c2w[11]]
        P = [o[:, k] + t * d[:, k] for k in range(3)]
        if prev_corners is not None:
            q, is_tri = prev_corners
            b0, b1, b2 = hits["b0"], hits["b1"], hits["b2"]
            P = [np.where(is_tri & ~miss, (b0 * q[:, 0, k] + b1 * q[:, 1, k]) + b2 * q[:, 2, k], P[k]) for k in range(3)]
        if camera.orthographic:
            P = [np.where(miss, o[:, k], P[k]) for k in range(3)]
        else:
            P = [np.where(miss, eye[k] + d[:, k], P[k]) for k in range(3)]
        X, Y, Z = P

        def row(k):
            return (m[4 * k] * X + m[4 * k + 1] * Y) + (m[4 * k + 2] * Z + m[4 * k + 3])

        xr, yr, zr, w = row(0), row(1), row(2), row(3)
        one = w == 1
        xq, yq = np.where(one, xr, xr / w), np.where(one, yr, yr / w)
        if prev_camera.orthographic:
            tq = zr * f32(10)
        else:
            e = [X - eye[0], Y - eye[1], Z - eye[2]]
            tq = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        tq = np.where(miss, f32(0), tq).astype(f32)
        ok = (w > 0) & finite(xq) & finite(yq) & finite(tq)
        motion = np.stack([xq, yq, tq, np.ones(n, f32)], 1).astype(f32)
        motion[~ok] = 0
        return motion, guide, prim.astype(np.int32)


# ---------------------------------------------------------------- gnxr_temporal_accumulate_device
def accumulate(color, motion, guide, prim, history, max_history, depth_tol, normal_cos, branches=None):
    """(out_color, out_stat) for arrays of shape (V, H, W, 4) and prim (V, H, W); history: None or the dict {"color", "stat", "guide",
    "prim"}.  branches: a dict that receives one boolean (V, H, W) mask per branch of the definition (which pixels took it)."""
    with np.errstate(all="ignore"):
        color, motion, guide = (np.ascontiguousarray(a, f32) for a in (color, motion, guide))
        V, H, W, _ = color.shape
        depth_tol, normal_cos, M = f32(depth_tol), f32(normal_cos), f32(max_history)
        c = [color[..., k] for k in range(3)]
        l = lum(*c)
        cur_ok = finite(c[0]) & finite(c[1]) & finite(c[2])
        zero = np.zeros((V, H, W), f32)
        sw, s1, s2, sN = zero.copy(), zero.copy(), zero.copy(), zero.copy()
        sc = [zero.copy(), zero.copy(), zero.copy()]
        br = {} if branches is None else branches
        if history is not None:
            hc, hs, hg = (np.ascontiguousarray(history[k], f32) for k in ("color", "stat", "guide"))
            hp = np.asarray(history["prim"], np.int32)
            flagged = motion[..., 3] != 0
            fx, fy = motion[..., 0] - f32(0.5), motion[..., 1] - f32(0.5)
            rx, ry = np.rint(fx).astype(f32), np.rint(fy).astype(f32)
            snap_x, snap_y = np.abs(fx - rx) <= f32(1 / 256), np.abs(fy - ry) <= f32(1 / 256)
            fx, fy = np.where(snap_x, rx, fx), np.where(snap_y, ry, fy)
            in_range = (fx >= -1) & (fx < f32(W)) & (fy >= -1) & (fy < f32(H))
            gather = flagged & in_range
            fx, fy = np.where(gather, fx, f32(0)), np.where(gather, fy, f32(0))   # (what follows is only used under `gather`)
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - x0, fy - y0
            ix, iy = x0.astype(np.int64), y0.astype(np.int64)
            tq = motion[..., 2]
            view = np.arange(V)[:, None, None]
            counted_any = np.zeros((V, H, W), bool)
            fails = {k: np.zeros((V, H, W), bool) for k in ("outside", "zero_length", "prim", "nonfinite", "depth", "normal")}
            close = {k: np.zeros((V, H, W), bool) for k in ("depth", "normal")}
            n_counted = np.zeros((V, H, W), np.int32)
            for i, j in ((0, 0), (1, 0), (0, 1), (1, 1)):
                b = (ax if i else f32(1) - ax) * (ay if j else f32(1) - ay)
                qx, qy = ix + i, iy + j
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                q_c, q_s, q_g, q_p = hc[view, cy, cx], hs[view, cy, cx], hg[view, cy, cx], hp[view, cy, cx]
                live = gather & (b > 0)
                ok_len = q_s[..., 2] > 0
                ok_prim = q_p == prim
                ok_fin = finite(q_c[..., 0]) & finite(q_c[..., 1]) & finite(q_c[..., 2]) & finite(q_s[..., 0]) & finite(q_s[..., 1])
                dz = np.abs(q_g[..., 3] - tq)
                ok_depth = (prim < 0) | (dz <= depth_tol * tq)
                cosn = (guide[..., 0] * q_g[..., 0] + guide[..., 1] * q_g[..., 1]) + guide[..., 2] * q_g[..., 2]
                ok_normal = (prim < 0) | (cosn >= normal_cos)
                ok = live & inside & ok_len & ok_prim & ok_fin & ok_depth & ok_normal
                rest = live & inside
                fails["outside"] |= live & ~inside
                fails["zero_length"] |= rest & ~ok_len
                fails["prim"] |= rest & ok_len & ~ok_prim
                fails["nonfinite"] |= rest & ok_len & ok_prim & ~ok_fin
                fails["depth"] |= rest & ok_len & ok_prim & ok_fin & ~ok_depth
                fails["normal"] |= rest & ok_len & ok_prim & ok_fin & ok_depth & ~ok_normal
                close["depth"] |= ok & (prim >= 0) & (dz > f32(0.9) * (depth_tol * tq))
                close["normal"] |= ok & (prim >= 0) & (cosn < normal_cos + f32(0.01))
                n_counted += ok
                sw = np.where(ok, sw + b, sw)
                for k in range(3):
                    sc[k] = np.where(ok, sc[k] + b * q_c[..., k], sc[k])
                s1 = np.where(ok, s1 + b * q_s[..., 0], s1)
                s2 = np.where(ok, s2 + b * q_s[..., 1], s2)
                sN = np.where(ok, sN + b * q_s[..., 2], sN)
            br.update({"flag0": ~flagged, "out_of_range": flagged & ~in_range, "snapped": gather & snap_x & snap_y, "fractional": gather & ~snap_x & ~snap_y,
                       "one_tap": n_counted == 1, "four_taps": n_counted == 4, "miss_pair": (n_counted > 0) & (prim < 0)})
            br.update({"tap_" + k: v for k, v in fails.items()})
            br.update({"close_" + k: v for k, v in close.items()})
        have = sw > 0
        Hc = [sc[k] / sw for k in range(3)]
        M1, M2, N = s1 / sw, s2 / sw, sN / sw
        Nn = np.minimum(N + f32(1), M)
        alpha = f32(1) / Nn
        blend = [Hc[k] + alpha * (c[k] - Hc[k]) for k in range(3)]
        m1 = M1 + alpha * (l - M1)
        m2 = M2 + alpha * (l * l - M2)

        def var(a, b):
            v = b - a * a
            return np.where(v > 0, v, f32(0))

        out_c, out_s = np.zeros((V, H, W, 4), f32), np.zeros((V, H, W, 4), f32)
        both, only_cur, only_hist = have & cur_ok, ~have & cur_ok, have & ~cur_ok
        for k in range(3):
            out_c[..., k] = np.where(both, blend[k], np.where(only_cur, c[k], np.where(only_hist, Hc[k], f32(0))))
        out_c[..., 3] = color[..., 3]
        for k, (a, b_, c_) in enumerate(((m1, l, M1), (m2, l * l, M2), (Nn, zero + f32(1), N), (var(m1, m2), zero, var(M1, M2)))):
            out_s[..., k] = np.where(both, a, np.where(only_cur, b_, np.where(only_hist, c_, f32(0))))
        br.update({"blend": both, "first": only_cur, "keep_history": only_hist, "nothing": ~have & ~cur_ok, "clamped": both & (N + f32(1) > M)})
        return out_c, out_s

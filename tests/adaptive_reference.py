"""Adaptive sampling (gnxr_render_adaptive_device, include/gnxr.h) restated in numpy float32.

TEST INFRASTRUCTURE: the plain model tests/test_adaptive.py compares the device rounds (csrc/adaptive_kernel.hip.h, csrc/api_adaptive.hip.h)
with.  It is sequential on purpose: one sample at a time, one float32 operation at a time (numpy rounds every elementwise float32
operation once, as the library built with -ffp-contract=off does), the guard window as a loop over its offsets.

    S, n, rounds = adaptive_reference(L, spp, min_spp, step_spp, threshold, floor, guard)

Schedule: round 0 gives every pixel min_spp samples, every later round gives the active pixels (n samples each) max(step_spp, n // 8)
more, cut at spp.

takes the per-sample radiance L[s, y, x, 3] (float32, s in [0, spp)) and returns the rgb sums S[y, x, 3] (float32), the sample counts
n[y, x] (int32) and the number of rounds.  adaptive_image(S, n) is the image the call writes: (S / (float)n, 1).
"""
import numpy as np

F = np.float32


def guard_window(noisy, guard):
    """out[y, x] = some q with |qx - x| <= guard and |qy - y| <= guard INSIDE the image has noisy[q]: shifted copies, clipped at the border"""
    noisy = np.asarray(noisy, bool)
    H, W = noisy.shape
    out = np.zeros((H, W), bool)
    for dy in range(-guard, guard + 1):
        for dx in range(-guard, guard + 1):
            # out[y, x] |= noisy[y + dy, x + dx] where that pixel exists
            y0, y1 = max(0, -dy), min(H, H - dy)
            x0, x1 = max(0, -dx), min(W, W - dx)
            if y0 < y1 and x0 < x1:
                out[y0:y1, x0:x1] |= noisy[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def criterion(S, A, n, threshold, floor):
    """noisy = !(e <= threshold * (m + floor * n)), every operation a single float32 one in the written order; a NaN is noisy"""
    S, A = np.asarray(S, F), np.asarray(A, F)
    with np.errstate(all="ignore"):
        d = [np.abs(S[..., c] - (A[..., c] + A[..., c])) for c in range(3)]
        e = (d[0] + d[1]) + d[2]
        m = (S[..., 0] + S[..., 1]) + S[..., 2]
        bound = F(threshold) * (m + F(floor) * np.asarray(n).astype(F))
        return ~(e <= bound)


def adaptive_reference(L, spp, min_spp, step_spp, threshold, floor, guard):
    L = np.asarray(L, F)
    assert L.ndim == 4 and L.shape[3] == 3 and L.shape[0] >= spp and 1 <= min_spp <= spp and step_spp >= 1 and 0 <= guard <= 8
    H, W = L.shape[1:3]
    S = np.zeros((H, W, 3), F)
    A = np.zeros((H, W, 3), F)
    n = np.zeros((H, W), np.int32)
    active = np.ones((H, W), bool)
    rounds = 0
    with np.errstate(all="ignore"):
        while active.any():
            # the schedule, per pixel: min_spp, then step_spp or an eighth of what the pixel has, whichever is more
            take = np.full((H, W), min_spp) if rounds == 0 else np.maximum(step_spp, n // 8)
            first = n.copy()
            while (active & (n < spp) & (n - first < take)).any():
                go = active & (n < spp) & (n - first < take)          # truncated at the budget
                s = n[go]                        # the next sample of every such pixel
                ys, xs = np.nonzero(go)
                l = L[s, ys, xs]
                S[go] = S[go] + l
                even = (s & 1) == 0
                A[ys[even], xs[even]] = A[ys[even], xs[even]] + l[even]
                n[go] += 1
            rounds += 1
            noisy = criterion(S, A, n, threshold, floor)
            active = active & (n < spp) & guard_window(active & noisy, guard)
    return S, n, rounds


def adaptive_image(S, n):
    img = np.ones(S.shape[:2] + (4,), F)
    with np.errstate(all="ignore"):
        img[..., :3] = S / n.astype(F)[..., None]
    return img

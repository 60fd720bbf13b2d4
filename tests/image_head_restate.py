"""TEST INFRASTRUCTURE: numpy restatement of the image head at the points (include/epnet_ops.h: epnet_image_head_points), tap by
tap from the rule alone:

    out[b, c, n] = sum over the in-bounds taps in the order nw, ne, sw, se of weight_tap * relu(shift[c] + sum_j wf[c, j] * d[j](tap))
    d(tap)       = cat_l(wd_l[Y % k_l, X % k_l, :, :]^T . F_l[b, :, Y // k_l, X // k_l])

Every sum runs in ascending index order in `dtype`, so that with float64 it is a yardstick and with float32 a restatement of
the kernels' arithmetic. No torch, no np.matmul.
"""
import numpy as np


def taps(xy, h, w, align_corners, dtype):
    """taps.h in `dtype`: (x0, y0) int arrays and the four weights (nw, ne, sw, se), each of xy's leading shape"""
    dt = np.dtype(dtype).type
    x, y = xy[..., 0].astype(dtype), xy[..., 1].astype(dtype)
    if align_corners:
        ix = ((x + dt(1)) / dt(2)) * dt(w - 1)
        iy = ((y + dt(1)) / dt(2)) * dt(h - 1)
    else:
        ix = ((x + dt(1)) * dt(w) - dt(1)) / dt(2)
        iy = ((y + dt(1)) * dt(h) - dt(1)) / dt(2)
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(ix), np.floor(iy)
        ok = (fx >= -1) & (fx <= w - 1) & (fy >= -1) & (fy <= h - 1)
    fx, fy, ix, iy = (np.where(ok, v, dt(-2)) for v in (fx, fy, ix, iy))
    x_e, y_s = fx + dt(1), fy + dt(1)
    weights = ((x_e - ix) * (y_s - iy), (ix - fx) * (y_s - iy), (x_e - ix) * (iy - fy), (ix - fx) * (iy - fy))
    return fx.astype(np.int64), fy.astype(np.int64), weights


def image_head_at_points(maps, weights, kernels, wf, shift, xy, align_corners=True, dtype=np.float64):
    """maps[l] (B, C_l, H / k_l, W / k_l), weights[l] (k_l, k_l, C_l, R_l), wf (q, sum R), shift (q), xy (B, N, 2) -> (B, q, N)"""
    maps = [np.asarray(m, dtype=dtype) for m in maps]
    weights = [np.asarray(v, dtype=dtype) for v in weights]
    wf, shift = np.asarray(wf, dtype=dtype), np.asarray(shift, dtype=dtype)
    b, n = xy.shape[:2]
    h, w = maps[0].shape[2] * kernels[0], maps[0].shape[3] * kernels[0]
    q, sum_r = wf.shape
    x0, y0, tw = taps(np.asarray(xy), h, w, align_corners, dtype)
    scene = np.arange(b)[:, None].repeat(n, 1)
    out = np.zeros((b, n, q), dtype=dtype)
    for t in range(4):
        px, py = x0 + (t & 1), y0 + (t >> 1)
        inside = (px >= 0) & (py >= 0) & (px < w) & (py < h)
        cx, cy = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
        d = []
        for fmap, wd, k in zip(maps, weights, kernels):
            col = fmap[scene, :, cy // k, cx // k]                 # (B, N, C)
            sl = wd[cy % k, cx % k]                                # (B, N, C, R)
            acc = np.zeros((b, n, wd.shape[3]), dtype=dtype)
            for ci in range(wd.shape[2]):
                acc = acc + sl[:, :, ci, :] * col[:, :, ci, None]
            d.append(acc)
        d = np.concatenate(d, axis=2)
        s = np.zeros((b, n, q), dtype=dtype)
        for j in range(sum_r):
            s = s + wf[None, None, :, j] * d[:, :, j, None]
        v = shift[None, None, :] + s
        v = np.where(v < 0, np.zeros((), dtype=dtype), v)
        out = out + np.where(inside[:, :, None], v * tw[t][:, :, None], np.zeros((), dtype=dtype))
    return np.ascontiguousarray(out.transpose(0, 2, 1))

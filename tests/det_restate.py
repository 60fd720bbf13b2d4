"""numpy restatements of the orders that the deterministic gradients promise (include/epnet_ops.h, "*_det" entry points).
Every function works in float32, one rounding per operation, and returns a new array; `start` is the buffer's incoming value.
Shared by tests/test_deterministic_cpu.py and tests/test_deterministic_gpu.py."""
import numpy as np

f32 = np.float32


def scatter_in_order(start, rows, flat_idx, n):
    """start (b, c, n); rows (b, c, p) terms in contract order; flat_idx (b, p) targets. np.add.at is unbuffered: the terms of a
    target are added one after the other in entry order, g[j] = g[j] + term. Targets outside [0, n) add nothing."""
    out = np.array(start, dtype=f32, copy=True)
    for bi in range(out.shape[0]):
        ok = (flat_idx[bi] >= 0) & (flat_idx[bi] < n)
        j = flat_idx[bi][ok]
        for ci in range(out.shape[1]):
            np.add.at(out[bi, ci], j, rows[bi, ci][ok])
    return out


def gather_points_grad(start, grad_out, idx):
    return scatter_in_order(start, grad_out, idx, start.shape[2])


def group_points_grad(start, grad_out, idx):
    b, c = grad_out.shape[:2]
    return scatter_in_order(start, grad_out.reshape(b, c, -1), idx.reshape(b, -1), start.shape[2])


def three_interpolate_grad(start, grad_out, idx, weight):
    """entries (unknown i, k = 0, 1, 2): term = grad_out[c, i] * weight[i, k]"""
    b, c, n = grad_out.shape
    terms = (grad_out[:, :, :, None].astype(f32) * weight[:, None, :, :].astype(f32)).astype(f32)
    return scatter_in_order(start, terms.reshape(b, c, n * 3), idx.reshape(b, n * 3), start.shape[2])


def taps(xy, h, w, align_corners):
    """taps_of (csrc/taps.h) in float32: xy (..., 2) -> pixel (..., 4) int64 (-1 where the tap is outside), weight (..., 4),
    taps in the order nw, ne, sw, se"""
    x, y = xy[..., 0].astype(f32), xy[..., 1].astype(f32)
    with np.errstate(invalid="ignore", over="ignore"):
        if align_corners:
            ix = ((x + f32(1)) / f32(2)) * f32(w - 1)
            iy = ((y + f32(1)) / f32(2)) * f32(h - 1)
        else:
            ix = ((x + f32(1)) * f32(w) - f32(1)) / f32(2)
            iy = ((y + f32(1)) * f32(h) - f32(1)) / f32(2)
        fx, fy = np.floor(ix).astype(f32), np.floor(iy).astype(f32)
        far = ~((fx >= -1) & (fx <= w - 1) & (fy >= -1) & (fy <= h - 1))
    fx, fy, ix, iy = [np.where(far, f32(-2), v).astype(f32) for v in (fx, fy, ix, iy)]
    x_e, y_s = fx + f32(1), fy + f32(1)
    wts = np.stack([(x_e - ix) * (y_s - iy), (ix - fx) * (y_s - iy), (x_e - ix) * (iy - fy), (ix - fx) * (iy - fy)], -1).astype(f32)
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    xs = np.stack([x0, x0 + 1, x0, x0 + 1], -1)
    ys = np.stack([y0, y0, y0 + 1, y0 + 1], -1)
    ok = (xs >= 0) & (ys >= 0) & (xs < w) & (ys < h)
    return np.where(ok, ys * w + xs, -1), wts


def feature_gather_grad(start, grad_out, xy, align_corners):
    """start (b, c, h, w); grad_out (b, c, n); xy (b, n, 2): points in order, taps nw, ne, sw, se, term = grad_out * weight"""
    b, c, h, w = start.shape
    n = grad_out.shape[2]
    pix, wts = taps(xy, h, w, align_corners)
    terms = (grad_out[:, :, :, None].astype(f32) * wts[:, None, :, :]).astype(f32)
    out = scatter_in_order(start.reshape(b, c, h * w), terms.reshape(b, c, n * 4), pix.reshape(b, n * 4), h * w)
    return out.reshape(b, c, h, w)


TILE, THREADS, WAVE = 4096, 256, 64


def group_linear_grad_w(start, grad_out, xyz, new_xyz, idx, chunk=256):
    """the fixed order of epnet_group_linear_grad_w_det: per scene, tiles of 4096 positions, slot i of a tile sums positions
    i, i + 256, ... in order from 0; xor butterfly over the 64 slots of each quarter; quarters in order from 0; tiles in
    order from 0; scenes in order from 0; grad_w = grad_w + total. (Scenes are restated `chunk` at a time, each on its own;
    the rounds of a lone tile that hold no position would leave every slot as it is and are left out.)"""
    b, c, npoint, ns = grad_out.shape
    p = npoint * ns
    tiles = -(-p // TILE)
    rounds = TILE // THREADS if tiles > 1 else -(-p // THREADS)
    present = np.zeros(tiles * rounds * THREADS, bool)
    present[:p] = True
    present = present.reshape(tiles, rounds, THREADS)
    total = np.zeros((c, 3), f32)
    for b0 in range(0, b, chunk):
        bs = np.arange(b0, min(b, b0 + chunk))
        ix = idx[bs].reshape(len(bs), p).astype(np.int64)
        d = (xyz[bs[:, None], ix] - np.repeat(new_xyz[bs], ns, axis=1)).astype(f32)                  # (k, p, 3)
        terms = (grad_out[bs].reshape(len(bs), c, p)[:, :, :, None] * d[:, None]).astype(f32)      # (k, c, p, 3)
        pad = np.zeros((len(bs), c, tiles * rounds * THREADS, 3), f32)
        pad[:, :, :p] = terms
        pad = pad.reshape(len(bs), c, tiles, rounds, THREADS, 3)
        acc = np.zeros((len(bs), c, tiles, THREADS, 3), f32)
        for k in range(rounds):
            acc = np.where(present[None, None, :, k, :, None], (acc + pad[:, :, :, k]).astype(f32), acc)
        acc = acc.reshape(len(bs), c, tiles, THREADS // WAVE, WAVE, 3)
        off = WAVE // 2
        while off >= 1:                 # lane l ^ off: the lanes as (WAVE / 2 off, 2, off), the middle axis reversed
            part = acc.reshape(acc.shape[:-2] + (WAVE // (2 * off), 2, off, 3))[..., ::-1, :, :].reshape(acc.shape)
            acc = (acc + part).astype(f32)
            off //= 2
        v = np.zeros((len(bs), c, tiles, 3), f32)
        for wv in range(THREADS // WAVE):
            v = (v + acc[:, :, :, wv, 0]).astype(f32)
        scene = np.zeros((len(bs), c, 3), f32)
        for t in range(tiles):
            scene = (scene + v[:, :, t]).astype(f32)
        for k in range(len(bs)):
            total = (total + scene[k]).astype(f32)
    return (np.asarray(start, f32) + total).astype(f32)

"""TEST INFRASTRUCTURE: numpy restatement of the RPN inputs from raw scans (include/epnet_ops.h: epnet_scan_prepare and
epnet_image_normalise; reference: the first half of get_rpn_with_li_fusion, lib/datasets/kitti_rcnn_dataset.py:281-356).

``transform`` is the contract's arithmetic one float32 operation at a time in the stated order (numpy rounds every elementwise
float32 operation once and fuses nothing; no np.dot). ``transform64`` evaluates the same formulas in float64 from the float32
inputs: the yardstick of the reference's BLAS products, whose summation order is not known. ``select`` is the table of cases,
``prepare`` one scene end to end, ``image_normalise`` the float64 expression rounded once.
"""
import os

import numpy as np

F = np.float32
SCOPE = np.array([[-40, 40], [-1, 3], [0, 70.4]], np.float64)      # the reference's PC_AREA_SCOPE (lib/config.py:26-28)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)             # lib/datasets/kitti_dataset.py:24-25
NEAR = 40.0


def composite(V2C, R0, dtype=F):
    V2C, R0 = np.asarray(V2C, dtype).reshape(3, 4), np.asarray(R0, dtype).reshape(3, 3)
    m = np.zeros((4, 3), dtype)
    for k in range(4):
        for j in range(3):
            m[k, j] = (V2C[0, k] * R0[j, 0] + V2C[1, k] * R0[j, 1]) + V2C[2, k] * R0[j, 2]
    return m


def _transform(pts, V2C, R0, P2, dtype):
    pts, P2 = np.asarray(pts, F).reshape(-1, 4).astype(dtype), np.asarray(P2, F).reshape(3, 4).astype(dtype)
    m = composite(np.asarray(V2C, F), np.asarray(R0, F), dtype)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    with np.errstate(all="ignore"):
        rect = [((x * m[0, j] + y * m[1, j]) + z * m[2, j]) + m[3, j] for j in range(3)]
        X, Y, Z = rect
        pr = [((X * P2[r, 0] + Y * P2[r, 1]) + Z * P2[r, 2]) + P2[r, 3] for r in range(3)]
        u, v = pr[0] / Z, pr[1] / Z
        depth = pr[2] - P2[2, 3]
    return np.stack(rect, axis=1), np.stack([u, v], axis=1), depth


def transform(pts, V2C, R0, P2):
    """pts (P,4) float32 -> rect (P,3), uv (P,2), depth (P), all float32 in the contract's order"""
    out = _transform(pts, V2C, R0, P2, F)
    assert all(a.dtype == F for a in out)
    return out


def transform64(pts, V2C, R0, P2):
    return _transform(pts, V2C, R0, P2, np.float64)


def classify(pts, num_raw, V2C, R0, P2, img_shape, reduce_by_range=True, scope=SCOPE, near_depth=NEAR):
    """-> rect, uv, valid (P) bool, near (P) bool (valid and Z < near_depth)"""
    rect, uv, depth = transform(pts, V2C, R0, P2)
    p = rect.shape[0]
    h, w = F(int(img_shape[0])), F(int(img_shape[1]))
    with np.errstate(invalid="ignore"):
        valid = (uv[:, 0] >= 0) & (uv[:, 0] < w) & (uv[:, 1] >= 0) & (uv[:, 1] < h) & (depth >= 0)
        if reduce_by_range:
            sc = np.asarray(scope, np.float64).reshape(3, 2)
            r64 = rect.astype(np.float64)
            for j in range(3):
                valid &= (r64[:, j] >= sc[j, 0]) & (r64[:, j] <= sc[j, 1])
        valid &= np.arange(p) < min(max(int(num_raw), 0), p)
        near = valid & (rect[:, 2] < F(near_depth))
    return rect, uv, valid, near


def smallest(members, keys, r):
    """the r members (raw indices, ascending) with the smallest (unsigned key, raw index), in raw order"""
    members = np.asarray(members, np.int64)
    k = np.asarray(keys).astype(np.int64) & 0xFFFFFFFF
    order = np.lexsort((members, k[members]))
    return np.sort(members[order[:r]])


def select(valid, near, keys, n):
    """-> L (n raw indices, or None in case 4), (V, F, case, r, q)"""
    vi, fi, ni = np.nonzero(valid)[0], np.nonzero(valid & ~near)[0], np.nonzero(near)[0]
    V, Fc = len(vi), len(fi)
    if V == 0:
        return None, (0, 0, 4, 0, 0)
    if V > n:
        if Fc <= n:
            case, s0, q, s1, r = 0, fi, 1, ni, n - Fc
        else:
            case, s0, q, s1, r = 5, fi[:0], 0, fi, n
    else:
        case = 1 if V == n else (2 if 2 * V >= n else 3)
        q = n // V if case == 3 else 1
        s0, s1, r = vi, vi, n - q * V
    L = np.concatenate([np.tile(s0, q), smallest(s1, keys, r)]).astype(np.int64)
    assert len(L) == n
    return L, (V, Fc, case, r, q)


def prepare(pts, num_raw, V2C, R0, P2, img_shape, keys, slot_perm, n, reduce_by_range=True, scope=SCOPE, near_depth=NEAR):
    """one scene -> dict of pts_rect (n,3), pts_intensity (n), pts_origin_xy (n,2), pts_input (n,4), choice (n) int32, scene_info (6) int32"""
    pts = np.asarray(pts, F).reshape(-1, 4)
    p = pts.shape[0]
    rect, uv, valid, near = classify(pts, num_raw, V2C, R0, P2, img_shape, reduce_by_range, scope, near_depth)
    L, (V, Fc, case, r, q) = select(valid, near, keys, n)
    out = {"pts_rect": np.zeros((n, 3), F), "pts_intensity": np.zeros(n, F), "pts_origin_xy": np.zeros((n, 2), F),
           "choice": np.full(n, -1, np.int32), "scene_info": np.array([min(max(int(num_raw), 0), p), V, Fc, case, r, q], np.int32)}
    if L is not None:
        slot = np.arange(n) if slot_perm is None else np.asarray(slot_perm, np.int64)
        out["pts_rect"][slot] = rect[L]
        out["pts_intensity"][slot] = pts[L, 3] - F(0.5)
        out["pts_origin_xy"][slot] = uv[L]
        out["choice"][slot] = L
    out["pts_input"] = np.concatenate([out["pts_rect"], out["pts_intensity"][:, None]], axis=1)
    return out


KEYS = ("pts_rect", "pts_intensity", "pts_origin_xy", "pts_input", "choice", "scene_info")


def prepare_batch(pts, num_raw, V2C, R0, P2, img_shape, keys, slot_perm, n, **kw):
    rows = [prepare(pts[k], num_raw[k], V2C[k], R0[k], P2[k], img_shape[k], keys[k], None if slot_perm is None else slot_perm[k], n, **kw)
            for k in range(len(pts))]
    return {key: np.stack([r[key] for r in rows]) for key in KEYS}


def image_normalise(img, img_shape=None, out_hw=(384, 1280), mean=MEAN, std=STD):
    """img (B,H,W,3) uint8 -> (B,3,h_out,w_out) float32: the reference's float64 expression, rounded once, zero padding"""
    img = np.asarray(img, np.uint8)
    b, h_in, w_in = img.shape[:3]
    out = np.zeros((b, 3, out_hw[0], out_hw[1]), F)
    for k in range(b):
        hk, wk = (h_in, w_in) if img_shape is None else (int(img_shape[k][0]), int(img_shape[k][1]))
        hk, wk = min(max(hk, 0), h_in, out_hw[0]), min(max(wk, 0), w_in, out_hw[1])
        im = img[k, :hk, :wk].astype(np.float64)
        im = im / 255.0
        im -= np.array(mean, np.float64)
        im /= np.array(std, np.float64)
        out[k, :, :hk, :wk] = im.astype(F).transpose(2, 0, 1)
    return out


# ---- seeded scenes with a wanted number of valid and far points (shared by the CPU and the GPU tests) ---------------------------
def calib(seed=0):
    """KITTI-typical V2C, R0, P2 (float32) and [h, w] = [375, 1242], perturbed by the seed"""
    rng = np.random.default_rng(1000 + seed)
    V2C = np.array([[7.5337e-03, -9.9997e-01, -6.1660e-04, -4.0698e-03], [1.4802e-02, 7.2807e-04, -9.9989e-01, -7.6316e-02],
                    [9.9986e-01, 7.5238e-03, 1.4808e-02, -2.7178e-01]]) + rng.normal(0, 1e-4, (3, 4))
    R0 = np.array([[9.9992e-01, 9.8378e-03, -7.4451e-03], [-9.8698e-03, 9.9994e-01, -4.2785e-03],
                   [7.4025e-03, 4.3516e-03, 9.9996e-01]]) + rng.normal(0, 1e-5, (3, 3))
    P2 = np.array([[7.2154e+02, 0.0, 6.0956e+02, 4.4857e+01], [0.0, 7.2154e+02, 1.7285e+02, 2.1638e-01], [0.0, 0.0, 1.0, 2.7459e-03]])
    P2[0, 2] += rng.normal(0, 2.0)
    return V2C.astype(F), R0.astype(F), P2.astype(F), np.array([375, 1242], np.int32)


def scene_with(p, num_raw, valid_far, valid_near, seed):
    """(p,4) velodyne points of which exactly valid_far + valid_near of the first num_raw pass the view and scope test (valid_far
    of them at 40 m or farther), at random rows; the others are behind the sensor. Returns pts and the calibration."""
    rng = np.random.default_rng(seed)
    V2C, R0, P2, shape = calib(seed)
    assert valid_far + valid_near <= num_raw <= p
    pts = np.zeros((p, 4))
    pts[:, 0] = -rng.uniform(2, 60, p)                                # behind: negative depth
    pts[:, 1], pts[:, 2], pts[:, 3] = rng.uniform(-20, 20, p), rng.uniform(-2, 0.5, p), rng.uniform(0, 1, p)
    rows = rng.permutation(num_raw)[:valid_far + valid_near] if num_raw else np.zeros(0, np.int64)
    k = len(rows)
    depth = np.concatenate([rng.uniform(42, 68, valid_far), rng.uniform(6, 38, valid_near)])
    pts[rows, 0] = depth
    pts[rows, 1] = rng.uniform(-0.2, 0.2, k) * depth                  # inside the image: |x / z| below 0.3 or so
    pts[rows, 2] = rng.uniform(-1.6, -0.4, k)
    # the padding rows beyond num_raw look valid: only the count keeps them out
    if num_raw < p:
        pts[num_raw:, 0], pts[num_raw:, 1], pts[num_raw:, 2] = 20.0, 1.0, -1.0
    pts = pts.astype(F)
    rect, uv, valid, near = classify(pts, num_raw, V2C, R0, P2, shape)
    assert int(valid.sum()) == valid_far + valid_near and int((valid & ~near).sum()) == valid_far, (valid.sum(), (valid & ~near).sum())
    return pts, V2C, R0, P2, shape


def fixture():
    """tests/golden/scan_prepare.npz -> list of scene dicts (inputs, tables, the reference's outputs)"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_prepare.npz"))
    scenes = []
    for i in range(int(z["scenes"])):
        pre = "s%d__" % i
        scenes.append({k[len(pre):]: z[k] for k in z.files if k.startswith(pre)})
    return scenes

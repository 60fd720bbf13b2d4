"""CPU restatement of the fused SA tail (include/epnet_ops.h: epnet_sa_tail_f32).

``fma32`` is a correctly rounded float32 fused multiply-add in numpy float64: the product of two float32 values is exact in
float64 (48 bits), the sum with the addend is rounded to ODD at 53 bits (TwoSum gives the exact rounding error of the float64
addition; where it is not zero and the sum's last bit is even, the sum moves one unit towards the error), and a value rounded
to odd at 53 >= 24 + 2 bits rounds to float32 -- normal or denormal -- as the exact value does. ``fma32_exact`` is the same
operation in rational arithmetic, for tests/test_sa_tail.py to hold ``fma32`` to.

``restate`` is the rule of the header, ``true_tail`` the same tail in float64 without any float32 rounding, ``stock_tail`` the
unfused module lines in stock torch ops.
"""
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """round_f32(a * b + c) for float32 arrays (broadcast), one rounding"""
    a, b, c = (np.asarray(v, dtype=F32) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p, c = np.broadcast_arrays(a.astype(F64) * b.astype(F64), c.astype(F64))   # the product is exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                   # TwoSum: s + err == p + c exactly
        bits = s.copy().view(np.int64)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
        up = (err > 0) == (s > 0)                         # away from zero: the bit pattern grows, whatever the sign
        bits = np.where(fix, np.where(up, bits + 1, bits - 1), bits)
        return bits.view(F64).astype(F32)


def round_f32_exact(v: Fraction) -> float:
    """a rational number rounded to the nearest float32 (ties to even, denormals kept, overflow to infinity)"""
    if v == 0:
        return 0.0
    sign, m = (-1.0 if v < 0 else 1.0), abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1
    assert Fraction(2) ** e <= m < Fraction(2) ** (e + 1)
    q = Fraction(2) ** (max(e, -126) - 23)
    n = m / q
    lo = n.numerator // n.denominator
    rest = n - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    r = lo * q
    if r >= Fraction(2) ** 128:
        return sign * float("inf")
    return sign * float(r)


def fma32_exact(a, b, c) -> float:
    return round_f32_exact(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _relu(v):
    return np.where((v > 0) | np.isnan(v), v, v.dtype.type(0))


def x_prime(x, s_in, t_in, relu_in):
    """float32 x' of the rule"""
    x = np.asarray(x, dtype=F32)
    if s_in is not None:
        x = fma32(x, np.asarray(s_in, F32)[None, :, None, None], np.asarray(t_in, F32)[None, :, None, None])
    return _relu(x) if relu_in else x


def restate(x, w, b, s_in=None, t_in=None, relu_in=False):
    """x (B,K,P,S), w (C,K), b (C) or None -> y (B,C,P) float32, the header's rule"""
    xp = x_prime(x, s_in, t_in, relu_in)
    w = np.asarray(w, dtype=F32)
    bsz, k, p, s = xp.shape
    acc = np.zeros((bsz, w.shape[0], p, s), dtype=F32)
    for kk in range(k):
        acc = fma32(w[None, :, kk, None, None], xp[:, kk][:, None], acc)
    with np.errstate(all="ignore"):
        m = acc.max(axis=3)                               # numpy's max keeps a NaN
        if b is not None:
            m = m + np.asarray(b, dtype=F32)[None, :, None]
        return _relu(m.astype(F32))


def true_tail(x, w, b, s_in=None, t_in=None, relu_in=False, with_bound=False):
    """the same tail in float64 on the float32 inputs. with_bound: also K * 2^-24 * max_s sum_k |w x'| per output, the bound of
    the float32 chain's distance from it (x' taken in float64: use it where s_in is None, so that x' is exact)"""
    x = np.asarray(x, dtype=F64)
    if s_in is not None:
        x = x * np.asarray(s_in, F64)[None, :, None, None] + np.asarray(t_in, F64)[None, :, None, None]
    if relu_in:
        x = _relu(x)
    w = np.asarray(w, dtype=F64)
    with np.errstate(all="ignore"):
        a = np.einsum("ck,bkps->bcps", w, x)
        m = a.max(axis=3)
        if b is not None:
            m = m + np.asarray(b, F64)[None, :, None]
        y = _relu(m)
        if not with_bound:
            return y
        mag = np.einsum("ck,bkps->bcps", np.abs(w), np.abs(x)).max(axis=3)
        return y, x.shape[1] * 2.0 ** -24 * mag


def ulp32(v):
    """the float32 unit in the last place at |v| (float64 array in, float64 out)"""
    v = np.abs(np.asarray(v, dtype=F64)).astype(F32)
    with np.errstate(all="ignore"):
        return (np.nextafter(v, F32(np.inf)) - v).astype(F64)


def stock_tail(hidden, layers, dtype=None):
    """the unfused module lines: the given layers (what the fused tail replaces: [bn,] relu, conv, [bn,] relu) and
    F.max_pool2d over the nsample axis, in stock torch ops; dtype=torch.float64 runs a float64 copy of the layers"""
    import copy

    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        h = hidden if dtype is None else hidden.to(dtype)
        for layer in layers:
            layer = copy.deepcopy(layer)
            if dtype is not None:
                layer = layer.to(dtype)
            h = layer.eval()(h)
        return F.max_pool2d(h, kernel_size=[1, h.size(3)]).squeeze(-1)


def bits_equal(got, want):
    """bit for bit, with -0 == +0 and every NaN equal to every NaN"""
    got, want = np.asarray(got, dtype=F32), np.asarray(want, dtype=F32)
    if got.shape != want.shape:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got[~nan_g], want[~nan_w]))


def random_case(rng, bsz, k, c, p, s, affine, scale=1.0):
    """seeded inputs of one case: x, w, b, s_in, t_in (None without `affine`)"""
    x = (rng.standard_normal((bsz, k, p, s)) * scale).astype(F32)
    w = (rng.standard_normal((c, k)) / np.sqrt(k)).astype(F32)
    b = (rng.standard_normal(c) * 0.5).astype(F32)
    s_in = t_in = None
    if affine:
        s_in = rng.uniform(0.5, 1.5, k).astype(F32) * rng.choice([-1.0, 1.0], k).astype(F32)
        t_in = (rng.standard_normal(k) * 0.3).astype(F32)
    return x, w, b, s_in, t_in

"""16-bit feature rows without a GPU: the library exports and validates the *_h entry points, and the restatement of the rule
(tests/rows16_restate.py, the yardstick of tests/test_rows16_gpu.py) agrees with stock CPU torch wherever stock torch defines
the answer."""
import pytest
import torch
import torch.nn.functional as F

import rows16_restate as R

EINVAL = -1
SYMBOLS = ("epnet_group_linear_h", "epnet_pool_max_h", "epnet_pool_max_grad_h", "epnet_three_interpolate_h")
P = 0x1000     # a non-null "pointer": validation fails before anything looks at it


def test_library_exports_the_entry_points(hiplib):
    from epnet_amd import _lib
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES
        assert getattr(hiplib, name) is not None
    assert hiplib.epnet_abi_version() == 1          # additive change


@pytest.mark.parametrize("dtype", [0, 3, -1, 16])
def test_unknown_dtype_is_rejected(hiplib, dtype):
    assert hiplib.epnet_group_linear_h(1, 1, 4, 1, 4, P, P, P, P, P, None, P, dtype, None) == EINVAL
    assert hiplib.epnet_pool_max_h(1, 4, P, P, None, dtype, None) == EINVAL
    assert hiplib.epnet_pool_max_grad_h(1, 4, P, P, P, dtype, None) == EINVAL
    assert hiplib.epnet_three_interpolate_h(1, 1, 4, 4, P, P, P, P, dtype, None) == EINVAL
    # also for an empty problem: the type is checked first
    assert hiplib.epnet_pool_max_h(0, 4, None, None, None, dtype, None) == EINVAL


@pytest.mark.parametrize("dtype", [1, 2])
def test_null_pointers_and_negative_sizes(hiplib, dtype):
    gl = hiplib.epnet_group_linear_h
    for k in range(7):          # xyz, new_xyz, z, idx, w_xyz, (bias may be NULL), out
        ptrs = [P] * 7
        ptrs[k] = None
        xyz, new_xyz, z, idx, w, out = ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[6]
        if k == 5:
            continue
        assert gl(1, 1, 4, 1, 4, xyz, new_xyz, z, idx, w, None, out, dtype, None) == EINVAL
    for sizes in ((-1, 1, 4, 1, 4), (1, -1, 4, 1, 4), (1, 1, -4, 1, 4), (1, 1, 4, -1, 4), (1, 1, 4, 1, -4), (1, 1, 0, 1, 4)):
        assert gl(*sizes, P, P, P, P, P, None, P, dtype, None) == EINVAL
    assert gl(0, 1, 4, 1, 4, None, None, None, None, None, None, None, dtype, None) == 0      # empty: nothing to look at

    pm, pg = hiplib.epnet_pool_max_h, hiplib.epnet_pool_max_grad_h
    assert pm(1, 4, None, P, None, dtype, None) == EINVAL and pm(1, 4, P, None, None, dtype, None) == EINVAL
    assert pm(-1, 4, P, P, None, dtype, None) == EINVAL and pm(1, 0, P, P, None, dtype, None) == EINVAL
    assert pm(0, 4, None, None, None, dtype, None) == 0
    assert pg(1, 4, None, P, P, dtype, None) == EINVAL and pg(1, 4, P, None, P, dtype, None) == EINVAL
    assert pg(1, 4, P, P, None, dtype, None) == EINVAL and pg(-1, 4, P, P, P, dtype, None) == EINVAL
    assert pg(1, 0, P, P, P, dtype, None) == EINVAL and pg(0, 4, None, None, None, dtype, None) == 0

    ti = hiplib.epnet_three_interpolate_h
    for k in range(4):
        ptrs = [P] * 4
        ptrs[k] = None
        assert ti(1, 1, 4, 4, *ptrs, dtype, None) == EINVAL
    for sizes in ((-1, 1, 4, 4), (1, -1, 4, 4), (1, 1, -4, 4), (1, 1, 4, -4)):
        assert ti(*sizes, P, P, P, P, dtype, None) == EINVAL
    assert ti(1, 0, 4, 4, None, None, None, None, dtype, None) == 0


def test_the_four_rounding_cases():
    """what `.to(T)` of CPU torch does, i.e. what the restatement's one rounding means"""
    bf = torch.bfloat16
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    assert R.rn(f(1.0) + f(2.0 ** -8), bf).item() == 1.0                                   # tie -> even (down)
    assert R.rn((f(1.0) + f(2.0 ** -7)) + f(2.0 ** -8), bf).item() == 1.015625             # tie -> even (up)
    tiny = R.rn(f(1e-39), bf)
    assert tiny.item() != 0.0 and abs(tiny.item() - 1e-39) <= 2.0 ** -134                  # a bf16 denormal, kept (step 2^-133)
    assert tiny.view(torch.int16).item() == 0x000B
    assert R.rn(f(3e38) + f(1e38), bf).item() == float("inf")                              # overflow
    assert torch.isnan(R.rn(f(float("nan")), bf)).item()
    # the same rule for float16
    h = torch.float16
    assert R.rn(f(1.0) + f(2.0 ** -11), h).item() == 1.0
    assert R.rn((f(1.0) + f(2.0 ** -10)) + f(2.0 ** -11), h).item() == 1.0 + 2.0 ** -9
    assert R.rn(f(2.0 ** -24), h).item() == 2.0 ** -24
    assert R.rn(f(60000.0) + f(60000.0), h).item() == float("inf")


@pytest.mark.parametrize("dtype", R.TYPES)
def test_pool_restatement_is_max_pool2d(dtype):
    g = torch.Generator().manual_seed(3)
    values = torch.tensor([-3.0, -1.5, -1.0, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0]).to(dtype)
    for ns in (1, 3, 8, 32, 257):
        x = values[torch.randint(0, 16, (2, 5, 7, ns), generator=g)]
        x[0, 0, 0] = 2.0                                    # a whole row of ties
        x[1, 4, 6, ns // 2:] = float("-inf")
        stock, stock_arg = F.max_pool2d(x.float(), kernel_size=[1, ns], return_indices=True)
        got, arg = R.pool_max(x.reshape(-1, ns))
        assert got.dtype == dtype
        assert torch.equal(got.float().reshape(2, 5, 7, 1), stock)                       # -0 == +0 here: the VALUE agrees
        assert torch.equal(arg.long().reshape(2, 5, 7, 1), stock_arg % ns)               # ties: the first, as the stock scan
        grad = values[torch.randint(0, 16, (2 * 5 * 7,), generator=g)]
        gx = R.pool_max_grad(grad, arg, ns)
        xs = x.float().requires_grad_(True)
        F.max_pool2d(xs, kernel_size=[1, ns]).backward(grad.float().reshape(2, 5, 7, 1))
        assert torch.equal(gx.float().reshape(2, 5, 7, ns), xs.grad)
    x = values[torch.randint(0, 16, (4, 8), generator=g)]
    x[1, 3] = float("nan")
    x[1, 5] = float("nan")
    got, arg = R.pool_max(x)
    assert torch.isnan(got[1]) and arg[1] == 3 and not torch.isnan(got[[0, 2, 3]]).any()


@pytest.mark.parametrize("dtype", R.TYPES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_group_linear_restatement_is_the_convolution(dtype, with_bias):
    """against conv(cat(grouped xyz - centre, grouped features)) in float64 -- the layer the op replaces -- within one ulp of
    T at the result (float32 arithmetic error, ~2^-21 relative, plus the one rounding, half an ulp)"""
    g = torch.Generator().manual_seed(5)
    b, c_in, c, n, m, ns = 2, 6, 5, 64, 5, 3
    xyz = torch.randn((b, n, 3), generator=g)
    new_xyz = xyz[:, :m].clone()
    feats = torch.randn((b, c_in, n), generator=g)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    w = torch.randn((c, 3 + c_in), generator=g)
    bias = torch.randn((c,), generator=g) if with_bias else None
    z = torch.matmul(w[:, 3:], feats).to(dtype)
    got = R.group_linear(xyz, new_xyz, z, idx, w[:, :3].contiguous(), bias)
    assert got.dtype == dtype and got.shape == (b, c, m, ns)
    # float64, from the SAME rounded z (the dense product is the caller's)
    grouped_xyz = torch.stack([xyz[k][idx[k].long()] for k in range(b)]).permute(0, 3, 1, 2) - new_xyz.transpose(1, 2)[..., None]
    ref = torch.einsum("cj,bjms->bcms", w[:, :3].double(), grouped_xyz.double()) + R.grouping(z, idx).double()
    if with_bias:
        ref = ref + bias.double().reshape(1, c, 1, 1)
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=1e-30))) - R.MANTISSA_BITS[dtype])
    assert bool(((got.double() - ref).abs() <= ulp).all())


@pytest.mark.parametrize("dtype", R.TYPES)
def test_three_interpolate_restatement(dtype):
    g = torch.Generator().manual_seed(7)
    points = torch.randn((2, 4, 9), generator=g).to(dtype)
    idx = torch.randint(0, 9, (2, 11, 3), generator=g, dtype=torch.int32)
    weight = torch.rand((2, 11, 3), generator=g)
    got = R.three_interpolate(points, idx, weight)
    ref = sum(weight[:, None, :, j].double() * torch.stack([points[k][:, idx[k, :, j].long()] for k in range(2)]).double()
              for j in range(3))
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=1e-30))) - R.MANTISSA_BITS[dtype])
    # three products of one sign-mixed sum: the float32 error is relative to the largest term, not to the result
    slack = 3 * 2.0 ** -23 * sum((weight[:, None, :, j].double() * 4).abs() for j in range(3))
    assert got.dtype == dtype and bool(((got.double() - ref).abs() <= ulp + slack).all())
